"""The inference path on the GPU: the forward-only level kernels and sweep (mmft.sweep.FORWARD_ONLY) and mmft.infer.Predictor.
Every comparison is torch.equal: the new path is tied bit for bit to paths that test_bf16_oracle*, test_model_gpu and
test_validate_with_frozen_statistics hold to the oracle."""
import contextlib
import copy

import numpy as np
import pytest
import torch

from mmft import lib
from test_unet_eval_gpu import snapshot, assert_unchanged

pytestmark = pytest.mark.gpu

KEPT = ('A', 'LSE', 'HS', 'HN', 'HN16', 'G', 'DA')
SHAPES = [(6000, 12), (40000, 8)]          # levels of 1 000 rows: 16-row workgroups (RB = 1); of 10 000 rows: 32-row workgroups (RB = 2)


def _designs(shape, fanin='regular'):
    from mmft.synth import synth_design
    return [synth_design(N=shape[0], L=shape[1], tile=32, seed=120 + i, end_frac=0.2, fanin=fanin) for i in range(2)]


def _sweep(pmodel, b, ends, grad, cone=False):
    """One whole sweep on a zeroed h -> (h[ends], h, {kernel name: launches})."""
    from mmft import sweep as S
    g = b.graph
    g.ndata['h'] = torch.zeros((b.N, 128), dtype=torch.float32, device=ends.device)
    lib.prof_reset()
    lib.prof_enable(True)
    try:
        with contextlib.nullcontext() if grad else torch.no_grad():
            out = S.sweep_forward_all(pmodel.gnn, g, b.level_nodes, ends, cone=cone)
        torch.cuda.synchronize()
    finally:
        lib.prof_enable(False)
    return out.detach().clone(), g.ndata['h'].clone(), {r['name']: r['launches'] for r in lib.prof_report()}


def _buf_bytes(g):
    return sum(t.numel() * t.element_size() for v in g._sweep_bufs.values() for t in (v if isinstance(v, tuple) else (v,))
               if torch.is_tensor(t))


# ------------------------------------------------------------------------------------------------ 3. regular designs
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('slots', [True, False])
@pytest.mark.parametrize('case', ['plain', 'no_relu', 'cone'])
def test_forward_only_sweep_equals_the_training_form(dev, shape, slots, case):
    from mmft import sweep as S
    from mmft.train import build_models, DesignBatch
    designs = _designs(shape)
    pmodel, _ = build_models(map_size=designs[0].map_size, device=dev, seed=8)
    if case == 'no_relu':
        pmodel.gnn.activation = None
    ids = [np.arange(0, 5) for d in designs] if case == 'cone' else [np.arange(0, d.num_paths, 3) for d in designs]
    twin, infer = ('level_fwd_slots_kernel', 'level_fwd_slots_infer_kernel') if slots else ('level_fwd_bf16_kernel', 'level_fwd_bf16_infer_kernel')
    saved = S.LEVEL_SLOTS
    S.LEVEL_SLOTS = slots
    try:
        with lib.math_mode('bf16'):
            res = []
            for grad in (True, False):
                b = DesignBatch(designs, dev)
                ends = b.select(ids)[0]
                res.append(_sweep(pmodel, b, ends, grad, cone=(case == 'cone')))
                assert b.graph._sweep.relu == (case != 'no_relu') and (b.graph._sweep.active is not None) == (case == 'cone')
    finally:
        S.LEVEL_SLOTS = saved
    (out_t, h_t, names_t), (out_i, h_i, names_i) = res
    # (the last level is a net level: its gather alone is a pair_fwd_gather launch in every form)
    others = {'level_fwd_slots_kernel', 'level_fwd_slots_infer_kernel', 'level_fwd_bf16_kernel', 'level_fwd_bf16_infer_kernel'}
    assert twin in names_t and not (others - {twin}) & set(names_t), sorted(names_t)
    assert infer in names_i and not (others - {infer}) & set(names_i), sorted(names_i)
    assert names_i[infer] == names_t[twin] == shape[1] // 2 - 1 and names_i.get('pair_fwd_gather_kernel') == names_t.get('pair_fwd_gather_kernel')
    assert bool(h_t.any()) and torch.equal(h_i, h_t) and torch.equal(out_i, out_t)
    if case == 'cone':
        assert bool((h_t == 0).all(dim=1).any())             # rows outside the cone were skipped by both


# ------------------------------------------------------------------------------------------------ 4. heavy fan-in
@pytest.mark.parametrize('shape', SHAPES)
def test_forward_only_sweep_with_heavy_fan_in_levels(dev, shape):
    from mmft.train import build_models, DesignBatch
    designs = _designs(shape, fanin='irregular')
    pmodel, _ = build_models(map_size=designs[0].map_size, device=dev, seed=8)
    ids = [np.arange(0, d.num_paths, 3) for d in designs]
    with lib.math_mode('bf16'):
        res = []
        for grad in (True, False):
            b = DesignBatch(designs, dev)
            res.append(_sweep(pmodel, b, b.select(ids)[0], grad) + (b,))
    (out_t, h_t, names_t, _), (out_i, h_i, names_i, b) = res
    fold = b.graph._sweep.fold
    assert all(fold[l]['heavy_in'] is not None for l in range(2, b.L, 2))
    assert 'pair_fwd_gather_kernel' in names_i and not [n for n in names_i if '_infer' in n], sorted(names_i)
    assert names_i['pair_fwd_gather_kernel'] == names_t['pair_fwd_gather_kernel']
    assert torch.equal(h_i, h_t) and torch.equal(out_i, out_t)
    assert not set(b.graph._sweep_bufs) & {'LSE', 'HS', 'HN', 'HN16', 'G', 'DA'}, sorted(b.graph._sweep_bufs)
    assert b.graph._sweep.HN is None


# ------------------------------------------------------------------------------------------------ 5. nothing kept
@pytest.mark.parametrize('shape', SHAPES)
def test_forward_only_sweep_keeps_and_writes_nothing_for_a_backward(dev, shape):
    from mmft.train import build_models, DesignBatch
    designs = _designs(shape)
    pmodel, _ = build_models(map_size=designs[0].map_size, device=dev, seed=8)
    ids = [np.arange(0, d.num_paths, 3) for d in designs]
    with lib.math_mode('bf16'):
        b = DesignBatch(designs, dev)
        out, h, names = _sweep(pmodel, b, b.select(ids)[0], grad=False)
        assert 'level_fwd_slots_infer_kernel' in names
        assert not set(b.graph._sweep_bufs) & set(KEPT), sorted(b.graph._sweep_bufs)
        st = b.graph._sweep
        assert st.HN is None and st.decided()['HN'] is None and st.PRE is not None
        assert _buf_bytes(b.graph) == b.N * 128 * 4 + 4 * 256 * 128 * 2          # PRE and the four weight packs
        # buffers of those names that happen to exist are not touched either
        b2 = DesignBatch(designs, dev)
        bufs = b2.graph._sweep_bufs
        bufs['key'] = (b2.N, 128, 256, h.device)
        for name in KEPT:
            width, dtype = (256 if name.startswith('H') else 128), (torch.bfloat16 if name == 'HN16' else torch.float32)
            bufs[name] = torch.full((b2.N, width), float('nan'), dtype=dtype, device=dev)
        out2, h2, names2 = _sweep(pmodel, b2, b2.select(ids)[0], grad=False)
        assert 'level_fwd_slots_infer_kernel' in names2
        for name in KEPT:
            assert bufs is b2.graph._sweep_bufs and bool(torch.isnan(bufs[name]).all()), name
        assert torch.equal(h2, h) and torch.equal(out2, out)


# ------------------------------------------------------------------------------------------------ 6. interleaving
@pytest.mark.parametrize('mode', ['sweep', 'dropin'])
def test_training_steps_around_a_forward_only_sweep_equal_a_twin_without_it(dev, mode):
    """A forward-only sweep between two training steps on the same graph (validate(), then a bare sweep): its recorded launches
    have keys of their own, so the next training step re-issues (or replays) the launches that store A / LSE / HN."""
    from mmft import sweep as S
    from mmft.evaluate import validate
    from mmft.synth import synth_design
    from mmft.train import build_models, TrainStep
    designs = [synth_design(N=6000, L=12, tile=32, seed=120 + i, end_frac=0.2) for i in range(2)]
    rng = np.random.default_rng(3)
    steps = 3 if mode == 'sweep' else 5             # drop-in: step 0 level by level, 1 speculative, 2 captures, 3 and 4 replay
    batches = [[rng.permutation(d.num_paths)[:40] for d in designs] for _ in range(steps + 2)]
    assert S.SWEEP_REPLAY and S.RECORD_LAUNCHES
    out = {}
    with lib.math_mode('bf16'):
        for visit in (True, False):
            pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=11)
            ts = TrainStep(pmodel, cnn, designs, dev, mode=mode)
            losses = [float(ts.step(ids)[0]) for ids in batches[:steps]]
            g = ts.batch.graph
            rec = g._sweep_bufs['replay']
            if mode == 'dropin':
                assert rec.fwd.graph is not None and rec.bwd.graph is not None
            if visit:
                m = validate(ts, frozen_stats=True)
                assert g._sweep_bufs['replay'] is rec and ('fi', 2) in rec.calls and ('f', 2) in rec.calls and np.isfinite(m['loss'])
                assert g._sweep.HN is None and not g._sweep.need_grad
                with torch.no_grad():
                    S.sweep_forward_all(pmodel.gnn, g, ts.batch.level_nodes, ts.batch.select(batches[0])[0])
            grads = []
            for ids in batches[steps:]:
                losses.append(float(ts.step(ids)[0]))
                grads.append(ts.optim.flat_grad.clone())
            torch.cuda.synchronize()
            assert g._sweep_bufs['replay'] is rec
            if mode == 'dropin':
                assert rec.fwd.calls == rec.bwd.calls == steps + 1          # the visit neither replayed nor re-captured them
            out[visit] = (losses, grads, ts.optim.flat_param.clone())
    assert out[True][0] == out[False][0]
    for a, b in zip(out[True][1], out[False][1]):
        assert bool(a.any()) and torch.equal(a, b)
    assert torch.equal(out[True][2], out[False][2])


# ------------------------------------------------------------------------------------------------ 7. the flag off, fp32 mode
def test_flag_off_runs_the_training_kernels_and_fp32_mode_runs_what_it_ran(dev):
    from mmft import sweep as S
    from mmft.train import build_models, DesignBatch
    designs = _designs(SHAPES[0])
    pmodel, _ = build_models(map_size=designs[0].map_size, device=dev, seed=8)
    ids = [np.arange(0, d.num_paths, 3) for d in designs]
    res = {}
    try:
        for mode in ('bf16', 'f32'):
            for key, flag, grad in (('train', True, True), ('on', True, False), ('off', False, False)):
                S.FORWARD_ONLY = flag
                with lib.math_mode(mode):
                    b = DesignBatch(designs, dev)
                    res[mode, key] = _sweep(pmodel, b, b.select(ids)[0], grad) + (set(b.graph._sweep_bufs),)
    finally:
        S.FORWARD_ONLY = True
    for mode in ('bf16', 'f32'):
        for key in ('on', 'off'):
            assert torch.equal(res[mode, key][1], res[mode, 'train'][1]) and torch.equal(res[mode, key][0], res[mode, 'train'][0])
        assert res[mode, 'off'][2] == res[mode, 'train'][2]                  # the flag off: the launches of the training forward
    assert 'level_fwd_slots_kernel' in res['bf16', 'off'][2] and 'level_fwd_slots_infer_kernel' in res['bf16', 'on'][2]
    assert {'A', 'LSE', 'HN16'} <= res['bf16', 'off'][3]
    assert res['f32', 'on'][2] == res['f32', 'train'][2] and not [n for n in res['f32', 'on'][2] if '_infer' in n]
    assert {'A', 'LSE', 'HS', 'HN'} <= res['f32', 'on'][3]


# ------------------------------------------------------------------------------------------------ 8. Predictor
def _reference(pmodel, cnn, designs, dev, frozen):
    """TrainStep(with_optimizer=False).forward over all paths under no_grad, the path validate() takes."""
    from mmft.evaluate import frozen_statistics
    from mmft.train import TrainStep
    ts = TrainStep(pmodel, cnn, designs, dev, with_optimizer=False)
    ids = [np.arange(d.num_paths) for d in designs]
    with torch.no_grad(), frozen_statistics(cnn, frozen):
        hats, _, ends_h = ts.forward(ids)
    torch.cuda.synchronize()
    return hats.clone(), np.asarray(ends_h)


def _models(designs, dev, seed=19):
    from mmft.train import build_models
    pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=seed)
    cnn.set_per_sample_stats(True)
    with torch.no_grad():                                   # running statistics and counters that are not the initial ones
        cnn.train()
        cnn(torch.from_numpy(np.stack([d.image for d in designs])).to(dev))
    return pmodel, cnn


@pytest.mark.parametrize('ndesigns', [2, 1])
def test_predictor_equals_the_validate_forward(dev, ndesigns, monkeypatch):
    from mmft.infer import Predictor
    from mmft.synth import synth_design
    designs = [synth_design(N=2048, L=12, tile=32, seed=700 + i, end_frac=0.25) for i in range(ndesigns)]
    with lib.math_mode('bf16'):
        pmodel, cnn = _models(designs, dev)
        ref = {fz: _reference(pmodel, cnn, designs, dev, fz) for fz in (False, True)}     # (batch statistics first: that call moves the running ones)
        assert not torch.equal(ref[True][0], ref[False][0])
        cnn.set_per_sample_stats(False)
        pmodel.mlp_fuse.eval()                                        # a mix of modes to hand back
        cnn.train()
        flags = [m.training for root in (pmodel, cnn) for m in root.modules()]
        assert True in flags and False in flags
        before = snapshot(pmodel), snapshot(cnn)

        def untouched(what, stats=True):
            assert flags == [m.training for root in (pmodel, cnn) for m in root.modules()], what
            assert not cnn.inc.per_sample_stats, what
            assert all(p.grad is None for root in (pmodel, cnn) for p in root.parameters()), what
            if stats:
                assert_unchanged(pmodel, before[0], what)
                assert_unchanged(cnn, before[1], what)

        p = Predictor(pmodel, cnn, designs, dev)
        untouched('construction')
        assert p.batch.B == ndesigns and np.array_equal(p.endpoints, ref[True][1])
        preds = []
        for k in range(5):                                            # eager, the capturing call, three replays
            y, ends = p.predict()
            preds.append(y.clone())
            assert ends is p.endpoints
            untouched(f'predict() call {k}')
        assert p._replay.graph is not None and p._replay.calls == 5
        for k, y in enumerate(preds):
            assert y.shape == ref[True][0].shape and torch.equal(y, ref[True][0]), k
        eager = Predictor(pmodel, cnn, designs, dev, graphed=False, overlap=False)
        for _ in range(2):
            assert torch.equal(eager.predict()[0], ref[True][0])
        assert eager._replay is None
        untouched('eager predict()')
        # the launches of an eager call (the profiler turns the replay off)
        lib.prof_reset()
        lib.prof_enable(True)
        try:
            y = p.predict()[0].clone()
            torch.cuda.synchronize()
        finally:
            lib.prof_enable(False)
        counts = {r['name']: r['launches'] for r in lib.prof_report()}
        assert torch.equal(y, ref[True][0]) and p._replay.calls == 5
        assert sum(n for k, n in counts.items() if k.startswith('u16_')) == 19, counts
        assert counts.get('level_fwd_slots_infer_kernel', 0) >= 1 and \
            counts['level_fwd_slots_infer_kernel'] + counts.get('level_fwd_bf16_infer_kernel', 0) == 5, counts     # cell levels 2 .. 10
        assert 'level_fwd_slots_kernel' not in counts and 'level_fwd_bf16_kernel' not in counts, counts
        assert not [k for k in counts if k.startswith(('level_bwd', 'u16_bn_', 'u16_conv3x3_kernel'))], counts
        assert not set(p.batch.graph._sweep_bufs) & set(KEPT)
        # an exception inside: modes handed back

        def boom(*a, **k):
            raise RuntimeError('boom')
        monkeypatch.setattr(pmodel, 'fuse_heads', boom)
        for q in (Predictor(pmodel, cnn, designs, dev), eager):       # (a replay runs no python: p itself would not notice)
            with pytest.raises(RuntimeError, match='boom'):
                q.predict()
            untouched('predict() that raised')
        monkeypatch.undo()
        assert torch.equal(eager.predict()[0], ref[True][0]) and torch.equal(p.predict()[0], ref[True][0])
        # batch statistics (the reference's own validate()): eager, moves the running statistics as TrainStep.forward does
        loose = Predictor(pmodel, cnn, designs, dev, frozen_stats=False)
        for _ in range(3):
            assert torch.equal(loose.predict()[0], ref[False][0])
        assert loose._replay is None
        untouched('predict(frozen_stats=False)', stats=False)
        assert int(cnn.state_dict()['inc.double_conv.1.num_batches_tracked']) > int(before[1]['inc.double_conv.1.num_batches_tracked'])


def test_predictor_update_equals_a_predictor_built_on_the_new_data(dev):
    from mmft.infer import Predictor
    from mmft.synth import synth_design
    designs = [synth_design(N=2048, L=12, tile=32, seed=700 + i, end_frac=0.25) for i in range(2)]
    rng = np.random.default_rng(5)
    moved = []
    for d in designs:
        e = copy.copy(d)
        e.cell_feat = (d.cell_feat + rng.standard_normal(d.cell_feat.shape) * 0.1).astype(np.float32)
        e.net_feat = (d.net_feat + rng.standard_normal(d.net_feat.shape) * 0.1).astype(np.float32)
        e.image = rng.random(d.image.shape).astype(np.float32)
        moved.append(e)
    with lib.math_mode('bf16'):
        pmodel, cnn = _models(designs, dev)
        p = Predictor(pmodel, cnn, designs, dev)
        first = [p.predict()[0].clone() for _ in range(3)]
        ptrs = [t.data_ptr() for t in (p.batch.graph.ndata['cell_feat'], p.batch.graph.ndata['net_feat'], p.batch.images, p.h)]
        p.update(0, cell_feat=moved[0].cell_feat, net_feat=torch.from_numpy(moved[0].net_feat), image=moved[0].image)
        half = p.predict()[0].clone()
        p.update(1, cell_feat=moved[1].cell_feat, net_feat=moved[1].net_feat, image=torch.from_numpy(moved[1].image).to(dev))
        full = p.predict()[0].clone()
        again = p.predict()[0].clone()
        assert p._replay.graph is not None and p._replay.calls == 6
        assert ptrs == [t.data_ptr() for t in (p.batch.graph.ndata['cell_feat'], p.batch.graph.ndata['net_feat'], p.batch.images, p.h)]
        fresh = Predictor(pmodel, cnn, moved, dev).predict()[0]
        fresh_half = Predictor(pmodel, cnn, [moved[0], designs[1]], dev, graphed=False).predict()[0]
        assert torch.equal(full, fresh) and torch.equal(again, fresh) and torch.equal(half, fresh_half)
        assert not torch.equal(first[0], fresh) and all(torch.equal(first[0], y) for y in first)
        with pytest.raises(ValueError):
            p.update(0, cell_feat=moved[0].cell_feat[:-1])
        with pytest.raises(TypeError):
            p.update(1, image=moved[1].image.astype(np.float64))
        with pytest.raises(IndexError):
            p.update(2, image=moved[1].image)
        assert torch.equal(p.predict()[0], fresh)


def test_predictor_cone_on_a_few_endpoints(dev):
    from mmft.infer import Predictor
    from mmft.synth import synth_design
    designs = [synth_design(N=6000, L=12, tile=32, seed=120 + i, end_frac=0.2) for i in range(2)]
    ids = [np.array([3, 11, 40]), np.array([0, 7])]
    with lib.math_mode('bf16'):
        pmodel, cnn = _models(designs, dev)
        full = Predictor(pmodel, cnn, designs, dev, path_ids_per_design=ids, graphed=False)
        y = full.predict()[0].clone()
        cone = Predictor(pmodel, cnn, designs, dev, path_ids_per_design=ids, cone=True)
        ys = [cone.predict()[0].clone() for _ in range(3)]
    assert y.shape[0] == 5 and np.array_equal(full.endpoints, cone.endpoints)
    assert all(torch.equal(y, z) for z in ys)
    assert cone.batch.graph._sweep.active is not None and bool((cone.h == 0).all(dim=1).any())


# ------------------------------------------------------------------------------------------------ 9. config B, full size
def test_predictor_at_full_size_config_b(dev):
    """The configuration bench.py times (8 x 65 536 nodes, 64 levels, 256 x 256 tiles, 1350 endpoints per design)."""
    from mmft.infer import Predictor
    from mmft.synth import synth_design
    from mmft.train import build_models
    designs = [synth_design(N=65536, L=64, tile=256, seed=9294 + i) for i in range(8)]
    rng = np.random.default_rng(6)
    ids = [rng.permutation(d.num_paths)[:1350] for d in designs]
    with lib.math_mode('bf16'):
        pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=9294)
        p = Predictor(pmodel, cnn, designs, dev, path_ids_per_design=ids)
        lib.prof_reset()
        lib.prof_enable(True)
        try:
            eager = p.predict()[0].clone()                       # the profiler is on: eager, and not counted as the replay's first call
            torch.cuda.synchronize()
        finally:
            lib.prof_enable(False)
        counts = {r['name']: r['launches'] for r in lib.prof_report()}
        ys = [p.predict()[0].clone() for _ in range(4)]
        torch.cuda.synchronize()
    assert p._replay.graph is not None and p._replay.calls == 4
    assert counts.get('level_fwd_slots_infer_kernel', 0) >= 1 and \
        counts['level_fwd_slots_infer_kernel'] + counts.get('level_fwd_bf16_infer_kernel', 0) == 31, counts      # cell levels 2 .. 62
    assert 'level_fwd_slots_kernel' not in counts and 'level_fwd_bf16_kernel' not in counts, counts
    assert sum(n for k, n in counts.items() if k.startswith('u16_')) == 19, counts
    assert eager.shape == (8 * 1350,) and bool(torch.isfinite(eager).all()) and float(eager.std()) > 0
    for y in ys:
        assert torch.equal(y, eager)
    g = p.batch.graph
    packs = 4 * 256 * 128 * 2
    print(f'\nconfig B: {_buf_bytes(g) / 1e6:.1f} MB in _sweep_bufs, N = {p.batch.N}, keys {sorted(g._sweep_bufs)}')
    assert not set(g._sweep_bufs) & set(KEPT)
    assert _buf_bytes(g) < 2 * p.batch.N * 128 * 4 + packs
