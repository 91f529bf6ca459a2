"""Incremental re-prediction on the GPU (include/mmft_incr.h, mmft.infer.Predictor(incremental=True)).  Every comparison is bitwise:
the cone against a numpy closure, the row writer against numpy, the masked feature MLP against the unmasked entry point, and
the Predictor - predictions AND the whole of h - against a Predictor built from scratch on the edited designs."""
import copy

import numpy as np
import pytest
import torch

import incr_cases as C
from mmft import lib, ops, prep

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the cone
@pytest.mark.parametrize('fanin', ['regular', 'irregular'])
def test_fanout_cone_mask_equals_the_numpy_closure(dev, fanin):
    from mmft import sweep as S
    from mmft.infer import design_permutations
    from mmft.train import DesignBatch
    b = DesignBatch(C.cone_designs(fanin), dev)
    g, N = b.graph, b.N
    csrs = [g.csr('in', 'net'), g.csr('in', 'cell')]
    edges = [C.csr_edges(ip.cpu().numpy(), ix.cpu().numpy()) for ip, ix in csrs]
    specs = S._level_specs(g, b.level_nodes)
    perm = design_permutations(b.old_of_new, b.node_off)
    rng = np.random.default_rng(2)
    cases = {'none': [], 'level0': [b.level_nodes[0][5]], 'levels_1_6_11': [b.level_nodes[l][3] for l in (1, 6, 11)],
             'design1': perm[1][rng.permutation(perm[1].size)[:50]].tolist(), 'all': list(range(N))}
    ends = torch.from_numpy(b.path2endpoint[[0, 1, 2, b.path_off[1], b.path_off[1] + 1]].astype(np.int32)).to(dev)
    within = prep.cone_mask(csrs, specs, ends)
    within_h = within.cpu().numpy()
    assert np.array_equal(within_h, C.fanin_cone(N, edges, ends.cpu().numpy())) and 0 < within_h.sum() < N
    out = torch.full((N,), 7, dtype=torch.uint8, device=dev)
    for name, ids in cases.items():
        seed_h = np.zeros(N, dtype=np.uint8)
        seed_h[np.asarray(ids, dtype=np.int64)] = 1
        seed = torch.from_numpy(seed_h).to(dev)
        ref = C.fanout_cone(N, edges, seed_h)
        got = prep.fanout_cone_mask(csrs, specs, seed, out=out)
        assert got is out and np.array_equal(got.cpu().numpy(), ref), name
        assert np.array_equal(seed.cpu().numpy(), seed_h), name                      # the seeds are read, not spent
        if name == 'none':
            assert not ref.any()
        elif name == 'all':
            assert ref.all()
        else:
            assert ref[seed_h != 0].all() and seed_h.sum() < ref.sum() < N, name
        if name == 'design1':
            assert not ref[perm[0]].any() and ref[perm[1]].any()
        got_w = prep.fanout_cone_mask(csrs, specs, seed, within=within).cpu().numpy()
        assert np.array_equal(got_w, ref & within_h) and np.array_equal(got_w, C.fanout_cone(N, edges, seed_h, within_h)), name
    with pytest.raises(ValueError):
        prep.fanout_cone_mask(csrs, specs, out, out=out)
    with pytest.raises(ValueError):
        prep.fanout_cone_mask(csrs, specs, out[:-1])


# ------------------------------------------------------------------------------------------------ 2. the row writer
@pytest.mark.parametrize('form', ['idx', 'row0'])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000])
@pytest.mark.parametrize('width', [36, 2])
def test_update_rows_diff_writes_the_rows_and_flags_the_ones_that_changed(dev, width, n, form):
    rng = np.random.default_rng(1000 * width + n)
    N, row0 = 1500, 211
    table = rng.standard_normal((N, width)).astype(np.float32)
    target = rng.permutation(N)[:n] if form == 'idx' else np.arange(row0, row0 + n)
    idx = torch.from_numpy(target.astype(np.int32)).to(dev) if form == 'idx' else None
    pre = (rng.random(N) < 0.05).astype(np.uint8)                                    # flags set beforehand survive
    pre[target[0]] = 0
    for k, kind in enumerate(C.DIFF_KINDS):
        old, new, changed = C.diff_case(kind, table[target], seed=k)
        start = table.copy()
        start[target] = old
        want = start.copy()
        want[target] = new
        flags = pre.copy()
        flags[target] |= changed
        dst, seed = torch.from_numpy(start).to(dev), torch.from_numpy(pre).to(dev)
        ops.update_rows_diff(dst, torch.from_numpy(new).to(dev), seed, idx=idx, row0=row0)
        assert np.array_equal(dst.cpu().numpy().view(np.uint32), want.view(np.uint32)), kind
        assert np.array_equal(seed.cpu().numpy(), flags), kind
        if kind in ('same', 'same_nan'):
            assert np.array_equal(dst.cpu().numpy().view(np.uint32), start.view(np.uint32)) and np.array_equal(flags, pre)
    # every row changed, a source with a wider pitch
    wide = torch.from_numpy(rng.standard_normal((n, width + 3)).astype(np.float32)).to(dev)
    dst, seed = torch.from_numpy(table).to(dev), torch.zeros(N, dtype=torch.uint8, device=dev)
    ops.update_rows_diff(dst, wide[:, :width], seed, idx=idx, row0=row0)
    want = table.copy()
    want[target] = wide[:, :width].cpu().numpy()
    flags = np.zeros(N, dtype=np.uint8)
    flags[target] = 1
    assert np.array_equal(dst.cpu().numpy(), want) and np.array_equal(seed.cpu().numpy(), flags)


# ------------------------------------------------------------------------------------------------ 3. the masked feature MLP
def _mlp(fin, dev, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, generator=g) * 0.3).to(dev)
    return mk(256, fin), mk(256), mk(128, 256), mk(128)


def _sentinel(N, dev):
    return torch.full((N, 128), int(C.SENTINEL), dtype=torch.int32, device=dev).view(torch.float32)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 200])
@pytest.mark.parametrize('row0', [0, 192])
@pytest.mark.parametrize('relu_out', [0, 1])
@pytest.mark.parametrize('fin', [36, 2])
def test_masked_feature_mlp_writes_flagged_rows_only_and_bitwise_the_unmasked_values(dev, fin, relu_out, row0, n):
    N = 400
    w1, b1, w2, b2 = _mlp(fin, dev, 5 + fin)
    x = torch.randn(N, fin, generator=torch.Generator().manual_seed(n + row0)).to(dev)
    sent = _sentinel(N, dev)
    with lib.math_mode('bf16'):
        ref = ops.mlp2_feat_fwd_bf16(x, (row0, n), w1, b1, w2, b2, sent.clone(), relu_out=bool(relu_out))
        inside = torch.zeros(N, dtype=torch.bool, device=dev)
        inside[row0:row0 + n] = True
        assert torch.equal(_bits(ref[~inside]), _bits(sent[~inside])) and not bool((_bits(ref[inside]) == int(C.SENTINEL)).any())
        for name, m in C.mlp_masks(n).items():
            active = torch.ones(N, dtype=torch.uint8, device=dev)                    # flags outside the launch's rows: ignored
            active[row0:row0 + n] = torch.from_numpy(m).to(dev)
            out = ops.mlp2_feat_fwd_bf16(x, (row0, n), w1, b1, w2, b2, sent.clone(), relu_out=bool(relu_out), active=active)
            on = inside & (active != 0)
            assert int(on.sum()) == int(m.sum()), name
            assert torch.equal(_bits(out[on]), _bits(ref[on])), name
            assert torch.equal(_bits(out[~on]), _bits(sent[~on])), name
            if name == 'all':
                assert torch.equal(_bits(out), _bits(ref))


def test_masked_feature_mlp_when_a_workgroup_walks_several_tiles(dev):
    """More tiles than the grid's 768 workgroups: a workgroup strides over tiles, skips the clear ones and prefetches the next
    set one.  Sparse flags (most tiles clear), a dense stretch, and whole workgroups without any tile."""
    n, row0, fin = 2 * 768 * 64 + 65, 64, 36
    N = row0 + n + 10
    w1, b1, w2, b2 = _mlp(fin, dev, 9)
    x = torch.randn(N, fin, generator=torch.Generator().manual_seed(3)).to(dev)
    rng = np.random.default_rng(8)
    m = np.zeros(n, dtype=np.uint8)
    m[rng.permutation(n)[:300]] = 1
    m[768 * 64 + 10:768 * 64 + 700] = 1
    m[-1] = 1
    assert (m.reshape(-1)[:n - 65].reshape(-1, 64).sum(axis=1) == 0).sum() > 1000
    active = torch.zeros(N, dtype=torch.uint8, device=dev)
    active[row0:row0 + n] = torch.from_numpy(m).to(dev)
    sent = _sentinel(N, dev)
    with lib.math_mode('bf16'):
        ref = ops.mlp2_feat_fwd_bf16(x, (row0, n), w1, b1, w2, b2, sent.clone())
        out = ops.mlp2_feat_fwd_bf16(x, (row0, n), w1, b1, w2, b2, sent.clone(), active=active)
    on = active != 0
    assert torch.equal(_bits(out[on]), _bits(ref[on])) and torch.equal(_bits(out[~on]), _bits(sent[~on]))


# ------------------------------------------------------------------------------------------------ 4. the Predictor
def _models(designs, dev, seed=19):
    from test_infer_gpu import _models as live
    return live(designs, dev, seed)


def _fresh(pmodel, cnn, designs, dev, **kw):
    """(predictions, h) of a Predictor built from scratch on these designs: one eager full sweep."""
    from mmft.infer import Predictor
    p = Predictor(pmodel, cnn, designs, dev, graphed=False, **kw)
    y = p.predict()[0].clone()
    return y, p.h.clone()


def _check(p, designs, pmodel, cnn, dev, dirty, what, **kw):
    """predict(): predictions and all of h equal a fresh Predictor on `designs`; dirty: per design its expected flags in the
    design's own numbering (None: all zero)."""
    y = p.predict()[0].clone()
    yf, hf = _fresh(pmodel, cnn, designs, dev, **kw)
    assert torch.equal(y, yf), what
    assert torch.equal(p.h, hf), what
    for i, want in enumerate(dirty):
        got = p.dirty_mask(i)
        assert got.dtype == np.uint8 and got.shape == (designs[i].N,)
        assert np.array_equal(got, np.zeros_like(got) if want is None else want), (what, i)
    return y


def _edit_sequence(dev, designs, levels=(1, 6, 11), small=True, **kw):
    """Three calls, edit A (sparse), nothing, edit B (the other design, both tables), revert A: after every step the
    incremental Predictor equals a fresh one, replayed."""
    from mmft.infer import Predictor
    d0, d1 = designs
    with lib.math_mode('bf16'):
        pmodel, cnn = _models(designs, dev)
        plain = Predictor(pmodel, cnn, designs, dev, **kw)
        p = Predictor(pmodel, cnn, designs, dev, incremental=True, **kw)
        for k in range(3):                                                         # eager, capturing, replay
            a, y = plain.predict()[0].clone(), p.predict()[0].clone()
            assert torch.equal(a, y) and torch.equal(p.h, plain.h), k
            assert p.incremental_active and bool(p.dirty_mask().all()) == (k == 0) and bool(p.dirty_mask().any()) == (k == 0), k
        assert p._replay.graph is not None and p._replay.calls == 3
        assert all(any(t is k for k in p._replay.keep) for t in (p.seed, p.dirty))
        seeds = C.pick_seeds(d0, d0.path2endpoint, levels)
        cone = C.design_cone(d0, seeds)
        assert 0 < cone.sum() <= (d0.N // 4 if small else d0.N - 1)                # the numpy closure: a real cone, and a small one
        e0 = C.edited(d0, seeds, seed=1)
        p.update(0, cell_feat=e0.cell_feat[seeds], rows=seeds)
        seed_sparse = p.seed.cpu().numpy().copy()
        assert seed_sparse.sum() == seeds.size
        y1 = _check(p, [e0, d1], pmodel, cnn, dev, [cone, None], 'edit A')
        assert not torch.equal(y1, y) and not p.seed.any()
        y2 = _check(p, [e0, d1], pmodel, cnn, dev, [None, None], 'no update')
        assert torch.equal(y2, y1) and not p.dirty_mask().any()
        rows_b = np.concatenate([d1.levels[l][2:4] for l in (0, d1.L // 2, d1.L // 2 + 1)]).astype(np.int64)
        e1 = C.edited(d1, rows_b, seed=2, net=True)
        p.update(1, cell_feat=torch.from_numpy(e1.cell_feat[rows_b]), net_feat=e1.net_feat[rows_b], rows=torch.from_numpy(rows_b))
        _check(p, [e0, e1], pmodel, cnn, dev, [None, C.design_cone(d1, rows_b)], 'edit B')
        p.update(0, cell_feat=d0.cell_feat[seeds], rows=seeds)
        y4 = _check(p, [d0, e1], pmodel, cnn, dev, [cone, None], 'revert A')
        assert p._replay.calls == 7 and p.incremental_active
    return p, pmodel, cnn, (e0, e1, seeds, cone, seed_sparse, y4)


def test_predictor_incremental_equals_a_fresh_predictor_after_every_edit(dev):
    from mmft.infer import Predictor
    designs = C.predictor_designs()
    p, pmodel, cnn, (e0, e1, seeds, cone, seed_sparse, y4) = _edit_sequence(dev, designs)
    d0 = designs[0]
    with lib.math_mode('bf16'):
        # the whole edited table without rows=: the same seeds, the same dirty rows
        q = Predictor(pmodel, cnn, designs, dev, incremental=True)
        for _ in range(2):
            q.predict()
        q.update(0, cell_feat=e0.cell_feat)
        assert np.array_equal(q.seed.cpu().numpy(), seed_sparse)
        _check(q, [e0, designs[1]], pmodel, cnn, dev, [cone, None], 'whole table')
        # an image alone marks nothing
        img = np.random.default_rng(4).random(d0.image.shape).astype(np.float32)
        d0i = copy.copy(d0)
        d0i.image = img
        p.update(0, image=img)
        assert not p.seed.any()
        # (with these models the U-Net's output is zero on every cell in front of its last ReLU - test_place_gpu._live_models -
        # so the new image need not move a prediction: what is checked is that it is taken, and that nothing is swept for it)
        _check(p, [d0i, e1], pmodel, cnn, dev, [None, None], 'image only')
        assert torch.equal(p.batch.images[0], torch.from_numpy(img).to(dev))
        # rows= without incremental: a plain sparse copy
        plain = Predictor(pmodel, cnn, designs, dev)
        plain.predict()
        plain.update(0, cell_feat=e0.cell_feat[seeds], rows=seeds)
        assert torch.equal(plain.predict()[0], _fresh(pmodel, cnn, [e0, designs[1]], dev)[0])
        with pytest.raises(RuntimeError):
            plain.dirty_mask()
        # refused before anything is written
        before = p.batch.graph.ndata['cell_feat'].clone()
        for kw, exc in ((dict(cell_feat=e0.cell_feat[seeds], rows=np.array([1, 1, 2])), ValueError),
                        (dict(cell_feat=e0.cell_feat[seeds], rows=np.array([1, 2, d0.N])), IndexError),
                        (dict(cell_feat=e0.cell_feat[seeds], rows=seeds.astype(np.int32)), TypeError),
                        (dict(cell_feat=e0.cell_feat[seeds[:2]], rows=seeds), ValueError)):
            with pytest.raises(exc):
                p.update(0, **kw)
        assert torch.equal(p.batch.graph.ndata['cell_feat'], before) and not p.seed.any()


def test_predictor_sweeps_everything_when_the_model_changed_or_it_was_told_to(dev):
    from mmft.infer import Predictor
    designs = C.predictor_designs()
    with lib.math_mode('bf16'):
        pmodel, cnn = _models(designs, dev)
        p = Predictor(pmodel, cnn, designs, dev, incremental=True)
        ys = [p.predict()[0].clone() for _ in range(3)]
        assert not p.dirty_mask().any()
        with torch.no_grad():
            pmodel.gnn.fc_cell_neigh.layers[0].weight.mul_(1.01)
        y = _check(p, designs, pmodel, cnn, dev, [np.ones(d.N, dtype=np.uint8) for d in designs], 'weight scaled in place')
        assert not torch.equal(y, ys[0]) and p.dirty_mask().all()
        _check(p, designs, pmodel, cnn, dev, [None, None], 'after it')
        h = p.h.clone()
        p.h.zero_()                                                                # h is no longer what the Predictor left
        p.invalidate()
        _check(p, designs, pmodel, cnn, dev, [np.ones(d.N, dtype=np.uint8) for d in designs], 'invalidate()')
        assert torch.equal(p.h, h) and p._replay.graph is not None


def test_predictor_sweeps_everything_after_the_projects_own_optimizer_stepped(dev, monkeypatch):
    """FlatAdam rewrites the parameters through raw pointers: no address, module mode or autograd version counter moves, only
    gradsink.param_epoch() - eagerly (TrainStep.step) and when the step is a replayed graph (GraphedTrainStep.step)."""
    from mmft.infer import Predictor
    from mmft.train import TrainStep, GraphedTrainStep
    designs = C.predictor_designs()
    ids = [np.arange(0, d.num_paths, 3) for d in designs]
    everything = [np.ones(d.N, dtype=np.uint8) for d in designs]
    with lib.math_mode('bf16'):
        pmodel, cnn = _models(designs, dev)
        ts = TrainStep(pmodel, cnn, designs, dev)                                  # (the optimizer re-homes p.data here)
        p = Predictor(pmodel, cnn, designs, dev, incremental=True)
        ys = [p.predict()[0].clone() for _ in range(3)]
        assert not p.dirty_mask().any()
        params = list(pmodel.gnn.parameters())
        for stepper in (ts, None):
            if stepper is None:
                stepper = GraphedTrainStep(ts, ids)                                # (its warm-up steps move the weights as well)
                _check(p, designs, pmodel, cnn, dev, everything, 'GraphedTrainStep built')
            before = [(t.data_ptr(), t._version) for t in params], p.h.clone()
            stepper.step(ids)
            torch.cuda.synchronize()
            assert before[0] == [(t.data_ptr(), t._version) for t in params]       # nothing torch can see has moved
            y = _check(p, designs, pmodel, cnn, dev, everything, type(stepper).__name__)
            assert not torch.equal(y, ys[0]) and not torch.equal(p.h, before[1])
            _check(p, designs, pmodel, cnn, dev, [None, None], 'after it')
        # under an outer capture the host's decision would be baked into the caller's graph: refused
        monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
        with pytest.raises(RuntimeError, match='outer stream capture'):
            p.predict()
        monkeypatch.undo()
        _check(p, designs, pmodel, cnn, dev, [None, None], 'after the refused call')  # (refused before anything was launched)


def test_predictor_in_fp32_mode_falls_back_to_the_full_sweep(dev):
    from mmft.infer import Predictor
    designs = C.predictor_designs()
    seeds = C.pick_seeds(designs[0], designs[0].path2endpoint)
    e0 = C.edited(designs[0], seeds, seed=1)
    with lib.math_mode('f32'):
        pmodel, cnn = _models(designs, dev)
        plain, p = Predictor(pmodel, cnn, designs, dev), Predictor(pmodel, cnn, designs, dev, incremental=True)
        for _ in range(2):
            assert torch.equal(plain.predict()[0], p.predict()[0]) and torch.equal(plain.h, p.h)
            assert not p.incremental_active and p.dirty_mask().all()
        p.update(0, cell_feat=e0.cell_feat[seeds], rows=seeds)
        y, h = _fresh(pmodel, cnn, [e0, designs[1]], dev)
        assert torch.equal(p.predict()[0], y) and torch.equal(p.h, h) and not p.incremental_active
    with lib.math_mode('bf16'):                                                    # the mode changed: a full masked sweep
        y, h = _fresh(pmodel, cnn, [e0, designs[1]], dev)
        assert torch.equal(p.predict()[0], y) and torch.equal(p.h, h) and p.incremental_active and p.dirty_mask().all()
        assert torch.equal(p.predict()[0], y) and not p.dirty_mask().any()


# ------------------------------------------------------------------------------------------------ 5. other shapes
@pytest.mark.parametrize('shape, fanin, levels', [((40000, 8), 'regular', (1, 4, 7)), ((6000, 12), 'irregular', (1, 6, 11))])
def test_the_edit_sequence_on_other_shapes(dev, shape, fanin, levels):
    """(40000, 8): levels of 10 000 rows, 32-row workgroups (RB = 2).  Irregular fan-in: the cell levels take the two-launch
    path (heavy rows), whose gather and MLP both read `active`."""
    designs = C.predictor_designs(shape, fanin)
    p, *_ = _edit_sequence(dev, designs, levels, small=False)
    fold = p.batch.graph._sweep.fold
    assert (fold[2]['heavy_in'] is not None) == (fanin == 'irregular')


# ------------------------------------------------------------------------------------------------ 6. with the fan-in cone
def test_predictor_incremental_inside_the_fan_in_cone(dev):
    from mmft.infer import Predictor, design_permutations
    designs = C.cone_designs('regular')
    ids = [np.array([3, 11, 40]), np.array([0, 7])]
    d0 = designs[0]
    seeds = C.pick_seeds(d0, d0.path2endpoint[ids[0]])
    e0 = C.edited(d0, seeds, seed=1)
    with lib.math_mode('bf16'):
        pmodel, cnn = _models(designs, dev)
        plain = Predictor(pmodel, cnn, designs, dev, path_ids_per_design=ids, cone=True)
        p = Predictor(pmodel, cnn, designs, dev, path_ids_per_design=ids, cone=True, incremental=True)
        for k in range(3):
            assert torch.equal(plain.predict()[0], p.predict()[0]), k
        within = p.batch.graph._cone_mask.cpu().numpy()
        assert 0 < within.sum() < p.batch.N and not p.dirty_mask().any()
        p.update(0, cell_feat=e0.cell_feat[seeds], rows=seeds)
        y = p.predict()[0].clone()
        fresh = Predictor(pmodel, cnn, [e0, designs[1]], dev, path_ids_per_design=ids, cone=True, graphed=False).predict()[0]
        assert y.shape[0] == 5 and torch.equal(y, fresh)
        dirty = p.dirty_mask()
        assert (dirty <= within).all()
        perm0 = design_permutations(p.batch.old_of_new, p.batch.node_off)[0]
        assert np.array_equal(p.dirty_mask(0), C.design_cone(d0, seeds) & within[perm0]) and not p.dirty_mask(1).any()
        p.invalidate()
        assert torch.equal(p.predict()[0], fresh) and np.array_equal(p.dirty_mask(), within)


def test_predictor_incremental_with_a_moving_placement_and_a_report(dev):
    """placement=True and report= next to incremental=True: one pin move and one edited row in the same call."""
    from mmft.infer import Predictor
    from test_place_gpu import _small_designs, _live_models, _moved_copy
    import place_cases as PC
    designs = list(_small_designs())
    d0 = designs[0]
    rows = np.array([int(d0.levels[6][0])], dtype=np.int64)
    xy = PC.move(d0, seed=60, frac=0.02)
    e0 = C.edited(_moved_copy(d0, xy), rows, seed=5)
    spec = dict(k=4, hist=None)
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        p = Predictor(pmodel, cnn, designs, dev, placement=True, report=spec, incremental=True)
        for _ in range(3):
            p.predict()
        p.update(0, cell_feat=e0.cell_feat[rows], rows=rows, pin_x=xy[0], pin_y=xy[1])
        y = p.predict()[0].clone()
        fresh = Predictor(pmodel, cnn, [e0, designs[1]], dev, placement=True, report=spec, graphed=False)
        assert torch.equal(y, fresh.predict()[0]) and torch.equal(p.h, fresh.h)
        assert np.array_equal(p.dirty_mask(0), C.design_cone(d0, rows)) and not p.dirty_mask(1).any()
        assert p.report() == fresh.report()
