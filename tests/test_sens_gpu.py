"""mmft.sensitivity on the GPU: the input-gradient kernel of the feature MLPs (mmft_mlp2_feat_dx_bf16) against fp64 math that
rounds where it rounds, and Sensitivity.run() end to end against the reference gradient of tests/sens_oracle.py.

End to end, bf16 mode: the three distances of tests/test_bf16_oracle_gpu.py, all to the fp64 ROUNDING oracle - e_hip (the
HIP result), e_32 (the rounding oracle in fp32), e_plain (the plain fp64 oracle) - every oracle run on the HIP run's own
feature map.  Rows d J / d cell_feat and d J / d net_feat in max-norm rel_err:  e_hip <= max(1.5e-3, 3 e_32),  e_hip <= 5e-3
(that file's gradient ceiling),  teeth e_plain > 10 x bound.  The floor is that file's floor for a per-row quantity that one
rounding-boundary flip moves: a feature-gradient row is not summed over rows the way a weight gradient is.  Predictions: that
file's predictions row (floor 1.5e-3, ceiling 2e-3).  fp32 mode: both gradients within 1e-4 of the plain fp64 reference."""
import copy

import numpy as np
import pytest
import torch

from conftest import rel_err
from mmft import lib, ops
from sens_oracle import batch_rows, level_parity_rows, oracle_sensitivity
from test_bf16_gpu import TOL, bf, rnd

pytestmark = pytest.mark.gpu
SEED = 9294
FLOOR, CEILING, PRED_CEILING, K, TEETH = 1.5e-3, 5e-3, 2e-3, 3.0, 10.0


# ------------------------------------------------------------------------------------------------ the kernel
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('fin,n,row0', [(36, 1, 0), (36, 63, 7), (36, 64, 0), (36, 65, 128), (2, 129, 3), (5, 33, 3),
                                        (36, 70000, 128)])
@pytest.mark.parametrize('representable', [True, False])
def test_feature_mlp_input_gradient_without_hidden_tensor(dev, fin, n, row0, representable):
    """mmft_mlp2_feat_dx_bf16 against fp64 math that rounds where the kernel rounds - operands and the hidden gradient go
    through bf16, everything accumulates in fp32 - with the comparison and the bars of test_feature_mlp_without_hidden_tensor
    (tests/test_bf16_gpu.py), for the reason written there.  Every pitch is wider than its row; the output is
    sentinel-filled: rows outside the range and columns beyond fin keep the sentinel's bits; two launches are bitwise equal.
    70 000 rows are more tiles (1094) than workgroups (256)."""
    N = row0 + n + 5
    x = rnd(N, fin, seed=1, representable=representable)
    w1 = rnd(256, fin, seed=2, representable=representable) * 0.25
    b1 = rnd(256, seed=3, representable=representable) * 0.25
    w2 = rnd(128, 256, seed=4, representable=representable) * 0.125
    g = rnd(N, 128, seed=6, representable=representable)
    if representable:
        w1, b1, w2 = bf(w1), bf(b1), bf(w2)
    sl = slice(row0, row0 + n)
    xb, w1b, w2b, gb = bf(x).double(), bf(w1).double(), bf(w2).double(), bf(g).double()
    pre = xb[sl] @ w1b.T + b1.double()
    dH = bf(((gb[sl] @ w2b) * (pre > 0)).float()).double()          # the hidden gradient is an MFMA operand: bf16
    ref = dH @ w1b
    with lib.math_mode('bf16'):
        xw = torch.full((N, fin + 3), 3.0, device=dev)
        xw[:, :fin] = x.to(dev)
        gw = torch.full((N, 132), 5.0, device=dev)
        gw[:, :128] = g.to(dev)
        outs = []
        for _ in range(2):
            out = torch.full((N, fin + 5), 7.0, device=dev)
            got = ops.mlp2_feat_dx_bf16(gw[:, :128], xw[:, :fin], (row0, n), w1.to(dev), b1.to(dev), w2.to(dev), dx=out)
            assert got is out and gw.stride(0) == 132 and xw.stride(0) == fin + 3 and out.stride(0) == fin + 5
            outs.append(out)
        torch.cuda.synchronize()
    out = outs[0]
    tol = 1e-3 if representable else TOL
    e = rel_err(out[sl, :fin], ref)
    print(f'\nfin {fin} n {n} row0 {row0} representable {representable}: rel_err {e:.2e} (bar {tol:.0e})')
    assert e < tol
    sentinel = _bits(torch.full((1,), 7.0))[0].item()
    keep = torch.ones((N, fin + 5), dtype=torch.bool)
    keep[sl, :fin] = False
    assert bool((_bits(out).cpu()[keep] == sentinel).all())         # rows outside the range, columns beyond fin
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    # without dx: zeros [N, fin], the range's rows filled
    with lib.math_mode('bf16'):
        z = ops.mlp2_feat_dx_bf16(gw[:, :128], xw[:, :fin], (row0, n), w1.to(dev), b1.to(dev), w2.to(dev))
    assert tuple(z.shape) == (N, fin) and torch.equal(_bits(z[sl]), _bits(out[sl, :fin]))
    assert float(z[:row0].abs().max()) == 0.0 if row0 else True
    assert float(z[row0 + n:].abs().max()) == 0.0


def test_the_wrapper_refuses_what_the_kernel_does_not_take(dev):
    g, x = torch.zeros(10, 128, device=dev), torch.zeros(10, 36, device=dev)
    w1, b1, w2 = torch.zeros(256, 36, device=dev), torch.zeros(256, device=dev), torch.zeros(128, 256, device=dev)
    with pytest.raises(ValueError, match='range'):
        ops.mlp2_feat_dx_bf16(g, x, torch.arange(4, dtype=torch.int32, device=dev), w1, b1, w2)
    with pytest.raises(ValueError, match='outside'):
        ops.mlp2_feat_dx_bf16(g, x, (8, 3), w1, b1, w2)
    with pytest.raises(ValueError, match='256 -> 128'):
        ops.mlp2_feat_dx_bf16(g, x, (0, 3), w1[:, :35].contiguous(), b1, w2)
    with pytest.raises(ValueError, match='dx must be'):
        ops.mlp2_feat_dx_bf16(g, x, (0, 3), w1, b1, w2, dx=torch.zeros(10, 35, device=dev))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.mlp2_feat_dx_bf16(g.cpu(), x.cpu(), (0, 3), w1.cpu(), b1.cpu(), w2.cpu())
    assert float(ops.mlp2_feat_dx_bf16(g, x, (4, 0), w1, b1, w2).abs().max()) == 0.0          # n == 0: nothing launched


# ------------------------------------------------------------------------------------------------ end to end
def _design(fanin='regular', N=2048, L=16, seed=SEED):
    from mmft.synth import synth_design
    return synth_design(N=N, L=L, tile=32, seed=seed, fanin=fanin)


def _models(d, dev):
    from mmft.train import build_models
    pmodel, cnn = build_models(map_size=d.map_size, device=dev, seed=SEED)
    state = {k: v.detach().cpu().clone() for k, v in pmodel.state_dict().items()}
    return pmodel, cnn, state


def _weights(T, seed=12):
    return torch.randn(T, generator=torch.Generator().manual_seed(seed))


def _host(grads):
    return [{k: v.detach().double().cpu() for k, v in g.items()} for g in grads]


def _oracles(d, ids, state, fm, w):
    """(fp64 rounding oracle, the same in fp32, plain fp64) on the HIP run's own feature map."""
    return tuple(oracle_sensitivity(d, ids, state, fm, w, dtype=dt, rounding=rd)
                 for rd, dt in (('bf16', torch.float64), ('bf16', torch.float32), (None, torch.float64)))


def _oracle_rows(title, hip, o64, o32, op, teeth=True):
    """The rows of the module docstring for one design; hip = dict(pred, cell, net).  Prints every row before it judges."""
    bad = []
    print(f'\n== {title}: quantity  e_hip  e_32  e_plain  bound')
    for key, ceiling, has_teeth in (('pred', PRED_CEILING, False), ('cell', CEILING, teeth), ('net', CEILING, teeth)):
        e_hip, e_32, e_plain = (rel_err(r[key], o64[key]) for r in (hip, o32, op))
        bound = max(FLOOR, K * e_32)
        print(f'   {key:5s} {e_hip:.2e} {e_32:.2e} {e_plain:.2e} {bound:.2e}')
        if e_hip > bound:
            bad.append(f'{key}: e_hip {e_hip:.3e} > bound {bound:.3e}')
        if e_hip > ceiling:
            bad.append(f'{key}: e_hip {e_hip:.3e} > ceiling {ceiling:.3e}')
        if has_teeth and not e_plain > TEETH * bound:
            bad.append(f'{key}: no teeth, e_plain {e_plain:.3e} <= {TEETH} x bound {bound:.3e}')
    assert not bad, bad


def _zero_rows_exact(d, g):
    even, odd = level_parity_rows(d)
    assert float(g['cell_feat'][torch.from_numpy(odd).to(g['cell_feat'].device)].abs().max()) == 0.0
    assert float(g['net_feat'][torch.from_numpy(even).to(g['net_feat'].device)].abs().max()) == 0.0
    assert float(g['cell_feat'].abs().max()) > 0.0 and float(g['net_feat'].abs().max()) > 0.0


@pytest.fixture(scope='module')
def runs(dev):
    """Per fan-in kind: the design, the model's host weights, the weights w, and Sensitivity.run() in bf16 mode on the fused
    route and on the generic-layer route, in fp32 mode, and the three oracle runs on the bf16 run's feature map - made once."""
    from mmft.sensitivity import Sensitivity
    cache = {}

    def get(fanin):
        if fanin in cache:
            return cache[fanin]
        d = _design(fanin)
        ids = list(range(d.num_paths))
        w = _weights(d.num_paths)
        pmodel, cnn, state = _models(d, dev)
        c = dict(d=d, ids=ids, w=w, state=state)
        with lib.math_mode('bf16'):
            s = Sensitivity(pmodel, cnn, [d], dev)
            pred, ends, grads = s.run(weights=w)
            c['fused'] = dict(pred=pred.double().cpu(), cell=_host(grads)[0]['cell_feat'], net=_host(grads)[0]['net_feat'],
                              hop=s.last_hop, ends=list(ends), grads=grads)
            c['fm'] = s.feat_map.detach().double().cpu()
            s.force_layers = True
            pred, ends, grads = s.run(weights=w.to(dev))
            c['layers'] = dict(pred=pred.double().cpu(), cell=_host(grads)[0]['cell_feat'], net=_host(grads)[0]['net_feat'],
                               hop=s.last_hop)
        s32 = Sensitivity(pmodel, cnn, [d], dev)
        pred, ends, grads = s32.run(weights=w)
        c['f32'] = dict(pred=pred.double().cpu(), cell=_host(grads)[0]['cell_feat'], net=_host(grads)[0]['net_feat'], hop=s32.last_hop,
                        fm=s32.feat_map.detach().double().cpu())
        torch.cuda.synchronize()
        c['oracles'] = _oracles(d, ids, state, c['fm'], w)
        cache[fanin] = c
        return c
    return get


@pytest.mark.parametrize('fanin', ['regular', 'irregular'])
def test_bf16_mode_vs_rounding_oracle(dev, runs, fanin):
    """Sensitivity.run(weights=seeded normal) over all 56 paths of synth_design(N=2048, L=16, tile=32), bf16 mode, the last hop
    on mmft_mlp2_feat_dx_bf16, against the fp64 rounding oracle on the run's own feature map.
    Measured on one MI355X (e_hip / e_32 / e_plain):
      regular    pred 1.31e-4 / 1.31e-4 / 6.68e-3   cell 5.93e-8 / 1.22e-4 / 1.44e-1   net 6.69e-5 / 5.29e-5 / 9.49e-2
      irregular  pred 3.46e-5 / 3.45e-5 / 6.31e-3   cell 1.10e-7 / 8.39e-8 / 1.11e-1   net 9.29e-8 / 9.29e-8 / 6.59e-2
    (the generic-layer route gave the same bits as the fused kernel on both designs; in a batch of two, design 0 / design 1:
    cell 9.43e-8 / 1.57e-7, net 7.86e-8 / 1.79e-7; fp32 mode against the plain fp64 reference: cell 3.7e-7 / 5.1e-7,
    net 3.3e-7 / 4.0e-7.)  The regular design's e_32 of 1.2e-4 on the cell gradient is a rounding-boundary flip in the fp32
    oracle, not in the kernels: hence the floor of the module docstring."""
    c = runs(fanin)
    o64, o32, op = c['oracles']
    assert c['fused']['hop'] == 'fused'
    assert c['fused']['ends'] == o64['targets']
    _oracle_rows(f'{fanin}: fused last hop', c['fused'], o64, o32, op)
    _zero_rows_exact(c['d'], c['fused']['grads'][0])
    assert tuple(c['fused']['grads'][0]['cell_feat'].shape) == c['d'].cell_feat.shape
    assert tuple(c['fused']['grads'][0]['net_feat'].shape) == c['d'].net_feat.shape
    assert c['fused']['grads'][0]['cell_feat'].dtype == torch.float32 and c['fused']['grads'][0]['cell_feat'].is_cuda


@pytest.mark.parametrize('fanin', ['regular', 'irregular'])
def test_generic_layer_route_passes_the_same_oracle_row(dev, runs, fanin):
    """The last hop forced onto linear_fwd / linear_dgrad(mask=H) / linear_dgrad (H materialised), bf16 mode: the same oracle
    row as the fused route.  The two are not asked to be bitwise equal (different tiles, different accumulation order)."""
    c = runs(fanin)
    assert c['layers']['hop'] == 'layers'
    _oracle_rows(f'{fanin}: generic-layer last hop', c['layers'], *c['oracles'])
    print(f"   fused vs layers: cell {rel_err(c['fused']['cell'], c['layers']['cell']):.2e} net {rel_err(c['fused']['net'], c['layers']['net']):.2e}")


@pytest.mark.parametrize('fanin', ['regular', 'irregular'])
def test_fp32_mode_vs_plain_fp64_reference(dev, runs, fanin):
    """fp32 mode (the last hop on the generic layers): both gradients within 1e-4 of the plain fp64 reference on the run's
    own feature map - the project's fp32 parity bar."""
    c = runs(fanin)
    assert c['f32']['hop'] == 'layers'
    ref = oracle_sensitivity(c['d'], c['ids'], c['state'], c['f32']['fm'], c['w'])
    errs = {k: rel_err(c['f32'][k], ref[k]) for k in ('pred', 'cell', 'net')}
    print(f'\n{fanin}, fp32 mode vs plain fp64:', {k: f'{v:.2e}' for k, v in errs.items()})
    assert all(v < 1e-4 for v in errs.values()), errs


def test_batch_of_two_designs_of_different_size(dev):
    """N = 2048 / L = 16 and N = 1024 / L = 12 in one batch, bf16 mode: each design's gradients pass its own oracle row on its
    own feature map and its zero rows are exact - what a missed un-permutation or node offset breaks."""
    from mmft.sensitivity import Sensitivity
    designs = [_design(), _design(N=1024, L=12, seed=SEED + 1)]
    ids = [list(range(d.num_paths)) for d in designs]
    pmodel, cnn, state = _models(designs[0], dev)
    T = sum(len(p) for p in ids)
    w = _weights(T, seed=13)
    with lib.math_mode('bf16'):
        s = Sensitivity(pmodel, cnn, designs, dev)
        pred, ends, grads = s.run(weights=w)
        assert s.last_hop == 'fused'
    torch.cuda.synchronize()
    rows = batch_rows(designs, ids)
    off = np.concatenate([[0], np.cumsum([d.N for d in designs])])
    assert len(grads) == 2 and pred.numel() == T == len(ends)
    for i, d in enumerate(designs):
        assert np.array_equal(np.nonzero(s.row_design == i)[0], rows[i])
        r = torch.from_numpy(rows[i])
        o64, o32, op = _oracles(d, ids[i], state, s.feat_map[i].detach().double().cpu(), w[r])
        assert (np.asarray(ends)[rows[i]] - off[i]).tolist() == o64['targets']
        assert tuple(grads[i]['cell_feat'].shape) == d.cell_feat.shape and tuple(grads[i]['net_feat'].shape) == d.net_feat.shape
        hip = dict(pred=pred.double().cpu()[r], cell=grads[i]['cell_feat'].double().cpu(), net=grads[i]['net_feat'].double().cpu())
        _oracle_rows(f'batch of two, design {i} (N = {d.N}, L = {d.L})', hip, o64, o32, op)
        _zero_rows_exact(d, grads[i])


@pytest.fixture(scope='module')
def resident(dev):
    """One Sensitivity on the regular design with its modules, bf16 mode entered by the tests that use it."""
    from mmft.sensitivity import Sensitivity
    d = _design()
    pmodel, cnn, _ = _models(d, dev)
    with lib.math_mode('bf16'):
        s = Sensitivity(pmodel, cnn, [d], dev)
    return d, pmodel, cnn, s


def _equal(a, b):
    return all(torch.equal(_bits(x[k]), _bits(y[k])) for x, y in zip(a, b) for k in ('cell_feat', 'net_feat'))


def test_weights_and_objectives(dev, resident):
    d, pmodel, cnn, s = resident
    with lib.math_mode('bf16'):
        pred, _, grads = s.run(weights=torch.zeros(s.T))
        assert all(float(g[k].abs().max()) == 0.0 for g in grads for k in g)                  # all-zero weights: exactly zero
        # half of the rows violate: the required times of the rows (a documented attribute) set to the median prediction
        s.required.fill_(float(pred.median()))
        pred_t, _, g_tns = s.run()                                                           # objective='tns' is the default
        w = ((s.required - pred_t) < 0).to(torch.float32)
        assert 0 < float(w.sum()) < s.T
        pred_w, _, g_w = s.run(weights=w)
        assert torch.equal(_bits(pred_t), _bits(pred_w)) and _equal(g_tns, g_w)
        _, _, g_w2 = s.run(weights=w.cpu().numpy())                                          # host weights, numpy
        assert _equal(g_tns, g_w2)
        _, _, g_sum = s.run(objective='sum')
        _, _, g_one = s.run(weights=torch.ones(s.T, device=dev))
        assert _equal(g_sum, g_one) and not _equal(g_sum, g_tns)
        for bad, exc in ((dict(weights=torch.ones(s.T - 1)), ValueError), (dict(weights=torch.ones(s.T, dtype=torch.float64)), TypeError),
                         (dict(objective='wns'), ValueError)):
            with pytest.raises(exc):
                s.run(**bad)


def _snapshot(pmodel, cnn):
    mods = [m for root in (pmodel, cnn) for m in root.modules()]
    named = [(n, t) for root in (pmodel, cnn) for n, t in list(root.named_parameters()) + list(root.named_buffers())]
    return dict(values=[(n, t.detach().clone()) for n, t in named],
                grads=[(n, None if getattr(t, 'grad', None) is None else t.grad.detach().clone()) for n, t in named],
                flags=[(n, t.requires_grad) for n, t in named], modes=[m.training for m in mods],
                per_sample=[getattr(m, 'per_sample_stats', None) for m in mods])


def _same_snapshot(a, b):
    for (n, x), (_, y) in zip(a['values'], b['values']):
        assert x.dtype == y.dtype and torch.equal(*((_bits(x), _bits(y)) if x.dtype == torch.float32 else (x, y))), n
    for (n, x), (_, y) in zip(a['grads'], b['grads']):
        assert (x is None) == (y is None) and (x is None or torch.equal(_bits(x), _bits(y))), n
    assert a['flags'] == b['flags'] and a['modes'] == b['modes'] and a['per_sample'] == b['per_sample']


def test_nothing_of_the_model_is_written(dev, resident):
    """Every parameter, buffer (running statistics, num_batches_tracked), .grad, requires_grad flag and module mode is bitwise
    what it was; a Predictor on the same modules predicts the same bits before and after; two runs give the same bits."""
    from mmft.infer import Predictor
    d, pmodel, cnn, s = resident
    w = _weights(s.T, seed=14)
    # a .grad that is not None must survive as it is, and a frozen parameter must stay frozen
    p_grad, p_frozen = pmodel.mlp_fuse.layers[0].bias, pmodel.mlp_alpha.layers[0].bias
    p_grad.grad = torch.full_like(p_grad, 0.25)
    p_frozen.requires_grad_(False)
    try:
        with lib.math_mode('bf16'):
            pr = Predictor(pmodel, cnn, [d], dev, graphed=False)
            before = pr.predict()[0].clone()
            snap = _snapshot(pmodel, cnn)
            pred1, _, g1 = s.run(weights=w)
            pred2, _, g2 = s.run(weights=w)
            torch.cuda.synchronize()
            _same_snapshot(snap, _snapshot(pmodel, cnn))
            after = pr.predict()[0].clone()
        assert torch.equal(_bits(before), _bits(after))
        assert torch.equal(_bits(pred1), _bits(pred2)) and _equal(g1, g2)
        # what Predictor.predict() returns: the same rows and - the forward-only sweep is bitwise the training form
        # (tests/test_infer_gpu.py) - the same bits
        assert np.array_equal(pr.endpoints, s.endpoints)
        assert torch.equal(_bits(pred1), _bits(before))
    finally:
        p_grad.grad = None
        p_frozen.requires_grad_(True)


def test_update_then_run_equals_a_fresh_object_on_the_edited_design(dev, resident):
    from mmft.sensitivity import Sensitivity
    d, pmodel, cnn, s = resident
    rows = np.array([5, 77, 1000, 2047], dtype=np.int64)
    new_c = np.random.default_rng(3).standard_normal((rows.size, d.cell_feat.shape[1])).astype(np.float32)
    new_n = np.random.default_rng(4).standard_normal((rows.size, d.net_feat.shape[1])).astype(np.float32)
    d2 = copy.copy(d)
    d2.cell_feat, d2.net_feat = d.cell_feat.copy(), d.net_feat.copy()
    d2.cell_feat[rows], d2.net_feat[rows] = new_c, new_n
    w = _weights(s.T, seed=15)
    with lib.math_mode('bf16'):
        old_c = torch.from_numpy(d.cell_feat[rows]), torch.from_numpy(d.net_feat[rows])
        _, _, g0 = s.run(weights=w)
        s.update(0, cell_feat=new_c, net_feat=new_n, rows=rows)
        pred_u, _, g_u = s.run(weights=w)
        fresh = Sensitivity(pmodel, cnn, [d2], dev)
        pred_f, _, g_f = fresh.run(weights=w)
        assert torch.equal(_bits(pred_u), _bits(pred_f)) and _equal(g_u, g_f) and not _equal(g_u, g0)
        s.update(0, cell_feat=old_c[0], net_feat=old_c[1], rows=torch.from_numpy(rows))       # back, for the tests that follow
        _, _, g_back = s.run(weights=w)
        assert _equal(g_back, g0)
        with pytest.raises(IndexError):
            s.update(1, cell_feat=new_c, rows=rows)


def test_refusals_on_the_device(dev, monkeypatch):
    """A model whose parameters carry gradient sinks - a TrainStep with the fused optimizer was built on it - is refused, at
    construction and at run(); so is run() under an outer stream capture, before anything is launched."""
    from mmft.sensitivity import Sensitivity
    from mmft.train import TrainStep
    d = _design()
    pmodel, cnn, _ = _models(d, dev)
    s = Sensitivity(pmodel, cnn, [d], dev)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='outer stream capture'):
        s.run()
    monkeypatch.undo()
    assert s.last_hop is None and s.feat_map is None            # refused before anything was launched
    for p in pmodel.gnn.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match='requires a gradient'):
        s.run()
    for p in pmodel.gnn.parameters():
        p.requires_grad_(True)
    assert s.last_hop is None
    ts = TrainStep(pmodel, cnn, [d], dev)                       # fused optimizer: sinks on every trainable parameter
    with pytest.raises(RuntimeError, match='gradient sinks'):
        s.run()
    with pytest.raises(RuntimeError, match='gradient sinks'):
        Sensitivity(pmodel, cnn, [d], dev)
    del ts
