"""The rounding mode of the CPU oracle (oracle/bf16.py, restatement.py rounding='bf16'): the conversion itself, each
primitive against formulas written out here, the ablation of every rounding class at config A, and the fp32 / fp64 spread
the GPU tests (tests/test_bf16_oracle_gpu.py) calibrate their bounds with.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from oracle import bf16 as B
from oracle import restatement as R

UNET_PREFIX = ('inc.', 'down', 'up', 'outc.')


# ------------------------------------------------------------------------------------------------------------- r()
def bf16_bits_reference(x32):
    """Round-to-nearest-even of fp32 bit patterns to bf16, on the integers (finite inputs)."""
    u = x32.view(np.uint32).astype(np.uint64)
    lsb = (u >> 16) & 1
    return (((u + 0x7FFF + lsb) >> 16) << 16).astype(np.uint32).view(np.float32)


def test_r_ties_near_ties_negatives_subnormals():
    vals = [1 + 2.0 ** -8,                      # tie between 1 and 1 + 2^-7: to even (1)
            1 + 3 * 2.0 ** -8,                  # tie between 1 + 2^-7 and 1 + 2^-6: to even (1 + 2^-6)
            1 + 2.0 ** -8 + 2.0 ** -23,         # just above the tie: up
            1 + 2.0 ** -8 - 2.0 ** -23,         # just below the tie: down
            3.0, 255.0, 257.0, 65535.0, 1e-3, 0.1, 1e30, 3.3895313892515355e38,
            2.0 ** -126, 2.0 ** -127, 3 * 2.0 ** -134, 2.0 ** -133 + 2.0 ** -141, 2.0 ** -149, 0.0]
    x = np.array(vals + [-v for v in vals], dtype=np.float32)
    rng = np.random.default_rng(0)
    x = np.concatenate([x, (rng.standard_normal(4096) * 10.0 ** rng.integers(-30, 30, 4096)).astype(np.float32)])
    # random exact ties and their fp32 neighbours
    t = (rng.integers(0, 2 ** 31, 2048, dtype=np.uint64) & ~np.uint64(0xFFFF) | np.uint64(0x8000)).astype(np.uint32)
    t = t[(t & 0x7F800000) != 0x7F800000].view(np.float32)
    x = np.concatenate([x, t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf)])
    got = B.r(torch.from_numpy(x)).numpy()
    ref = bf16_bits_reference(x)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert B.r(torch.tensor([1 + 2.0 ** -8], dtype=torch.float32)).item() == 1.0
    assert B.r(torch.tensor([1 + 3 * 2.0 ** -8], dtype=torch.float32)).item() == 1 + 2.0 ** -6
    assert np.array_equal(B.r(torch.from_numpy(x.astype(np.float64))).numpy(), got.astype(np.float64))


def test_r_rounds_fp64_through_fp32():
    """The chosen conversion: fp64 -> fp32 -> bf16, the rounding of the fp32 value the kernels hold.  1 + 2^-8 + 2^-30 becomes
    the fp32 tie 1 + 2^-8 first and then 1.0; one direct rounding of the fp64 value would give 1 + 2^-7."""
    v = 1 + 2.0 ** -8 + 2.0 ** -30
    assert float(np.float32(v)) == 1 + 2.0 ** -8
    assert B.r(torch.tensor([v], dtype=torch.float64)).item() == 1.0
    assert B.r(torch.tensor([-v], dtype=torch.float64)).item() == -1.0
    assert B.r(torch.tensor([v], dtype=torch.float64)).dtype == torch.float64


# ------------------------------------------------------------------------------------------------------ primitives
def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def rb(t):
    return t.float().bfloat16().double()


def test_stored_rounds_value_and_gradient():
    x, g = rnd(7, 5, seed=1).requires_grad_(True), rnd(7, 5, seed=2)
    y = B.stored(x)
    assert torch.equal(y, rb(x.detach()))
    y.backward(g)
    assert torch.equal(x.grad, rb(g))
    x.grad = None
    B.stored(x, value=False).backward(g)
    assert torch.equal(x.grad, rb(g))
    x.grad = None
    y = B.stored(x, grad=False)
    assert torch.equal(y, rb(x.detach()))
    y.backward(g)
    assert torch.equal(x.grad, g)


def test_linear_bf16_forward_backward():
    x, w, b, g = rnd(33, 20, seed=1), rnd(12, 20, seed=2), rnd(12, seed=3), rnd(33, 12, seed=4)
    xl, wl, bl = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = B.linear_bf16(xl, wl, bl)
    xn, wn, gn = rb(x).numpy(), rb(w).numpy(), g.numpy()
    assert np.allclose(y.detach().numpy(), xn @ wn.T + b.numpy()[None, :], rtol=1e-13, atol=1e-13)
    y.backward(g)
    gr = rb(g).numpy()
    assert np.allclose(xl.grad.numpy(), gr @ wn, rtol=1e-13, atol=1e-13)
    assert np.allclose(wl.grad.numpy(), gr.T @ xn, rtol=1e-13, atol=1e-13)
    assert np.allclose(bl.grad.numpy(), gn.sum(0), rtol=1e-13, atol=1e-13)          # the fp32 gradient, not rounded


def test_conv2d_bf16_forward_backward():
    N, Ci, Co, H, W = 2, 5, 6, 7, 9
    x, w, g = rnd(N, Ci, H, W, seed=1), rnd(Co, Ci, 3, 3, seed=2), rnd(N, Co, H, W, seed=3)
    xl, wl = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = B.conv2d_bf16(xl, wl, 1)
    xp = F.pad(rb(x), [1, 1, 1, 1])
    wr, gr = rb(w), rb(g)
    ref = torch.zeros(N, Co, H, W, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            ref += torch.einsum('nihw,oi->nohw', xp[:, :, ky:ky + H, kx:kx + W], wr[:, :, ky, kx])
    assert torch.allclose(y, ref, rtol=1e-12, atol=1e-12)
    y.backward(g)
    dw = torch.zeros_like(w)
    dxp = torch.zeros_like(xp)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = torch.einsum('nohw,nihw->oi', gr, xp[:, :, ky:ky + H, kx:kx + W])
            dxp[:, :, ky:ky + H, kx:kx + W] += torch.einsum('nohw,oi->nihw', gr, wr[:, :, ky, kx])
    assert torch.allclose(wl.grad, dw, rtol=1e-12, atol=1e-12)
    assert torch.allclose(xl.grad, dxp[:, :, 1:-1, 1:-1], rtol=1e-12, atol=1e-12)


def test_conv_transpose2d_bf16_forward_backward():
    N, Ci, Co, h, w_ = 2, 6, 3, 4, 5
    x, w, b, g = rnd(N, Ci, h, w_, seed=1), rnd(Ci, Co, 2, 2, seed=2), rnd(Co, seed=3), rnd(N, Co, 2 * h, 2 * w_, seed=4)
    xl, wl, bl = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = B.conv_transpose2d_bf16(xl, wl, bl)
    xr, wr, gr = rb(x), rb(w), rb(g)
    ref = torch.zeros(N, Co, 2 * h, 2 * w_, dtype=torch.float64)
    for a in range(2):
        for c in range(2):
            ref[:, :, a::2, c::2] = torch.einsum('nihw,io->nohw', xr, wr[:, :, a, c]) + b[None, :, None, None]
    assert torch.allclose(y, ref, rtol=1e-12, atol=1e-12)
    y.backward(g)
    dx = sum(torch.einsum('nohw,io->nihw', gr[:, :, a::2, c::2], wr[:, :, a, c]) for a in range(2) for c in range(2))
    dw = torch.stack([torch.stack([torch.einsum('nihw,nohw->io', xr, gr[:, :, a::2, c::2]) for c in range(2)], -1)
                      for a in range(2)], -2)
    assert torch.allclose(xl.grad, dx, rtol=1e-12, atol=1e-12)
    assert torch.allclose(wl.grad, dw, rtol=1e-12, atol=1e-12)
    assert torch.allclose(bl.grad, g.sum((0, 2, 3)), rtol=1e-12, atol=1e-12)


def test_rounding_none_is_the_plain_oracle():
    """rounding=None and the empty class set run the plain code: bit for bit the default call."""
    torch.manual_seed(3)
    import Unet
    sd = {k: v.double() for k, v in Unet.UNet('max').state_dict().items()}
    x = torch.rand(1, 3, 16, 32, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    ys = []
    for kw in ({}, dict(rounding=None), dict(rounding=())):
        p = {k: v.clone() for k, v in sd.items()}
        ys.append(R.unet_forward(p, x, 'max', **kw))
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    y = R.unet_forward({k: v.clone() for k, v in sd.items()}, x, 'max', rounding='bf16')
    assert not torch.equal(y, ys[0])
    with pytest.raises(ValueError):
        B.classes({'nope'})


# ------------------------------------------------------------------------------------- config A: ablation, spread
def _step(d, path_ids, pm_state, pc_state, rounding, dtype, feat_map=None):
    o = R.OracleTrainer(pm_state, pc_state, dtype=dtype, rounding=rounding)
    feat = feat_map.to(dtype).clone().requires_grad_(True) if feat_map is not None else None
    hats, tl, _ = o.forward(d, R.design_csr(d), path_ids, feat_map=feat)
    arr = torch.from_numpy(d.arrival_time).to(dtype)[torch.tensor(tl)].squeeze(-1)
    loss = F.mse_loss(hats, arr)
    loss.backward()
    grads = {k: v.grad.detach().double() for k, v in list(o.pm.items()) + list(o.pc.items())
             if isinstance(v, torch.Tensor) and v.grad is not None}
    return dict(hats=hats.detach().double(), loss=float(loss.detach()), grads=grads,
                run={k: v.double() for k, v in o.pc.items() if 'running' in k},
                feat_grad=feat.grad.double() if feat is not None else None)


def _rel_l2(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def _dists_sweep(r, ref):
    """The GPU test's rows for the sweep + head on a given feature map (max norm), with their floors."""
    out = {'predictions': (rel_err(r['hats'], ref['hats']), 1e-4),
           'loss': (abs(r['loss'] - ref['loss']) / ref['loss'], 1e-5),
           'd loss / d feature map': (rel_err(r['feat_grad'], ref['feat_grad']), 1e-4)}
    for k, g in ref['grads'].items():
        if float(g.abs().max()) > 0:
            out[k] = (rel_err(r['grads'][k], g), 1e-4)
    return out


def _dists_unet(r, ref):
    """The GPU test's U-Net rows (relative L2 per gradient tensor and their mean, running statistics), with their floors.
    OutConv's bias gradient is left out here: the GPU test measures it against the sum of |g| of the step."""
    keys = [k for k, g in ref['grads'].items() if k.startswith(UNET_PREFIX) and k != 'outc.conv.0.bias'
            and float(g.abs().max()) > 0]
    out = {k: (_rel_l2(r['grads'][k], ref['grads'][k]), 2e-2) for k in keys}
    out['U-Net mean'] = (float(np.mean([out[k][0] for k in keys])), 2e-2)
    for k, v in ref['run'].items():
        out[k] = (rel_err(r['run'][k], v), 1e-4)
    return out


def _ratios(e, e32):
    """e / bound per row, bound = max(floor, 3 e_32) as in tests/test_bf16_oracle_gpu.py."""
    return {k: e[k][0] / max(e[k][1], 3 * e32[k][0]) for k in e}


@pytest.fixture(scope='module')
def config_a():
    """Config A with the GPU test's split: the U-Net coupled, the sweep + head on the fp64 rounding oracle's own feature
    map.  Returns (run coupled, run decoupled, references, fp32 spreads)."""
    from mmft.synth import config_design
    from mmft.train import build_models
    d = config_design('A')
    pmodel, cnn = build_models(map_size=d.map_size, device='cpu', seed=9294)
    pm_state = {k: v.detach().clone() for k, v in pmodel.state_dict().items()}
    pc_state = {k: v.detach().clone() for k, v in cnn.state_dict().items()}
    path_ids = np.random.default_rng(1).permutation(d.num_paths)[:100].tolist()
    pc = {k: v.double().clone() for k, v in pc_state.items()}
    feat = R.unet_forward(pc, torch.from_numpy(d.image).double(), 'max', True, rounding='bf16').detach().reshape(-1)
    run = lambda rounding, dtype=torch.float64: _step(d, path_ids, pm_state, pc_state, rounding, dtype)
    srun = lambda rounding, dtype=torch.float64: _step(d, path_ids, pm_state, pc_state, rounding, dtype, feat)
    o64, s64 = run('bf16'), srun('bf16')
    return run, srun, o64, s64, _dists_unet(run('bf16', torch.float32), o64), _dists_sweep(srun('bf16', torch.float32), s64)


@pytest.mark.parametrize('cls', ['sweep', 'head'])
def test_ablation_sweep_and_head_classes_exceed_the_gpu_bound(config_a, cls):
    """Turning the sweep's or the head's rounding off moves some row of the GPU test's decoupled comparison by more than
    ten times its bound: the bound sees where those kernels round."""
    _, srun, _, s64, _, s32 = config_a
    ratio = _ratios(_dists_sweep(srun(set(B.CLASSES) - {cls}), s64), s32)
    worst = max(ratio, key=ratio.get)
    assert ratio[worst] > 10.0, (worst, ratio[worst])


@pytest.mark.parametrize('cls', ['conv', 'act', 'bnstats'])
def test_ablation_unet_classes_exceed_the_gpu_bound(config_a, cls):
    """Turning one U-Net rounding class off moves some U-Net row (gradient, mean or running statistic) past its bound."""
    run, _, o64, _, u32, _ = config_a
    ratio = _ratios(_dists_unet(run(set(B.CLASSES) - {cls}), o64), u32)
    worst = max(ratio, key=ratio.get)
    assert ratio[worst] > 1.0, (worst, ratio[worst])


def test_ablation_gradient_storage_moves_only_unet_gradients(config_a):
    """Rounding the U-Net's stored gradients (g, dz, gcat, gp) changes ONLY the U-Net's gradients: predictions, loss,
    running statistics and every GNN / head gradient stay bit for bit.  How far the U-Net gradients move is printed; at
    config A it is below the fp32 spread of the forward pass, so the bitwise kernel tests of tests/test_unet16_gpu.py
    are what pin this class on the GPU."""
    run, _, o64, _, u32, _ = config_a
    r = run(set(B.CLASSES) - {'grad'})
    assert torch.equal(r['hats'], o64['hats']) and r['loss'] == o64['loss']
    assert all(torch.equal(r['run'][k], o64['run'][k]) for k in o64['run'])
    moved = [k for k in o64['grads'] if not torch.equal(r['grads'][k], o64['grads'][k])]
    assert moved and all(k.startswith(UNET_PREFIX) for k in moved), moved
    ratio = _ratios(_dists_unet(r, o64), u32)
    print('stored U-Net gradients off: largest row / bound', max(ratio.values()))


def test_ablation_hidden_storage_only_moves_db1(config_a):
    """storing fc_cell_neigh's HN / DHN as bf16 changes nothing but that MLP's first bias gradient (the
    only consumer that sums the rounded DHN instead of rounding it as an MFMA operand) - bitwise on the oracle side."""
    _, srun, _, s64, _, _ = config_a
    r = srun(set(B.CLASSES) - {'hidden'})
    assert torch.equal(r['hats'], s64['hats']) and r['loss'] == s64['loss'] and torch.equal(r['feat_grad'], s64['feat_grad'])
    moved = [k for k in s64['grads'] if not torch.equal(r['grads'][k], s64['grads'][k])]
    assert moved == ['gnn.fc_cell_neigh.layers.0.bias'], moved


def test_fp32_spread_is_nonzero_and_below_the_plain_distance(config_a):
    """The calibration of the GPU bounds: the rounding oracle in fp32 differs from itself in fp64, and the plain fp64 oracle
    is further away - more than ten times the bound on every sweep / head row (measured: 17x on mlp_fuse's output bias,
    30 - 450x elsewhere), but only 2-3x on the U-Net (a last-bit difference crosses bf16 rounding boundaries and every
    later layer rounds again; measured mean relative L2 0.12 vs 0.33)."""
    run, srun, o64, s64, u32, s32 = config_a
    sp = _dists_sweep(srun(None), s64)
    assert all(s32[k][0] >= 0 for k in s32) and s32['predictions'][0] > 0
    ratio = _ratios(sp, s32)
    assert min(ratio.values()) > 10.0, min(ratio.items(), key=lambda kv: kv[1])
    up = _dists_unet(run(None), o64)
    assert 0 < u32['U-Net mean'][0] and 2 * u32['U-Net mean'][0] < up['U-Net mean'][0]


def test_oracle_trainer_step_with_rounding():
    """OracleTrainer(rounding='bf16').step: the loss of the rounding forward, then one Adam step - from zero moments every
    parameter with a gradient moves by lr against the sign of its gradient (|g| >> eps)."""
    from mmft.synth import config_design
    from mmft.train import build_models
    d = config_design('A', L=8)
    pmodel, cnn = build_models(map_size=d.map_size, device='cpu', seed=9294)
    pm_state = {k: v.detach().clone() for k, v in pmodel.state_dict().items()}
    pc_state = {k: v.detach().clone() for k, v in cnn.state_dict().items()}
    path_ids = np.random.default_rng(1).permutation(d.num_paths)[:50].tolist()
    ref = _step(d, path_ids, pm_state, pc_state, 'bf16', torch.float64)
    t = R.OracleTrainer(pm_state, pc_state, dtype=torch.float64, rounding='bf16')
    before = {k: v.detach().clone() for k, v in list(t.pm.items()) + list(t.pc.items()) if v.requires_grad}
    loss, _, _ = t.step(d, R.design_csr(d), path_ids)
    assert loss == ref['loss']
    for k, v in before.items():
        g = ref['grads'].get(k)
        now = t.pm.get(k, t.pc.get(k)).detach()
        if g is None:
            assert torch.equal(now, v), k
            continue
        big = g.abs() > 1e-4
        assert torch.allclose((now - v)[big], -1e-3 * g[big].sign(), rtol=1e-3, atol=0), k


def test_oracle_trainer_resumes_adam_mid_run():
    """OracleTrainer.load_adam (the GPU trajectory tests start the oracle from the HIP optimizer's moments and step counter):
    a trainer built from the parameters and running statistics after one step, its Adam state loaded, and stepped twice
    equals three uninterrupted torch.optim.Adam steps bit for bit; loaded with the wrong step count it does not.  In fp64:
    the fp32 CPU oracle is not bitwise repeatable run to run (threaded weight-gradient GEMMs), so bit for bit means fp64."""
    dtype = torch.float64
    from mmft.synth import config_design
    from mmft.train import build_models
    d = config_design('A', L=8)
    csr = R.design_csr(d)
    pmodel, cnn = build_models(map_size=d.map_size, device='cpu', seed=9294)
    pm_state = {k: v.detach().clone() for k, v in pmodel.state_dict().items()}
    pc_state = {k: v.detach().clone() for k, v in cnn.state_dict().items()}
    rng = np.random.default_rng(8)
    batches = [rng.permutation(d.num_paths)[:30].tolist() for _ in range(3)]
    whole = R.OracleTrainer(pm_state, pc_state, dtype=dtype)
    for ids in batches:
        whole.step(d, csr, ids)
    first = R.OracleTrainer(pm_state, pc_state, dtype=dtype)
    first.step(d, csr, batches[0])
    names = [k for k, v in list(first.pm.items()) + list(first.pc.items()) if first.optim.state.get(v)]
    assert names and all(int(first.optim.state[first.leaf(k)]['step']) == 1 for k in names)
    m = {k: first.optim.state[first.leaf(k)]['exp_avg'] for k in names}
    v = {k: first.optim.state[first.leaf(k)]['exp_avg_sq'] for k in names}
    state = lambda t: ({k: x.detach().clone() for k, x in t.pm.items()}, {k: x.detach().clone() for k, x in t.pc.items()})

    def resumed(step):
        t = R.OracleTrainer(*state(first), dtype=dtype)
        t.load_adam(m, v, step)
        for ids in batches[1:]:
            t.step(d, csr, ids)
        return t
    r = resumed(1)
    for k in list(whole.pm) + list(whole.pc):
        a, b = whole.pm.get(k, whole.pc.get(k)), r.pm.get(k, r.pc.get(k))
        assert torch.equal(a.detach(), b.detach()), k
    wrong = resumed(0)
    assert not all(torch.equal(whole.leaf(k).detach(), wrong.leaf(k).detach()) for k in names)
