"""Kernel-level parity of the fp32 layer kernels of csrc/cnn.hip (BatchNorm, 2x2 pooling, bilinear x2, pixel shuffle, region
copy, layout changes) - what parity mode, LayoutNet and every non-fused fallback run: each entry point called by name through
the C ABI against the torch functional of the same layer in fp64 on the CPU and its autograd."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from mmft import lib
from mmft.detrand import det_uniform, det_ints

pytestmark = pytest.mark.gpu
F = torch.nn.functional
TOL = 2e-5          # as tests/test_kernels_gpu.py
EPS24 = 2.0 ** -24
SENT = 4321.0


def T_(shape, seed, dev, lo=-1.0, hi=1.0):
    return torch.from_numpy(det_uniform(shape, seed, lo, hi)).to(dev)


# --------------------------------------------------------------------------------------------- BatchNorm
def _bn_case(dev, C, rows, groups, offset):
    x_h = det_uniform((groups, rows, C), 1, -1, 1) + np.float32(offset)
    if C > 1:
        x_h[:, :, 1] = np.float32(0.75) + np.float32(offset)        # one channel held constant: variance 0
    return dict(x=torch.from_numpy(x_h).to(dev), gamma=T_((C,), 2, dev, 0.5, 1.5), beta=T_((C,), 3, dev, -0.5, 0.5),
                rm=T_((C,), 4, dev, -0.1, 0.1), rv=T_((C,), 5, dev, 0.5, 1.5), gy=T_((groups, rows, C), 6, dev))


def _bn_ref(c, groups, momentum, eps):
    """fp64 F.batch_norm per group (sequential momentum updates of shared running statistics); y [groups, rows, C] before ReLU."""
    x = c['x'].double().cpu().requires_grad_(True)
    gamma, beta = c['gamma'].double().cpu().requires_grad_(True), c['beta'].double().cpu().requires_grad_(True)
    rm, rv = c['rm'].double().cpu().clone(), c['rv'].double().cpu().clone()
    ys = [F.batch_norm(x[g], rm, rv, gamma, beta, True, momentum, eps) for g in range(groups)]
    xd = x.detach()
    mean = xd.mean(1)
    invstd = 1.0 / torch.sqrt(xd.var(1, unbiased=False) + eps)
    return x, gamma, beta, torch.stack(ys), rm, rv, mean, invstd


def _chan(got, ref, C):
    """per channel: max|got - ref| / max|ref| of that channel (a channel with large values does not hide the others)."""
    g, r = got.detach().double().cpu().reshape(-1, C), ref.detach().double().cpu().reshape(-1, C)
    return (g - r).abs().amax(0) / (r.abs().amax(0) + 1e-30)


def _bn_fp32_spread(c, groups, momentum, eps, mask, ref):
    """torch's own fp32 F.batch_norm + autograd against the fp64 one on the same input, on the CPU: the largest per-channel
    relative spread of (y, dx, dgamma, dbeta) over the channels that are not held constant."""
    C = c['x'].shape[-1]
    x = c['x'].cpu().clone().requires_grad_(True)
    gamma, beta = c['gamma'].cpu().clone().requires_grad_(True), c['beta'].cpu().clone().requires_grad_(True)
    rm, rv = c['rm'].cpu().clone(), c['rv'].cpu().clone()
    y = torch.stack([F.batch_norm(x[g], rm, rv, gamma, beta, True, momentum, eps) for g in range(groups)])
    (y * (c['gy'].cpu() * mask.float())).sum().backward()
    keep = [i for i in range(C) if i != 1]
    return [float(_chan(y, ref[0], C)[keep].max()), _joint(x.grad, ref[1], C, keep), _vec(gamma.grad, ref[2], keep),
            _vec(beta.grad, ref[3], keep)]


def _joint(got, ref, C, keep):
    """max|got - ref| over the channels `keep` of a [.., C] tensor, relative to the largest |ref| in those channels."""
    g, r = got.detach().double().cpu().reshape(-1, C)[:, keep], ref.detach().double().cpu().reshape(-1, C)[:, keep]
    return float((g - r).abs().max() / r.abs().max())


def _vec(got, ref, keep):
    """max|got - ref| over the channels `keep`, relative to the largest |ref| among them."""
    g, r = got.detach().double().cpu().reshape(-1)[keep], ref.detach().double().cpu().reshape(-1)[keep]
    return float((g - r).abs().max() / r.abs().max())


def _bn_check(dev, C, rows, groups, offset):
    momentum, eps = 0.1, 1e-5
    c = _bn_case(dev, C, rows, groups, offset)
    x64, g64, b64, y64, rm64, rv64, mean64, invstd64 = _bn_ref(c, groups, momentum, eps)
    need = lib.query('mmft_bn_workspace_bytes', groups, rows, C)
    ws = torch.full((need // 4 + 16,), SENT, device=dev)
    d, st = lib.stream_args(c['x'])
    res = {}
    for relu in (0, 1):
        y = torch.full((groups * rows * C + 16,), SENT, device=dev)
        rm, rv = c['rm'].clone(), c['rv'].clone()
        sm, si = torch.empty((groups, C), device=dev), torch.empty((groups, C), device=dev)
        lib.call('mmft_bn_train_fwd', c['x'], y, c['gamma'], c['beta'], rm, rv, momentum, eps, groups, rows, C, sm, si, relu, ws, need, d, st)
        assert bool((y[groups * rows * C:] == SENT).all()) and bool((ws[need // 4:] == SENT).all())
        y = y[:groups * rows * C].reshape(groups, rows, C)
        # saved statistics against fp64: the mean is rounded to fp32 once; its sum carries TOL of the spread
        spread = float((x64.detach() - mean64[:, None]).abs().max())
        assert float((sm.double().cpu() - mean64).abs().max()) <= EPS24 * float(mean64.abs().max()) + TOL * spread
        assert float(((si.double().cpu() - invstd64) / invstd64).abs().max()) < TOL
        if C > 1:                                                 # the constant channel: variance 0, invstd = 1 / sqrt(eps)
            assert float((si[:, 1].double().cpu() * np.sqrt(eps) - 1.0).abs().max()) < 1e-6
            assert torch.equal(sm[:, 1].cpu(), c['x'][:, 0, 1].cpu())
        # y per channel, relative to the channel's largest pre-activation: TOL; with a large mean, or with two rows (where the
        # fp32 rounding of the saved mean is not small against x - mean when the two values are close), 4x what torch's
        # fp32 batch_norm itself loses against fp64 on this input
        yr = torch.relu(y64.detach()) if relu else y64.detach()
        err = (y.double().cpu() - yr).abs().reshape(-1, C).amax(0) / y64.detach().abs().reshape(-1, C).amax(0)
        hard = bool(offset) or rows == 2
        if hard:
            spread_y = _bn_fp32_spread(c, groups, momentum, eps, torch.ones_like(y64), (y64, y64, g64, b64))[0]
            print(f'bn C={C} rows={rows} groups={groups} offset={offset}: torch fp32 y spread {spread_y:.3e}, kernel {float(err.max()):.3e}')
        tol_y = max(TOL, 4 * spread_y) if hard else TOL
        assert float(err.max()) < tol_y, (relu, float(err.max()))
        if C > 1:                                                 # the constant channel: exactly beta
            assert torch.equal(y[:, :, 1].cpu(), (torch.relu(c['beta'][1]) if relu else c['beta'][1]).cpu().expand(groups, rows))
        # running statistics: `groups` sequential momentum updates with the unbiased variance
        assert rel_err(rm, rm64) < TOL and rel_err(rv, rv64) < TOL
        res[relu] = (y, sm, si)
    # eval mode from given running statistics
    ye = torch.empty((groups, rows, C), device=dev)
    lib.call('mmft_bn_eval_fwd', c['x'], ye, c['gamma'], c['beta'], c['rm'], c['rv'], eps, groups * rows, C, 1, d, st)
    rme, rve = c['rm'].double().cpu(), c['rv'].double().cpu()
    pre = F.batch_norm(x64.detach().reshape(-1, C), rme, rve, g64.detach(), b64.detach(), False, momentum, eps)
    assert float((ye.double().cpu().reshape(-1, C) - torch.relu(pre)).abs().max()) <= TOL * float(pre.abs().max())
    # backward.  The ReLU mask is taken from the kernel's own output (checked above): an element within rounding of zero may
    # fall on either side in fp32 and fp64, and the gradient is discontinuous there.
    for relu in (0, 1):
        y, sm, si = res[relu]
        mask = (y > 0).double().cpu() if relu else torch.ones_like(y64)
        for t in (x64, g64, b64):
            t.grad = None
        (y64 * (c['gy'].double().cpu() * mask)).sum().backward(retain_graph=True)
        outs = []
        for variant in (('beta',) if not relu else ('beta', 'y')):
            dx = torch.full((groups * rows * C + 16,), SENT, device=dev)
            dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
            lib.call('mmft_bn_train_bwd', c['gy'], c['x'], y if variant == 'y' else None, c['gamma'],
                     c['beta'] if variant == 'beta' and relu else None, sm, si, dx, dg, db, groups, rows, C, relu, ws, need, d, st)
            assert bool((dx[groups * rows * C:] == SENT).all()) and bool((ws[need // 4:] == SENT).all())
            outs.append((dx[:groups * rows * C].reshape(groups, rows, C), dg, db))
        dx, dg, db = outs[0]
        keep = [i for i in range(C) if i != 1]
        ec = _chan(dx, x64.grad, C)
        e = (rel_err(dx, x64.grad), rel_err(dg, g64.grad), rel_err(db, b64.grad))
        print(f'bn C={C} rows={rows} groups={groups} offset={offset} relu={relu}: dx {e[0]:.3e} (per channel {float(ec.max()):.3e}) '
              f'dgamma {e[1]:.3e} dbeta {e[2]:.3e}')
        if not (offset or rows == 2):
            # within TOL of the largest reference magnitude (the measure of tests/test_kernels_gpu.py), dx also per channel
            assert e[0] < TOL and e[1] < TOL and e[2] < TOL and float(ec.max()) < TOL
        else:
            # A mean of 1000: xhat is formed from the saved fp32 mean, whose rounding (2^-24 |mean|) no fp32 BatchNorm escapes.
            # Two rows: xhat = +-1 and the three terms of dx = gamma invstd (g - mean(g) - xhat mean(g xhat)) cancel
            # analytically to an eps / var remainder, so dx is mostly the rounding of its terms.  Bound for the channels that
            # vary: 4x the spread of torch's fp32 autograd against fp64 on this input (same mask), in the same measure; the
            # constant channel, whose mean is exact and whose xhat is 0, stays at TOL.
            sp = _bn_fp32_spread(c, groups, momentum, eps, mask, (y64, x64.grad, g64.grad, b64.grad))
            ek = (_joint(dx, x64.grad, C, keep), _vec(dg, g64.grad, keep), _vec(db, b64.grad, keep))
            print(f'    channels that vary: dx {ek[0]:.3e} dgamma {ek[1]:.3e} dbeta {ek[2]:.3e}; '
                  f'torch fp32 spread: dx {sp[1]:.3e} dgamma {sp[2]:.3e} dbeta {sp[3]:.3e}')
            for k, spk in zip(ek, sp[1:]):
                assert k < max(TOL, 4 * spk), (k, spk)
            if C > 1:
                for got, ref in ((dg, g64.grad), (db, b64.grad)):
                    assert abs(float(got[1]) - float(ref[1])) <= TOL * float(ref.abs().max())
                assert float(ec[1]) < TOL
        if relu:                                                  # mask recomputed from x (beta) and read from y: bitwise equal
            assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))


@pytest.mark.parametrize('groups', [1, 3])
@pytest.mark.parametrize('rows', [2, 511, 513, 20000])
@pytest.mark.parametrize('C', [3, 16, 48, 256])
def test_batchnorm_train_eval_bwd(dev, C, rows, groups):
    """mmft_bn_train_fwd / mmft_bn_eval_fwd / mmft_bn_train_bwd against fp64 F.batch_norm and autograd.  C = 3: the scalar
    path; C = 48: 12 channel groups (no divisor of 256, 1024 no multiple of C: the per-element form of apply and backward);
    C = 256: the limit of the in-kernel running-statistics update.  rows 2 / 511 / 513 / 20000: one block, the block boundary,
    the many-workgroup regime.  groups = 3: per-sample statistics, three sequential momentum updates.  One channel is held
    constant (variance 0).  ReLU on and off; backward with beta (mask recomputed) and with y: bitwise equal.

    Everything within TOL of the largest reference magnitude, y and dx also channel by channel.  Only rows = 2 needs more: xhat
    = +-1 there, dx cancels analytically to an eps / var remainder, and where the two values of a channel are close the fp32
    rounding of the saved mean is not small against x - mean.  Those cases are held to max(TOL, 4 x spread), the spread being
    torch's own fp32 F.batch_norm + autograd against the fp64 one on the same input and mask, computed on the CPU inside the
    test over the channels that vary (the constant channel stays at TOL).  Measured spreads at rows = 2 (y per channel / dx
    over those channels; dgamma and dbeta stay below 1e-5): C = 3: 9e-8 / 8e-7 ... 9e-5; C = 16: 3e-7 ... 3e-6 / 6e-6 ... 9e-5;
    C = 48: 5e-7 ... 7e-6 / 2e-7 ... 9e-6; C = 256: 9e-6 ... 1.5e-5 / 4e-6."""
    _bn_check(dev, C, rows, groups, 0.0)


@pytest.mark.parametrize('groups', [1, 3])
@pytest.mark.parametrize('C', [3, 16])
def test_batchnorm_large_mean(dev, C, groups):
    """Mean 1000, spread 1 - what the shifted sums exist for: save_mean / save_invstd against fp64, and everything else.

    The saved mean is an fp32 number: its rounding (up to 2^-24 * 1000 = 6e-5, times invstd = 1.7 in xhat) is in every fp32
    BatchNorm.  So y, dx, dgamma and dbeta of the channels that vary are held to max(TOL, 4 x spread), the spread being torch's
    own fp32 F.batch_norm + autograd against the fp64 one on the same input, computed on the CPU inside the test.  Measured
    (C, groups: y / dx per channel, dgamma / dbeta over the channels): 3, 1: 1.3e-5 / 7.6e-7 / 4.3e-6 (1.0e-5 with ReLU) / 2.2e-7;
    3, 3: 6.5e-5 / 4.2e-6 / 3.6e-5 / 1.1e-6; 16, 1: 1.2e-4 / 1.2e-5 / 1.3e-4 / 1.1e-7; 16, 3: 1.2e-4 / 1.6e-5 / 1.5e-4 / 2.0e-7.
    The constant channel, whose mean is exact, stays at TOL and its y is exactly beta (torch's fp32 y is off by 0.17 there)."""
    _bn_check(dev, C, 513, groups, 1000.0)


# --------------------------------------------------------------------------------------------- pooling
def _nhwc(a, dev):
    """numpy [N, H, W, C] -> (device NHWC tensor, fp64 CPU NCHW leaf)."""
    t = torch.from_numpy(a).to(dev)
    return t, torch.from_numpy(a).double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)


@pytest.mark.parametrize('mode', ['max', 'avg'])
@pytest.mark.parametrize('C', [1, 16])
@pytest.mark.parametrize('H,W', [(2, 2), (5, 7), (8, 64)])
def test_pool2x2(dev, H, W, C, mode):
    """mmft_pool2x2_fwd / _bwd against F.max_pool2d / F.avg_pool2d and autograd.  Data from {0, 1, 2}: every window has ties and
    the gradient goes to the first maximum in row-major order; the last row and column of an odd input get exactly 0.  All
    values are small integers or their quarters: exact equality."""
    N = 2
    x_h = det_ints((N, H, W, C), 1, 0, 3).astype(np.float32)
    x_h[:, 0, 0] = x_h[:, 0, 1] = 2.0                         # the first window's maximum sits in its first two elements
    win = x_h[:, :H // 2 * 2, :W // 2 * 2].reshape(N, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(-1, 4)
    assert ((win == win.max(1, keepdims=True)).sum(1) > 1).any()              # windows with tied maxima
    assert all(len(set(r)) < 4 for r in win.tolist())                           # and a tie of some kind in every window
    x, x64 = _nhwc(x_h, dev)
    gy_h = det_uniform((N, H // 2, W // 2, C), 2)
    gy = torch.from_numpy(gy_h).to(dev)
    y64 = F.max_pool2d(x64, 2) if mode == 'max' else F.avg_pool2d(x64, 2)
    y64.backward(torch.from_numpy(gy_h).double().permute(0, 3, 1, 2))
    code = 0 if mode == 'max' else 1
    y = torch.full((N * (H // 2) * (W // 2) * C + 8,), SENT, device=dev)
    dx = torch.full((N * H * W * C + 8,), SENT, device=dev)
    d, st = lib.stream_args(x)
    lib.call('mmft_pool2x2_fwd', x, y, N, H, W, C, code, d, st)
    lib.call('mmft_pool2x2_bwd', x, gy, dx, N, H, W, C, code, d, st)
    assert bool((y[-8:] == SENT).all()) and bool((dx[-8:] == SENT).all())
    y, dx = y[:-8].reshape(N, H // 2, W // 2, C), dx[:-8].reshape(N, H, W, C)
    assert torch.equal(y.double().cpu(), y64.detach().permute(0, 2, 3, 1))
    assert torch.equal(dx.double().cpu(), x64.grad.permute(0, 2, 3, 1))
    if H % 2:
        assert bool((dx[:, H - 1] == 0).all())
    if W % 2:
        assert bool((dx[:, :, W - 1] == 0).all())


def test_pool2x2_nan_propagates_as_torch(dev):
    """One NaN in a window: the maximum is NaN and the gradient goes to the NaN's position (max), the mean is NaN (avg)."""
    N, H, W, C = 1, 5, 7, 16
    x_h = det_ints((N, H, W, C), 1, 0, 3).astype(np.float32)
    x_h[0, 1, 2, 3] = np.nan                                       # second row, first column of window (0, 1), channel 3
    x_h[0, 2, 4, 5] = np.nan                                       # first element of window (1, 2), channel 5
    x, x64 = _nhwc(x_h, dev)
    gy_h = det_uniform((N, H // 2, W // 2, C), 2)
    gy = torch.from_numpy(gy_h).to(dev)
    d, st = lib.stream_args(x)
    for code, fn in ((0, F.max_pool2d), (1, F.avg_pool2d)):
        x64.grad = None
        y64 = fn(x64, 2)
        y64.backward(torch.from_numpy(gy_h).double().permute(0, 3, 1, 2))
        y, dx = torch.empty((N, H // 2, W // 2, C), device=dev), torch.empty((N, H, W, C), device=dev)
        lib.call('mmft_pool2x2_fwd', x, y, N, H, W, C, code, d, st)
        lib.call('mmft_pool2x2_bwd', x, gy, dx, N, H, W, C, code, d, st)
        yr = y64.detach().permute(0, 2, 3, 1)
        assert int(torch.isnan(yr).sum()) == 2
        assert torch.equal(torch.isnan(y).cpu(), torch.isnan(yr)) and torch.equal(torch.nan_to_num(y.double().cpu(), 9.0), torch.nan_to_num(yr, 9.0))
        assert torch.equal(dx.double().cpu(), x64.grad.permute(0, 2, 3, 1))


# --------------------------------------------------------------------------------------------- bilinear x2
@pytest.mark.parametrize('H,W', [(1, 1), (1, 5), (2, 3), (7, 9), (128, 3)])
def test_upsample_bilinear2x(dev, H, W):
    """mmft_upsample_bilinear2x_fwd / _bwd against F.interpolate(scale_factor=2, mode='bilinear', align_corners=True) in fp64
    and autograd, 1e-6 relative.  H = 128 is the largest the U-Net uses: no contributing output row may be dropped from the
    backward's candidate range, and the interpolation weight of source row 127 must still be good to 1e-6."""
    N, C = 2, 3
    x_h = det_uniform((N, H, W, C), 1)
    x, x64 = _nhwc(x_h, dev)
    gy_h = det_uniform((N, 2 * H, 2 * W, C), 2)
    gy = torch.from_numpy(gy_h).to(dev)
    y64 = F.interpolate(x64, scale_factor=2, mode='bilinear', align_corners=True)
    y64.backward(torch.from_numpy(gy_h).double().permute(0, 3, 1, 2))
    y = torch.full((N * 4 * H * W * C + 8,), SENT, device=dev)
    dx = torch.full((N * H * W * C + 8,), SENT, device=dev)
    d, st = lib.stream_args(x)
    lib.call('mmft_upsample_bilinear2x_fwd', x, y, N, H, W, C, d, st)
    lib.call('mmft_upsample_bilinear2x_bwd', gy, dx, N, H, W, C, d, st)
    assert bool((y[-8:] == SENT).all()) and bool((dx[-8:] == SENT).all())
    e1 = rel_err(y[:-8].reshape(N, 2 * H, 2 * W, C), y64.permute(0, 2, 3, 1))
    e2 = rel_err(dx[:-8].reshape(N, H, W, C), x64.grad.permute(0, 2, 3, 1))
    print(f'bilinear {H}x{W}: forward {e1:.3e}, backward {e2:.3e}')
    assert e1 < 1e-6 and e2 < 1e-6


# --------------------------------------------------------------------------------------------- data movement
SHUF = [(1, 3, 5, 3), (2, 5, 7, 8)]        # 180 and 2240 elements: no multiple of 256, one block and several


@pytest.mark.parametrize('N,H,W,Co', SHUF)
def test_pixel_shuffle_and_unshuffle(dev, N, H, W, Co):
    """mmft_pixel_shuffle2 / _into (ldc > Co, c_off > 0; bias and none) and mmft_pixel_unshuffle2 / _from: exact, and the bytes
    outside the written slice keep their sentinel."""
    inp_h = det_uniform((N, H, W, 4 * Co), 1)
    bias_h = det_uniform((Co,), 2)
    inp, bias = torch.from_numpy(inp_h).to(dev), torch.from_numpy(bias_h).to(dev)
    d, st = lib.stream_args(inp)

    def shuffled(b):
        v = inp_h.reshape(N, H, W, 2, 2, Co) + (b if b is not None else np.float32(0))
        return v.transpose(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, Co).astype(np.float32)
    n_out = N * 4 * H * W * Co
    for b_h, b in ((bias_h, bias), (None, None)):
        out = torch.full((n_out + 8,), SENT, device=dev)
        lib.call('mmft_pixel_shuffle2', inp, b, out, N, H, W, Co, d, st)
        assert np.array_equal(out[:n_out].cpu().numpy().reshape(N, 2 * H, 2 * W, Co), shuffled(b_h)) and bool((out[n_out:] == SENT).all())
        ldc, c_off = Co + 5, 2
        big = torch.full((N, 2 * H, 2 * W, ldc), SENT, device=dev)
        lib.call('mmft_pixel_shuffle2_into', inp, b, big, N, H, W, Co, ldc, c_off, d, st)
        exp = np.full((N, 2 * H, 2 * W, ldc), SENT, dtype=np.float32)
        exp[..., c_off:c_off + Co] = shuffled(b_h)
        assert np.array_equal(big.cpu().numpy(), exp)
    # unshuffle: the inverse move
    src_h = det_uniform((N, 2 * H, 2 * W, Co), 3)
    unsh = src_h.reshape(N, H, 2, W, 2, Co).transpose(0, 1, 3, 2, 4, 5).reshape(N, H, W, 4 * Co)
    out = torch.full((n_out + 8,), SENT, device=dev)
    lib.call('mmft_pixel_unshuffle2', torch.from_numpy(src_h).to(dev), out, N, H, W, Co, d, st)
    assert np.array_equal(out[:n_out].cpu().numpy().reshape(N, H, W, 4 * Co), unsh) and bool((out[n_out:] == SENT).all())
    ldc, c_off = Co + 5, 3
    big_h = det_uniform((N, 2 * H, 2 * W, ldc), 4)
    big_h[..., c_off:c_off + Co] = src_h
    out = torch.full((n_out + 8,), SENT, device=dev)
    lib.call('mmft_pixel_unshuffle2_from', torch.from_numpy(big_h).to(dev), out, N, H, W, Co, ldc, c_off, d, st)
    assert np.array_equal(out[:n_out].cpu().numpy().reshape(N, H, W, 4 * Co), unsh) and bool((out[n_out:] == SENT).all())


@pytest.mark.parametrize('reverse', [0, 1])
def test_copy_region_nhwc(dev, reverse):
    """mmft_copy_region_nhwc with channel, row and column offsets, both directions; everything outside the region keeps its
    value.  1 * 3 * 5 * 7 = 105 and 2 * 9 * 11 * 6 = 1188 elements: no multiples of 256."""
    for (N, Hs, Ws, Cs, Hd, Wd, Cd, c_off, y_off, x_off) in ((1, 3, 5, 7, 4, 9, 12, 5, 1, 4), (2, 9, 11, 6, 12, 11, 8, 1, 3, 0)):
        src_h, dst_h = det_uniform((N, Hs, Ws, Cs), 1), det_uniform((N, Hd, Wd, Cd), 2)
        src, dst = torch.from_numpy(src_h).to(dev), torch.from_numpy(dst_h).to(dev)
        d, st = lib.stream_args(src)
        lib.call('mmft_copy_region_nhwc', src, N, Hs, Ws, Cs, dst, Hd, Wd, Cd, c_off, y_off, x_off, reverse, d, st)
        if reverse:
            assert np.array_equal(src.cpu().numpy(), dst_h[:, y_off:y_off + Hs, x_off:x_off + Ws, c_off:c_off + Cs])
            assert np.array_equal(dst.cpu().numpy(), dst_h)
        else:
            exp = dst_h.copy()
            exp[:, y_off:y_off + Hs, x_off:x_off + Ws, c_off:c_off + Cs] = src_h
            assert np.array_equal(dst.cpu().numpy(), exp) and np.array_equal(src.cpu().numpy(), src_h)


@pytest.mark.parametrize('N,C,H,W,Cpad', [(1, 3, 5, 7, 3), (2, 3, 5, 7, 4), (2, 5, 9, 13, 16)])
def test_layout_nchw_nhwc(dev, N, C, H, W, Cpad):
    """mmft_nchw_to_nhwc (zero-filled padding channels when Cpad > C) and mmft_nhwc_to_nchw (padding channels dropped): exact,
    sentinels behind both outputs survive.  105, 280 and 1872 padded elements: no multiples of 256."""
    a_h = det_uniform((N, C, H, W), 1)
    a = torch.from_numpy(a_h).to(dev)
    n_pad = N * H * W * Cpad
    out = torch.full((n_pad + 8,), SENT, device=dev)
    d, st = lib.stream_args(a)
    lib.call('mmft_nchw_to_nhwc', a, out, N, C, H, W, Cpad, d, st)
    exp = np.zeros((N, H, W, Cpad), dtype=np.float32)
    exp[..., :C] = a_h.transpose(0, 2, 3, 1)
    assert np.array_equal(out[:n_pad].cpu().numpy().reshape(N, H, W, Cpad), exp) and bool((out[n_pad:] == SENT).all())
    b_h = det_uniform((N, H, W, Cpad), 2)
    back = torch.full((N * C * H * W + 8,), SENT, device=dev)
    lib.call('mmft_nhwc_to_nchw', torch.from_numpy(b_h).to(dev), back, N, C, H, W, Cpad, d, st)
    assert np.array_equal(back[:N * C * H * W].cpu().numpy().reshape(N, C, H, W), b_h[..., :C].transpose(0, 3, 1, 2))
    assert bool((back[N * C * H * W:] == SENT).all())
