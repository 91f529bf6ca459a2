"""The image gradient of mmft.sensitivity without a GPU: the ledger of include/mmft_sens_image.h (the rules test_sens_cpu.py
applies to include/mmft_sens.h), the host-side refusals of its two entry points - every one of them comes before the device
is looked at - the plain oracle of tests/sens_image_oracle.py against the fixtures the REFERENCE's module produced
(tests/golden/make_golden_eval_grad.py) and against central differences of the eval forward, and the refusals of
Sensitivity(image=True) that need no device."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from abi_ledger import call_sites, declared as _declared, others
from conftest import rel_err
from mmft import lib
from mmft.detrand import det_uniform, det_state_dict
import sens_image_oracle as SI
import unet_eval_oracle as E

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
NAMES = ['mmft_u16_conv3x3_dgrad_image', 'mmft_u16_frozen_bwd']
NARGS = {'mmft_u16_frozen_bwd': 16, 'mmft_u16_conv3x3_dgrad_image': 8}
OTHER_HEADERS = others('mmft_sens_image.h')
FIXTURES = [('max', 8, 32, 2), ('avg', 16, 64, 1)]


# ------------------------------------------------------------------------------------------------ the ledger
def test_image_header_declares_exactly_the_two_names_and_overlaps_no_other_header():
    hd = _declared('mmft_sens_image.h')
    decls = lib.simg_decls()
    assert sorted(hd) == NAMES == sorted(decls)
    assert {n: len(decls[n][1]) for n in NAMES} == hd == NARGS
    for other in OTHER_HEADERS:
        assert not set(hd) & set(_declared(other)), other
    assert sorted(_declared('mmft_sens.h')) == ['mmft_mlp2_feat_dx_bf16']                 # the neighbouring header is what it was
    for used in ('mmft_u16_outconv_bwd', 'mmft_u16_conv3x3', 'mmft_u16_convt_dgrad', 'mmft_u16_pool_bwd'):
        assert used in _declared('mmft.h')                                                # the rest of the walk lives there
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert decls['mmft_u16_frozen_bwd'] == (I, [P, I, P, I, P, P, P, F, P, I, I, I, I, I, I, P])
    assert decls['mmft_u16_conv3x3_dgrad_image'] == (I, [P, P, P, I, I, I, I, P])
    for foreign in ('mmft_version', 'mmft_u16_pool_bwd', 'mmft_mlp2_feat_dx_bf16'):
        with pytest.raises(RuntimeError, match='not declared'):
            lib.simg(foreign)
    # the accessor's name is its own: the ledgers match call sites by attribute name
    assert lib.simg not in (lib.call, lib.query, lib.ext, lib.place, lib.incr, lib.crit, lib.head, lib.csum, lib.sens)


def test_every_simg_call_site_matches_the_header():
    protos = _declared('mmft_sens_image.h')
    checked, bad, seen, product = 0, [], set(), set()
    for name, n, f, lineno in call_sites('simg'):
        if n is None or name not in protos:                         # (a list built elsewhere; the refusal test above)
            continue
        checked += 1
        seen.add(name)
        if os.sep + 'mmft' + os.sep in f:
            product.add(name)
        if protos.get(name) != n:
            bad.append((name, protos.get(name), n, f, lineno))
    assert checked >= 2 and seen == set(NAMES) and product == set(NAMES) and not bad, bad


# ------------------------------------------------------------------------------------------------ host-side refusals
def _fb(**change):
    """A full argument list of mmft_u16_frozen_bwd made of host integers: nothing can be launched on it, and nothing is."""
    a = dict(a=64, lda=32, g=128, ldg=32, gp=None, gamma=192, running_var=256, eps=1e-5, dz=320, N=1, H=8, W=32, C=16, pool_mode=0,
             device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def _di(**change):
    a = dict(dz1=64, w=128, dx=192, N=1, H=8, W=32, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def test_the_built_library_exports_the_names_and_refuses_bad_arguments_on_the_host():
    L = lib.load()
    assert not [n for n in NAMES if not hasattr(L, n)]
    assert L.mmft_version() >= 209
    assert len(_fb()) == NARGS['mmft_u16_frozen_bwd'] and len(_di()) == NARGS['mmft_u16_conv3x3_dgrad_image']
    refused = dict(null_a=dict(a=None), null_g=dict(g=None), null_gamma=dict(gamma=None), null_rv=dict(running_var=None),
                   null_dz=dict(dz=None), c8=dict(C=8), c24=dict(C=24, lda=24, ldg=24), c48=dict(C=48, lda=48, ldg=48),
                   c256=dict(C=256, lda=256, ldg=256), c0=dict(C=0), short_a_pitch=dict(lda=8), odd_a_pitch=dict(lda=20),
                   short_g_pitch=dict(ldg=8), odd_g_pitch=dict(ldg=20), odd_a=dict(a=66), odd_g=dict(g=136), odd_dz=dict(dz=322),
                   odd_gp=dict(gp=392), h0=dict(H=0), w0=dict(W=0), h_neg=dict(H=-8), n_neg=dict(N=-1),
                   pooled_odd_h=dict(gp=384, H=7), pooled_odd_w=dict(gp=384, W=31), pooled_mode2=dict(gp=384, pool_mode=2),
                   pooled_mode_neg=dict(gp=384, pool_mode=-1), pooled_short_skip_pitch=dict(gp=384, ldg=8))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_u16_frozen_bwd failed \(-1\): u16_frozen_bwd'):
            lib.simg('mmft_u16_frozen_bwd', *_fb(**change))
    # N == 0 returns 0 and looks at no pointer - but its sizes are still judged
    assert lib.simg('mmft_u16_frozen_bwd', *_fb(N=0)) == 0
    assert lib.simg('mmft_u16_frozen_bwd', *_fb(N=0, a=None, g=None, gamma=None, running_var=None, dz=None)) == 0
    assert lib.simg('mmft_u16_frozen_bwd', *_fb(N=0, gp=384, pool_mode=1)) == 0
    with pytest.raises(RuntimeError, match='bad sizes'):
        lib.simg('mmft_u16_frozen_bwd', *_fb(N=0, C=24, lda=24, ldg=24))
    refused = dict(null_dz1=dict(dz1=None), null_w=dict(w=None), null_dx=dict(dx=None), odd_dz1=dict(dz1=72), odd_w=dict(w=130),
                   odd_dx=dict(dx=194), h4=dict(H=4), h12=dict(H=12), h0=dict(H=0), w16=dict(W=16), w48=dict(W=48), w0=dict(W=0),
                   n_neg=dict(N=-1))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_u16_conv3x3_dgrad_image failed \(-1\): u16_conv3x3_dgrad_image'):
            lib.simg('mmft_u16_conv3x3_dgrad_image', *_di(**change))
    assert lib.simg('mmft_u16_conv3x3_dgrad_image', *_di(N=0)) == 0
    assert lib.simg('mmft_u16_conv3x3_dgrad_image', *_di(N=0, dz1=None, w=None, dx=None)) == 0
    with pytest.raises(RuntimeError, match='bad sizes'):
        lib.simg('mmft_u16_conv3x3_dgrad_image', *_di(N=0, W=48))


# ------------------------------------------------------------------------------------------------ the plain oracle
def grad_fixture(pooling, H, W, N):
    """(fixture, state_dict, input) exactly as make_golden_eval_grad.py built them."""
    import Unet
    g = np.load(os.path.join(GOLD, f'unet_eval_input_grad_{pooling}_{H}x{W}_n{N}.npz'))
    seed = int(g['seed'])
    sd = det_state_dict(Unet.UNet(pooling), seed)
    sd['outc.conv.0.bias'] = torch.full((1,), float(g['outc_bias']))
    x = torch.from_numpy(det_uniform((N, 3, H, W), seed + 100, 0.0, 1.0))
    return g, sd, x


@pytest.mark.parametrize('pooling,H,W,N', FIXTURES)
def test_plain_oracle_matches_the_reference_input_gradient(pooling, H, W, N):
    """unet_eval_vjp without rounding, on its own forward's activations, against autograd of the reference's module in eval
    mode: 2e-6 in fp32 (make_golden.py's bar; the script that wrote the fixtures also held fp64 to 1e-12)."""
    g, sd, x = grad_fixture(pooling, H, W, N)
    dx, gout = torch.from_numpy(g['dx']), torch.from_numpy(g['gout'])
    assert dx.shape == (N, 3, H, W) and gout.shape == (N, 1, H // 2, W // 2) and sorted(g.files) == ['dx', 'gout', 'outc_bias', 'seed']
    assert float((dx != 0).double().mean()) == 1.0 and all(float(dx[i].abs().max()) > 1e-3 for i in range(N))
    errs = {}
    for dtype in (torch.float32, torch.float64):
        p = E.cast_state(sd, dtype)
        out, acts = SI.unet_eval_acts(p, x.to(dtype), pooling)
        assert torch.equal(out, E.unet_eval_forward(p, x.to(dtype), pooling))                # the same forward
        errs[dtype] = rel_err(SI.unet_eval_vjp(p, acts, gout, pooling, dtype), dx)
    print(f'\nunet eval input gradient {pooling} {H}x{W} N={N}: plain oracle vs reference fp32 {errs[torch.float32]:.2e}, '
          f'fp64 {errs[torch.float64]:.2e}')
    assert errs[torch.float32] <= 2e-6 and errs[torch.float64] <= 2e-6


@pytest.mark.parametrize('pooling', ['max', 'avg'])
def test_plain_oracle_agrees_with_central_differences(pooling):
    """fp64, 1 x 8 x 32, three seeded directions v: <dx, v> against (J(x + h v) - J(x - h v)) / 2h, J = sum(out * gout),
    h = 1e-6.  J is piecewise linear in x, so away from a ReLU / max-pool boundary the difference quotient is exact up to
    cancellation: ~1e-16 |J| / h = 1e-10 relative to the terms of the dot product; the bar of 1e-6 of sum |dx| |v| is
    test_sens_cpu.py's bar for the same comparison."""
    _, sd, _ = grad_fixture(pooling, *[f for f in FIXTURES if f[0] == pooling][0][1:])
    p = E.cast_state(sd, torch.float64)
    x = torch.from_numpy(det_uniform((1, 3, 8, 32), 77, 0.0, 1.0)).double()
    out, acts = SI.unet_eval_acts(p, x, pooling)
    gout = torch.from_numpy(det_uniform(tuple(out.shape), 78, -1.0, 1.0)).double()
    dx = SI.unet_eval_vjp(p, acts, gout, pooling)
    assert float((out > 0).double().mean()) > 0.2 and float(dx.abs().max()) > 0
    J = lambda t: float((E.unet_eval_forward(p, t, pooling) * gout).sum())
    h, worst = 1e-6, 0.0
    for k in range(3):
        v = torch.from_numpy(det_uniform(tuple(x.shape), 80 + k, -1.0, 1.0)).double()
        fd, an = (J(x + h * v) - J(x - h * v)) / (2 * h), float((dx * v).sum())
        worst = max(worst, abs(fd - an) / float((dx.abs() * v.abs()).sum()))
    print(f'\n{pooling}: central differences vs <dx, v>, worst of three directions {worst:.2e}')
    assert worst < 1e-6, worst


def test_rounded_walk_is_linear_in_gout_only_through_its_roundings():
    """On given activations the unrounded walk is linear in gout (to fp64 rounding); the bf16 walk differs from it by its
    roundings - a few bf16 steps, not more - and the 'operands' ablation lies between the two."""
    g, sd, x = grad_fixture('max', 8, 32, 2)
    p = E.cast_state(sd, torch.float64)
    _, acts = SI.unet_eval_acts(p, x.double(), 'max', 'bf16')
    gout = torch.from_numpy(g['gout']).double()
    plain = SI.unet_eval_vjp(p, acts, gout, 'max')
    assert rel_err(SI.unet_eval_vjp(p, acts, 2.0 * gout, 'max'), 2.0 * plain) < 1e-12
    e_bf, e_op = (rel_err(SI.unet_eval_vjp(p, acts, gout, 'max', rounding=r), plain) for r in ('bf16', 'operands'))
    print(f'\nbf16 walk vs unrounded walk on the same activations {e_bf:.2e}, operands only {e_op:.2e}')
    assert 0 < e_op < e_bf < 5e-2
    with pytest.raises(ValueError, match='unknown rounding'):
        SI.unet_eval_vjp(p, acts, gout, 'max', rounding='fp8')


# ------------------------------------------------------------------------------------------------ Sensitivity's refusals
def test_sensitivity_refuses_on_the_host_what_has_no_image_gradient():
    """image=True: no CNN, no masked projection (at construction); fp32 mode, a net that is not the U-Net, batch statistics,
    a shape outside the fused eval path (at run(), before anything is launched) - functions that touch no device."""
    import Unet
    from mmft import sensitivity as S
    from mmft.train import build_models
    pm, layoutnet = build_models(map_size=16, device='cpu', seed=9294, unet=False)
    unet = Unet.UNet('max')
    S.check_image_model(pm, unet)
    with pytest.raises(ValueError, match='no CNN'):
        S.check_image_model(pm, None)
    with pytest.raises(ValueError, match='no CNN'):
        S.Sensitivity(pm, None, [], 'cpu', image=True)                   # right after check_model, before any device work
    with pytest.raises(ValueError, match='no masked projection'):
        S.check_image_model(types.SimpleNamespace(fcn=None), unet)
    img = torch.zeros(1, 3, 64, 64)
    assert lib.get_math_mode() == 'f32'
    with pytest.raises(ValueError, match='fp32'):
        S.check_image_route(unet, img, True)
    with lib.math_mode('bf16'):
        if layoutnet is not None:
            with pytest.raises(ValueError, match='not the U-Net'):
                S.check_image_route(layoutnet, img, True)
        with pytest.raises(ValueError, match='not the U-Net'):
            S.check_image_route(torch.nn.Conv2d(3, 1, 1), img, True)
        unet.train()
        with pytest.raises(ValueError, match='batch statistics'):
            S.check_image_route(unet, img, False)
        # frozen statistics: the route is judged in the modes run() would set, and the modes come back as they were
        with pytest.raises(ValueError, match='outside the fused eval path'):
            S.check_image_route(unet, img, True)                          # a host tensor: unet16.supported says no
        assert all(m.training for m in unet.modules())
        unet.eval()
        with pytest.raises(ValueError, match='outside the fused eval path'):
            S.check_image_route(unet, torch.zeros(1, 3, 37, 45), False)
        assert not any(m.training for m in unet.modules())
    assert lib.get_math_mode() == 'f32'
