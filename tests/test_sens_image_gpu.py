"""The image gradient of mmft.sensitivity on the GPU (include/mmft_sens_image.h, mmft.unet16.unet_eval_input_grad,
Sensitivity(image=True)).

Kernels.  mmft_u16_frozen_bwd bit for bit against a torch fp32 restatement on operands whose products are exact, and within
ONE bf16 rounding on arbitrary data (the rule of test_eval_conv_arbitrary_data_within_one_rounding: 2^-8 of the element plus
1e-6 of the tensor's scale for the fp32 sum and product in front of the rounding).  mmft_u16_conv3x3_dgrad_image exact on
small-integer operands and under the non-representable bar of tests/test_bf16_gpu.py (TOL) on arbitrary ones.

The chain.  unet_eval_input_grad against tests/sens_image_oracle.unet_eval_vjp fed the HIP run's OWN tape: every ReLU mask
and pooling argmax is then the HIP run's, the walk is linear in gout, and the project's decoupled gradient row applies, all
distances in max-norm rel_err to the fp64 rounding oracle:  e_hip <= max(1.5e-3, 3 e_32),  e_hip <= 5e-3,  teeth
e_plain > 10 x bound (the plain fp64 reference on its own forward), and the walk WITHOUT the gradient roundings must exceed
the bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from mmft import lib, ops, unet16
import sens_image_oracle as SI
import unet_eval_oracle as E
from test_bf16_gpu import TOL
from test_unet_eval_gpu import assert_unchanged, profiled, recipe_a_hip, snapshot

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FLOOR, CEILING, K, TEETH = 1.5e-3, 5e-3, 3.0, 10.0
SENTINEL, GUARD = 7.0, 64
FWD_LAUNCHES = {'u16_pack_kernel': 1, 'u16_conv3x3_eval_kernel': 14, 'u16_convt_fwd_kernel': 3, 'u16_outconv_fwd_kernel': 1}
BWD_LAUNCHES = {'u16_outconv_bwd_kernel': 1, 'u16_frozen_bwd_kernel': 11, 'u16_frozen_bwd_pool_kernel': 3, 'u16_conv3x3_kernel': 13,
                'u16_convt_dgrad_kernel': 3, 'u16_conv3x3_dgrad_image_kernel': 1}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


# ------------------------------------------------------------------------------------------------ the frozen backward kernel
def grid(shape, gen, step, lo, hi):
    """Multiples of `step` in [lo, hi], fp32."""
    return torch.randint(int(round(lo / step)), int(round(hi / step)) + 1, shape, generator=gen).float() * step


def frozen_case(N, H, W, C, form, seed, exact):
    """Host operands (fp32 values that bf16 holds exactly; NHWC) of one launch: a, g, gp (or None), gamma, rv, eps."""
    gen = torch.Generator().manual_seed(seed)
    if exact:
        a = grid((N, H, W, C), gen, 0.125, -1.0, 2.0).clamp_(min=0.0)       # exact zeros, few values: ties in every window
        a[0, H // 2, W // 3, C // 2] = float('nan')
        g = grid((N, H, W, C), gen, 0.0625, -4.0, 4.0)
        gp = grid((N, H // 2, W // 2, C), gen, 0.0625, -4.0, 4.0)
        gamma = (2.0 ** torch.randint(-2, 3, (C,), generator=gen).float()) * (torch.randint(0, 2, (C,), generator=gen).float() * 2 - 1)
        rv = 4.0 ** torch.randint(-1, 3, (C,), generator=gen).float()        # 0.25, 1, 4, 16
        eps = 0.0
    else:
        a = torch.relu(torch.randn((N, H, W, C), generator=gen)).to(BF).float()
        g = torch.randn((N, H, W, C), generator=gen).to(BF).float()
        gp = torch.randn((N, H // 2, W // 2, C), generator=gen).to(BF).float()
        gamma = torch.randn(C, generator=gen) * 0.7 + 1.0
        rv = torch.rand(C, generator=gen) + 0.5
        eps = E.EPS
    return a, g, (gp if form != 'plain' else None), gamma, rv, eps


def frozen_reference(a, g, gp, gamma, rv, eps, form, dtype):
    """The restatement: scale by the kernel's fp32 sequence, then (g + route(gp)) * scale under the mask a > 0, in `dtype`
    (fp32: the kernel's own operations, one at a time; fp64: the unrounded value)."""
    invstd = torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(rv + torch.tensor(eps, dtype=torch.float32))
    scale = (gamma * invstd).to(dtype)
    s = g.to(dtype)
    if form != 'plain':
        an, gpn = a.permute(0, 3, 1, 2), gp.to(dtype).permute(0, 3, 1, 2)
        if form == 'max':
            _, idx = F.max_pool2d(an, 2, return_indices=True)               # torch's rule: first maximum, a NaN wins
            routed = F.max_unpool2d(gpn.contiguous(), idx, 2, output_size=an.shape[2:])
        else:
            routed = 0.25 * gpn.repeat_interleave(2, 2).repeat_interleave(2, 3)
        s = s + routed.permute(0, 2, 3, 1)
    return torch.where(a > 0, s * scale, torch.zeros((), dtype=dtype))


def run_frozen(dev, a, g, gp, gamma, rv, eps, form, pitched=True):
    """mmft_u16_frozen_bwd; a and g sit in the first C channels of buffers of pitch 2C, dz between two guard zones."""
    N, H, W, C = a.shape
    ld = 2 * C if pitched else C
    ab = torch.full((N, H, W, ld), SENTINEL, dtype=BF)
    gb = torch.full((N, H, W, ld), SENTINEL, dtype=BF)
    ab[..., :C], gb[..., :C] = a.to(BF), g.to(BF)
    ab, gb = ab.to(dev), gb.to(dev)
    gpd = gp.to(BF).to(dev) if gp is not None else None
    n = N * H * W * C
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=BF, device=dev)
    dz = buf[GUARD:GUARD + n]
    d, s = lib.stream_args(buf)
    lib.simg('mmft_u16_frozen_bwd', ab, ld, gb, ld, gpd, gamma.to(dev), rv.to(dev), float(eps), dz, N, H, W, C,
             ops.POOL_AVG if form == 'avg' else ops.POOL_MAX, d, s)
    torch.cuda.synchronize()
    guards = torch.cat([buf[:GUARD], buf[GUARD + n:]]).float().cpu()
    assert bool((guards == SENTINEL).all()), 'written outside dz'
    assert bool((ab[..., C:].float() == SENTINEL).all()) and bool((gb[..., C:].float() == SENTINEL).all())
    return dz.cpu().reshape(N, H, W, C)


def check_frozen(dev, N, H, W, C, form, seed):
    # 1. bit for bit where every fp32 operation of the kernel is exact or a single rounding
    ops_ = frozen_case(N, H, W, C, form, seed, exact=True)
    want = frozen_reference(*ops_, form, torch.float32).to(BF)
    got = run_frozen(dev, *ops_, form)
    assert torch.equal(_bits(got), _bits(want)), (N, H, W, C, form)
    assert float((want.float() != 0).float().mean()) > 0.2
    assert torch.equal(_bits(run_frozen(dev, *ops_, form)), _bits(got))                 # same inputs, same bits
    # 2. arbitrary data: within one bf16 rounding of the unrounded value
    ops_ = frozen_case(N, H, W, C, form, seed + 1, exact=False)
    ref = frozen_reference(*ops_, form, torch.float64)
    got = run_frozen(dev, *ops_, form).double()
    worst = float(((got - ref).abs() / ((2.0 ** -8) * ref.abs() + 1e-6 * float(ref.abs().max()))).max())
    return worst


@pytest.mark.parametrize('form', ['plain', 'max', 'avg'])
@pytest.mark.parametrize('C', [16, 32, 64, 128])
def test_frozen_backward_kernel(dev, C, form):
    """Both forms on (1, 8, 32) and (2, 16, 32), a and g at pitch 2C: bitwise on exact operands (eps = 0, running_var in
    {0.25, 1, 4, 16}, gamma a power of two, g / gskip / gp multiples of 2^-4, activations with exact zeros, ties in the
    pooling windows and one NaN), within one rounding on arbitrary data, two launches bitwise equal, nothing written around
    dz or into the unused half of the pitch."""
    for k, (N, H, W) in enumerate([(1, 8, 32), (2, 16, 32)]):
        worst = check_frozen(dev, N, H, W, C, form, 100 * C + 10 * k)
        print(f'\nfrozen_bwd C {C} {form} {N}x{H}x{W}: arbitrary data, error / one-rounding bound {worst:.3f}')
        assert worst <= 1.0, worst


@pytest.mark.parametrize('form,C,N,H,W', [('plain', 16, 1, 264, 1024), ('max', 64, 1, 528, 512)])
def test_frozen_backward_kernel_above_the_grid_cap(dev, form, C, N, H, W):
    """The element-wise grid is capped at 2048 workgroups of 256 items (ew_grid): 540 672 items - (pixels or windows) x
    groups of 8 channels - need the grid-stride loop, in which a thread must keep its channel group."""
    items = N * H * W * (C // 8) // (1 if form == 'plain' else 4)
    assert items > 2048 * 256
    ops_ = frozen_case(N, H, W, C, form, 5, exact=True)
    want = frozen_reference(*ops_, form, torch.float32).to(BF)
    got = run_frozen(dev, *ops_, form, pitched=False)
    assert torch.equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------------ the image gradient kernel
def run_dgrad_image(dev, dz, w):
    """dz (N,16,H,W), w (16,3,3,3) on the host -> dx (N,3,H,W) fp32 from two launches (asserted bitwise equal)."""
    N, _, H, W = dz.shape
    dzd = dz.permute(0, 2, 3, 1).contiguous().to(BF).to(dev)
    wd = w.float().to(dev).contiguous(memory_format=torch.channels_last)
    outs = []
    for _ in range(2):
        dx = torch.full((N, 3, H, W), SENTINEL, dtype=torch.float32, device=dev)
        d, s = lib.stream_args(dx)
        lib.simg('mmft_u16_conv3x3_dgrad_image', dzd, wd, dx, N, H, W, d, s)
        outs.append(dx)
    torch.cuda.synchronize()
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    return outs[0].cpu()


@pytest.mark.parametrize('N,H,W', [(1, 8, 32), (2, 16, 64), (1, 40, 96)])
def test_image_gradient_kernel(dev, N, H, W):
    """One tile with all four borders, several tiles with the seam between two images, a grid of 5 x 3 tiles.  Small-integer
    operands (dz in -4 .. 4, w multiples of 2^-3 in +-1: every partial sum is exact in fp32) against
    torch.nn.grad.conv2d_input in fp64 to 1e-6; arbitrary operands against fp64 math on the bf16-rounded operands under TOL."""
    gen = torch.Generator().manual_seed(N * 1000 + H + W)
    dz = torch.randint(-4, 5, (N, 16, H, W), generator=gen).double()
    w = torch.randint(-8, 9, (16, 3, 3, 3), generator=gen).double() * 0.125
    ref = torch.nn.grad.conv2d_input((N, 3, H, W), w, dz, padding=1)
    e_exact = rel_err(run_dgrad_image(dev, dz, w), ref)
    dz = torch.randn((N, 16, H, W), generator=gen).to(BF).double()
    w = (torch.randn((16, 3, 3, 3), generator=gen) / 12.0).float()
    ref = torch.nn.grad.conv2d_input((N, 3, H, W), w.to(BF).double(), dz, padding=1)
    e_arb = rel_err(run_dgrad_image(dev, dz, w), ref)
    print(f'\ndgrad_image {N}x{H}x{W}: small integers {e_exact:.2e} (bar 1e-6), arbitrary {e_arb:.2e} (bar {TOL:.0e})')
    assert e_exact <= 1e-6 and e_arb < TOL


# ------------------------------------------------------------------------------------------------ the chain on the HIP run's tape
def chain_rows(title, dx, sd, x, acts, gout, pooling, teeth=True):
    """The rows of the module docstring for one image gradient; prints every figure before it judges.  acts: the HIP tape's
    activations as {i: (N,C,H,W) fp64}; x, gout on the host."""
    p64, p32 = E.cast_state(sd, torch.float64), E.cast_state(sd, torch.float32)
    o64 = SI.unet_eval_vjp(p64, acts, gout.double(), pooling, torch.float64, 'bf16')
    o32 = SI.unet_eval_vjp(p32, {i: t.float() for i, t in acts.items()}, gout.float(), pooling, torch.float32, 'bf16')
    onr = SI.unet_eval_vjp(p64, acts, gout.double(), pooling, torch.float64, 'operands')
    _, own = SI.unet_eval_acts(p64, x.double(), pooling)
    op = SI.unet_eval_vjp(p64, own, gout.double(), pooling)
    e_hip, e_32, e_plain, e_nr = (rel_err(t, o64) for t in (dx, o32, op, onr))
    bound = max(FLOOR, K * e_32)
    print(f'\n== {title}: e_hip {e_hip:.2e}  e_32 {e_32:.2e}  e_plain {e_plain:.2e}  unrounded-backward {e_nr:.2e}  bound {bound:.2e}')
    bad = []
    if not float(o64.abs().max()) > 0:
        bad.append('the reference gradient is zero')
    if e_hip > bound:
        bad.append(f'e_hip {e_hip:.3e} > bound {bound:.3e}')
    if e_hip > CEILING:
        bad.append(f'e_hip {e_hip:.3e} > ceiling {CEILING:.3e}')
    if teeth and not e_plain > TEETH * bound:
        bad.append(f'no teeth: e_plain {e_plain:.3e} <= {TEETH} x bound {bound:.3e}')
    if teeth and not e_nr > bound:
        bad.append(f'no teeth: the walk without gradient roundings {e_nr:.3e} <= bound {bound:.3e}')
    assert not bad, bad
    return e_hip


@pytest.mark.parametrize('N,H,W,pooling', [(2, 64, 64, 'max'), (1, 40, 96, 'avg'), (2, 8, 32, 'max')])
def test_eval_input_gradient_vs_rounding_oracle_on_its_own_tape(dev, N, H, W, pooling):
    """recipe_a_hip nets; the taped forward is the eval forward (19 launches, the same bits), the gradient is 32 launches,
    none of them a BatchNorm backward, a pooling backward, a weight gradient, a slab reduction or a weight pack; nothing of
    the model is written; the result against the rounding oracle on the tape's activations.
    Measured on one MI355X (e_hip / e_32 / e_plain / unrounded backward / bound):
      2 x 64 x 64 max   9.73e-4 / 9.73e-4 / 4.47e-1 / 6.26e-3 / 2.92e-3
      1 x 40 x 96 avg   9.08e-4 / 9.08e-4 / 1.80e-1 / 5.44e-3 / 2.72e-3
      2 x 8 x 32 max    1.05e-7 / 1.53e-4 / 1.52e-1 / 7.17e-3 / 1.50e-3
    (where e_hip equals e_32 the kernels and the fp32 oracle crossed the same bf16 rounding boundary.)"""
    net, x, sd = recipe_a_hip(dev, N, H, W, pooling)
    xd = x.to(dev)
    gout = torch.rand((N, 1, H // 2, W // 2), generator=torch.Generator().manual_seed(21)) * 2 - 1
    before = snapshot(net)
    with lib.math_mode('bf16'), torch.no_grad():
        y = net(xd)
        (out, tape), cf = profiled(lambda: unet16.unet_forward_eval_taped(net, xd))
        dx, cb = profiled(lambda: unet16.unet_eval_input_grad(net, tape, gout.to(dev)))
        dx2 = unet16.unet_eval_input_grad(net, tape, gout.to(dev))
        torch.cuda.synchronize()
    print(f'\ntaped forward: {cf}\ninput gradient: {cb}')
    assert cf == FWD_LAUNCHES and sum(cf.values()) == 19, cf
    assert cb == BWD_LAUNCHES and sum(cb.values()) == 32, cb
    assert torch.equal(_bits(out), _bits(y))
    assert dx.shape == (N, 3, H, W) and dx.dtype == torch.float32 and torch.equal(_bits(dx), _bits(dx2))
    assert_unchanged(net, before, 'taped forward + input gradient')
    assert sorted(tape.acts) == sorted(name for name, _ in unet16._eval_sizes(N, H, W))
    chain_rows(f'{N}x{H}x{W} {pooling}', dx, sd, x, SI.acts_from_tape(tape.acts), gout, pooling)


def test_eval_input_gradient_refuses_a_stale_or_foreign_tape(dev):
    net, x, _ = recipe_a_hip(dev, 1, 8, 32, 'max')
    other, _, _ = recipe_a_hip(dev, 1, 8, 32, 'max')
    g = torch.zeros(1, 1, 4, 16, device=dev)
    with lib.math_mode('bf16'), torch.no_grad():
        _, tape = unet16.unet_forward_eval_taped(net, x.to(dev))
        with pytest.raises(ValueError, match='another network'):
            unet16.unet_eval_input_grad(other, tape, g)
        for bad in (torch.zeros(1, 1, 4, 8, device=dev), g.double(), g.cpu()):
            with pytest.raises(ValueError, match='gout must be'):
                unet16.unet_eval_input_grad(net, tape, bad)
        assert float(unet16.unet_eval_input_grad(net, tape, g).abs().max()) == 0.0      # zero in, exactly zero out
        net.up2.up.weight.add_(0.0)                                                     # written after the forward
        with pytest.raises(ValueError, match='moved or were written'):
            unet16.unet_eval_input_grad(net, tape, g)
    with lib.math_mode('bf16'), pytest.raises(NotImplementedError, match='no_grad'):
        net(x.to(dev))                                                                  # UNet.forward is what it was


# ------------------------------------------------------------------------------------------------ end to end
from test_sens_gpu import SEED, _design, _models, _same_snapshot, _snapshot, _weights        # noqa: E402


def feat_rows(title, hip, d, ids, state, fm, w):
    """d J / d feature map against oracle_feat_grad on the run's own feature map, the same row as the chain."""
    o64, o32, op = (SI.oracle_feat_grad(d, ids, state, fm, w, dtype=dt, rounding=rd)
                    for rd, dt in (('bf16', torch.float64), ('bf16', torch.float32), (None, torch.float64)))
    e_hip, e_32, e_plain = (rel_err(t, o64['feat']) for t in (hip, o32['feat'], op['feat']))
    bound = max(FLOOR, K * e_32)
    print(f'\n== {title}: feat_grad  e_hip {e_hip:.2e}  e_32 {e_32:.2e}  e_plain {e_plain:.2e}  bound {bound:.2e}')
    assert float(o64['feat'].abs().max()) > 0
    assert e_hip <= bound and e_hip <= CEILING, (e_hip, bound)
    assert e_plain > TEETH * bound, (e_plain, bound)


@pytest.mark.parametrize('fanin', ['regular', 'irregular'])
def test_sensitivity_image_gradient_end_to_end(dev, fanin):
    """Sensitivity(image=True).run() on synth_design(N=2048, L=16, tile=32): pred and the cell_feat / net_feat gradients are
    bitwise those of image=False; feat_grad meets the oracle row on the run's own feature map; grads[0]['image'] is bitwise
    what unet_eval_input_grad returns for feat_grad on a tape of the same forward, and meets the chain row; two runs give
    the same bits; nothing of the model is written.
    Measured on one MI355X, regular / irregular: feat_grad e_hip 2.64e-7 / 1.57e-7 (e_32 3.28e-7 / 1.14e-7, e_plain 6.41e-2 /
    2.15e-2); image gradient e_hip 4.57e-8 / 2.07e-4 (e_32 7.45e-8 / 2.07e-4)."""
    from mmft.evaluate import frozen_statistics
    from mmft.sensitivity import Sensitivity
    d = _design(fanin)
    ids = list(range(d.num_paths))
    w = _weights(d.num_paths)
    pmodel, cnn, state = _models(d, dev)
    with lib.math_mode('bf16'):
        s0 = Sensitivity(pmodel, cnn, [d], dev)
        s1 = Sensitivity(pmodel, cnn, [d], dev, image=True)
        snap = _snapshot(pmodel, cnn)
        pred0, ends0, g0 = s0.run(weights=w)
        pred1, ends1, g1 = s1.run(weights=w)
        fg = s1.feat_grad.clone()
        pred2, _, g2 = s1.run(weights=w)
        torch.cuda.synchronize()
        _same_snapshot(snap, _snapshot(pmodel, cnn))
        with frozen_statistics(cnn), torch.no_grad():
            out, tape = unet16.unet_forward_eval_taped(cnn, s1.batch.images)
            dx = unet16.unet_eval_input_grad(cnn, tape, s1.feat_grad)
        torch.cuda.synchronize()
    assert sorted(g0[0]) == ['cell_feat', 'net_feat'] and sorted(g1[0]) == ['cell_feat', 'image', 'net_feat']
    assert s0.feat_grad is None and np.array_equal(ends0, ends1)
    assert torch.equal(_bits(pred0), _bits(pred1)) and torch.equal(_bits(pred1), _bits(pred2))
    for k in ('cell_feat', 'net_feat'):
        assert torch.equal(_bits(g0[0][k]), _bits(g1[0][k])), k
    img = g1[0]['image']
    assert img.dtype == torch.float32 and img.is_cuda and tuple(img.shape) == tuple(s1.batch.images.shape[1:])
    assert torch.equal(_bits(img), _bits(g2[0]['image'])) and torch.equal(_bits(fg), _bits(s1.feat_grad))
    assert torch.equal(_bits(out.reshape(1, -1)), _bits(s1.feat_map)) and torch.equal(_bits(img), _bits(dx[0]))
    assert tuple(s1.feat_grad.shape) == tuple(s1.feat_map.shape) and float(img.abs().max()) > 0
    feat_rows(fanin, s1.feat_grad[0], d, ids, state, s1.feat_map[0].detach().double().cpu(), w)
    sd = {k: v.detach().cpu().clone() for k, v in cnn.state_dict().items()}
    chain_rows(f'{fanin}: image gradient', img.unsqueeze(0), sd, s1.batch.images.cpu(), SI.acts_from_tape(tape.acts),
               s1.feat_grad.reshape(out.shape).cpu(), 'max', teeth=False)


def test_sensitivity_image_gradient_in_a_batch_of_two(dev):
    """Two designs of different size in one batch: each design's image gradient meets the chain row on its own slice of the
    tape and of feat_grad - what a missed image offset breaks.  Measured on one MI355X: e_hip 1.17e-4 / 4.11e-4
    (e_32 3.71e-8 / 4.11e-4, bound 1.5e-3)."""
    from mmft.evaluate import frozen_statistics
    from mmft.sensitivity import Sensitivity
    designs = [_design(), _design(N=1024, L=12, seed=SEED + 1)]
    pmodel, cnn, _ = _models(designs[0], dev)
    T = sum(d.num_paths for d in designs)
    w = _weights(T, seed=13)
    with lib.math_mode('bf16'):
        s = Sensitivity(pmodel, cnn, designs, dev, image=True)
        _, _, grads = s.run(weights=w)
        with frozen_statistics(cnn), torch.no_grad():
            out, tape = unet16.unet_forward_eval_taped(cnn, s.batch.images)
        torch.cuda.synchronize()
    assert tuple(s.feat_grad.shape) == (2, out[0].numel())
    sd = {k: v.detach().cpu().clone() for k, v in cnn.state_dict().items()}
    acts = SI.acts_from_tape(tape.acts)
    for i in range(2):
        gi = s.feat_grad[i].reshape(1, *out.shape[1:]).cpu()
        chain_rows(f'batch of two, design {i}', grads[i]['image'].unsqueeze(0), sd, s.batch.images[i:i + 1].cpu(),
                   {k: t[i:i + 1] for k, t in acts.items()}, gi, 'max', teeth=False)
    assert not torch.equal(grads[0]['image'], grads[1]['image'])


def test_sensitivity_image_refusals_on_the_device(dev, monkeypatch):
    """fp32 mode, frozen_stats=False on a train-mode net, a shape outside the fused eval path, LayoutNet: ValueError before
    anything is launched; no CNN / no masked projection: ValueError at construction."""
    from mmft.sensitivity import Sensitivity
    from mmft.train import build_models
    d = _design()
    pmodel, cnn, _ = _models(d, dev)
    with pytest.raises(ValueError, match='no CNN'):
        Sensitivity(pmodel, None, [d], dev, image=True)
    s = Sensitivity(pmodel, cnn, [d], dev, image=True)
    with pytest.raises(ValueError, match='fp32'):
        s.run()
    assert s.feat_map is None and s.last_hop is None and s.feat_grad is None
    with lib.math_mode('bf16'):
        cnn.train()
        s_live = Sensitivity(pmodel, cnn, [d], dev, image=True, frozen_stats=False)
        with pytest.raises(ValueError, match='batch statistics'):
            s_live.run()
        monkeypatch.setattr(unet16, 'ENABLED', False)
        with pytest.raises(ValueError, match='outside the fused eval path'):
            s.run()
        monkeypatch.undo()
        pm2, layoutnet = build_models(map_size=d.map_size, device=dev, seed=SEED, unet=False)
        with pytest.raises(ValueError, match='not the U-Net'):
            Sensitivity(pm2, layoutnet, [d], dev, image=True).run()
        assert s.feat_map is None and s_live.feat_map is None
        assert 'image' in s.run()[2][0]                                                  # and the same object still runs
