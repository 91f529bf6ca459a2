"""GPU: the U-Net in EVAL mode - BatchNorm from its running statistics, nothing written (src/Unet.py:16-21 after .eval()).

fp32 math mode against the fixtures the REFERENCE's own module produced in eval mode (tests/golden/make_golden_eval.py,
1e-4 of the scale - the project's fp32 parity bound); bf16 math mode: the convolution with the affine + ReLU (+ pooling)
epilogue (mmft_u16_conv3x3_eval) bit for bit on representable operands and within one bf16 rounding on arbitrary ones,
the whole network against the eval rounding oracle (tests/unet_eval_oracle.py) under the output row of
test_bf16_oracle_gpu.test_unet_module_vs_rounding_oracle: max(2e-3, 3 e_32), ceiling 3e-2.
"""
import numpy as np
import pytest
import torch

from conftest import rel_err
from mmft import lib, ops, unet16
from oracle import bf16 as B
from oracle import restatement as R
import unet_eval_oracle as E
from test_unet_eval_cpu import FIXTURES, CASES, fixture_state

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def snapshot(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def assert_unchanged(net, before, what):
    after = net.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), f'{what}: {k} changed'


def hip_net(dev, pooling, sd=None, seed=3):
    import Unet
    torch.manual_seed(seed)
    net = Unet.UNet(pooling).to(dev)
    if sd is not None:
        net.load_state_dict(sd)
    return net


def profiled(fn):
    """fn() under the library's launch profiler -> (result, {kernel name without template arguments: launches})."""
    lib.prof_reset()
    lib.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.prof_enable(False)
    counts = {}
    for r in lib.prof_report():
        name = r['name'].split('<')[0]
        counts[name] = counts.get(name, 0) + r['launches']
    return out, counts


# ------------------------------------------------------------------------------------------------ 1. fp32 mode vs the reference
@pytest.mark.parametrize('pooling,H,W,N', FIXTURES)
def test_fp32_eval_matches_the_reference_fixtures(dev, pooling, H, W, N):
    g, sd, x = fixture_state(pooling, H, W, N)
    net = hip_net(dev, pooling, sd).eval()
    before = snapshot(net)
    with torch.no_grad():
        y = net(x.to(dev))
        y3 = net(x[0].to(dev))                                      # (C,H,W): SURVEY D3
    out = torch.from_numpy(g['out'])
    e, e3 = rel_err(y, out), rel_err(y3, out[:1])
    print(f'\nfp32 eval {pooling} {H}x{W} N={N}: {e:.2e}, (C,H,W) {e3:.2e}')
    assert y.shape == out.shape and e < 1e-4 and e3 < 1e-4
    assert_unchanged(net, before, 'fp32 eval forward')


def test_fp32_eval_after_our_own_running_statistic_updates(dev):
    """Two train-mode forwards on image 0 (our kernels update the running statistics), .eval(), a forward of the batch:
    the reference's `out_after_train`, and the running statistics it had when it produced it."""
    g, sd, x = fixture_state('max', 64, 64, 2)
    net = hip_net(dev, 'max', sd).train()
    xd = x.to(dev)
    with torch.no_grad():
        net(xd[:1])
        net(xd[:1])
    net.eval()
    before = snapshot(net)
    with torch.no_grad():
        y = net(xd)
    assert_unchanged(net, before, 'eval after train')
    nsd = net.state_dict()
    for k, name in (('rm_inc1', 'inc.double_conv.1.running_mean'), ('rv_inc1', 'inc.double_conv.1.running_var'),
                    ('rm_up2_4', 'up2.conv.double_conv.4.running_mean'), ('rv_up2_4', 'up2.conv.double_conv.4.running_var')):
        assert rel_err(nsd[name], torch.from_numpy(g[k])) < 1e-4, k
    assert int(nsd['inc.double_conv.1.num_batches_tracked']) == int(g['nbt']) == 2
    e = rel_err(y, torch.from_numpy(g['out_after_train']))
    print(f'\nfp32 eval after two train-mode forwards: {e:.2e}')
    assert e < 1e-4


# ------------------------------------------------------------------------------------------------ 2. nothing is mutated
@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('N,H,W,fused', [(2, 64, 64, True), (1, 37, 45, False), (2, 64, 64, False)])
def test_eval_forward_writes_no_parameter_and_no_buffer(dev, mode, N, H, W, fused, monkeypatch):
    net = hip_net(dev, 'max', seed=4)
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(7)).to(dev)
    with torch.no_grad():
        net.train()
        net(x)                                                      # non-trivial running statistics and counters
    net.eval()
    if not fused:
        monkeypatch.setattr(unet16, 'ENABLED', False)
    before = snapshot(net)
    assert int(before['inc.double_conv.1.num_batches_tracked']) == 1
    with lib.math_mode(mode), torch.no_grad():
        (_, counts) = profiled(lambda: (net(x), net(x)))
    assert ('u16_conv3x3_eval_kernel' in counts) == (mode == 'bf16' and fused), counts
    assert_unchanged(net, before, f'{mode} eval forward')
    assert torch.equal(net._batch_counters(), torch.ones(14, dtype=torch.int64, device=dev))


# ------------------------------------------------------------------------------------------------ 3. / 4. the kernel
LAYERS = sorted({(v[0], v[1]) for v in unet16._CONV.values()})
GEOMS = [(2, 10, 72), (2, 10, 40)]             # 4 x 64 tiles / 8 x 32 tiles, partial tiles in both directions, even sides


def grid_vals(shape, seed, step, lim):
    """Multiples of `step` in [-lim, lim]: exact in bf16 when lim / step <= 128."""
    g = torch.Generator().manual_seed(seed)
    n = int(round(lim / step))
    return torch.randint(-n, n + 1, shape, generator=g).double() * step


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def run_eval_conv(dev, x, w, bn, eps, lda, pool, N, H, W, Ci, Co):
    """mmft_u16_conv3x3_eval on x (N,Ci,H,W) fp64, w (Co,Ci,3,3) fp64, bn = (gamma, beta, rm, rv) fp32 ->
    (a [N,H,W,lda] bf16 pre-filled with 7, pooled [N,H/2,W/2,Co] or None)."""
    rgb = Ci == 3
    xd = nhwc(x).float().to(dev) if rgb else nhwc(x).to(BF).to(dev)
    wd = w.float().to(dev).contiguous(memory_format=torch.channels_last)
    buf, table, offs, lanes = unet16.pack_table([unet16.conv_pack_entries('w', wd)], dev)
    unet16.pack_run(buf, table, 1, lanes)
    a = torch.full((N, H, W, lda), 7.0, dtype=BF, device=dev)
    pooled = torch.full((N, H // 2, W // 2, Co), 7.0, dtype=BF, device=dev) if pool else None
    gamma, beta, rm, rv = [t.to(dev) for t in bn]
    d, s = lib.stream_args(a)
    lib.call('mmft_u16_conv3x3_eval', xd, int(rgb), buf, gamma, beta, rm, rv, float(eps), a, lda, pooled,
             ops.POOL_AVG if pool == 'avg' else ops.POOL_MAX, N, H, W, Ci, Co, d, s)
    torch.cuda.synchronize()
    return a.cpu(), (pooled.cpu() if pool else None)


@pytest.mark.parametrize('N,H,W', GEOMS)
@pytest.mark.parametrize('Ci,Co', LAYERS)
def test_eval_conv_exact_on_representable_operands(dev, Ci, Co, N, H, W):
    """Operands on bf16 grids as in test_unet16_gpu (x multiples of 2^-3 in +-2, w multiples of 2^-4 in +-1: the fp32
    accumulator is exact, a multiple of 2^-7 below 2^12); eps = 0, running_var in {1, 4}, gamma in +-{0.5, 1, 2}: scale is
    a power of two in 0.25 .. 2; running_mean, beta multiples of 2^-3: shift exact.  fma(acc, scale, shift) is then a multiple
    of 2^-9 below 2^13 (23 bits: exact) and the sum of four stored values has at most 24 bits (exact), so the kernel's
    output and pooled output must equal the fp64 result rounded to bf16 BIT FOR BIT; the rest of the pitch stays as it was."""
    x = grid_vals((N, Ci, H, W), 1, 0.125, 2.0)
    w = grid_vals((Co, Ci, 3, 3), 2, 0.0625, 1.0)
    g = torch.Generator().manual_seed(3)
    gamma = (2.0 ** torch.randint(-1, 2, (Co,), generator=g).double()) * (torch.randint(0, 2, (Co,), generator=g).double() * 2 - 1)
    rv = 4.0 ** torch.randint(0, 2, (Co,), generator=g).double()
    rm, beta = grid_vals((Co,), 4, 0.125, 1.0), grid_vals((Co,), 5, 0.125, 2.0)
    scale = gamma / rv.sqrt()
    shift = beta - rm * scale
    z = torch.nn.functional.conv2d(x, w, padding=1)
    want = nhwc(torch.relu(z * scale[None, :, None, None] + shift[None, :, None, None])).to(BF)
    assert float((want > 0).double().mean()) > 0.2
    bn = [t.float() for t in (gamma, beta, rm, rv)]
    for pool, lda in ((None, Co), ('max', 2 * Co), ('avg', 2 * Co)):
        a, pooled = run_eval_conv(dev, x, w, bn, 0.0, lda, pool, N, H, W, Ci, Co)
        assert torch.equal(a[..., :Co], want), (pool, lda)
        assert bool((a[..., Co:].float() == 7.0).all())
        if pool:
            win = want.double().reshape(N, H // 2, 2, W // 2, 2, Co)
            exp = (win.amax((2, 4)) if pool == 'max' else win.mean((2, 4))).to(BF)
            assert torch.equal(pooled, exp), pool


def test_eval_conv_arbitrary_data_within_one_rounding(dev):
    """Arbitrary fp32 weights / BatchNorm state on every layer shape: the stored activation is within ONE bf16 rounding
    (2^-8 of the element, DESIGN 5's bound for stored element-wise results) of the rounding oracle's unrounded value.  The
    absolute slack 1e-5 x the layer's scale covers fp32 accumulation over <= 1152 products (K u with u = 2^-24 against the
    root-mean-square size of the sum).  An oracle that applies the affine to a bf16-ROUNDED pre-activation (the train
    path's map) must break that bound on at least one layer: the kernel does not round z."""
    worst, worst_z = {}, {}
    for (Ci, Co) in LAYERS:
        N, H, W = GEOMS[0] if Co <= 32 else GEOMS[1]
        g = torch.Generator().manual_seed(10 + Ci + Co)
        x = B.r(torch.randn((N, Ci, H, W), generator=g).double()) if Ci != 3 else torch.rand((N, Ci, H, W), generator=g).float().double()
        w = (torch.randn((Co, Ci, 3, 3), generator=g) / (3.0 * Ci ** 0.5)).float()
        p = {'c': w.double(), 'b.weight': (torch.rand(Co, generator=g) + 0.5).float(), 'b.bias': (torch.randn(Co, generator=g) * 0.3).float(),
             'b.running_mean': (torch.randn(Co, generator=g) * 0.3).float(), 'b.running_var': (torch.rand(Co, generator=g) + 0.5).float()}
        scale, shift = E.scale_shift(p, 'b.')
        z = B.conv2d_bf16(x, p['c'], 1)
        c = lambda t: t.double()[None, :, None, None]
        t = nhwc(torch.relu(z * c(scale) + c(shift)))
        tz = nhwc(torch.relu(B.r(z) * c(scale) + c(shift)))
        for pool in ('max', 'avg'):
            a, pooled = run_eval_conv(dev, x, w.double(), [p['b.weight'], p['b.bias'], p['b.running_mean'], p['b.running_var']],
                                      E.EPS, 2 * Co, pool, N, H, W, Ci, Co)
            got = a[..., :Co].double()
            slack = 1e-5 * float(t.abs().max())
            m = float(((got - t).abs() / ((2.0 ** -8) * t.abs() + slack)).max())
            mz = float(((got - tz).abs() / ((2.0 ** -8) * tz.abs() + slack)).max())
            worst[(Ci, Co, pool)], worst_z[(Ci, Co, pool)] = m, mz
            win = got.reshape(N, H // 2, 2, W // 2, 2, Co)
            if pool == 'max':
                assert torch.equal(pooled.double(), win.amax((2, 4)))
            else:
                mean = win.mean((2, 4))
                assert float(((pooled.double() - mean).abs() - (2.0 ** -8) * mean.abs()).max()) < 1e-6
    print('\nlayer (Ci, Co, pool): error / bound against the eval map, against the rounded-z map')
    for k in worst:
        print(f'   {k}: {worst[k]:.3f}  {worst_z[k]:.3f}')
    assert max(worst.values()) <= 1.0, worst
    assert max(worst_z.values()) > 1.0, worst_z


# ------------------------------------------------------------------------------------------------ 5. bf16 mode, whole net
def recipe_a_hip(dev, N, H, W, pooling):
    """The HIP net, default-initialised under torch.manual_seed(3), after two train-mode forwards in fp32 mode; its
    state_dict is the common starting point of the HIP eval forward and of the oracles."""
    net = hip_net(dev, pooling, seed=3).train()
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        net(x.to(dev))
        net(x.to(dev))
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    return net.eval(), x, sd


@pytest.mark.parametrize('N,H,W,pooling', CASES)
def test_bf16_eval_net_vs_rounding_oracle(dev, N, H, W, pooling):
    net, x, sd = recipe_a_hip(dev, N, H, W, pooling)
    with lib.math_mode('bf16'), torch.no_grad():
        y, counts = profiled(lambda: net(x.to(dev)))
    o64 = E.unet_eval_forward(E.cast_state(sd, torch.float64), x.double(), pooling, 'bf16')
    o32 = E.unet_eval_forward(E.cast_state(sd, torch.float32), x, pooling, 'bf16')
    op = E.unet_eval_forward(E.cast_state(sd, torch.float64), x.double(), pooling)
    e_hip, e_32, e_plain = rel_err(y, o64), rel_err(o32, o64), rel_err(op, o64)
    bound = max(2e-3, 3.0 * e_32)
    print(f'\nbf16 eval U-Net {N}x{H}x{W} {pooling}: e_hip {e_hip:.2e}  e_32 {e_32:.2e}  e_plain {e_plain:.2e}  bound {bound:.2e}')
    print('   launches:', counts)
    assert counts.get('u16_conv3x3_eval_kernel') == 14, counts
    assert not [k for k in counts if k.startswith(('u16_bn_finalize_kernel', 'u16_bn_apply'))], counts
    assert e_hip <= bound and e_hip <= 3e-2


# ------------------------------------------------------------------------------------------------ 6. batch independence
@pytest.mark.parametrize('pooling', ['max', 'avg'])
def test_fused_eval_output_does_not_depend_on_the_batch(dev, pooling):
    net, _, _ = recipe_a_hip(dev, 1, 64, 96, pooling)
    x = torch.rand(3, 3, 64, 96, generator=torch.Generator().manual_seed(8)).to(dev)
    with lib.math_mode('bf16'), torch.no_grad():
        (y, counts) = profiled(lambda: net(x))
        singles = torch.cat([net(x[i:i + 1]) for i in range(3)])
        net.set_per_sample_stats(True)
        y_ps = net(x)
        net.set_per_sample_stats(False)
    assert counts.get('u16_conv3x3_eval_kernel') == 14, counts       # a batch of several images stays on the fused path
    assert torch.equal(y, singles)
    assert torch.equal(y, y_ps)


# ------------------------------------------------------------------------------------------------ 7. train path untouched
@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_train_after_eval_equals_a_twin_that_never_left_train_mode(dev, mode):
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(9)).to(dev)
    gy = torch.randn(2, 1, 32, 32, generator=torch.Generator().manual_seed(10)).to(dev)
    res = []
    with lib.math_mode(mode):
        for visit_eval in (True, False):
            net = hip_net(dev, 'max', seed=11)
            net.set_per_sample_stats(True)
            net.train()
            with torch.no_grad():
                net(x)
            if visit_eval:
                net.eval()
                with torch.no_grad():
                    net(x)
                    net(x[:1])
                net.train()
            y = net(x)
            y.backward(gy)
            torch.cuda.synchronize()
            res.append((y.detach().clone(), snapshot(net), {k: p.grad.detach().clone() for k, p in net.named_parameters()}))
    (ya, sa, ga), (yb, sb, gb) = res
    assert torch.equal(ya, yb)
    assert int(sa['inc.double_conv.1.num_batches_tracked']) == 4
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


# ------------------------------------------------------------------------------------------------ 8. grad guard
@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_eval_forward_refuses_to_build_a_backward(dev, mode):
    net = hip_net(dev, 'max', seed=12).eval()
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(13)).to(dev)
    before = snapshot(net)
    with lib.math_mode(mode):
        with pytest.raises(NotImplementedError, match='no_grad'):
            net(x)
        net.inc.double_conv[1].train()                               # a mix of modes is refused the same way
        with pytest.raises(NotImplementedError, match='no_grad'):
            net(x)
        net.eval()
        assert_unchanged(net, before, 'refused eval forward')
        with torch.no_grad():
            y = net(x)
        for p in net.parameters():
            p.requires_grad_(False)
        y2 = net(x)                                                   # grad mode on, nothing requires grad: runs
        with pytest.raises(NotImplementedError, match='no_grad'):
            net(x.clone().requires_grad_(True))
    assert not y2.requires_grad and torch.equal(y, y2)


def test_mixed_modes_take_the_per_operator_path(dev):
    """One BatchNorm layer in eval mode, the others in train mode: decided layer by layer (cnn.bn_relu); only the
    train-mode layers count their batch and move their running statistics."""
    net = hip_net(dev, 'max', seed=14).train()
    net.set_per_sample_stats(True)
    frozen = net.down2.maxpool_conv[1].double_conv[4]
    frozen.eval()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(15)).to(dev)
    before = snapshot(net)
    with lib.math_mode('bf16'), torch.no_grad():
        y, counts = profiled(lambda: net(x))
    assert 'bn_eval_kernel' in counts and 'u16_conv3x3_eval_kernel' not in counts and 'u16_conv3x3_kernel' not in counts, counts
    after = net.state_dict()
    pre = 'down2.maxpool_conv.1.double_conv.4.'
    for k in before:
        if k.startswith(pre):
            assert torch.equal(after[k], before[k]), k
        elif k.endswith('num_batches_tracked'):
            assert int(after[k]) == int(before[k]) + 2, k
        elif k.endswith('running_mean'):
            assert not torch.equal(after[k], before[k]), k
    sd = E.cast_state(before, torch.float64)
    assert torch.isfinite(y).all() and y.shape == (2, 1, 32, 32) and sd[pre + 'running_var'].shape == (64,)


# ------------------------------------------------------------------------------------------------ 9. capture
def test_fused_eval_forward_is_capturable(dev):
    net, _, _ = recipe_a_hip(dev, 2, 64, 64, 'max')
    gen = torch.Generator().manual_seed(16)
    xs = [torch.rand(2, 3, 64, 64, generator=gen).to(dev) for _ in range(4)]
    with lib.math_mode('bf16'), torch.no_grad():
        static_x = xs[0].clone()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            net(static_x)                                             # eager warm-up: builds the weight-pack table
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode='thread_local'):
            static_y = net(static_x)
        for x in xs[1:]:
            static_x.copy_(x)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(static_y, net(x))


# ------------------------------------------------------------------------------------------------ 10. launch count
@pytest.mark.parametrize('N,H,W', [(8, 256, 256), (2, 64, 32)])
def test_fused_eval_launch_count(dev, N, H, W):
    """14 convolutions + 3 transposed convolutions + OutConv + the weight pack = 19 launches (the pooling of convolutions
    2, 4, 6 is in their epilogue in both tile shapes); the input's layout pass is not an instrumented launch."""
    net = hip_net(dev, 'max', seed=17).eval()
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(18)).to(dev)
    with lib.math_mode('bf16'), torch.no_grad():
        net(x)
        _, counts = profiled(lambda: net(x))
    print(f'\nfused eval forward {N}x{H}x{W}:', counts)
    assert counts == {'u16_pack_kernel': 1, 'u16_conv3x3_eval_kernel': 14, 'u16_convt_fwd_kernel': 3, 'u16_outconv_fwd_kernel': 1}, counts
    assert sum(counts.values()) <= 22


# ------------------------------------------------------------------------------------------------ 11. validate(frozen_stats=True)
def test_validate_with_frozen_statistics(dev):
    from mmft.evaluate import validate_designs
    from mmft.synth import synth_design
    from mmft.train import build_models
    designs = [synth_design(N=2048, L=12, tile=32, seed=700 + i, end_frac=0.25) for i in range(2)]
    pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=19)
    today = validate_designs(pmodel, cnn, designs, dev)               # train mode; moves the running statistics
    again = validate_designs(pmodel, cnn, designs, dev, frozen_stats=False)
    assert again == today                                             # batch statistics do not depend on the running ones
    pm_state = {k: v.detach().cpu().clone() for k, v in pmodel.state_dict().items()}
    pc_state = {k: v.detach().cpu().clone() for k, v in cnn.state_dict().items()}
    assert int(pc_state['inc.double_conv.1.num_batches_tracked']) == 4
    for was_training in (True, False):
        cnn.train(was_training)
        before = snapshot(cnn)
        res = validate_designs(pmodel, cnn, designs, dev, frozen_stats=True)
        assert all(m.training == was_training for m in cnn.modules())
        assert_unchanged(cnn, before, 'validate(frozen_stats=True)')
        for d, case in zip(designs, res['cases']):
            orc = R.OracleTrainer(pm_state, pc_state, dtype=torch.float64)
            feat = E.unet_eval_forward(E.cast_state(pc_state, torch.float64), torch.from_numpy(d.image).double(), 'max')
            with torch.no_grad():
                hats, tl, _ = R.sweep_forward(orc.pm, orc.pc, d, R.design_csr(d), list(range(d.num_paths)), update_running=False,
                                              dtype=torch.float64, feat_map=feat)
            arr = torch.from_numpy(d.arrival_time).double()[torch.tensor(tl)].squeeze(-1)
            assert case['n'] == d.num_paths
            assert abs(case['loss'] - float(((hats - arr) ** 2).mean())) < 1e-4 * float(((hats - arr) ** 2).mean()) + 1e-9
            assert abs(case['endpoint_slack_mae'] - float((hats - arr).abs().mean())) < 1e-4
            lvl = torch.from_numpy(d.path2level[np.argsort(d.path2level, kind='stable')])
            for m in case['levels']:
                sel = lvl == m['level']
                assert m['n'] == int(sel.sum())
                assert abs(m['mape'] - float(((hats[sel] - arr[sel]) / arr[sel]).abs().mean())) < 1e-4
        assert res['cases'][0]['loss'] != today['cases'][0]['loss']     # not the train-mode result
    cnn.train()
    with pytest.raises(Exception):
        validate_designs(pmodel, cnn, [designs[0], None], dev, frozen_stats=True)     # the second design cannot be batched
    assert all(m.training for m in cnn.modules())                     # handed back as it came, also on an exception
