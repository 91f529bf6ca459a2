"""bf16 math mode against the fp64 oracle that rounds to bf16 where the kernels round (oracle/bf16.py, rounding='bf16').

For every compared quantity Q three distances are taken, all to the fp64 ROUNDING oracle:
  e_hip    the HIP result,
  e_32     the same rounding oracle evaluated in fp32: what fp32 arithmetic alone costs at this input,
  e_plain  the plain fp64 oracle (no rounding at all),
and every row asserts  e_hip <= bound = max(floor_Q, 3 e_32)  and  e_hip <= ceiling_Q.  The teeth check (the plain oracle
would fail, so the test sees where rounding happens) depends on the part of the model:

  * netlist sweep + fusion head.  Compared DECOUPLED from the U-Net: all three oracle runs take the HIP step's own
    feature map (the U-Net output) as their input, so the sweep kernels (level_fwd_slots, level_bwd_pair, mlp2_feat,
    rows_outer) and the bf16 GEMMs of the head are judged on identical inputs.  Rows: predictions, loss, every GNN / head
    gradient (max norm) and the gradient the head sends into the U-Net (d loss / d feature map).  Ceilings 2e-3
    (predictions), 1e-3 (loss), 5e-3 (gradients), and per row  e_plain > 10 x bound - except predictions, whose max norm
    carries a 1.5e-3 floor: one rounding-boundary flip moves one endpoint (1.0e-3 measured at config A).
  Measured on one MI355X (e_hip / e_32 / e_plain), config A: predictions 1.0e-3 / 6.4e-5 / 2.8e-2, loss 5.8e-6 / 3.7e-8 /
    3.1e-3, d loss / d feature map 1.6e-7 / 1.1e-7 / 2.9e-2; irregular fan-in: predictions 2.5e-6 / 2.9e-6 / 3.8e-3,
    loss 7.3e-8 / 7.3e-8 / 2.6e-3.  U-Net gradient means 0.175 / 0.157 / 0.345 (2 x 64²), 0.090 / 0.252 / 0.309
    (3 x 40 x 96 avg), 0.167 / 0.155 / 0.325 (1 x 256²), 0.14 / 0.13 / 0.33 (8 x 64²).
  * U-Net.  A last-bit difference in front of a bf16 rounding moves the stored value by a whole bf16 step once it crosses
    a rounding boundary and every later layer rounds again, so through 14 BatchNorm layers fp32 arithmetic (the kernels'
    and the fp32 oracle's) is promoted to bf16-sized differences: the fp32 rounding oracle sits 0.03 - 0.18 relative L2
    from the fp64 one and the plain oracle only 2-3 x further (tests/test_oracle_bf16_cpu.py pins that spread).  Rows:
    every parameter gradient in relative L2 (ceiling 0.35; OutConv's bias gradient, one cancelling sum of +-g, relative to
    the sum of |g| it adds up), the mean over all tensors (ceiling 0.25), output and running statistics; teeth per group:
    the plain oracle's mean distance exceeds 1.5 x the HIP result's.  The proposed 2e-2 ceiling and 10 x teeth are out of
    reach here for the reason above.  These whole-network bounds are therefore loose - a wrong BatchNorm backward term or
    a misrouted gradient would pass them - and tests/test_unet_stages_gpu.py is where a wrong stage is caught: it feeds
    every stage of one real step its own stored inputs and holds it to the fp64 stage reference almost bit for bit.
"""
import numpy as np
import pytest
import torch

from conftest import rel_err
from mmft import lib
from oracle import restatement as R

pytestmark = pytest.mark.gpu

UNET_PREFIX = ('inc.', 'down', 'up', 'outc.')
K, TEETH_ROW, TEETH_GROUP = 3.0, 10.0, 1.5


def rel_l2(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


class Bounds:
    """The bound rule of the module docstring over many quantities: every row is measured and printed before the test
    fails on the rows that break it.  Teeth are checked per group of rows (see the module docstring)."""

    def __init__(self, title, hip, o32, op):
        self.title, self.runs, self.rows, self.bad = title, (hip, o32, op), [], []

    def __call__(self, name, dist, floor, ceiling, group=None, teeth=False):
        """group: rows whose teeth are checked together (mean e_plain > TEETH_GROUP x mean e_hip); teeth: this row's own
        check, e_plain > TEETH_ROW x bound."""
        e_hip, e_32, e_plain = (dist(r) for r in self.runs)
        bound = max(floor, K * e_32)
        self.rows.append((name, e_hip, e_32, e_plain, bound, group))
        if e_hip > bound:
            self.bad.append(f'{name}: e_hip {e_hip:.3e} > bound {bound:.3e}')
        if e_hip > ceiling:
            self.bad.append(f'{name}: e_hip {e_hip:.3e} > ceiling {ceiling:.3e}')
        if teeth and not e_plain > TEETH_ROW * bound:
            self.bad.append(f'{name}: no teeth, e_plain {e_plain:.3e} <= {TEETH_ROW} x bound {bound:.3e}')

    def verdict(self):
        print(f'\n== {self.title}: quantity  e_hip  e_32  e_plain  bound')
        for name, eh, e3, ep, b, _ in self.rows:
            print(f'   {name:60s} {eh:.2e} {e3:.2e} {ep:.2e} {b:.2e}')
        for g in sorted({r[5] for r in self.rows if r[5]}):
            eh = np.mean([r[1] for r in self.rows if r[5] == g])
            ep = np.mean([r[3] for r in self.rows if r[5] == g])
            print(f'   teeth {g}: mean e_plain / mean e_hip = {ep / eh:.2f}')
            if not ep > TEETH_GROUP * eh:
                self.bad.append(f'no teeth in {g}: mean e_plain {ep:.3e} <= {TEETH_GROUP} x mean e_hip {eh:.3e}')
        assert not self.bad, self.bad


def oracle_step(d, path_ids, pm_state, pc_state, rounding, dtype, feat_map=None):
    """One oracle step; feat_map (the HIP step's U-Net output): the sweep and head run on it instead of the oracle's U-Net,
    and its gradient is returned as 'feat_grad'."""
    o = R.OracleTrainer(pm_state, pc_state, dtype=dtype, rounding=rounding)
    feat = feat_map.to(dtype).clone().requires_grad_(True) if feat_map is not None else None
    hats, tl, _ = o.forward(d, R.design_csr(d), path_ids, feat_map=feat)
    arr = torch.from_numpy(d.arrival_time).to(dtype)[torch.tensor(tl)].squeeze(-1)
    loss = torch.nn.functional.mse_loss(hats, arr)
    loss.backward()
    grads = {k: v.grad.detach().double() for k, v in list(o.pm.items()) + list(o.pc.items())
             if isinstance(v, torch.Tensor) and v.grad is not None}
    run = {k: v.double() for k, v in o.pc.items() if 'running' in k}
    return dict(hats=hats.detach().double(), loss=float(loss.detach()), grads=grads, run=run, targets=tl,
                feat_grad=feat.grad.double().reshape(-1) if feat is not None else None)


STEP_KERNELS = {'level_fwd_slots_kernel', 'level_bwd_pair_kernel', 'mlp2_feat_fwd_kernel', 'mlp2_feat_bwd_kernel',
                'rows_outer_kernel', 'u16_conv3x3_kernel', 'u16_conv3x3_wgrad_kernel', 'u16_bn_apply_kernel',
                'u16_bn_apply_pool_kernel', 'u16_bn_bwd_apply_kernel', 'u16_convt_fwd_kernel', 'u16_convt_dgrad_kernel',
                'u16_convt_wgrad_kernel', 'u16_pool_bwd_kernel', 'u16_outconv_fwd_kernel', 'u16_outconv_bwd_kernel'}


def hip_step(d, path_ids, dev, seed=9294):
    """One bf16-mode train step (forward, MSE, backward) on the HIP path, profiled once."""
    from mmft.train import build_models, TrainStep
    from mmft.fusion import mse_loss
    pmodel, cnn = build_models(map_size=d.map_size, device=dev, seed=seed)
    pm_state = {k: v.detach().cpu().clone() for k, v in pmodel.state_dict().items()}
    pc_state = {k: v.detach().cpu().clone() for k, v in cnn.state_dict().items()}
    feats = []

    def keep(module, inputs, out):
        out.retain_grad()
        feats.append(out)
    hook = cnn.register_forward_hook(keep)
    with lib.math_mode('bf16'):
        ts = TrainStep(pmodel, cnn, [d], dev)
        lib.prof_reset()
        lib.prof_enable(True)
        try:
            hats, ends_d, ends_h = ts.forward([path_ids])
            loss = mse_loss(hats, ts.batch.arrival[ends_d.long()].squeeze(-1))
            ts.optim.zero_grad()
            loss.backward()
            torch.cuda.synchronize()
        finally:
            lib.prof_enable(False)
            hook.remove()
        names = {r['name'].split('<')[0] for r in lib.prof_report()}
    assert len(feats) == 1 and feats[0].grad is not None
    grads = {k: p.grad.detach().double().cpu() for k, p in list(pmodel.named_parameters()) + list(cnn.named_parameters())
             if p.grad is not None}
    run = {k: v.detach().double().cpu() for k, v in cnn.state_dict().items() if 'running' in k}
    out = dict(hats=hats.detach().double().cpu(), loss=float(loss), grads=grads, run=run, targets=ends_h.tolist(),
               feat=feats[0].detach().float().cpu().reshape(-1), feat_grad=feats[0].grad.double().cpu().reshape(-1))
    return out, names, pm_state, pc_state, ts.batch


def unet_grad_rows(q, ref, keys, scale_bias):
    """Per-tensor relative L2 of the U-Net gradients (OutConv's bias: |difference| / scale_bias, the sum of |g| it adds up)
    and their mean."""
    def dist(k):
        if k == 'outc.conv.0.bias':
            return lambda r: float((r['grads'][k] - ref['grads'][k]).abs().sum() / scale_bias)
        return lambda r: rel_l2(r['grads'][k], ref['grads'][k])
    for k in keys:
        q('grad ' + k, dist(k), 2e-2 if k != 'outc.conv.0.bias' else 1e-3, 0.35)
    q('U-Net gradients, mean', lambda r: float(np.mean([dist(k)(r) for k in keys])), 2e-2, 0.25, 'U-Net gradients (mean)')
    for k in ref['run']:
        q('running ' + k, lambda r, k=k: rel_err(r['run'][k], ref['run'][k]), 1e-4, 2e-3, 'running statistics')


def sweep_head_rows(title, hip, run):
    """The sweep + head rows of the module docstring, all three oracle runs on the HIP step's feature map."""
    s64, s32, sp = (run(rd, dt, hip['feat']) for rd, dt in (('bf16', torch.float64), ('bf16', torch.float32),
                                                            (None, torch.float64)))
    assert hip['targets'] == s64['targets']
    q = Bounds(title, hip, s32, sp)
    # one operand element that lands on the other side of a bf16 rounding boundary (hardware exp / log, fp32 order) moves
    # one endpoint: measured 1.0e-3 of the scale at config A while e_32 was 6e-5 and every gradient stayed inside 3 e_32 -
    # hence the floor, and no 10 x row check here (the loss and every gradient keep theirs)
    q('predictions', lambda r: rel_err(r['hats'], s64['hats']), 1.5e-3, 2e-3)
    q('loss', lambda r: abs(r['loss'] - s64['loss']) / s64['loss'], 1e-5, 1e-3, teeth=True)
    head = [k for k in s64['grads'] if float(s64['grads'][k].abs().max()) > 0]
    assert not any(k.startswith(UNET_PREFIX) for k in head) and set(head) <= set(hip['grads'])
    for k in head:
        q('grad ' + k, lambda r, k=k: rel_err(r['grads'][k], s64['grads'][k]), 1e-4, 5e-3, teeth=True)
    q('d loss / d feature map', lambda r: rel_err(r['feat_grad'], s64['feat_grad']), 1e-4, 5e-3, teeth=True)
    return q


def test_config_a_step_vs_rounding_oracle(dev):
    """One config-A train step (100 paths; U-Net on the bf16-storage path, 32-level sweep on the slot-table forward and
    paired reverse kernels, feature MLPs without a hidden tensor, row-contraction weight gradients, fusion head on the bf16
    GEMMs) against the fp64 rounding oracle: the sweep and head decoupled from the U-Net (predictions, loss, every GNN /
    head gradient, d loss / d feature map), the U-Net's gradients and running statistics from the coupled step."""
    from mmft.synth import config_design
    d = config_design('A')
    path_ids = np.random.default_rng(1).permutation(d.num_paths)[:100].tolist()
    hip, names, pm_state, pc_state, _ = hip_step(d, path_ids, dev)
    print('\nkernels:', sorted(names))
    assert STEP_KERNELS <= names, sorted(STEP_KERNELS - names)
    assert any(n.startswith('gemm_bf16_kernel') for n in names), sorted(names)
    run = lambda rounding, dtype, feat=None: oracle_step(d, path_ids, pm_state, pc_state, rounding, dtype, feat)
    q = sweep_head_rows('config A: sweep + head on the HIP feature map', hip, run)
    # the U-Net, coupled
    o64, o32, op = (run(rd, dt) for rd, dt in (('bf16', torch.float64), ('bf16', torch.float32), (None, torch.float64)))
    unet = [k for k in o64['grads'] if k.startswith(UNET_PREFIX) and float(o64['grads'][k].abs().max()) > 0]
    assert set(unet) <= set(hip['grads'])
    u = Bounds('config A: U-Net', hip, o32, op)
    unet_grad_rows(u, o64, unet, float(hip['feat_grad'].abs().sum()))
    for b in (q, u):
        b.verdict()


def test_irregular_fanin_step_vs_rounding_oracle(dev):
    """Irregular fan-in (synth_design(N=9000, tile=32, fanin='irregular')): heavy drivers cut into parts in the paired
    reverse kernel's tile table and pins with more than four cell consumers (the slot table's CSR tail); the sweep and
    head of one train step against the rounding oracle, decoupled from the U-Net as in the config-A case."""
    from mmft.synth import synth_design
    d = synth_design(N=9000, L=12, tile=32, seed=220, end_frac=0.2, fanin='irregular')
    path_ids = np.random.default_rng(2).permutation(d.num_paths)[:100].tolist()
    hip, names, pm_state, pc_state, batch = hip_step(d, path_ids, dev)
    print('\nkernels:', sorted(names))
    pairs = batch.graph.level_bwd_pairs(batch.level_nodes)
    assert pairs is not None
    assert sum(int((p['tiles'][:, 3] > 0).sum()) for p in pairs[1] if p is not None) > 0      # heavy drivers in parts
    assert int((pairs[0][:, 3] <= -2).sum()) > 0                                                # slot-table CSR tails
    core = {'level_bwd_pair_kernel', 'mlp2_feat_fwd_kernel', 'mlp2_feat_bwd_kernel', 'rows_outer_kernel'}
    assert core <= names and any(n.startswith('gemm_bf16_kernel') for n in names), sorted(names)
    run = lambda rounding, dtype, feat=None: oracle_step(d, path_ids, pm_state, pc_state, rounding, dtype, feat)
    sweep_head_rows('irregular fan-in: sweep + head on the HIP feature map', hip, run).verdict()


def unet_case(dev, N, H, W, pooling):
    """UNet.forward + backward on the bf16-storage path against the rounding oracle run image by image (per-image
    statistics, as the step uses them)."""
    import Unet
    torch.manual_seed(3)
    net = Unet.UNet(pooling).to(dev)
    net.set_per_sample_stats(True)
    net.train()
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(5))
    gy = torch.randn(N, 1, H // 2, W // 2, generator=torch.Generator().manual_seed(6))
    with lib.math_mode('bf16'):
        lib.prof_reset()
        lib.prof_enable(True)
        try:
            y = net(x.to(dev))
            y.backward(gy.to(dev))
            torch.cuda.synchronize()
        finally:
            lib.prof_enable(False)
        names = {r['name'].split('<')[0] for r in lib.prof_report()}
    hip = dict(y=y.detach().double().cpu(), grads={k: p.grad.double().cpu() for k, p in net.named_parameters()},
               run={k: v.double().cpu() for k, v in net.state_dict().items() if 'running' in k})

    def oracle(rounding, dtype):
        pc = {k: (v.to(dtype).clone().requires_grad_('running' not in k) if v.dtype.is_floating_point else v.clone())
              for k, v in sd.items()}
        yo = torch.cat([R.unet_forward(pc, x[i:i + 1].to(dtype), pooling, True, rounding=rounding) for i in range(N)])
        yo.backward(gy.to(dtype))
        return dict(y=yo.detach().double(), grads={k: pc[k].grad.double() for k in hip['grads']},
                    run={k: pc[k].double() for k in hip['run']})
    return hip, names, gy, oracle('bf16', torch.float64), oracle('bf16', torch.float32), oracle(None, torch.float64)


UNET_KERNELS = {'u16_pack_kernel', 'u16_conv3x3_kernel', 'u16_conv3x3_wgrad_kernel', 'u16_bn_finalize_kernel',
                'u16_bn_apply_kernel', 'u16_bn_apply_pool_kernel', 'u16_bn_bwd_partial_kernel', 'u16_bn_bwd_finalize_kernel',
                'u16_bn_bwd_apply_kernel', 'u16_convt_fwd_kernel', 'u16_convt_dgrad_kernel', 'u16_convt_wgrad_kernel',
                'u16_pool_bwd_kernel', 'u16_outconv_fwd_kernel', 'u16_outconv_bwd_kernel'}


@pytest.mark.parametrize('N,H,W,pooling', [(2, 64, 64, 'max'), (3, 40, 96, 'avg'), (1, 256, 256, 'max'), (8, 64, 64, 'max')])
def test_unet_module_vs_rounding_oracle(dev, N, H, W, pooling):
    """The bf16-storage U-Net on its own: output, every parameter gradient (relative L2 per tensor and the mean over all
    tensors) and the running statistics against the fp64 rounding oracle.  The convolutions take 4 x 64 pixel tiles where
    a level is at least 64 wide and 8 x 32 tiles below (unet16_conv.hip:13): 64 x 64 uses both, 40 x 96 adds partial tiles
    of both kinds, 256 x 256 (one image, the benched tile size) is the bench's shape, 8 x 64 x 64 the bench's image count
    (per-image BatchNorm statistics of images 4-7)."""
    hip, names, gy, o64, o32, op = unet_case(dev, N, H, W, pooling)
    assert UNET_KERNELS <= names, sorted(UNET_KERNELS - names)
    q = Bounds(f'U-Net {N}x{H}x{W} {pooling}', hip, o32, op)
    q('output', lambda r: rel_err(r['y'], o64['y']), 2e-3, 3e-2, 'output')
    unet_grad_rows(q, o64, list(o64['grads']), float(gy.abs().sum()))
    q.verdict()
