"""Module-level parity on the GPU: the drop-in model.py / Unet.py classes (HIP path, through the C ABI)
against the committed golden vectors that the REFERENCE's own code produced (tests/golden/make_golden.py)
and against the CPU oracle on seeded inputs.  Tolerance: 1e-4 relative fp32 (BASELINE.json north_star);
most checks are far tighter."""
import os
import numpy as np
import pytest
import torch

from conftest import rel_err
from mmft.detrand import det_uniform, det_state_dict
from mmft.pingraph import PinGraph
from mmft import ops
from oracle import restatement as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TOL = 1e-4


def gold(name):
    return np.load(os.path.join(GOLD, name + '.npz'))


def close(a, ref, tol=TOL, what=''):
    ref = ref.detach() if torch.is_tensor(ref) else torch.as_tensor(np.asarray(ref))
    e = rel_err(a, ref)
    assert e < tol, f'{what}: rel err {e:.3e} >= {tol}'


def load_det(module, seed, dev, extra=None):
    sd = det_state_dict(module, seed)
    if extra:
        sd.update(extra)
    module.load_state_dict(sd)
    return module.to(dev)


@pytest.mark.parametrize('i', [0, 1, 2, 3])
def test_mlp_golden(dev, i):
    import model
    g = gold(f'mlp_{i}')
    sizes, slope, seed = [int(s) for s in g['sizes']], float(g['slope']), int(g['seed'])
    net = load_det(model.MLP(*sizes, negative_slope=slope), seed, dev)
    x = torch.from_numpy(det_uniform((9, sizes[0]), seed + 100)).to(dev).requires_grad_(True)
    y = net(x)
    wts = torch.from_numpy(det_uniform(tuple(y.shape), seed + 200)).to(dev)
    (y * wts).sum().backward()
    close(y, g['out'], what='out')
    close(x.grad, g['dx'], what='dx')
    gw = net.layers[0].weight.grad
    close(gw[::max(sizes[1] // 16, 1)], g['g_w0'], what='g_w0')
    close(net.layers[0].bias.grad, g['g_b0'], what='g_b0')


def test_cell_msg_reduce_golden(dev):
    g = gold('cell_msg_reduce')
    for deg in range(1, 9):
        mail = torch.from_numpy(det_uniform((6, deg, 16), 400 + deg, -3.0, 3.0))
        h = mail.reshape(6 * deg, 16).to(dev)
        src = np.arange(6 * deg)
        dst = 6 * deg + np.repeat(np.arange(6), deg)
        gr = PinGraph(6 * deg + 6, {'cell': (src, dst), 'net': ((), ())}).to(dev)
        hh = torch.cat([h, torch.zeros((6, 16), device=dev)])
        A = torch.zeros_like(hh)
        rows = torch.arange(6 * deg, 6 * deg + 6, dtype=torch.int32, device=dev)
        ops.seg_softmax_sum_fwd(hh, gr.csr('in', 'cell'), rows, A, torch.zeros_like(hh))
        close(A[6 * deg:], g[f'deg{deg}'], 1e-5, f'deg{deg}')


@pytest.mark.parametrize('name,pooling,hw', [('unet_max_64x64', 'max', (64, 64)), ('unet_avg_64x64', 'avg', (64, 64)),
                                             ('unet_max_37x45', 'max', (37, 45))])
def test_unet_golden(dev, name, pooling, hw):
    import Unet
    g = gold(name)
    seed = int(g['seed'])
    net = Unet.UNet(pooling)
    net = load_det(net, seed, dev, {'outc.conv.0.bias': torch.full((1,), float(g['outc_bias']))})
    net.train()
    x = torch.from_numpy(det_uniform((1, 3) + hw, seed + 100, 0.0, 1.0)).to(dev).requires_grad_(True)
    y = net(x)
    assert tuple(y.shape) == tuple(g['out'].shape)
    wts = torch.from_numpy(det_uniform(tuple(y.shape), seed + 200)).to(dev)
    (y * wts).sum().backward()
    close(y, g['out'], what='out')
    close(x.grad[0, :, ::3, ::3], g['dx'], 2e-4, 'dx')
    P = dict(net.named_parameters())
    close(P['inc.double_conv.0.weight'].grad, g['g_inc0'], 2e-4, 'g_inc0')
    close(P['inc.double_conv.1.weight'].grad, g['g_inc_bn_w'], 2e-4, 'g_inc_bn_w')
    close(P['inc.double_conv.1.bias'].grad, g['g_inc_bn_b'], 2e-4, 'g_inc_bn_b')
    close(P['down3.maxpool_conv.1.double_conv.3.weight'].grad[::8, ::8], g['g_down3_3'], 2e-4, 'g_down3_3')
    close(P['up1.up.weight'].grad[::8, ::8], g['g_up1_up_w'], 2e-4, 'g_up1_up_w')
    close(P['up1.up.bias'].grad, g['g_up1_up_b'], 2e-4, 'g_up1_up_b')
    close(P['up3.conv.double_conv.0.weight'].grad[:, ::4], g['g_up3_conv0'], 2e-4, 'g_up3_conv0')
    close(P['outc.conv.0.weight'].grad, g['g_outc_w'], 2e-4, 'g_outc_w')
    close(P['outc.conv.0.bias'].grad, g['g_outc_b'], 2e-4, 'g_outc_b')
    sd = net.state_dict()
    close(sd['inc.double_conv.1.running_mean'], g['rm_inc1'], 1e-5, 'rm')
    close(sd['inc.double_conv.1.running_var'], g['rv_inc1'], 1e-5, 'rv')
    close(sd['up2.conv.double_conv.4.running_mean'], g['rm_up2_4'], 1e-4, 'rm2')
    close(sd['up2.conv.double_conv.4.running_var'], g['rv_up2_4'], 1e-4, 'rv2')
    assert int(sd['inc.double_conv.1.num_batches_tracked']) == int(g['nbt'])
    # 3-D input is accepted and equals the 4-D result
    with torch.no_grad():
        net2 = load_det(Unet.UNet(pooling), seed, dev, {'outc.conv.0.bias': torch.full((1,), float(g['outc_bias']))})
        y3 = net2(x.detach()[0])
    close(y3, g['out'], what='3-D input')


@pytest.mark.parametrize('tag,s1,s2,seed', [('even', (1, 16, 8, 8), (1, 16, 16, 16), 81), ('odd', (2, 16, 7, 9), (2, 16, 15, 19), 82)])
def test_up_bilinear_golden(dev, tag, s1, s2, seed):
    """Up(32, 16, bilinear=True) (src/Unet.py:48-51): align_corners=True x2 up-sampling kernel (forward + gather backward),
    centre padding to the skip size, concat, DoubleConv - against the reference module's output and gradients."""
    import Unet
    g = gold('up_bilinear_' + tag)
    up = load_det(Unet.Up(32, 16, bilinear=True), seed, dev)
    up.train()
    x1 = torch.from_numpy(det_uniform(s1, seed + 100)).to(dev).requires_grad_(True)
    x2 = torch.from_numpy(det_uniform(s2, seed + 200)).to(dev).requires_grad_(True)
    y = up(x1, x2)
    wts = torch.from_numpy(det_uniform(tuple(y.shape), seed + 300)).to(dev)
    (y * wts).sum().backward()
    close(y, g['out'], what='out')
    close(x1.grad, g['dx1'], 2e-4, 'dx1')
    close(x2.grad, g['dx2'], 2e-4, 'dx2')
    close(up.conv.double_conv[0].weight.grad, g['g_conv0'], 2e-4, 'g_conv0')
    close(up.conv.double_conv[1].weight.grad, g['g_bn1_w'], 2e-4, 'g_bn1_w')
    # the whole UNet with bilinear=True is unusable in the reference too (up3: 8 channels, OutConv: 16) - same failure
    net = Unet.UNet('max', bilinear=True).to(dev)
    with pytest.raises((ValueError, RuntimeError), match='channels'):
        net(torch.zeros(1, 3, 16, 16, device=dev))


@pytest.mark.parametrize('pooling', ['max', 'avg'])
def test_layoutnet_golden(dev, pooling):
    import model
    g = gold(f'layoutnet_{pooling}')
    seed = int(g['seed'])
    net = load_det(model.LayoutNet(pooling), seed, dev)
    x = torch.from_numpy(det_uniform((1, 2, 32, 32), seed + 100, 0.0, 1.0)).to(dev).requires_grad_(True)
    y = net(x)
    wts = torch.from_numpy(det_uniform(tuple(y.shape), seed + 200)).to(dev)
    (y * wts).sum().backward()
    close(y, g['out'], what='out')
    close(net(x.detach()[0]), g['out3d'], what='3-D input')
    close(x.grad, g['dx'], 2e-4, 'dx')
    P = dict(net.named_parameters())
    close(P['encode.0.weight'].grad[::4], g['g_e0_w'], 2e-4, 'g_e0_w')
    close(P['encode.0.bias'].grad, g['g_e0_b'], 2e-4, 'g_e0_b')
    close(P['encode.3.weight'].grad[::8, ::8], g['g_e3_w'], 2e-4, 'g_e3_w')
    close(P['encode.8.weight'].grad, g['g_e8_w'], 2e-4, 'g_e8_w')
    close(P['encode.8.bias'].grad, g['g_e8_b'], 2e-4, 'g_e8_b')


def _fixture_design(g):
    class D:
        pass
    d = D()
    d.N = int(g['cell_feat'].shape[0])
    sizes = g['level_sizes']
    starts = np.concatenate([[0], np.cumsum(sizes)])
    d.levels = [g['level_nodes'][starts[i]:starts[i + 1]] for i in range(len(sizes))]
    d.L = len(sizes)
    for k in ('net_src', 'net_dst', 'cell_src', 'cell_dst', 'cell_feat', 'net_feat', 'path2level', 'path2endpoint',
              'mask_indptr', 'mask_cols'):
        setattr(d, k, g[k])
    d.arrival_time = g['arrival']
    return d


def _run_sweep(model_, graph, d, path_ids, feat_map, P, dev, sparse):
    """The reference loop src/train.py:476-511 against the drop-in PathModel."""
    from mmft.fusion import PathMasks, MaskedPathMap
    ends, paths = R.bucket_paths(path_ids, d.path2level, d.path2endpoint)
    masks = PathMasks(d.mask_indptr, d.mask_cols, P, dev) if sparse else None
    hats, tl = None, []
    for level_id in range(d.L):
        nodes = [int(v) for v in d.levels[level_id]]
        targets = ends.get(level_id, [])
        pids = paths.get(level_id, [])
        tl.extend(targets)
        pm = None
        if pids:
            if sparse:
                pm = MaskedPathMap(masks, pids, feat_map)
            else:
                pm = R.dense_mask_rows(d.mask_indptr, d.mask_cols, pids, P).to(dev) * feat_map
        cur = model_(graph, nodes, None, targets, level_id, torch.tensor([float(level_id)], device=dev), pm)
        if cur is None:
            continue
        hats = cur if hats is None else torch.cat((hats, cur), 0)
    return hats, tl


@pytest.mark.parametrize('sparse', [False, True])
def test_sweep_golden(dev, sparse):
    """Full multi-level sweep + fusion head + MSE backward on the 64-node fixture DAG (duplicate targets)."""
    import model
    g = gold('sweep_small')
    d = _fixture_design(g)
    D, P = 16, 64
    gnn = model.PathConv(D, D, 36, 2)
    fcn = torch.nn.Linear(P, 24)
    fuse = model.MLP(D + 24 + 32, 2 * (D + 24 + 32), 1)
    pmodel = load_det(model.PathModel(gnn, None, fcn, None, None, fuse), 51, dev)
    feat_map = torch.from_numpy(det_uniform((1, P), 52, 0.0, 1.0)).to(dev).requires_grad_(True)
    graph = PinGraph(d.N, {'net': (d.net_src, d.net_dst), 'cell': (d.cell_src, d.cell_dst)})
    graph.ndata['cell_feat'] = torch.from_numpy(d.cell_feat)
    graph.ndata['net_feat'] = torch.from_numpy(d.net_feat)
    graph.ndata['h'] = torch.zeros((d.N, D))
    graph = graph.to(dev)
    path_ids = [int(v) for v in g['path_ids']]
    hats, tl = _run_sweep(pmodel, graph, d, path_ids, feat_map, P, dev, sparse)
    assert tl == [int(v) for v in g['targets']]
    arrival = torch.from_numpy(d.arrival_time).to(dev)[torch.tensor(tl, device=dev)].squeeze(-1)
    loss = torch.nn.functional.mse_loss(hats, arrival)
    loss.backward(retain_graph=True)                      # as src/train.py:553
    close(hats, g['hats'], what='hats')
    close(loss, g['loss'], what='loss')
    close(graph.ndata['h'], g['h_final'], what='h')
    close(feat_map.grad, g['dfeat'], 2e-4, 'dfeat')
    for k, prm in pmodel.named_parameters():
        key = 'g_' + k.replace('.', '_')
        if key in g.files:
            close(prm.grad, g[key], 3e-4, key)
        else:
            assert prm.grad is None, f'{k} should not receive a gradient (unused in forward)'


@pytest.mark.parametrize('entry', ['dropin', 'sweep'])
def test_attention_branch_golden(dev, entry):
    """PathConv(flag_attn=True) (src/model.py:56-58,119-136,190-198) against what the reference's unmodified
    PathConv.forward produced on the fixture DAG with a synthetic ndata['key'] (tests/golden/sweep_attn.npz): outputs,
    final embeddings, ndata['h_drive'] and every parameter gradient incl. fc_key / fc_attn; per-level drop-in calls and
    the whole-sweep entry."""
    import model
    from test_oracle_golden import attn_level_targets
    from mmft import sweep as S
    g, gd = gold('sweep_attn'), gold('sweep_small')
    d = _fixture_design(gd)
    D = 16
    gnn = load_det(model.PathConv(D, D, 36, 2, flag_attn=True), 72, dev)
    graph = PinGraph(d.N, {'net': (d.net_src, d.net_dst), 'cell': (d.cell_src, d.cell_dst)})
    graph.ndata['cell_feat'] = torch.from_numpy(d.cell_feat)
    graph.ndata['net_feat'] = torch.from_numpy(d.net_feat)
    graph.ndata['key'] = torch.from_numpy(det_uniform((d.N, 1), 73, -2.0, 2.0))
    graph.ndata['h'] = torch.zeros((d.N, D))
    graph = graph.to(dev)
    targets = attn_level_targets(gd)
    if entry == 'dropin':
        out = torch.cat([gnn(graph, [int(v) for v in d.levels[l]], None, targets[l], l) for l in range(d.L)], 0)
    else:
        # the whole-sweep entry returns the targets in one gather after the last level (rows are final once written)
        flat = torch.tensor([t for tl in targets for t in tl], dtype=torch.int32, device=dev)
        out = S.sweep_forward_all(gnn, graph, [[int(v) for v in lv] for lv in d.levels], flat)
    wts = torch.from_numpy(det_uniform(tuple(out.shape), 74)).to(dev)
    (out * wts).sum().backward()
    close(out, g['out'], what='out')
    close(graph.ndata['h'], g['h_final'], what='h')
    assert float((graph.ndata['h_drive'].cpu() - torch.from_numpy(g['h_drive'])).abs().max()) < 1e-6
    for k, prm in gnn.named_parameters():
        key = 'g_' + k.replace('.', '_')
        if key in g.files:
            close(prm.grad, g[key], 3e-4, key)
        else:
            assert prm.grad is None, f'{k} should not receive a gradient (unused in forward)'


def test_pathmodel_variants_golden(dev):
    import model
    g = gold('pathmodel_variants')
    gs = gold('sweep_small')
    d = _fixture_design(gs)
    D, P = 16, 64
    for tag, (use_gnn, use_fcn) in (('nognn', (False, True)), ('nofcn', (True, False))):
        gnn = model.PathConv(D, D, 36, 2)
        fcn = torch.nn.Linear(P, 24)
        width = (D if use_gnn else 0) + (24 if use_fcn else 0) + 32
        fuse = model.MLP(width, 2 * width, 1)
        pm = load_det(model.PathModel(gnn if use_gnn else None, None, fcn if use_fcn else None, None, None, fuse), 61, dev)
        graph = PinGraph(d.N, {'net': (d.net_src, d.net_dst), 'cell': (d.cell_src, d.cell_dst)})
        graph.ndata['cell_feat'] = torch.from_numpy(d.cell_feat)
        graph.ndata['net_feat'] = torch.from_numpy(d.net_feat)
        graph.ndata['h'] = torch.zeros((d.N, D))
        graph = graph.to(dev)
        nodes0 = [int(v) for v in d.levels[0]]
        targets = nodes0[:2] + nodes0[:1]
        pmap = torch.from_numpy(det_uniform((len(targets), P), 62, 0.0, 1.0)).to(dev)
        lvl = torch.tensor([0.0], device=dev)
        with torch.no_grad():
            y = pm(graph, nodes0, None, targets, 0, lvl, pmap if use_fcn else None)
            close(y, g[tag], what=tag)
            graph.ndata['h'] = torch.zeros((d.N, D), device=dev)
            assert pm(graph, nodes0, None, [], 0, lvl, None) is None          # T = 0 -> None (src/model.py:282-283)


def test_config_a_step_vs_oracle(dev):
    """BASELINE config A shape (4k nodes, 64x64 tile): one full train step vs the CPU oracle, <= 1e-4."""
    import model
    import Unet
    from mmft.synth import config_design
    from mmft.train import build_models, TrainStep
    d = config_design('A')
    torch.manual_seed(0)
    pmodel, cnn = build_models(map_size=d.map_size, device=dev, seed=9294)
    pm_state = {k: v.detach().cpu().clone() for k, v in pmodel.state_dict().items()}
    pc_state = {k: v.detach().cpu().clone() for k, v in cnn.state_dict().items()}
    # The oracle runs in fp64: on this net the CPU *fp32* path itself sits 2e-3..2e-2 away from the fp64
    # result in the early encoder gradients (one ReLU/max-pool decision flips), while the HIP fp32 path
    # stays within ~3e-6 of fp64 (tools/diag_grad_precision.py) - so fp64 is the only meaningful judge.
    oracle = R.OracleTrainer(pm_state, pc_state, dtype=torch.float64)
    csr = R.design_csr(d)
    rng = np.random.default_rng(1)
    path_ids = rng.permutation(d.num_paths)[:100].tolist()
    hats_o, tl_o, _ = oracle.forward(d, csr, path_ids)
    arr_o = torch.from_numpy(d.arrival_time).double()[torch.tensor(tl_o)].squeeze(-1)
    loss_o = torch.nn.functional.mse_loss(hats_o, arr_o)
    loss_o.backward()
    ts = TrainStep(pmodel, cnn, [d], dev, fused_optimizer=True)
    hats, ends_d, ends_h = ts.forward([path_ids])
    assert ends_h.tolist() == tl_o
    from mmft.fusion import mse_loss
    loss = mse_loss(hats, ts.batch.arrival[ends_d.long()].squeeze(-1))
    ts.optim.zero_grad()
    loss.backward()
    close(hats, hats_o, TOL, 'predicted arrival')
    close(loss, loss_o, TOL, 'loss')
    for k, prm in pmodel.named_parameters():
        if oracle.pm[k].grad is not None:
            close(prm.grad, oracle.pm[k].grad, TOL, 'grad ' + k)
        else:
            assert prm.grad is None or float(prm.grad.abs().max()) == 0.0
    for k, prm in cnn.named_parameters():
        close(prm.grad, oracle.pc[k].grad, TOL, 'cnn grad ' + k)
    for k, v in cnn.state_dict().items():
        if 'running' in k:
            close(v, oracle.pc[k], TOL, 'cnn ' + k)


def test_flat_adam_matches_torch(dev):
    """mmft_adam_step against torch.optim.Adam on identical gradients, 5 steps, with weight decay."""
    from mmft.fusion import FlatAdam
    torch.manual_seed(3)
    shapes = [(37, 5), (128,), (16, 3, 3, 3), (1,)]
    ps = [torch.randn(s, device=dev).requires_grad_(True) for s in shapes]
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    qs[2].data = qs[2].data.contiguous(memory_format=torch.channels_last)
    ref = torch.optim.Adam(ps, 1e-3, weight_decay=0.01)
    mine = FlatAdam(qs, lr=1e-3, weight_decay=0.01)
    for it in range(5):
        gs = [torch.randn(s, device=dev) for s in shapes]
        for p, q, g in zip(ps, qs, gs):
            p.grad = g.clone()
            q.grad.copy_(g)
        ref.step()
        mine.step()
    for p, q in zip(ps, qs):
        close(q, p, 1e-6, 'adam')


def test_gradient_sinks_shared_weights_and_second_backward(dev):
    """mmft.gradsink: with FlatAdam the backward kernels store into the flat buffer.  A weight used twice in one
    graph, a second backward without zero_grad (retain_graph, src/train.py:553) and a conv / BatchNorm / ConvT
    stack must leave the same .grad as plain autograd accumulation (torch modules, fp64)."""
    import torch.nn as nn
    from mmft.fusion import FlatAdam
    from mmft.functional import linear_act
    from mmft import cnn as C
    torch.manual_seed(11)
    lin = nn.Linear(24, 24).to(dev)
    conv = nn.Conv2d(4, 8, 3, padding=1).to(dev).to(memory_format=torch.channels_last)
    bn = nn.BatchNorm2d(8).to(dev)
    up = nn.ConvTranspose2d(8, 4, 2, stride=2).to(dev)
    up.weight.data = up.weight.data.permute(2, 3, 1, 0).contiguous().permute(3, 2, 0, 1)
    params = list(lin.parameters()) + list(conv.parameters()) + list(bn.parameters()) + list(up.parameters())
    ref = [p.detach().double().clone().requires_grad_(True) for p in params]
    x = torch.randn(50, 24, device=dev)
    img = torch.randn(2, 4, 8, 8, device=dev)
    opt = FlatAdam(params, lr=1e-3)

    def mine():
        y = linear_act(linear_act(x, lin.weight, lin.bias, 0.0), lin.weight, lin.bias, None)      # shared weight
        z = C.conv_transpose2x2(C.bn_relu(C.conv2d(img, conv.weight, conv.bias, 1), bn), up.weight, up.bias)
        return (y * y).sum() + (z * z).sum()

    def theirs():
        lw, lb, cw, cb, g, b, uw, ub = ref
        F = torch.nn.functional
        y = F.linear(F.relu(F.linear(x.double(), lw, lb)), lw, lb)
        z = F.conv2d(img.double(), cw, cb, padding=1)
        z = F.relu(F.batch_norm(z, None, None, g, b, training=True, eps=bn.eps))
        z = F.conv_transpose2d(z, uw, ub, stride=2)
        return (y * y).sum() + (z * z).sum()

    opt.zero_grad()
    loss = mine()
    loss.backward(retain_graph=True)
    loss.backward()                                   # accumulates on top of the first
    lr = theirs()
    lr.backward(retain_graph=True)
    lr.backward()
    def check(scale):
        for p, r in zip(params, ref):
            if float(r.grad.abs().max()) < 1e-9:          # conv bias in front of BatchNorm: exactly zero in theory
                assert float(p.grad.abs().max()) < 1e-3
            else:
                close(p.grad, scale * r.grad.float(), 2e-5, 'sink grad')

    check(1.0)
    opt.zero_grad()                                   # a new step stores again (no stale accumulation)
    mine().backward()
    check(0.5)


@pytest.mark.parametrize('B', [1, 3])
def test_sweep_entry_equals_dropin(dev, B):
    """PathModel.forward_sweep (whole-sweep entry) vs the per-level drop-in loop: same predictions and
    gradients, for one design and for several designs merged block-diagonally (per-image BN statistics)."""
    from mmft.synth import synth_design
    from mmft.train import build_models, TrainStep
    from mmft.fusion import mse_loss
    designs = [synth_design(N=2048, L=12, tile=32, seed=100 + i, end_frac=0.25) for i in range(B)]
    rng = np.random.default_rng(5)
    ids = [rng.permutation(d.num_paths)[:40].tolist() + [0, 0] for d in designs]      # with duplicates
    res = {}
    for mode in ('dropin', 'sweep'):
        pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=7)
        ts = TrainStep(pmodel, cnn, designs, dev, mode=mode)
        hats, ends_d, ends_h = ts.forward(ids)
        loss = mse_loss(hats, ts.batch.arrival[ends_d.long()].squeeze(-1))
        ts.optim.zero_grad()
        loss.backward()
        grads = {k: p.grad.clone() for k, p in list(pmodel.named_parameters()) + [('cnn.' + a, b) for a, b in cnn.named_parameters()]
                 if p.grad is not None}
        res[mode] = (hats.detach().clone(), grads, ts.h.clone())
    close(res['sweep'][0], res['dropin'][0], 1e-5, 'hats')
    close(res['sweep'][2], res['dropin'][2], 1e-5, 'h')
    assert set(res['sweep'][1]) == set(res['dropin'][1])
    for k in res['dropin'][1]:
        close(res['sweep'][1][k], res['dropin'][1][k], 5e-5, 'grad ' + k)


def test_batched_designs_equal_single(dev):
    """Merging designs block-diagonally (per-image BatchNorm statistics) gives every design the predictions it
    gets when stepped alone, as the reference does (one design at a time)."""
    from mmft.synth import synth_design
    from mmft.train import build_models, TrainStep
    designs = [synth_design(N=2048, L=12, tile=32, seed=200 + i, end_frac=0.25) for i in range(3)]
    rng = np.random.default_rng(6)
    ids = [rng.permutation(d.num_paths)[:30].tolist() for d in designs]
    pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=7)
    sd_m = {k: v.clone() for k, v in pmodel.state_dict().items()}
    sd_c = {k: v.clone() for k, v in cnn.state_dict().items()}
    ts = TrainStep(pmodel, cnn, designs, dev)
    with torch.no_grad():
        hats_all, ends_d, ends_h = ts.forward(ids)
    for i, d in enumerate(designs):
        pm_i, cnn_i = build_models(map_size=d.map_size, device=dev, seed=7)
        pm_i.load_state_dict(sd_m); cnn_i.load_state_dict(sd_c)
        t1 = TrainStep(pm_i, cnn_i, [d], dev)
        with torch.no_grad():
            h1, e1, eh1 = t1.forward([ids[i]])
        # rows of design i inside the merged batch: endpoints in [node_off[i], node_off[i+1])
        lo, hi = ts.batch.node_off[i], ts.batch.node_off[i + 1]
        sel = torch.from_numpy(((ends_h >= lo) & (ends_h < hi))).to(dev)
        assert (ends_h[(ends_h >= lo) & (ends_h < hi)] - lo).tolist() == eh1.tolist()
        close(hats_all[sel], h1, 2e-5, f'design {i}')


def test_graphed_step_equals_eager(dev):
    """GraphedTrainStep (whole step replayed from one HIP graph) follows the eager TrainStep step for step."""
    from mmft.synth import synth_design
    from mmft.train import build_models, TrainStep, GraphedTrainStep
    designs = [synth_design(N=2048, L=12, tile=32, seed=300 + i, end_frac=0.25) for i in range(2)]
    rng = np.random.default_rng(9)
    batches = [[rng.permutation(d.num_paths)[:32].tolist() for d in designs] for _ in range(6)]
    out = {}
    for kind in ('eager', 'graph'):
        pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=11)
        ts = TrainStep(pmodel, cnn, designs, dev)
        losses = []
        if kind == 'graph':
            gs = GraphedTrainStep(ts, batches[0], warmup=0)     # capture only (no extra optimizer steps)
            stepper = gs
        else:
            stepper = ts
            ts.forward(batches[0])                              # the capture's dry run also advances BN running stats
        for ids in batches:
            loss, hats, tl = stepper.step(ids)
            losses.append(float(loss))
        out[kind] = (losses, hats.clone(), {k: v.clone() for k, v in pmodel.state_dict().items()})
    np.testing.assert_allclose(out['graph'][0], out['eager'][0], rtol=2e-4)
    close(out['graph'][1], out['eager'][1], 2e-4, 'hats after 6 steps')


def test_eval_metrics_match_reference_formulas(dev):
    """mmft.evaluate (one sums kernel) against the reference's metric formulas computed with torch on the host."""
    from mmft.evaluate import eval_sums, metrics_from_sums
    torch.manual_seed(0)
    n = 5000
    y = torch.rand(n) * 2 + 0.1
    p = y + 0.2 * torch.randn(n)
    req = torch.full((n,), 1.2)
    lab = ((req - y) < 0).float()
    m = metrics_from_sums(eval_sums(p.to(dev), y.to(dev), req.to(dev), lab.to(dev)).cpu().tolist())
    pd, yd = p.double(), y.double()
    assert abs(m['loss'] - float(((pd - yd) ** 2).mean())) < 1e-9
    assert abs(m['r2'] - float(R.r2_score(pd, yd))) < 1e-9
    assert abs(m['endpoint_slack_mae'] - float((pd - yd).abs().mean())) < 1e-9
    pc = R.judge_critical(p, req)                              # src/train.py:391-395
    tp = int(((pc != 0) & (lab != 0)).sum()); fn = int(((pc == 0) & (lab != 0)).sum())
    fp = int(((pc != 0) & (lab == 0)).sum()); tn = int(((pc == 0) & (lab == 0)).sum())
    assert (m['tp'], m['fp'], m['tn'], m['fn']) == (tp, fp, tn, fn)
    assert abs(m['recall'] - tp / (tp + fn)) < 1e-12 and abs(m['precision'] - tp / (tp + fp)) < 1e-12


def test_per_level_metrics_and_validate_loop(dev):
    """Per-level R2 / MAPE (src/test.py:211-216) from the segmented sums kernel against the reference's formulas, and the
    per-design validate() loop (src/train.py:137-291) against the fp64 oracle's predictions on every design."""
    from mmft.evaluate import eval_sums_by_level, level_metrics_from_sums, validate_designs
    from mmft.synth import synth_design
    from mmft.train import build_models
    torch.manual_seed(1)
    n, L = 3000, 9
    lv = torch.randint(0, L, (n,), dtype=torch.int32)
    lv[lv == 4] = 5                                                   # an empty level
    lv[:1] = 7
    lv[1:][lv[1:] == 7] = 6                                           # a level with ONE prediction: not reported
    y = torch.rand(n) * 2 + 0.1
    p = y + 0.2 * torch.randn(n)
    req = torch.full((n,), 1.2)
    lab = ((req - y) < 0).float()
    rows = eval_sums_by_level(p.to(dev), y.to(dev), req.to(dev), lab.to(dev), lv.to(dev), L).cpu().tolist()
    got = {m['level']: m for m in level_metrics_from_sums(rows)}
    assert 4 not in got and 7 not in got
    for l in range(L):
        sel = lv == l
        if int(sel.sum()) < 2:
            continue
        pd, yd = p[sel].double(), y[sel].double()
        assert got[l]['n'] == int(sel.sum())
        assert abs(got[l]['r2'] - float(R.r2_score(pd, yd))) < 1e-9
        assert abs(got[l]['mape'] - float(((pd - yd) / yd).abs().mean())) < 1e-9
    # validate(): one batch per design over all of its paths
    designs = [synth_design(N=2048, L=12, tile=32, seed=600 + i, end_frac=0.25) for i in range(2)]
    pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=13)
    pm_state = {k: v.detach().cpu().clone() for k, v in pmodel.state_dict().items()}
    pc_state = {k: v.detach().cpu().clone() for k, v in cnn.state_dict().items()}
    res = validate_designs(pmodel, cnn, designs, dev)
    assert len(res['cases']) == 2 and set(res['overall']) >= {'loss', 'r2', 'f1', 'endpoint_slack_mae'}
    for d, case in zip(designs, res['cases']):
        orc = R.OracleTrainer(pm_state, pc_state, dtype=torch.float64)
        with torch.no_grad():
            hats, tl, _ = R.sweep_forward(orc.pm, orc.pc, d, R.design_csr(d), list(range(d.num_paths)), update_running=False,
                                          dtype=torch.float64)
        arr = torch.from_numpy(d.arrival_time).double()[torch.tensor(tl)].squeeze(-1)
        assert case['n'] == d.num_paths
        assert abs(case['loss'] - float(((hats - arr) ** 2).mean())) < 1e-4 * float(((hats - arr) ** 2).mean()) + 1e-9
        assert abs(case['endpoint_slack_mae'] - float((hats - arr).abs().mean())) < 1e-4
        lvl = torch.from_numpy(d.path2level[np.argsort(d.path2level, kind='stable')])
        for m in case['levels']:
            sel = lvl == m['level']
            assert m['n'] == int(sel.sum())
            assert abs(m['mape'] - float(((hats[sel] - arr[sel]) / arr[sel]).abs().mean())) < 1e-4
    assert abs(res['overall']['loss'] - np.mean([c['loss'] for c in res['cases']])) < 1e-12


def test_classification_task(dev):
    """--task cls (src/train.py:32,513-519; src/options.py:32,49): a 2-wide head, CrossEntropy on ndata['label'], argmax
    prediction.  Loss and gradients of one step against the fp64 oracle, then a few optimizer steps and the evaluation."""
    from mmft.synth import synth_design
    from mmft.train import build_models, TrainStep, GraphedTrainStep
    from mmft.evaluate import validate
    d = synth_design(N=4096, L=16, tile=32, seed=41, end_frac=0.25)
    # make ~40 % of the endpoints "critical" so that both classes occur
    ends = d.path2endpoint
    d.label[ends[::5], 0] = 1
    d.label[ends[1::5], 0] = 1
    pmodel, cnn = build_models(map_size=d.map_size, device=dev, seed=17, nlabels=2)
    pm_state = {k: v.detach().cpu().clone() for k, v in pmodel.state_dict().items()}
    pc_state = {k: v.detach().cpu().clone() for k, v in cnn.state_dict().items()}
    ts = TrainStep(pmodel, cnn, [d], dev, task='cls')
    ids = np.random.default_rng(3).permutation(d.num_paths)[:96].tolist()
    hats, ends_d, ends_h = ts.forward([ids])
    assert tuple(hats.shape) == (96, 2)
    loss = ts.loss(hats, ends_d)
    ts.optim.zero_grad()
    loss.backward()
    orc = R.OracleTrainer(pm_state, pc_state, dtype=torch.float64)
    hats_o, tl, _ = orc.forward(d, R.design_csr(d), ids)
    assert ends_h.tolist() == tl
    lab = torch.from_numpy(d.label)[torch.tensor(tl)].squeeze(-1)
    loss_o = torch.nn.functional.cross_entropy(hats_o, lab)
    loss_o.backward()
    close(hats, hats_o, TOL, 'logits')
    close(loss, loss_o, TOL, 'cross entropy')
    for k in ('mlp_fuse.layers.2.weight', 'mlp_fuse.layers.0.bias', 'fcn.weight', 'gnn.fc_cell_neigh.layers.0.weight'):
        close(dict(pmodel.named_parameters())[k].grad, orc.pm[k].grad, 2e-4, k)
    close(cnn.inc.double_conv[0].weight.grad, orc.pc['inc.double_conv.0.weight'].grad, 5e-4, 'cnn grad')
    # training + evaluation
    rng = np.random.default_rng(4)
    gs = GraphedTrainStep(ts, [ids], warmup=0)
    losses = [float(gs.step([rng.permutation(d.num_paths)[:96].tolist()])[0]) for _ in range(30)]
    assert np.mean(losses[-5:]) < np.mean(losses[:5])
    ev = TrainStep(pmodel, cnn, [d], dev, overlap=False, with_optimizer=False, task='cls')
    m = validate(ev)
    with torch.no_grad():
        z, e_d, _ = ev.forward([np.arange(d.num_paths)])
        y = ev.batch.graph.ndata['label'][e_d.long()].squeeze(-1)
    pred = torch.argmax(torch.softmax(z, 1), dim=1)                                     # src/train.py:516
    assert m['n'] == d.num_paths and abs(m['acc'] - float((pred == y).double().mean())) < 1e-9
    assert (m['tp'], m['fn']) == (int(((pred != 0) & (y != 0)).sum()), int(((pred == 0) & (y != 0)).sum()))
    assert abs(m['loss'] - float(torch.nn.functional.cross_entropy(z.double(), y))) < 1e-5


def test_training_trajectory_vs_oracle(dev):
    """20 Adam steps on one small design: HIP path vs the fp64 CPU oracle, same init / data / batch order.
    Loss trajectory and held-out endpoint-slack MAE must track (the accuracy half of BASELINE.json's metric)."""
    from mmft.synth import synth_design
    from mmft.train import build_models, TrainStep
    from mmft.evaluate import validate
    d = synth_design(N=2048, L=12, tile=32, seed=41, end_frac=0.5)
    pmodel, cnn = build_models(map_size=d.map_size, device=dev, seed=9294)
    pm_state = {k: v.detach().cpu().clone() for k, v in pmodel.state_dict().items()}
    pc_state = {k: v.detach().cpu().clone() for k, v in cnn.state_dict().items()}
    oracle = R.OracleTrainer(pm_state, pc_state, dtype=torch.float64)
    csr = R.design_csr(d)
    ts = TrainStep(pmodel, cnn, [d], dev)
    rng = np.random.default_rng(0)
    lo, lg = [], []
    for it in range(20):
        ids = rng.permutation(d.num_paths)[:64].tolist()
        l_o, _, _ = oracle.step(d, csr, ids)
        l_g, _, _ = ts.step([ids])
        lo.append(l_o); lg.append(float(l_g))
    np.testing.assert_allclose(lg, lo, rtol=2e-2, atol=1e-4)   # fp32 vs fp64 trajectories, losses down to 1e-3
    assert lo[-1] < lo[0]                                       # it learns
    m = validate(ts)
    hats_o, tl_o, _ = oracle.forward(d, csr, list(range(d.num_paths)))
    mae_o = float((hats_o.detach() - torch.from_numpy(d.arrival_time).double()[torch.tensor(tl_o)].squeeze(-1)).abs().mean())
    assert abs(m["endpoint_slack_mae"] - mae_o) < 2e-2 * max(mae_o, 1e-6) + 1e-4


def test_reference_style_training_loop(dev):
    """The reference's own loop shape (src/train.py:431-443,461-562) run verbatim against the drop-in modules:
    torch.optim.Adam over chain(model, cnn), nn.MSELoss, DataLoader(PathDataset) batches, dense
    `path_mask.to_dense()*feat_map`, per-level model(...) calls, loss.backward(retain_graph=True), fresh zero
    ndata['h'] and a re-run of the CNN after every step.  Three steps vs the fp64 oracle on the same batches."""
    import itertools
    import model as M
    from MyDataloader import PathDataset
    from torch.utils.data import DataLoader
    from mmft.synth import synth_design
    from mmft.train import build_models
    d = synth_design(N=2048, L=10, tile=32, seed=61, end_frac=0.5)
    pmodel, cnn = build_models(map_size=d.map_size, device=dev, seed=9294)
    oracle = R.OracleTrainer({k: v.detach().cpu().clone() for k, v in pmodel.state_dict().items()},
                             {k: v.detach().cpu().clone() for k, v in cnn.state_dict().items()}, dtype=torch.float64)
    csr = R.design_csr(d)
    graph = PinGraph.from_synth(d).to(dev)
    topo_levels = d.topo_levels()
    path2level = {p: int(l) for p, l in enumerate(d.path2level)}
    path2endpoint = {p: int(e) for p, e in enumerate(d.path2endpoint)}
    rows = np.repeat(np.arange(d.num_paths), np.diff(d.mask_indptr))
    path_masks = torch.sparse_coo_tensor(np.stack([rows, d.mask_cols]), torch.ones(rows.shape[0], dtype=torch.int64),
                                         (d.num_paths, d.map_size ** 2)).coalesce()
    cnn_inputs = torch.from_numpy(d.image)
    Loss = torch.nn.MSELoss()
    optim = torch.optim.Adam(itertools.chain(pmodel.parameters(), cnn.parameters()), 1e-3, weight_decay=0)
    cnn.train(); pmodel.train()
    torch.manual_seed(0)
    loader = DataLoader(PathDataset(list(range(d.num_paths))), batch_size=48, shuffle=True, drop_last=True)
    graph.ndata['h'] = torch.zeros((graph.number_of_nodes(), 128), dtype=torch.float).to(dev)
    feat_map = cnn(cnn_inputs.to(dev)).reshape((1, -1))
    losses, losses_o = [], []
    for bidx, path_ids in enumerate(loader):
        if bidx == 3:
            break
        path_ids = list(path_ids.numpy().tolist())
        sampled_ends, sampled_paths = {}, {}
        for pathid in path_ids:
            level, endpoint = path2level[pathid], path2endpoint[pathid]
            sampled_ends.setdefault(level, []).append(endpoint)
            sampled_paths.setdefault(level, []).append(pathid)
        label_hats, target_list = None, []
        for level_id, level in enumerate(topo_levels):
            nodes, eids = level[:2]
            targets, paths = sampled_ends.get(level_id, []), sampled_paths.get(level_id, [])
            target_list.extend(targets)
            if len(paths) == 0:
                path_map = None
            else:
                path_mask = torch.index_select(path_masks, 0, torch.tensor(paths)).to(dev)
                path_map = path_mask.to_dense() * feat_map
            cur = pmodel(graph, nodes, eids, targets, level_id,
                         torch.tensor(level_id, dtype=torch.float).unsqueeze(0).to(dev), path_map)
            if len(paths) == 0:
                continue
            label_hats = cur if label_hats is None else torch.cat((label_hats, cur), dim=0)
        arrival_time = graph.ndata['arrival_time'][target_list].squeeze()
        train_loss = Loss(label_hats, arrival_time)
        optim.zero_grad()
        train_loss.backward(retain_graph=True)
        optim.step()
        losses.append(float(train_loss.detach()))
        graph.ndata['h'] = torch.zeros((graph.number_of_nodes(), 128), dtype=torch.float).to(dev)
        feat_map = cnn(cnn_inputs.to(dev)).reshape((1, -1))
        lo, _, tl_o = oracle.step(d, csr, path_ids)      # its CNN forward = the feat_map computed before this step
        assert tl_o == target_list
        losses_o.append(lo)
    R.unet_forward(oracle.pc, torch.from_numpy(d.image).double())    # the loop's trailing cnn(...) call
    np.testing.assert_allclose(losses, losses_o, rtol=2e-3)
    sd = cnn.state_dict()
    close(sd['inc.double_conv.1.running_var'], oracle.pc['inc.double_conv.1.running_var'], 1e-3, 'running_var')
    assert int(sd['inc.double_conv.1.num_batches_tracked']) == int(oracle.pc['inc.double_conv.1.num_batches_tracked'])


def test_dropin_loop_with_changing_level_lists(dev):
    """the drop-in loop speculates that a graph is swept with the same level lists every step.  A training step
    whose list differs at a LATER level cannot be completed from the speculative sweep: it raises once, speculation is
    switched off for that graph, and the same step run again (fresh h) takes the strict per-level path and equals the
    whole-sweep entry on the same lists."""
    from mmft.synth import synth_design
    from mmft.train import build_models, TrainStep
    from mmft.fusion import mse_loss
    d = synth_design(N=2048, L=12, tile=32, seed=321, end_frac=0.25)
    ids = [np.random.default_rng(3).permutation(d.num_paths)[:40].tolist()]
    pmodel, cnn = build_models(map_size=d.map_size, device=dev, seed=7)
    ts = TrainStep(pmodel, cnn, [d], dev, mode='dropin')
    for _ in range(2):                                   # records the lists, then sweeps speculatively
        ts.step(ids)
    assert ts.batch.graph.__dict__.get('_spec_lists') is not None
    full = list(ts.batch.level_nodes[5])
    ts.batch.level_nodes[5] = list(reversed(full))       # same nodes, another list object with another order
    with pytest.raises(RuntimeError, match='Speculation is now disabled'):
        ts.step(ids)
    assert ts.batch.graph.__dict__.get('_spec_disabled')
    hats, ends_d, _ = ts.forward(ids)                    # the retry: strict per-level execution
    loss = mse_loss(hats, ts.batch.arrival[ends_d.long()].squeeze(-1))
    ts.optim.zero_grad()
    loss.backward()
    got = {k: p.grad.clone() for k, p in pmodel.named_parameters() if p.grad is not None}
    state = {k: v.clone() for k, v in pmodel.state_dict().items()}, {k: v.clone() for k, v in cnn.state_dict().items()}
    pm2, cnn2 = build_models(map_size=d.map_size, device=dev, seed=7)
    pm2.load_state_dict(state[0]); cnn2.load_state_dict(state[1])
    ts2 = TrainStep(pm2, cnn2, [d], dev, mode='sweep')
    ts2.batch.level_nodes[5] = list(reversed(full))
    hats2, ends2, _ = ts2.forward(ids)
    loss2 = mse_loss(hats2, ts2.batch.arrival[ends2.long()].squeeze(-1))
    ts2.optim.zero_grad()
    loss2.backward()
    close(hats, hats2, 1e-5, 'hats')
    for k, g in got.items():
        close(g, dict(pm2.named_parameters())[k].grad, 5e-5, 'grad ' + k)


def test_dropin_unet_graph_replay_in_bf16_mode(dev):
    """bf16 mode, eager callers: from the second step on UNet.forward / backward replay captured HIP graphs
    (mmft.unet16._Replay).  Five drop-in steps with replay equal five steps without it bit for bit, an evaluation forward in
    between (no-grad, other geometry) does not disturb it, and two forwards before a backward fall back to fresh buffers."""
    from mmft import lib, unet16
    from mmft.synth import synth_design
    from mmft.train import build_models, TrainStep
    d = synth_design(N=2048, L=12, tile=64, seed=322, end_frac=0.25)
    rng = np.random.default_rng(4)
    batches = [[rng.permutation(d.num_paths)[:40].tolist()] for _ in range(5)]
    out = {}
    with lib.math_mode('bf16'):
        for replay in (True, False):
            unet16.REPLAY = replay
            try:
                pmodel, cnn = build_models(map_size=d.map_size, device=dev, seed=9)
                ts = TrainStep(pmodel, cnn, [d], dev, mode='dropin')
                losses = []
                for i, ids in enumerate(batches):
                    losses.append(float(ts.step(ids)[0]))
                    if i == 2:
                        with torch.no_grad():
                            cnn(torch.rand(1, 3, 32, 64, device=dev))
                rp = cnn.__dict__.get('_u16_replay')
                assert (rp is not None and rp.fwd.graph is not None and rp.bwd.graph is not None) == replay
                out[replay] = (losses, ts.optim.flat_param.clone())
                if replay:                                   # two forwards, then both backwards: the second takes fresh buffers
                    x = ts.batch.images
                    y1 = cnn(x)
                    y2 = cnn(x)
                    (y1.sum() + y2.sum()).backward()
                    assert torch.equal(y1, y2)
            finally:
                unet16.REPLAY = True
    assert out[True][0] == out[False][0] and torch.equal(out[True][1], out[False][1])


def test_dropin_sweep_opt_in_paths_equal_the_default(dev):
    """The opt-in forms of the speculative drop-in sweep - on a stream of its own (sweep.SPEC_SIDE_STREAM: the engine joins it
    at the end of backward through the sweep node's anchor leaf), replayed from captured HIP graphs (sweep.SWEEP_REPLAY),
    without the recorded launches (sweep.RECORD_LAUNCHES = False) - train exactly like the default: the same losses and
    parameters after six steps, bit for bit."""
    from mmft import lib, sweep as S
    from mmft.synth import synth_design
    from mmft.train import build_models, TrainStep
    designs = [synth_design(N=6000, L=12, tile=64, seed=420 + i, end_frac=0.2) for i in range(2)]
    rng = np.random.default_rng(7)
    batches = [[rng.permutation(d.num_paths)[:60] for d in designs] for _ in range(6)]
    out = {}
    saved = (S.SPEC_SIDE_STREAM, S.SWEEP_REPLAY, S.RECORD_LAUNCHES)
    try:
        with lib.math_mode('bf16'):
            for name, flags in (('default', saved), ('side', (True, False, True)), ('replay', (True, True, True)),
                                ('plain', (False, False, False))):
                S.SPEC_SIDE_STREAM, S.SWEEP_REPLAY, S.RECORD_LAUNCHES = flags
                pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=11)
                ts = TrainStep(pmodel, cnn, designs, dev, mode='dropin')
                losses = [float(ts.step(ids)[0]) for ids in batches]
                torch.cuda.synchronize()
                rp = ts.batch.graph.__dict__.get('_sweep_bufs', {}).get('replay')
                if name == 'replay':
                    assert rp is not None and rp.fwd.graph is not None and rp.bwd.graph is not None   # captured and used
                out[name] = (losses, ts.optim.flat_param.clone())
    finally:
        S.SPEC_SIDE_STREAM, S.SWEEP_REPLAY, S.RECORD_LAUNCHES = saved
    for name in ('side', 'replay', 'plain'):
        assert out[name][0] == out['default'][0], name
        assert torch.equal(out[name][1], out['default'][1]), name


def test_dropin_replayed_graphs_own_their_scratch_and_tables(dev):
    """bf16 drop-in loop: the sweep's reverse graph (replayed on the sweep's own stream) and the U-Net's backward graph
    (replayed on the caller's stream, concurrently) each own their scratch - disjoint buffers, neither a stream-keyed
    lib.workspace buffer.  The sweep record keeps the slot and pair tables its recorded launches and graphs read: once
    PinGraph's schedule cache has dropped them, one more step still equals training without replay bit for bit."""
    from mmft import lib, sweep as S, unet16
    from mmft.synth import synth_design
    from mmft.train import build_models, TrainStep
    designs = [synth_design(N=6000, L=12, tile=64, seed=420 + i, end_frac=0.2) for i in range(2)]
    rng = np.random.default_rng(7)
    batches = [[rng.permutation(d.num_paths)[:60] for d in designs] for _ in range(6)]
    span = lambda t: (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())
    disjoint = lambda a, b: span(a)[1] <= span(b)[0] or span(b)[1] <= span(a)[0]
    out = {}
    saved = (S.SWEEP_REPLAY, unet16.REPLAY)
    try:
        with lib.math_mode('bf16'):
            for replay in (False, True):
                S.SWEEP_REPLAY = unet16.REPLAY = replay
                pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=11)
                ts = TrainStep(pmodel, cnn, designs, dev, mode='dropin')
                losses = [float(ts.step(ids)[0]) for ids in batches[:5]]
                g = ts.batch.graph
                rec = g._sweep_bufs['replay']
                tables = rec.keep
                if replay:
                    u16 = cnn._u16_replay
                    assert rec.bwd.graph is not None and u16.bwd.graph is not None
                    a, b = rec.bwd.scratch, u16.bwd.scratch
                    assert disjoint(a, b)
                    assert all(disjoint(a, w) and disjoint(b, w) for w in list(lib._workspace.values()) + lib._retired)
                    assert tables[0] is g.level_slots(rec.lists) and tables[1] is g.level_bwd_pairs(rec.lists)
                for _ in range(g.LIST_CACHE_MAX):             # the same schedule in new list objects: other cache entries
                    other = [list(n) for n in rec.lists]
                    g.level_slots(other)
                    g.level_bwd_pairs(other)
                assert ('slots',) + g._lists_key(rec.lists) not in g._level_cache
                assert ('bwd_pairs',) + g._lists_key(rec.lists) not in g._level_cache
                losses.append(float(ts.step(batches[5])[0]))
                torch.cuda.synchronize()
                assert g._sweep_bufs['replay'] is rec and rec.keep[0] is tables[0] and rec.keep[1] is tables[1]
                out[replay] = (losses, ts.optim.flat_param.clone())
    finally:
        S.SWEEP_REPLAY, unet16.REPLAY = saved
    assert out[True][0] == out[False][0]
    assert torch.equal(out[True][1], out[False][1])


def test_forward_sweep_takes_endpoints_in_any_order(dev):
    """PathModel.forward_sweep is a public entry: the same endpoints shuffled (with their levels, path-map rows and loss
    weights) give the predictions of the level-ordered call, permuted, and the same mlp_alpha gradients.  fuse_heads'
    sorted segment sum (gather_rows(..., ascending=True)) is only right for callers that order the endpoints by level."""
    from mmft.synth import synth_design
    from mmft.train import build_models
    d = synth_design(N=2048, L=12, tile=32, seed=61, end_frac=0.25)
    pmodel, _ = build_models(map_size=d.map_size, device=dev, seed=5)
    g = PinGraph.from_synth(d, out_dim=128).to(dev)
    levels = [l.tolist() for l in d.levels]
    rng = np.random.default_rng(3)
    pids = rng.permutation(d.num_paths)[:64]
    pids = pids[np.argsort(d.path2level[pids], kind='stable')]
    ends = torch.from_numpy(d.path2endpoint[pids].astype(np.int32))
    lvs = torch.from_numpy(d.path2level[pids].astype(np.int32))
    assert len(set(lvs.tolist())) > 3
    pmap = torch.rand(len(pids), d.map_size ** 2, generator=torch.Generator().manual_seed(4))
    w = torch.randn(len(pids), generator=torch.Generator().manual_seed(5))

    def run(perm):
        g.ndata['h'] = torch.zeros((d.N, 128), device=dev)
        pmodel.zero_grad()
        hats = pmodel.forward_sweep(g, levels, ends[perm].to(dev), lvs[perm].to(dev), pmap[perm].to(dev))
        (hats * w[perm].to(dev)).sum().backward()
        return hats.detach(), {k: p.grad.detach().clone() for k, p in pmodel.mlp_alpha.named_parameters()}
    perm = torch.from_numpy(rng.permutation(len(pids)))
    assert not bool((lvs[perm][1:] >= lvs[perm][:-1]).all())
    h0, g0 = run(torch.arange(len(pids)))
    h1, g1 = run(perm)
    assert rel_err(h1, h0[perm.to(dev)]) < 1e-6
    for k in g0:
        assert float(g0[k].abs().max()) > 0 and rel_err(g1[k], g0[k]) < 1e-6, k
