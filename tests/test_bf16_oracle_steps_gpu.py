"""bf16 math mode against the fp64 rounding oracle beyond one eager step on one design: the bench's batch of eight designs,
a teacher-forced Adam trajectory (eager and replayed from a HIP graph) and the drop-in entry.

The bound rule, the three oracle runs (e_hip / e_32 / e_plain) and the ceilings are those of tests/test_bf16_oracle_gpu.py.
The sweep + head rows are DECOUPLED: every design's three oracle runs take that design's image of the HIP step's feature
map, the per-design results are merged as the batch merges them (predictions through the endpoint ids, loss and gradients
weighted by the design's share of the endpoints), and d loss / d feature map is one row per image.  The U-Net rows run the
oracle U-Net image by image (per-image statistics, running statistics updated image after image) and drive its backward
with the HIP step's own d loss / d feature map: the U-Net is judged on the inputs the HIP U-Net had.

Teacher forcing: before step k the HIP state - parameters (FlatAdam.flat_param), Adam moments (m, v through
FlatAdam.offsets), the device step counter (FlatAdam.state) and the BatchNorm running statistics - is copied to the CPU;
all three oracle runs start from it (OracleTrainer.load_adam), take step k's feature map and run one step.  The update
rows compare  theta_{k+1} - theta_k  per tensor in relative L2: Adam divides every element by its own sqrt(v), so an
element with a near-zero gradient moves by up to lr on a last-bit difference of that gradient and a max norm would measure
the smallest gradients, not the arithmetic.  The update carries the bias corrections of step k + 1, so a wrong device
counter moves every row.

Measured on one MI355X (e_hip / e_32 / e_plain; max over a group's rows, the smallest e_plain): see each test's docstring.
No row needed a floor above 3 e_32 beyond the existing ones except the GNN / head updates (update_rows: 1e-3).
"""
import numpy as np
import pytest
import torch

from conftest import rel_err
from mmft import lib
from oracle import bf16 as B
from oracle import restatement as R
from test_bf16_oracle_gpu import Bounds, STEP_KERNELS, UNET_PREFIX, oracle_step, rel_l2, unet_grad_rows

pytestmark = pytest.mark.gpu

EVERY_CLASS = 'bf16'
NO_HIDDEN = tuple(c for c in B.CLASSES if c != 'hidden')      # st.hid16 off: fc_cell_neigh's HN / DHN stay fp32


def flat_params(ts):
    """(name, parameter, offset in the flat buffers) in FlatAdam order, state-dict names of PathModel and the U-Net."""
    names = {id(p): n for n, p in list(ts.pmodel.named_parameters()) + list(ts.cnn.named_parameters())}
    return [(names[id(p)], p, o) for p, o in zip(ts.optim.params, ts.optim.offsets)]


def snapshot(ts):
    """The HIP state a step starts from, on the CPU: state dicts (parameters and running statistics), Adam moments per
    parameter name (read from the flat buffers through FlatAdam.offsets) and the device step counter."""
    o = ts.optim
    torch.cuda.synchronize()
    view = lambda buf, p, off: torch.as_strided(buf, p.shape, p.stride(), off).detach().cpu().clone()
    fp = flat_params(ts)
    return dict(pm={k: v.detach().cpu().clone() for k, v in ts.pmodel.state_dict().items()},
                pc={k: v.detach().cpu().clone() for k, v in ts.cnn.state_dict().items()},
                m={n: view(o.m, p, off) for n, p, off in fp}, v={n: view(o.v, p, off) for n, p, off in fp},
                step=int(o.state[0, 0]), flat=o.flat_param.clone())


def hip_train_step(ts, ids, profile=False):
    """One TrainStep.step (forward, loss, backward, Adam) with the U-Net output and its gradient kept."""
    feats = []

    def keep(module, inputs, out):
        out.retain_grad()
        feats.append(out)
    hook = ts.cnn.register_forward_hook(keep)
    if profile:
        lib.prof_reset()
        lib.prof_enable(True)
    try:
        loss, hats, ends_h = ts.step(ids)
        torch.cuda.synchronize()
    finally:
        if profile:
            lib.prof_enable(False)
        hook.remove()
    names = {r['name'].split('<')[0] for r in lib.prof_report()} if profile else set()
    assert len(feats) == 1 and feats[0].grad is not None
    f = feats[0]
    out = dict(hats=hats.double().cpu(), loss=float(loss), ends=list(ends_h),
               grads={n: p.grad.detach().double().cpu().clone() for n, p, _ in flat_params(ts)},
               run={k: v.detach().double().cpu() for k, v in ts.cnn.state_dict().items() if 'running' in k},
               feat=f.detach().float().cpu().reshape(f.shape[0], -1), feat_grad=f.grad.double().cpu().reshape(f.shape[0], -1))
    return out, names


def oracle_step_alpha_cut(d, ids, pm, pc, rounding, dtype, feat):
    """oracle_step with mlp_alpha's output of every level cut loose (a leaf): returns {level: d loss / d alpha(level)} as
    'alpha_grad' and no mlp_alpha gradients - those are taken after the designs are merged (oracle_sweep_head)."""
    real, cut = R.mlp, {}

    def mlp(p, prefix, x, **kw):
        y = real(p, prefix, x, **kw)
        if prefix != 'mlp_alpha.':
            return y
        y = cut[int(x.item())] = y.detach().requires_grad_(True)
        return y
    R.mlp = mlp
    try:
        r = oracle_step(d, ids, pm, pc, rounding, dtype, feat)
    finally:
        R.mlp = real
    r['alpha_grad'] = {l: y.grad for l, y in cut.items() if y.grad is not None}
    return r


def oracle_sweep_head(designs, ids, node_off, pm, pc, feat, rounding, dtype):
    """Every design's oracle step on its own image of the HIP feature map, merged as the batch merges them: predictions
    in the batch's endpoint order (level, then design, then order of appearance), loss and gradients weighted by each
    design's share of the T endpoints (one MSE over the batch), d loss / d feature map per image.  mlp_alpha is shared by
    the designs through the level id: the batch sums the gradients of a level's endpoints over ALL designs before its bf16
    GEMM rounds them (fuse_heads: one gather over the batch), so the merged per-level gradients go through one oracle
    mlp_alpha backward; rounding per design and summing after measured 2.3e-3 (one bf16 step of one element) from the
    HIP gradient."""
    runs = [oracle_step_alpha_cut(d, ids[i], pm, pc, rounding, dtype, feat[i]) for i, d in enumerate(designs)]
    T = sum(len(r['targets']) for r in runs)
    order = []
    for i, (d, r) in enumerate(zip(designs, runs)):
        lv = sorted((int(d.path2level[p]), j) for j, p in enumerate(ids[i]))         # bucket_paths: by level, stable
        order += [(l, i, j) for j, (l, _) in enumerate(lv)]
    order.sort()
    out = dict(hats=torch.stack([runs[i]['hats'][j] for _, i, j in order]),
               ends=[runs[i]['targets'][j] + int(node_off[i]) for _, i, j in order],
               loss=sum(r['loss'] * len(r['targets']) / T for r in runs), grads={},
               feat_grad=torch.stack([r['feat_grad'] * len(r['targets']) / T for r in runs]))
    for r in runs:
        for k, g in r['grads'].items():
            out['grads'][k] = out['grads'].get(k, 0) + g * len(r['targets']) / T
    L = max(d.L for d in designs)
    G = torch.zeros((L, 32), dtype=dtype)
    for r in runs:
        for l, g in r['alpha_grad'].items():
            G[l] += g.reshape(32) * len(r['targets']) / T
    pa = {k: v.to(dtype).clone().requires_grad_(True) for k, v in pm.items() if k.startswith('mlp_alpha.')}
    head = 'bf16' if 'head' in B.classes(rounding) else None
    R.mlp(pa, 'mlp_alpha.', torch.arange(L, dtype=dtype).reshape(L, 1), rounding=head).backward(G)
    out['grads'].update({k: v.grad.double() for k, v in pa.items()})
    return out


def oracle_unet(pc, images, feat_grad, rounding, dtype):
    """The oracle U-Net image by image, its backward driven by the HIP step's d loss / d feature map."""
    p = {k: (v.to(dtype).clone().requires_grad_('running' not in k) if v.dtype.is_floating_point else v.clone())
         for k, v in pc.items()}
    y = torch.cat([R.unet_forward(p, images[i:i + 1].to(dtype), 'max', True, rounding=rounding)
                   for i in range(images.shape[0])])
    y.backward(feat_grad.reshape(y.shape).to(dtype))
    return dict(grads={k: v.grad.double() for k, v in p.items() if v.requires_grad},
                run={k: v.double() for k, v in p.items() if 'running' in k})


def oracle_runs(designs, ids, node_off, state, hip, images, sweep_rounding):
    """The three oracle runs of one step from `state`: fp64 rounding (the reference), fp32 rounding, fp64 plain; each
    with its sweep + head merged over the designs, its U-Net, and one Adam step from the HIP optimizer state."""
    runs = []
    for rd, ud, dt in ((sweep_rounding, EVERY_CLASS, torch.float64), (sweep_rounding, EVERY_CLASS, torch.float32),
                       (None, None, torch.float64)):
        r = oracle_sweep_head(designs, ids, node_off, state['pm'], state['pc'], hip['feat'], rd, dt)
        u = oracle_unet(state['pc'], images, hip['feat_grad'], ud, dt)
        r['grads'].update(u['grads'])
        r['run'] = u['run']
        runs.append(r)
    return runs


def adam_update(state, grads, dtype):
    """theta_{k+1} - theta_k of one torch.optim.Adam step from the HIP optimizer state with the given gradients."""
    o = R.OracleTrainer(state['pm'], state['pc'], dtype=dtype)
    o.load_adam({k: state['m'][k] for k in grads}, {k: state['v'][k] for k in grads}, state['step'])
    before = {k: o.leaf(k).detach().clone() for k in grads}
    for k, g in grads.items():
        o.leaf(k).grad = g.to(dtype).reshape(o.leaf(k).shape).clone()
    o.optim.step()
    return {k: (o.leaf(k).detach() - before[k]).double() for k in grads}


def batch_rows(title, hip, runs):
    """The sweep + head rows (ceilings and floors of tests/test_bf16_oracle_gpu.py), one d loss / d feature map row per
    image, and the U-Net rows (gradients, running statistics)."""
    s64, s32, sp = runs
    assert hip['ends'] == s64['ends']
    q = Bounds(title, hip, s32, sp)
    # predictions: the 1.5e-3 floor of test_bf16_oracle_gpu.sweep_head_rows (one rounding-boundary flip moves one endpoint)
    q('predictions', lambda r: rel_err(r['hats'], s64['hats']), 1.5e-3, 2e-3)
    q('loss', lambda r: abs(r['loss'] - s64['loss']) / s64['loss'], 1e-5, 1e-3, teeth=True)
    head = [k for k in s64['grads'] if not k.startswith(UNET_PREFIX) and float(s64['grads'][k].abs().max()) > 0]
    assert head and set(head) <= set(hip['grads'])
    for k in head:
        # mlp_fuse's last bias gradient is the sum of d loss / d prediction: rounding reaches it only through the
        # predictions (measured e_plain 4.0e-4, e_hip 2.4e-8 at the trajectory's step 0), so its teeth are a group's
        last = k == 'mlp_fuse.layers.2.bias'
        q('grad ' + k, lambda r, k=k: rel_err(r['grads'][k], s64['grads'][k]), 1e-4, 5e-3, 'head output bias' if last else None,
          teeth=not last)
    for i in range(hip['feat_grad'].shape[0]):
        q(f'd loss / d feature map, image {i}', lambda r, i=i: rel_err(r['feat_grad'][i], s64['feat_grad'][i]), 1e-4, 5e-3,
          teeth=True)
    keys = [k for k in s64['grads'] if k.startswith(UNET_PREFIX) and float(s64['grads'][k].abs().max()) > 0]
    unet_grad_rows(q, s64, keys, float(hip['feat_grad'].abs().sum()))
    return q


def update_rows(q, updates):
    """theta_{k+1} - theta_k per GNN / head tensor, relative L2 (see the module docstring), against the fp64 rounding
    oracle's; teeth per group.  Floor 1e-3 (the gradient rows' 1e-4 is below what the first Adam step leaves): measured
    3.7e-4 on fcn.weight at step 0, where every element moves by lr * sign(g) and the masked projection has elements whose
    gradient is within fp32 noise of zero, while e_32 was 1.6e-6; every other GNN / head row measured <= 1.2e-5.  The U-Net's
    updates are not compared with the oracle's: its gradients are only within 0.35 relative L2 of the oracle's (module
    docstring of tests/test_bf16_oracle_gpu.py) and Adam's first steps turn that into sign flips (measured e_32 0.3 - 0.7);
    they are judged by assert_adam_update instead."""
    u64 = updates[0]
    for k in u64:
        if k.startswith(UNET_PREFIX) or float(u64[k].abs().max()) == 0:
            continue
        q('update ' + k, lambda r, k=k: rel_l2(r['update'][k], u64[k]), 1e-3, 5e-3, 'GNN / head updates')


def assert_adam_update(state, hip, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """Every tensor's theta_{k+1} equals theta_k plus one fp64 torch.optim.Adam step from the HIP state with the HIP step's
    own gradients: the moments, the device step counter (bias corrections of step k + 1) and the Adam kernel.  Per element
    within 1e-5 of the update's terms (the kernel's fp32 arithmetic: where the new moment cancels, beta1 m against
    (1 - beta1) g, its error is that of the terms, not of the small result) plus one fp32 ulp of the new parameter."""
    ref = adam_update(state, hip['grads'], torch.float64)
    t = state['step'] + 1
    bc1, bc2 = 1 - betas[0] ** t, 1 - betas[1] ** t
    bad = {}
    for k, u in ref.items():
        theta = state['pm'].get(k, state['pc'].get(k)).double().reshape(u.shape)
        g, m, v = hip['grads'][k].reshape(u.shape), state['m'][k].double().reshape(u.shape), state['v'][k].double().reshape(u.shape)
        vn = betas[1] * v + (1 - betas[1]) * g * g
        terms = lr / bc1 * (betas[0] * m.abs() + (1 - betas[0]) * g.abs()) / ((vn / bc2).sqrt() + eps)
        err = (hip['update'][k] - u).abs()
        tol = 1e-5 * terms + torch.finfo(torch.float32).eps * (theta + u).abs() + 1e-30
        if not bool((err <= tol).all()):
            bad[k] = float((err / tol).max())
    assert not bad, bad


def teacher_forced_step(ts, designs, ids, title, sweep_rounding, check_packs=True):
    """One HIP step and its rows, the oracle started from the HIP state the step started from.  sweep_rounding: the
    oracle's rounding classes for the sweep + head, or a function of the step's sweep state that picks them."""
    b = ts.batch
    state = snapshot(ts)
    hip, _ = hip_train_step(ts, ids)
    if callable(sweep_rounding):
        sweep_rounding = sweep_rounding(b.graph._sweep)
    if check_packs:
        assert_packs_current(ts, state['flat'])
    runs = oracle_runs(designs, ids, b.node_off, state, hip, b.images.cpu(), sweep_rounding)
    theta = {n: torch.as_strided(ts.optim.flat_param, p.shape, p.stride(), o).detach().double().cpu()
             for n, p, o in flat_params(ts)}
    hip['update'] = {k: theta[k] - state['pm'].get(k, state['pc'].get(k)).double() for k in theta}
    for r, dt in zip(runs, (torch.float64, torch.float32, torch.float64)):
        r['update'] = adam_update(state, {k: r['grads'][k] for k in theta if k in r['grads']}, dt)
    q = batch_rows(title, hip, runs)
    update_rows(q, [r['update'] for r in runs])
    assert_adam_update(state, hip)
    return q, hip, state


def assert_packs_current(ts, flat_k):
    """Every bf16 weight pack the step read is the rounding of the parameters it started from, bit for bit: the sweep's
    fc_cell_neigh packs (W1, W2, W2^T, W1^T) and the U-Net's pack buffer, against packs made afresh from theta_k."""
    from mmft import ops, unet16
    st = ts.batch.graph._sweep
    now = ts.optim.flat_param.clone()
    ts.optim.flat_param.copy_(flat_k)
    try:
        nb = ts.pmodel.gnn.fc_cell_neigh.layers
        w1, w2 = nb[0].weight.detach(), nb[2].weight.detach()
        fresh = (ops.pack_bf16(w1), ops.pack_bf16(w2), ops.pack_bf16(w2, transpose=True), ops.pack_bf16(w1, transpose=True))
        for j, (a, f) in enumerate(zip(st.wpack if st.wpack is not None else (), fresh)):
            assert torch.equal(a.view(torch.int16), f.view(torch.int16)), f'sweep pack {j} is not pack(theta_k)'
        packs = ts.cnn.__dict__['_u16_packs']
        ref = unet16._Packs(ts.cnn, flat_k.device)
        ref.refresh(ts.cnn)
        torch.cuda.synchronize()
        assert ref.off == packs.off and torch.equal(ref.buf.view(torch.int16), packs.buf.view(torch.int16)), \
            'U-Net pack is not pack(theta_k)'
    finally:
        ts.optim.flat_param.copy_(now)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- 1. batch of eight
def test_bench_step_shape_batch_of_eight_vs_rounding_oracle(dev):
    """The bench's step shape at 16 384 nodes per design: eight designs (seeds 800..807)
    merged into one bf16 TrainStep, 40 paths each.  Same-index levels are concatenated, so level pairs reach ~8 500 rows and
    the forward slot kernel takes its 32-row form (level_fwd_slots_kernel<2>: max(net rows, cell rows) >= 32 x 192,
    mlp2_bf16.hip:738), which config A never reaches; the reverse pair kernel cuts heavy drivers into parts; the U-Net runs
    eight images with per-image BatchNorm statistics (indices 4-7 of the statistics tiles); the masked projection and the
    head span eight designs.  Rows: the decoupled sweep + head (predictions, loss, every GNN / head gradient, d loss /
    d feature map per image) and the U-Net driven by the HIP feature-map gradient (gradients, running statistics).
    All eight designs have regular fan-in: with an irregular one in the batch (synth_design(..., fanin='irregular')) the
    merged levels lose the slot-table forward altogether (no level_fwd_slots_kernel launch, measured), so the 32-row form
    could not be judged; irregular fan-in keeps its own case in tests/test_bf16_oracle_gpu.py.
    Measured on one MI355X (e_hip / e_32 / e_plain): predictions 8.9e-4 / 8.9e-4 / 2.1e-2, loss 3.2e-6 / 2.3e-6 / 3.4e-3,
    GNN gradients <= 3.9e-5 / 3.8e-5 / >= 5.7e-3, head gradients <= 1.1e-5 / 1.1e-5 / >= 1.6e-3, d loss / d feature map
    <= 1.7e-7 / 2.0e-7 / >= 1.6e-2 per image, U-Net gradient mean 0.16 / 0.16 / 0.30, running statistics <= 5.2e-4 /
    3.0e-4; 279 heavy-driver parts."""
    from mmft.synth import synth_design
    from mmft.train import build_models, TrainStep
    designs = [synth_design(N=16384, L=16, tile=64, seed=800 + i) for i in range(8)]
    rng = np.random.default_rng(12)
    ids = [rng.permutation(d.num_paths)[:40].tolist() for d in designs]
    with lib.math_mode('bf16'):
        pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=9294)
        ts = TrainStep(pmodel, cnn, designs, dev)
        b, g = ts.batch, ts.batch.graph
        state = snapshot(ts)
        hip, names = hip_train_step(ts, ids, profile=True)
    print('\nkernels:', sorted(names))
    assert STEP_KERNELS <= names, sorted(STEP_KERNELS - names)
    sizes = [len(n) for n in b.level_nodes]
    rows_max = max(max(sizes[l - 1], sizes[l]) for l in range(2, b.L, 2))
    print('level sizes:', sizes)
    assert rows_max >= 32 * 192, rows_max                                      # the <2> form ran for at least one pair
    pairs = g.level_bwd_pairs(b.level_nodes)
    assert pairs is not None
    parts = sum(int((p['tiles'][:, 3] > 0).sum()) for p in pairs[1] if p is not None)
    print('heavy drivers cut into parts:', parts)
    assert parts > 0
    assert g._sweep.hid16                                     # the oracle's 'hidden' class applies
    runs = oracle_runs(designs, ids, b.node_off, state, hip, b.images.cpu(), EVERY_CLASS)
    batch_rows('batch of eight: sweep + head on the HIP feature map, U-Net on its gradient', hip, runs).verdict()


# ------------------------------------------------------------------------------------------------- 2. Adam trajectory
def _two_designs():
    from mmft.synth import synth_design
    designs = [synth_design(N=4096, L=16, tile=64, seed=830 + i) for i in range(2)]
    rng = np.random.default_rng(13)
    return designs, [[rng.permutation(d.num_paths)[:40].tolist() for d in designs] for _ in range(6)]


def test_adam_trajectory_teacher_forced_vs_rounding_oracle(dev):
    """Six eager bf16 steps on two designs (4 096 nodes, 16 levels), each judged against the three oracle runs started from
    the HIP state the step started from: the decoupled sweep + head rows, the U-Net rows and the update of every tensor.
    Every step's bf16 weight packs are the rounding of that step's parameters, bit for bit.  Negative control: with the
    sweep's repack a no-op after step 0 the packs and rows of steps 1 and 2 fail.  A GraphedTrainStep from the same
    initialisation over the same batches follows the eager loss and predictions within 1e-4 at every step.
    Measured on one MI355X over the six steps (e_hip / e_32 / e_plain): predictions <= 3.7e-5 / 1.1e-4 / >= 2.4e-3, loss
    <= 1.6e-6 / 1.2e-5 / >= 1.2e-3, GNN gradients <= 9.0e-6 / 1.9e-5 / >= 5.1e-3, head gradients <= 3.3e-5 / 3.3e-5 /
    >= 4.0e-4, d loss / d feature map <= 1.9e-7 / 2.7e-7 / >= 1.3e-2, U-Net gradient mean 0.07 - 0.15 / 0.07 - 0.18 /
    0.25 - 0.33, GNN / head updates <= 3.7e-4 / 1.0e-4 (mean e_plain / mean e_hip 768 - 4930).  Control, stale sweep pack
    at steps 1 and 2: loss 3.4e-2, GNN gradients 0.38, updates up to 0.53 - every sweep row fails."""
    from mmft import ops
    from mmft.train import build_models, TrainStep, GraphedTrainStep
    designs, batches = _two_designs()
    eager = []
    with lib.math_mode('bf16'):
        pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=31)
        ts = TrainStep(pmodel, cnn, designs, dev)
        bounds = []
        for k, ids in enumerate(batches):
            assert ts.optim.device_step_count() == k
            q, hip, _ = teacher_forced_step(ts, designs, ids, f'trajectory step {k}', EVERY_CLASS)
            assert ts.batch.graph._sweep.hid16
            eager.append((hip['loss'], hip['hats']))
            bounds.append(q)
        for q in bounds:
            q.verdict()
        del ts, pmodel, cnn

        # negative control: a stale sweep pack (the repack skipped after step 0) is caught by the pack check and by the rows
        pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=31)
        ts = TrainStep(pmodel, cnn, designs, dev)
        teacher_forced_step(ts, designs, batches[0], 'control step 0', EVERY_CLASS)[0].verdict()
        real = ops.pack_bf16
        ops.pack_bf16 = lambda w, transpose=False, out=None: out if out is not None else real(w, transpose)
        try:
            for k in (1, 2):
                q, _, state = teacher_forced_step(ts, designs, batches[k], f'control step {k}, stale sweep pack',
                                                  EVERY_CLASS, check_packs=False)
                with pytest.raises(AssertionError, match='sweep pack'):
                    assert_packs_current(ts, state['flat'])
                with pytest.raises(AssertionError):
                    q.verdict()
                assert any(b.startswith('update gnn.fc_cell_neigh') for b in q.bad), q.bad
        finally:
            ops.pack_bf16 = real
        del ts, pmodel, cnn

        pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=31)
        ts = TrainStep(pmodel, cnn, designs, dev)
        gs = GraphedTrainStep(ts, batches[0], warmup=0)
        for k, ids in enumerate(batches):
            loss, hats, _ = gs.step(ids)
            torch.cuda.synchronize()
            el, eh = eager[k]
            assert abs(float(loss) - el) < 1e-4 * abs(el) and rel_err(hats, eh) < 1e-4, k


# ------------------------------------------------------------------------------------------------- 3. drop-in entry
def test_dropin_teacher_forced_vs_rounding_oracle(dev):
    """TrainStep(mode='dropin') in bf16: four teacher-forced steps on the designs of the trajectory test, with its rows.  A
    no-grad U-Net forward runs before the TrainStep exists, so packs and descriptor tables first see the parameter storage
    that FlatAdam then re-points.  The sweep's forward / reverse graphs and the U-Net's forward / backward graphs are
    captured on the second step and replayed from then on.  The oracle's sweep classes follow what the step ran: 'hidden'
    only where the sweep stored HN / DHN as bf16 (st.hid16): step 0 sweeps level by level without the packed weights
    (no hid16), steps 1 - 3 run the speculative whole sweep with hid16 set.
    Measured on one MI355X over the four steps (e_hip / e_32 / e_plain): predictions <= 2.0e-5 / 2.0e-5 / >= 1.2e-3, loss
    <= 4.3e-7 / 1.3e-6 / >= 4.2e-4, GNN gradients <= 1.3e-5 / 1.9e-5 / >= 5.5e-3, head gradients <= 1.8e-6 / 1.8e-6 /
    >= 4.1e-4, U-Net gradient mean 0.04 - 0.14 / 0.07 - 0.13 / 0.25 - 0.40, GNN / head updates <= 1.1e-4 / 2.4e-5."""
    from mmft.train import build_models, TrainStep
    designs, batches = _two_designs()

    def classes(st):
        print('dropin sweep: wpack', st.wpack is not None, 'hid16', getattr(st, 'hid16', None))
        return EVERY_CLASS if getattr(st, 'hid16', False) else NO_HIDDEN
    with lib.math_mode('bf16'):
        pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=37)
        with torch.no_grad():
            cnn(torch.from_numpy(np.stack([d.image for d in designs])).to(dev))
        ts = TrainStep(pmodel, cnn, designs, dev, mode='dropin')
        bounds, rec, calls = [], None, []
        for k, ids in enumerate(batches[:4]):
            q, _, _ = teacher_forced_step(ts, designs, ids, f'drop-in step {k}', classes)
            bounds.append(q)
            g = ts.batch.graph
            rp = cnn.__dict__.get('_u16_replay')
            # the U-Net replays from its second call (step 1); the speculative whole sweep starts once one step has swept
            # level by level (step 0), so its graphs are captured on step 2
            calls.append((rp.fwd.calls, rp.bwd.calls))
            if k >= 1:
                assert rp.fwd.graph is not None and rp.bwd.graph is not None and calls[k][0] == calls[k - 1][0] + 1 and \
                    calls[k][1] == calls[k - 1][1] + 1, calls
            if k >= 2:
                rec = rec or g._sweep_bufs['replay']
                assert g._sweep_bufs['replay'] is rec
                assert rec.fwd.graph is not None and rec.bwd.graph is not None and rec.fwd.calls == rec.bwd.calls == k, \
                    (rec.fwd.calls, rec.bwd.calls)
        for q in bounds:
            q.verdict()
