"""The fused fusion-head MLP (include/mmft_head.h, csrc/head_mlp.hip) on the GPU, bf16 math mode.

KERNEL LEVEL.  T in {1, tile - 1, tile, tile + 1, 3 tile + 1} for the 64-row tile, x and dx with a row pitch of 304 > 288.
Seeded inputs hold an all-zero row that meets 64 zero biases (h exactly 0: the mask must be false), a row whose hidden units
are all dead, and duplicate rows.  The reference is fp64 torch with oracle.bf16's r / linear_bf16 at the places of the header's
table.  The bound is measured, not chosen: on the same inputs
    e_unfused  the layer path of the parent commit (FUSED_HEAD_MLP = False) against the reference,
    e_fp32     the same rounded formula in plain fp32 torch against the reference,
and every tensor (pred, the saved r(h), dx, dW1, db1, dW2, db2) must satisfy  e_fused <= 2 max(e_unfused, e_fp32)  in relative
max norm; the 2 is for a different but equally long fp32 summation order.  Measured on one MI355X at T = 193 (e_fused /
e_unfused / e_fp32): see DESIGN 5, "fused head MLP".

accumulate != 0 adds into what the sink holds.  The sinks are pre-filled with seeded values of the gradients' own size (the
guard rows keep the sentinel).  The accumulated result is the fixed-order fp32 sum of 17 terms {sink, 16 lane partials}, the
stored one that of the same 16 partials, so by the standard bound (n - 1) u sum |x_i| of recursive summation, u = 2^-24, the two
differ from sink + gradient by at most (16 + 15) u (|sink| + sum |terms|) (1 + 1e-3); the last factor covers the second-order
terms and the partials' own rounding against the exact sum of absolute values the test computes in fp64.

MODULE LEVEL, two designs of synth_design(N=2048, L=12, tile=32), 40 endpoints each, one TrainStep forward + backward with
the switch on and off.  A hook on mlp_fuse takes what it was given (x, the upstream gradient) and what it returned (dx), and
the SAME rule as at kernel level judges the step: the fp64 formula on those inputs is the reference, and predictions, loss, dx,
dW1, db1, dW2, db2 of the fused step must lie within 2 max(e_unfused, e_fp32) of it.  x is bitwise the same in both steps
(nothing upstream changed).  Every gradient outside mlp_fuse must be BITWISE what the layer path gives: dx keeps the layer
path's summation order, and the upstream gradient enters every contraction rounded to bf16, where the last-bit differences
of the predictions vanish unless one crosses a rounding boundary - none does on these inputs; if a change of the inputs makes
one cross, that flip is to be stated here, not the assertion dropped.  (The bf16-storage U-Net backward turns a last-bit
difference of dx into 1e-2 of the max norm of its gradients, so nothing between "bitwise" and "loose" is worth asserting.)
Under torch.no_grad() the same forward runs the kernel without the saved tensor and predicts the same bits.  Only bf16 mode,
ReLU and (288, 576, 1) take the fused kernels.  GraphedTrainStep follows the eager TrainStep over 4 steps (2e-4, the tolerance
of test_graphed_step_equals_eager) with the same batch twice in a row: a pack that outlived its call would repeat the
predictions after the Adam update."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from mmft import functional as MF
from mmft import lib
from oracle.bf16 import linear_bf16, r

pytestmark = pytest.mark.gpu

TILE, IN, HD, LD = 64, 288, 576, 304
SIZES = [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 1]
FIELDS = ('pred', 'hid', 'dx', 'dw1', 'db1', 'dw2', 'db2')
SENT = 12345.0
UNET_PREFIX = ('inc.', 'down', 'up', 'outc.')


def make_inputs(T, seed=5):
    g = torch.Generator().manual_seed(seed + T)
    w1 = torch.randn(HD, IN, generator=g) / IN ** 0.5
    w1[:, IN - 1] = w1[:, IN - 1].abs() + 0.1                     # a positive column: x = -100 e_287 kills every hidden unit
    b1 = 0.1 * torch.randn(HD, generator=g)
    b1[:64] = 0.0                                                 # zero biases: the all-zero row gives h exactly 0 there
    w2 = torch.randn(1, HD, generator=g) / HD ** 0.5
    b2 = 0.1 * torch.randn(1, generator=g)
    x = torch.randn(T, IN, generator=g)
    x[0] = 0.0                                                    # the all-zero row
    if T > 1:
        x[1] = 0.0
        x[1, IN - 1] = -100.0                                     # the dead row
    if T > 8:
        x[5] = x[T - 1]                                           # duplicates, in different 16-row blocks
        x[T - 2] = x[3]
    dpred = torch.randn(T, generator=g)
    if T > 4:
        dpred[4] = 0.0
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, dpred=dpred)


def formula(inp, dtype):
    """The table of include/mmft_head.h in torch at `dtype` (fp64: the reference; fp32: what fp32 arithmetic alone costs),
    plus - fp64 only use - the sums of absolute values behind every parameter gradient."""
    t = {k: v.to(dtype).clone().requires_grad_(k != 'dpred') for k, v in inp.items()}
    h = torch.relu(linear_bf16(t['x'], t['w1'], t['b1']))
    pred = linear_bf16(h, t['w2'], t['b2'])
    pred.backward(t['dpred'].reshape(-1, 1))
    out = dict(pred=pred.detach().reshape(-1), hid=r(h.detach()), dx=t['x'].grad, dw1=t['w1'].grad, db1=t['b1'].grad,
               dw2=t['w2'].grad.reshape(-1), db2=t['b2'].grad)
    with torch.no_grad():
        dp, hd = r(t['dpred']).reshape(-1, 1), h.detach()
        g1 = (dp * r(t['w2'].detach())) * (hd > 0)
        mass = dict(dw1=r(g1).abs().T @ r(t['x'].detach()).abs(), db1=g1.abs().sum(0), dw2=(dp.abs() * r(hd).abs()).sum(0),
                    db2=t['dpred'].abs().sum().reshape(1))
    return {k: v.detach().double() for k, v in out.items()}, mass


def unfused(inp, dev):
    """The layer path of the parent commit on the same inputs."""
    import model
    m = model.MLP(IN, HD, 1).to(dev)
    with torch.no_grad():
        for p, k in zip((m.layers[0].weight, m.layers[0].bias, m.layers[2].weight, m.layers[2].bias), ('w1', 'b1', 'w2', 'b2')):
            p.copy_(inp[k])
    x = inp['x'].to(dev).requires_grad_(True)
    MF.FUSED_HEAD_MLP = False
    try:
        pred = m(x)
        pred.backward(inp['dpred'].to(dev).reshape(-1, 1))
        with torch.no_grad():      # the fp32 h its first layer saves (the same launch again), rounded as its consumers round it
            hid = r(MF.linear_act(x.detach(), m.layers[0].weight, m.layers[0].bias, 0))
    finally:
        MF.FUSED_HEAD_MLP = True
    l0, l2 = m.layers[0], m.layers[2]
    return dict(pred=pred.detach().reshape(-1), hid=hid, dx=x.grad, dw1=l0.weight.grad, db1=l0.bias.grad,
                dw2=l2.weight.grad.reshape(-1), db2=l2.bias.grad)


class Buffers:
    """Outputs and scratch of the two entry points with guard rows behind them, all filled with a sentinel."""

    def __init__(self, T, dev):
        f = lambda *s: torch.full(s, SENT, dtype=torch.float32, device=dev)
        self.T = T
        self.pred, self.hid = f(T + 8), torch.full((T + 4, HD), 77.0, dtype=torch.bfloat16, device=dev)
        self.dx = f(T + 4, LD)
        self.dw1, self.db1, self.dw2, self.db2 = f(HD + 2, IN), f(HD + 8), f(HD + 8), f(8)
        self.need = lib.head('mmft_head_mlp_workspace_bytes', T)
        assert self.need % 16 == 0
        self.ws = f(self.need // 4 + 4096)

    def guards_intact(self):
        T = self.T
        return all(bool((t == v).all()) for t, v in (
            (self.pred[T:], SENT), (self.hid[T:], 77.0), (self.dx[T:], SENT), (self.dx[:T, IN:], SENT), (self.dw1[HD:], SENT),
            (self.db1[HD:], SENT), (self.dw2[HD:], SENT), (self.db2[1:], SENT), (self.ws[self.need // 4:], SENT)))

    def results(self):
        T = self.T
        return dict(pred=self.pred[:T].clone(), hid=self.hid[:T].clone(), dx=self.dx[:T, :IN].clone(), dw1=self.dw1[:HD].clone(),
                    db1=self.db1[:HD].clone(), dw2=self.dw2[:HD].clone(), db2=self.db2[:1].clone())


def run_fused(d, b, keep=True, accumulate=0):
    T = b.T
    x = d['xp']
    lib.head('mmft_head_mlp_fwd', x, x.stride(0), d['w1'], d['b1'], d['w2'], d['b2'], b.hid if keep else None, b.pred, T, IN, HD, 1,
             *lib.stream_args(x))
    if keep:
        lib.head('mmft_head_mlp_bwd', d['dpred'], b.hid, x, x.stride(0), d['w1'], d['w2'], b.dx, b.dx.stride(0), b.dw1, b.db1, b.dw2,
                 b.db2, T, IN, HD, 1, accumulate, b.ws, b.need, *lib.stream_args(x))
    torch.cuda.synchronize()


@pytest.mark.parametrize('T', SIZES)
def test_fused_head_mlp_against_the_fp64_reference(dev, T):
    inp = make_inputs(T)
    ref, mass = formula(inp, torch.float64)
    f32, _ = formula(inp, torch.float32)
    assert float(ref['hid'][0, :64].abs().max()) == 0.0 and (T == 1 or float(ref['hid'][1].abs().max()) == 0.0)      # the cases hold
    with lib.math_mode('bf16'):
        unf = unfused(inp, dev)
        d = {k: v.to(dev).contiguous() for k, v in inp.items()}
        xp = torch.full((T, LD), SENT, dtype=torch.float32, device=dev)      # pitch 304; the padding is never read
        xp[:, :IN] = d['x']
        d['xp'] = xp[:, :IN]
        b = Buffers(T, dev)
        run_fused(d, b)
        got = b.results()
        assert b.guards_intact()
        # determinism: a second run into fresh buffers gives the same bits; without the saved tensor the same predictions
        b2 = Buffers(T, dev)
        run_fused(d, b2)
        again = b2.results()
        assert all(torch.equal(got[k], again[k]) for k in FIELDS)
        b3 = Buffers(T, dev)
        run_fused(d, b3, keep=False)
        assert torch.equal(b3.pred[:T], got['pred']) and b3.guards_intact() and bool((b3.hid == 77.0).all())
        # accumulate: added to what the sinks hold (the guard rows hold the same sentinel and stay what they were)
        b4 = Buffers(T, dev)
        b4.hid.copy_(b.hid)
        gen = torch.Generator().manual_seed(77 + T)
        fill = {}
        for k, t in (('dw1', b4.dw1[:HD]), ('db1', b4.db1[:HD]), ('dw2', b4.dw2[:HD]), ('db2', b4.db2[:1])):
            scale = float(got[k].abs().max()) or 1.0                         # the gradient's own size
            fill[k] = (scale * torch.randn(t.shape, generator=gen)).float()
            t.copy_(fill[k])
        lib.head('mmft_head_mlp_bwd', d['dpred'], b4.hid, d['xp'], LD, d['w1'], d['w2'], None, 0, b4.dw1, b4.db1, b4.dw2, b4.db2, T, IN, HD,
                 1, 1, b4.ws, b4.need, *lib.stream_args(xp))
        torch.cuda.synchronize()
        acc = b4.results()
        assert b4.guards_intact() and bool((b4.dx == SENT).all())            # dx = NULL: not written
    print(f'\n== fused head MLP, T = {T}: tensor  e_fused  e_unfused  e_fp32  bound')
    bad = []
    for k in FIELDS:
        e_f = rel_err(got[k].float(), ref[k])
        e_u = rel_err(unf[k], ref[k])
        e_3 = rel_err(f32[k], ref[k])
        bound = 2 * max(e_u, e_3)
        print(f'   {k:5s} {e_f:.2e} {e_u:.2e} {e_3:.2e} {bound:.2e}')
        if not e_f <= bound:
            bad.append((k, e_f, bound))
    for k in ('dw1', 'db1', 'dw2', 'db2'):
        want = fill[k].double() + got[k].double().cpu()
        tol = (16 + 15) * 2.0 ** -24 * (fill[k].double().abs() + mass[k].double().reshape(want.shape)) * (1 + 1e-3)
        over = float(((acc[k].double().cpu() - want).abs() - tol).max())
        print(f'   accumulate {k}: worst excess over the summation bound {over:.2e}')
        if over > 0:
            bad.append(('accumulate ' + k, over))
    assert not bad, bad


def _train_pair(dev):
    from mmft.synth import synth_design
    designs = [synth_design(N=2048, L=12, tile=32, seed=300 + i, end_frac=0.25) for i in range(2)]
    rng = np.random.default_rng(9)
    batches = [[rng.permutation(d.num_paths)[:40].tolist() for d in designs] for _ in range(3)]
    return designs, batches


def _profiled(fn):
    """fn() with the launch profiler on -> (result, set of kernel names)."""
    lib.prof_reset()
    lib.prof_enable(True)
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        lib.prof_enable(False)
    return res, {row['name'] for row in lib.prof_report()}


FUSED_KERNELS = {'head_mlp_fwd_kernel<keep>', 'head_mlp_bwd_dx_kernel', 'head_mlp_wgrad_kernel'}
MLP_KEYS = {'dw1': 'mlp_fuse.layers.0.weight', 'db1': 'mlp_fuse.layers.0.bias', 'dw2': 'mlp_fuse.layers.2.weight',
            'db2': 'mlp_fuse.layers.2.bias'}


def test_train_step_with_the_switch_on_and_off(dev):
    from mmft.train import build_models, TrainStep
    designs, batches = _train_pair(dev)
    out = {}
    with lib.math_mode('bf16'):
        for on in (True, False):
            MF.FUSED_HEAD_MLP = on
            try:
                pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=11)
                ts = TrainStep(pmodel, cnn, designs, dev)
                seen = {}

                def hook(module, inputs, result):
                    if torch.is_grad_enabled():
                        seen['x'] = inputs[0].detach().clone()
                        inputs[0].register_hook(lambda g: seen.__setitem__('dx', g.detach().clone()))
                        result.register_hook(lambda g: seen.__setitem__('dpred', g.detach().reshape(-1).clone()))
                handle = pmodel.mlp_fuse.register_forward_hook(hook)
                if on:       # no gradient wanted: the kernel without the saved tensor, the same bits
                    with torch.no_grad():
                        (hats_ng, _, _), names = _profiled(lambda: ts.forward(batches[0]))
                    assert 'head_mlp_fwd_kernel<nokeep>' in names and 'head_mlp_fwd_kernel<keep>' not in names, sorted(names)
                    hats_ng = hats_ng.clone()

                def step():
                    hats, ends_d, _ = ts.forward(batches[0])
                    loss = ts.loss(hats, ends_d)
                    ts.optim.zero_grad()
                    loss.backward()
                    return hats, ends_d, loss
                (hats, ends_d, loss), names = _profiled(step)
                handle.remove()
                assert FUSED_KERNELS <= names and 'head_mlp_fwd_kernel<nokeep>' not in names if on else \
                    not [n for n in names if n.startswith('head_mlp')], sorted(names)
                if on:
                    assert torch.equal(hats_ng, hats.detach())
                grads = {k: p.grad.detach().clone() for k, p in list(pmodel.named_parameters()) + list(cnn.named_parameters())
                         if p.grad is not None}
                l0, l2 = pmodel.mlp_fuse.layers[0], pmodel.mlp_fuse.layers[2]
                inp = dict(x=seen['x'], w1=l0.weight, b1=l0.bias, w2=l2.weight, b2=l2.bias, dpred=seen['dpred'])
                arrival = ts.batch.arrival[ends_d.long()].reshape(-1).detach().cpu()
                out[on] = dict(inp={k: v.detach().cpu().clone() for k, v in inp.items()}, arrival=arrival, grads=grads,
                               got=dict(pred=hats.detach().reshape(-1), loss=loss.detach().reshape(1), dx=seen['dx'],
                                        **{k: grads[name].reshape(-1) if k == 'dw2' else grads[name] for k, name in MLP_KEYS.items()}))
            finally:
                MF.FUSED_HEAD_MLP = True

    def judged(run, dtype):
        """The formula on the inputs mlp_fuse was given in that step, and the step's MSE on its predictions."""
        ref, _ = formula(run['inp'], dtype)
        ref['loss'] = ((ref['pred'].to(dtype) - run['arrival'].to(dtype)) ** 2).mean().reshape(1).double()
        return ref
    fus, unf = out[True], out[False]
    assert torch.equal(fus['inp']['x'], unf['inp']['x']) and all(torch.equal(fus['inp'][k], unf['inp'][k]) for k in ('w1', 'b1', 'w2', 'b2'))
    ref_f, ref_u, f32 = judged(fus, torch.float64), judged(unf, torch.float64), judged(fus, torch.float32)
    print('\n== one train step, switch on / off: tensor  e_fused  e_unfused  e_fp32  bound')
    bad = []
    for k in ('pred', 'loss', 'dx', 'dw1', 'db1', 'dw2', 'db2'):
        e_f, e_u, e_3 = rel_err(fus['got'][k], ref_f[k]), rel_err(unf['got'][k], ref_u[k]), rel_err(f32[k], ref_f[k])
        bound = 2 * max(e_u, e_3)
        print(f'   {k:5s} {e_f:.2e} {e_u:.2e} {e_3:.2e} {bound:.2e}')
        if not e_f <= bound:
            bad.append((k, e_f, bound))
    g1, g0 = fus['grads'], unf['grads']
    assert set(g1) == set(g0) and set(MLP_KEYS.values()) <= set(g1)
    others = sorted(k for k in g1 if not k.startswith('mlp_fuse.'))
    assert len(others) > 40 and any(k.startswith(UNET_PREFIX) for k in others) and any(k.startswith('gnn.') for k in others)
    bad += [('not bitwise the layer path\'s', k, rel_err(g1[k], g0[k])) for k in others if not torch.equal(g1[k], g0[k])]
    assert not bad, bad


def test_only_the_bf16_relu_288_576_1_case_takes_the_fused_kernels(dev):
    """functional.head_mlp_usable past its first clause: f32 mode, LeakyReLU, other shapes (two labels, another hidden width,
    mlp_alpha's 1 -> 64 -> 32) and the switch keep the generic layers; the one supported case launches the fused forward."""
    import model
    torch.manual_seed(3)

    def names_of(mlp, width, mode):
        x = torch.randn(70, width, device=dev)
        with lib.math_mode(mode):
            return _profiled(lambda: mlp.to(dev)(x))[1]
    fused = lambda names: [n for n in names if n.startswith('head_mlp')]
    assert fused(names_of(model.MLP(IN, HD, 1), IN, 'bf16')) == ['head_mlp_fwd_kernel<keep>']
    assert not fused(names_of(model.MLP(IN, HD, 1), IN, 'f32'))
    assert not fused(names_of(model.MLP(IN, HD, 1, negative_slope=0.1), IN, 'bf16'))
    for sizes in ((IN, HD, 2), (IN, 512, 1), (256, HD, 1), (1, 64, 32)):
        assert not fused(names_of(model.MLP(*sizes), sizes[0], 'bf16')), sizes
    MF.FUSED_HEAD_MLP = False
    try:
        assert not fused(names_of(model.MLP(IN, HD, 1), IN, 'bf16'))
    finally:
        MF.FUSED_HEAD_MLP = True


def test_graphed_step_follows_eager_with_the_fused_head_and_sees_the_new_weights(dev):
    from mmft.train import build_models, TrainStep, GraphedTrainStep
    designs, batches = _train_pair(dev)
    batches = [batches[0], batches[0], batches[1], batches[2]]          # the same batch twice: only the weights differ
    out = {}
    with lib.math_mode('bf16'):
        for kind in ('eager', 'graph'):
            pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=11)
            ts = TrainStep(pmodel, cnn, designs, dev)
            if kind == 'graph':
                stepper = GraphedTrainStep(ts, batches[0], warmup=0)    # capture only (no extra optimizer steps)
            else:
                stepper = ts
                ts.forward(batches[0])                                  # the capture's dry run also advances BN running stats
            losses, hats = [], []
            for ids in batches:
                loss, h, _ = stepper.step(ids)
                losses.append(float(loss))
                hats.append(h.clone())
            out[kind] = (losses, hats)
    np.testing.assert_allclose(out['graph'][0], out['eager'][0], rtol=2e-4)
    for i, (a, b) in enumerate(zip(out['graph'][1], out['eager'][1])):
        e = rel_err(a, b)
        assert e < 2e-4, f'hats of step {i}: rel err {e:.3e}'
    # replayed after an Adam update, on the same endpoints: the predictions moved, as the eager ones did
    assert not torch.equal(out['graph'][1][0], out['graph'][1][1])
    assert rel_err(out['graph'][1][1], out['graph'][1][0]) > 0.5 * rel_err(out['eager'][1][1], out['eager'][1][0]) > 0
