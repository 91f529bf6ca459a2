"""CPU oracle of the eval-mode U-Net's INPUT gradient and of d J / d feature map  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

`unet_eval_acts` is tests/unet_eval_oracle.py's forward keeping every post-ReLU activation; `unet_eval_vjp` is the backward
walk of mmft.unet16.unet_eval_input_grad on GIVEN activations - its own forward's, or the HIP run's tape (`acts_from_tape`).
Fed the tape, every decision (ReLU masks, max-pool argmax) is the HIP run's own and the walk is LINEAR in gout: what is left
between the two is rounding and accumulation order.

Rounding map of the walk, `rounding='bf16'` (r() = round to bf16 through fp32, oracle.bf16.r):
  * every STORED gradient is rounded once on store: OutConv's dx (g14), every convolution input gradient (g_i, gcat_k,
    gp_k), every transposed-convolution input gradient (g12, g10, g8), every dz_i;
  * dz_i = r(a_i > 0 ? g_i * scale_i : 0); at the pooled layers 6, 4, 2: dz_i = r(a_i > 0 ? (gskip + route(gp)) * scale_i : 0)
    - the fp32 sum, the product and the mask first, ONE rounding (the skip half of the concatenation's gradient and the
    routed gradient of the pooled copy are never stored as a sum);
  * route: max pooling sends the window's gradient to torch's first maximum of the STORED values (a NaN wins), average
    pooling a quarter to each pixel;
  * masks and argmax come from the stored activations a_i, never from a recomputed pre-activation;
  * scale_i fp32 by the forward's sequence (unet_eval_oracle.scale_shift): invstd = 1 / sqrtf(rv + eps); scale = gamma * invstd;
  * convolution / transposed-convolution input gradients: bf16 operands (r(w), the stored dz / gcat slice), fp32 accumulation;
  * OutConv: fp32 weights; its pooling argmax and final ReLU mask from the pixel values recomputed from the stored a14;
  * the image gradient (layer 1's input gradient) is fp32 and NOT rounded.
`rounding=None`: nothing is rounded and scale is formed in the working dtype (the plain reference: on its own forward's
activations it is autograd of the reference's module).  `rounding='operands'`: the ablation - bf16 operands and the fp32
scale, but no stored gradient is rounded."""
import torch
import torch.nn.functional as F

from oracle import bf16 as B
from oracle import restatement as R
import unet_eval_oracle as E

DC = ['inc.', 'down1.maxpool_conv.1.', 'down2.maxpool_conv.1.', 'down3.maxpool_conv.1.', 'up1.conv.', 'up2.conv.', 'up3.conv.']
UP = ['up1.', 'up2.', 'up3.']
# conv i (1-based) -> (buffer, channels): mmft.unet16._ACT / _CONV, restated so that this file does not import the product
ACT = {1: ('a1', 16), 2: ('cat3', 16), 3: ('a3', 32), 4: ('cat2', 32), 5: ('a5', 64), 6: ('cat1', 64), 7: ('a7', 128), 8: ('a8', 128),
       9: ('a9', 64), 10: ('a10', 64), 11: ('a11', 32), 12: ('a12', 32), 13: ('a13', 16), 14: ('a14', 16)}
ROUNDINGS = (None, 'bf16', 'operands')


def _names(i):
    k, j = (i - 1) // 2, (i - 1) % 2
    return DC[k] + ('double_conv.0.weight' if j == 0 else 'double_conv.3.weight'), DC[k] + ('double_conv.1.' if j == 0 else 'double_conv.4.')


@torch.no_grad()
def unet_eval_acts(p, x, pooling='max', rounding=None):
    """(out, {i: activation of convolution i, (N, C, H, W)}) of unet_eval_oracle.unet_eval_forward (the same arithmetic)."""
    rnd = 'bf16' if rounding else None
    acts = {}

    def dc(k, t):
        for j in (0, 1):
            cw, bp = _names(2 * k + 1 + j)
            t = E.conv_bn_relu(p, cw, bp, t, rnd)
            acts[2 * k + 1 + j] = t
        return t
    x1 = dc(0, x)
    x2 = dc(1, E.pool(x1, pooling, rnd))
    x3 = dc(2, E.pool(x2, pooling, rnd))
    y = dc(3, E.pool(x3, pooling, rnd))
    for k, skip in ((4, x3), (5, x2), (6, x1)):
        pre = UP[k - 4]
        if rnd:
            u = B.r(B.conv_transpose2d_bf16(y, p[pre + 'up.weight'], p[pre + 'up.bias']))
        else:
            u = F.conv_transpose2d(y, p[pre + 'up.weight'], p[pre + 'up.bias'], stride=2)
        y = dc(k, torch.cat([skip, u], 1))
    out = torch.relu(E.pool(F.conv2d(y, p['outc.conv.0.weight'], p['outc.conv.0.bias']), pooling))
    return out, acts


def acts_from_tape(tape_acts, dtype=torch.float64):
    """{i: (N, C, H, W)} from mmft.unet16.EvalTape.acts (bf16 NHWC; layers 2, 4, 6 live in the first channels of a
    concatenation buffer)."""
    return {i: tape_acts[name][..., :C].detach().cpu().to(dtype).permute(0, 3, 1, 2).contiguous() for i, (name, C) in ACT.items()}


def _route(a, gp, pooling):
    if pooling == 'avg':
        return 0.25 * gp.repeat_interleave(2, 2).repeat_interleave(2, 3)
    _, idx = F.max_pool2d(a, 2, return_indices=True)
    return F.max_unpool2d(gp, idx, 2, output_size=a.shape[2:])


@torch.no_grad()
def unet_eval_vjp(p, acts, gout, pooling='max', dtype=torch.float64, rounding=None):
    """d (sum of out * gout) / d x, (N, 3, H, W) in `dtype`, by the walk of the module docstring on the activations `acts`
    ({i: (N, C, H, W)}, i = 1 .. 14).  p: state_dict-like; gout: (N, 1, H/2, W/2)."""
    if rounding not in ROUNDINGS:
        raise ValueError(f'unknown rounding {rounding!r}')
    S = B.r if rounding == 'bf16' else (lambda t: t)              # a stored gradient
    O = B.r if rounding else (lambda t: t)                        # an operand of a contraction
    c = lambda t: t.detach().to(dtype)
    a = {i: c(t) for i, t in acts.items()}

    def scale_of(bp):
        if rounding:
            return c(E.scale_shift(p, bp)[0])
        return c(p[bp + 'weight']) / torch.sqrt(c(p[bp + 'running_var']) + E.EPS)

    # OutConv: pixel values from the stored a14, pooling, ReLU; fp32 weights
    wo, bo = c(p['outc.conv.0.weight']), c(p['outc.conv.0.bias'])
    z = F.conv2d(a[14], wo, bo)
    pz = F.max_pool2d(z, 2) if pooling == 'max' else F.avg_pool2d(z, 2)
    g = _route(z, c(gout).reshape(pz.shape) * (pz > 0).to(dtype), pooling)
    g = S(F.conv_transpose2d(g, wo))

    def layer(i, g, gp=None):
        cw, bp = _names(i)
        if gp is not None:
            g = g + _route(a[i], gp, pooling)
        dz = S(g * scale_of(bp)[None, :, None, None] * (a[i] > 0).to(dtype))
        w = O(c(p[cw]))
        shape = list(a[i].shape)
        shape[1] = w.shape[1]
        return torch.nn.grad.conv2d_input(shape, w, O(dz), padding=1)

    def up(k, gcat):
        C = gcat.shape[1] // 2
        return gcat[:, :C], S(F.conv2d(O(gcat[:, C:]), O(c(p[UP[k] + 'up.weight'])), None, stride=2))

    g = S(layer(14, g)); g = S(layer(13, g)); gs1, g = up(2, g)
    g = S(layer(12, g)); g = S(layer(11, g)); gs2, g = up(1, g)
    g = S(layer(10, g)); g = S(layer(9, g)); gs3, g = up(0, g)
    g = S(layer(8, g)); gp3 = S(layer(7, g))
    g = S(layer(6, gs3, gp3)); gp2 = S(layer(5, g))
    g = S(layer(4, gs2, gp2)); gp1 = S(layer(3, g))
    g = S(layer(2, gs1, gp1))
    return layer(1, g)                                            # the image gradient is not rounded


def oracle_feat_grad(d, path_ids, pm_state, feat_map, weights, dtype=torch.float64, rounding=None):
    """sens_oracle.oracle_sensitivity with the FEATURE MAP as a leaf: dict(pred [T], feat [P]) - the predictions and
    d J / d feat_map of design d, fp64, J = sum_r w_r pred_r."""
    import numpy as np
    p = {k: (v.detach().to(dtype) if v.dtype.is_floating_point else v.clone()) for k, v in pm_state.items()}
    extra = dict(rounding=rounding) if rounding is not None else {}
    cf = torch.from_numpy(np.asarray(d.cell_feat)).to(dtype)
    nf = torch.from_numpy(np.asarray(d.net_feat)).to(dtype)
    fm = feat_map.detach().cpu().to(dtype).reshape(1, -1).clone().requires_grad_(True)
    csr = R.design_csr(d)
    h = torch.zeros((d.N, p['gnn.fc_cell_self.layers.2.weight'].shape[0]), dtype=dtype)
    ends, paths = R.bucket_paths(path_ids, d.path2level, d.path2endpoint)
    P = d.map_size * d.map_size
    outs = []
    for level_id in range(d.L):
        tg, pids = ends.get(level_id, []), paths.get(level_id, [])
        path_map = R.dense_mask_rows(d.mask_indptr, d.mask_cols, pids, P, dtype) * fm if len(pids) else None
        lvl = torch.tensor([float(level_id)], dtype=dtype)
        h, y = R.pathmodel_level(p, csr, h, cf, nf, d.levels[level_id], tg, level_id, lvl, path_map, **extra)
        if y is not None:
            outs.append(y)
    pred = torch.cat(outs, 0)
    w = torch.as_tensor(weights).detach().cpu().to(dtype)
    assert w.shape == pred.shape
    (pred * w).sum().backward()
    return dict(pred=pred.detach().double(), feat=fm.grad.reshape(-1).double())
