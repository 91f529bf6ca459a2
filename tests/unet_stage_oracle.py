"""Stage-by-stage CPU reference of the bf16-storage U-Net train step  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

One function per stage of the step (mmft/unet16.py runs about 55 forward and 120 backward launches): each takes the
stage's inputs as plain (N,C,H,W) tensors plus the parameters, in fp64 or fp32, and returns the stage's outputs rounded to
bf16 exactly where the rounding map of oracle/bf16.py (rows "U-Net ...") says the kernels round.  The backward stages are
written out as formulas; nothing here calls autograd, and nothing imports the product package.  The rounding primitives
(`r`, `conv2d_bf16`, `conv_transpose2d_bf16`) are oracle.bf16's own.

A judge feeds every stage the step's OWN stored inputs (teacher forcing), so the amplification through 14 chained
BatchNorm layers that loosens the whole-network bounds (tests/test_bf16_oracle_gpu.py) does not apply: one stage on given
bf16 operands differs between fp32 and fp64 evaluation in a few elements per 10 000 at the most.

`WIRING` states, a second time and independently of the product's tables, which tensor every convolution layer and Up
block reads and writes (src/Unet.py:98-119 of the reference and oracle.restatement.unet_forward); `reference_step` chains
the stages along it - tests/test_unet_stages_cpu.py holds that chain to autograd of the rounding oracle.

Keyword flags that default to the correct formula switch ONE deliberate error on each (the mutants of the teeth checks).
"""
import torch
import torch.nn.functional as F

from oracle import bf16 as B

EPS, MOMENTUM = 1e-5, 0.1

# ------------------------------------------------------------------------------------------------ the wiring, stated once more
# Tensors: 'image'; act1 .. act14, the ReLU outputs of the 14 convolution layers in forward order (two per DoubleConv:
# inc, down1, down2, down3, up1.conv, up2.conv, up3.conv); pool1 .. pool3, the inputs of down1 .. down3; cat1 .. cat3, the
# concatenations torch.cat([x2, x1], dim=1) of up1 .. up3 (src/Unet.py:67: the skip tensor first, the upsampled one second).
# A (tensor, lo, hi) triple is a channel slice; level k works at (H >> k, W >> k).
_DC = ('inc.', 'down1.maxpool_conv.1.', 'down2.maxpool_conv.1.', 'down3.maxpool_conv.1.', 'up1.conv.', 'up2.conv.', 'up3.conv.')


def _layer(i, ci, co, level, src, dst, pooled, grad_to):
    dc, j = _DC[(i - 1) // 2], (i - 1) % 2
    return dict(i=i, conv=f'{dc}double_conv.{3 * j}.weight', bn=f'{dc}double_conv.{3 * j + 1}.', ci=ci, co=co, level=level,
                src=src, dst=dst, pooled=pooled, grad_to=grad_to)


# grad_to: the tensor whose gradient this layer's input gradient IS (None: the image needs none).  A skip activation's
# gradient (act2, act4, act6) is not written by a convolution: it is the pool backward's sum, SKIPS below.
LAYERS = (
    _layer(1, 3, 16, 0, 'image', ('act1', 0, 16), None, None),                    # inc              src/Unet.py:98,111
    _layer(2, 16, 16, 0, 'act1', ('cat3', 0, 16), 'pool1', 'act1'),               #   x1 -> skip of up3, pooled for down1
    _layer(3, 16, 32, 1, 'pool1', ('act3', 0, 32), None, 'pool1'),                # down1            :99,112
    _layer(4, 32, 32, 1, 'act3', ('cat2', 0, 32), 'pool2', 'act3'),               #   x2 -> skip of up2, pooled for down2
    _layer(5, 32, 64, 2, 'pool2', ('act5', 0, 64), None, 'pool2'),                # down2            :100,113
    _layer(6, 64, 64, 2, 'act5', ('cat1', 0, 64), 'pool3', 'act5'),               #   x3 -> skip of up1, pooled for down3
    _layer(7, 64, 128, 3, 'pool3', ('act7', 0, 128), None, 'pool3'),              # down3            :103,114
    _layer(8, 128, 128, 3, 'act7', ('act8', 0, 128), None, 'act7'),               #   x4
    _layer(9, 128, 64, 2, 'cat1', ('act9', 0, 64), None, 'cat1'),                 # up1.conv         :104,115
    _layer(10, 64, 64, 2, 'act9', ('act10', 0, 64), None, 'act9'),
    _layer(11, 64, 32, 1, 'cat2', ('act11', 0, 32), None, 'cat2'),                # up2.conv         :105,116
    _layer(12, 32, 32, 1, 'act11', ('act12', 0, 32), None, 'act11'),
    _layer(13, 32, 16, 0, 'cat3', ('act13', 0, 16), None, 'cat3'),                # up3.conv         :106,117
    _layer(14, 16, 16, 0, 'act13', ('act14', 0, 16), None, 'act13'),              #   -> OutConv     :108,118
)
# Up blocks: ConvTranspose2d(ci, ci / 2, 2, 2) of `src` (at `level`) into the SECOND half of the concatenation; its input
# gradient, read from that half of the concatenation's gradient, is the whole gradient of `src`.
UPS = (dict(k=1, prefix='up1.up.', ci=128, level=3, src='act8', dst=('cat1', 64, 128), grad_to='act8'),
       dict(k=2, prefix='up2.up.', ci=64, level=2, src='act10', dst=('cat2', 32, 64), grad_to='act10'),
       dict(k=3, prefix='up3.up.', ci=32, level=1, src='act12', dst=('cat3', 16, 32), grad_to='act12'))
# skip activations: (activation, its slice of the concatenation, the pooled copy, level, channels); the activation's
# gradient = r(gradient of the slice + the pooled copy's gradient routed back)
SKIPS = (dict(act='act6', cat=('cat1', 0, 64), pooled='pool3', level=2, c=64),
         dict(act='act4', cat=('cat2', 0, 32), pooled='pool2', level=1, c=32),
         dict(act='act2', cat=('cat3', 0, 16), pooled='pool1', level=0, c=16))
CHANNELS = {'cat1': 128, 'cat2': 64, 'cat3': 32}
WIRING = dict(layers=LAYERS, ups=UPS, skips=SKIPS, out=dict(src='act14', weight='outc.conv.0.weight', bias='outc.conv.0.bias', grad_to='act14'))

r = B.r


def _c(t):
    """(N, C) or (C,) per-channel values against (N,C,H,W)."""
    return t[:, :, None, None] if t.dim() == 2 else t[None, :, None, None]


# ------------------------------------------------------------------------------------------------ forward stages
def conv_fwd(x, w):
    """z = r(conv3x3(r(x), r(W))), pad 1, no bias."""
    return r(B.conv2d_bf16(x, w, 1))


def conv_fwd_mass(x, w):
    """Sum of |terms| of every output element (for the fp32 accumulation bound) and the number of terms."""
    return F.conv2d(r(x).abs(), r(w).abs(), None, padding=1), 9 * x.shape[1]


def bn_stats(z, gamma, beta, eps=EPS, per_image=True, unbiased_invstd=False):
    """Statistics of the STORED z per image: dict of (N, C) mean, invstd, var (biased), scale, shift.
    Mutants: per_image=False (one set over the batch, repeated per image), unbiased_invstd (n / (n - 1) inside invstd)."""
    dims = (2, 3) if per_image else (0, 2, 3)
    mean, var = z.mean(dims), z.var(dims, unbiased=False)
    if not per_image:
        mean, var = mean.expand(z.shape[0], -1), var.expand(z.shape[0], -1)
    n = z.shape[2] * z.shape[3] * (1 if per_image else z.shape[0])
    invstd = 1.0 / torch.sqrt((var * n / (n - 1) if unbiased_invstd else var) + eps)
    scale = gamma[None, :] * invstd
    return dict(mean=mean, invstd=invstd, var=var, scale=scale, shift=beta[None, :] - mean * scale)


def running_update(rm, rv, mean, var, n, momentum=MOMENTUM, unbiased=True):
    """N sequential momentum updates (one per image, in image order) with the unbiased variance var n / (n - 1).
    Mutant: unbiased=False."""
    for i in range(mean.shape[0]):
        rm = (1 - momentum) * rm + momentum * mean[i]
        rv = (1 - momentum) * rv + momentum * (var[i] * n / (n - 1) if unbiased and n > 1 else var[i])
    return rm, rv


def bn_pre(z, scale, shift, fma32):
    """fma(z, scale, shift) per image.  fma32: one rounding to fp32, as the kernels form it (the fp64 product of a bf16 and an
    fp32 value is exact, so the fp64 sum rounded to fp32 is the fused result - tests/unet_eval_oracle.affine_relu_rounded)."""
    t = z.double() * _c(scale).double() + _c(shift).double()
    return t.float() if fma32 else t.to(z.dtype)


def bn_apply(z, scale, shift, fma32=True):
    """a = r(relu(fma(z, scale, shift))), value kept in z's dtype."""
    return r(torch.relu(bn_pre(z, scale, shift, fma32))).to(z.dtype)


def bn_apply_mass(z, scale, shift):
    return z.abs() * _c(scale).abs() + _c(shift).abs(), 2


def _windows(a):
    """(N,C,H,W) -> the four members of every 2x2 window, (4, N, C, H/2, W/2), in torch's scan order (0,0) (0,1) (1,0) (1,1)."""
    return torch.stack([a[:, :, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)])


def _unwindows(v):
    """Inverse of _windows."""
    _, N, C, h, w = v.shape
    out = v.new_zeros((N, C, 2 * h, 2 * w))
    for k, (dy, dx) in enumerate((dy, dx) for dy in (0, 1) for dx in (0, 1)):
        out[:, :, dy::2, dx::2] = v[k]
    return out


def pool_fwd(a, pooling):
    """2x2 pool of the STORED a: max is exact, avg = r(0.25 * sum)."""
    v = _windows(a)
    if pooling == 'max':
        return v.amax(0)
    return r(0.25 * (((v[0] + v[1]) + v[2]) + v[3]))


def pool_fwd_mass(a):
    return 0.25 * _windows(a.abs()).sum(0), 5


def convt_fwd(x, w, b):
    """r(convT(r(x), r(W)) + b), k = 2, s = 2."""
    return r(B.conv_transpose2d_bf16(x, w, b))


def convt_fwd_mass(x, w, b):
    return F.conv_transpose2d(r(x).abs(), r(w).abs(), b.abs(), stride=2), x.shape[1] + 1


def _argmax_first(v, last=False):
    """Index (0..3) of the window's maximum: torch's first maximum (`val > best` in scan order).  Mutant: last."""
    best, arg = v[0], torch.zeros(v.shape[1:], dtype=torch.long)
    for k in range(1, 4):
        upd = (v[k] >= best) if last else (v[k] > best)
        arg = torch.where(upd, torch.full_like(arg, k), arg)
        best = torch.where(upd, v[k], best)
    return arg


def _route(gp, a, pooling, last_max=False):
    """The pooled tensor's gradient sent back through the 2x2 pool of a."""
    if pooling == 'max':
        arg = _argmax_first(_windows(a), last_max)
        return _unwindows(torch.stack([torch.where(arg == k, gp, torch.zeros_like(gp)) for k in range(4)]))
    return _unwindows(torch.stack([0.25 * gp] * 4))


def outconv_fwd(a, w, b, pooling):
    """relu(pool(conv1x1(a, W) + b)): fp32 weights, fp32 output, nothing rounded."""
    y = F.conv2d(a, w, b)
    v = _windows(y)
    return torch.relu(v.amax(0) if pooling == 'max' else 0.25 * (((v[0] + v[1]) + v[2]) + v[3]))


# ------------------------------------------------------------------------------------------------ backward stages
def outconv_bwd(a, w, b, gout, pooling):
    """(dx rounded, dw, db) of outconv_fwd: gm = gout [out > 0]; gy = gm routed through the pool of y (max: first maximum);
    dx = r(gy W);  dw[c] = sum gy a[c];  db = sum gy."""
    y = F.conv2d(a, w, b)
    v = _windows(y)
    out = v.amax(0) if pooling == 'max' else 0.25 * (((v[0] + v[1]) + v[2]) + v[3])
    gy = _route(gout * (out > 0), y, pooling)                                   # (N,1,H,W)
    dx = r(gy * w.reshape(1, -1, 1, 1))
    dw = (gy * a).sum((0, 2, 3)).reshape(w.shape)
    return dx, dw, gy.sum().reshape(1)


def outconv_dx_mass(a, w, b, gout, pooling):
    return outconv_bwd(a, w, b, gout, pooling)[0].abs(), 2


def bn_relu_bwd(g, z, st, fma32=True, xhat_term=True):
    """(dz rounded, dgamma, dbeta) of a = relu(bn(z)) per image, st = bn_stats' rows:
    gm = g [fma(z, scale, shift) > 0];  xhat = (z - mean) invstd;
    dz = r(scale (gm - mean(gm) - xhat mean(gm xhat)));  dgamma = sum gm xhat, dbeta = sum gm over pixels AND images.
    Mutant: xhat_term=False drops xhat mean(gm xhat)."""
    dt = g.dtype
    gm = g * (bn_pre(z, st['scale'], st['shift'], fma32) > 0)
    xh = (z - _c(st['mean']).to(dt)) * _c(st['invstd']).to(dt)
    c0, c1 = gm.mean((2, 3)), (gm * xh).mean((2, 3))
    dz = _c(st['scale']).to(dt) * (gm - _c(c0) - (xh * _c(c1) if xhat_term else 0))
    return r(dz), (gm * xh).sum((0, 2, 3)), gm.sum((0, 2, 3))


def bn_relu_bwd_mass(g, z, st, fma32=True):
    """|scale| (|gm| + mean |gm| + |xhat| mean |gm xhat|); the means are sums over all pixels of an image."""
    dt = g.dtype
    gm = (g * (bn_pre(z, st['scale'], st['shift'], fma32) > 0)).abs()
    xh = ((z - _c(st['mean']).to(dt)) * _c(st['invstd']).to(dt)).abs()
    return _c(st['scale']).to(dt).abs() * (gm + _c(gm.mean((2, 3))) + xh * _c((gm * xh).mean((2, 3)))), z.shape[2] * z.shape[3]


def conv_bwd(x, w, dz, need_dx=True, flipped=True):
    """(dW, dx rounded) of conv_fwd: dW from the stored x and dz (both exact in bf16), dx = r(dz * flipped r(W)).
    Mutant: flipped=False correlates dz with the UNflipped kernel (the transposed pack without the 180 degree turn)."""
    xr, wr, gr = r(x), r(w), r(dz)
    dw = torch.nn.grad.conv2d_weight(xr, wr.shape, gr, padding=1)
    if not need_dx:
        return dw, None
    if flipped:
        dx = torch.nn.grad.conv2d_input(xr.shape, wr, gr, padding=1)
    else:
        dx = torch.nn.grad.conv2d_input(xr.shape, wr.flip(2, 3), gr, padding=1)
    return dw, r(dx)


def conv_dx_mass(x, w, dz):
    return torch.nn.grad.conv2d_input(x.shape, r(w).abs(), r(dz).abs(), padding=1), 9 * w.shape[0]


def pool_bwd(a, gskip, gp, pooling, last_max=False, skip=True):
    """g = r(gskip + route(gp)) of a stored activation that feeds a concatenation's first half AND a 2x2 pool.
    Mutants: last_max (max pooling's gradient to the window's LAST maximum), skip=False (the skip add dropped)."""
    routed = _route(gp, a, pooling, last_max)
    return r(gskip + routed if skip else routed)


def convt_bwd(x, w, g, bias_taps=4):
    """(dW, db, dx rounded) of convt_fwd; g: the gradient of its output (a slice of the concatenation's, stored bf16).
    dW[ci,co,a,b] = sum x[n,ci,y,x] g[n,co,2y+a,2x+b];  db = sum g;  dx = r(conv_stride2(g, r(W))).
    Mutant: bias_taps=1 sums the bias gradient over one tap (a = b = 0) of the four."""
    xr, wr, gr = r(x), r(w), r(g)
    N, Co, H2, W2 = gr.shape
    gq = gr.reshape(N, Co, H2 // 2, 2, W2 // 2, 2)
    dw = torch.einsum('nixy,noxayb->ioab', xr, gq)
    db = g.sum((0, 2, 3)) if bias_taps == 4 else gq[:, :, :, 0, :, 0].sum((0, 2, 3))
    return dw, db, r(F.conv2d(gr, wr, None, stride=2))


def convt_dx_mass(w, g):
    return F.conv2d(r(g).abs(), r(w).abs(), None, stride=2), 4 * w.shape[1]


# ------------------------------------------------------------------------------------------------ the cases and the chain
# the smallest geometries that keep the bf16-storage path (H % 8 == 0, W % 32 == 0, H >= 8) and reach its edges:
# two images; three images whose deepest level is 1 x 12 pixels, average pooling; a deepest level of 5 rows (odd)
# (N, H, W, pooling, seed of x; gout takes the next one).  The deepest tensors hold 2560 .. 4608 elements, where ONE element
# is 2.2e-4 .. 3.9e-4 of the tensor: the seeds of x are those of 40 tried (5, 7, .. 83) at which the fp32 evaluation of every
# stage differs from the fp64 one in the fewest elements (tests/test_unet_stages_cpu.py holds them below a third of the cap)
GEOMETRIES = ((2, 16, 64, 'max', 61), (3, 8, 96, 'avg', 5), (1, 40, 32, 'max', 9))


def seeded_case(unet_cls, N, H, W, pooling, seed):
    """(net on the CPU, x, gout): the network seeded as in the module test (tests/test_unet16_gpu.py); unet_cls is Unet.UNet,
    handed in because this module imports nothing of the product."""
    torch.manual_seed(3)
    net = unet_cls(pooling)
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(seed))
    gout = torch.randn(N, 1, H // 2, W // 2, generator=torch.Generator().manual_seed(seed + 1))
    return net, x, gout


def cast_state(sd, dtype):
    return {k: (v.detach().cpu().to(dtype).clone() if v.dtype.is_floating_point else v.detach().cpu().clone()) for k, v in sd.items()}


def reference_step(p, x, gout, pooling, fma32=False):
    """Every stage in order, each fed the previous stage's reference output; p: {state_dict name: tensor} in x's dtype.
    Returns (tensors, grads, running): tensors holds 'z%d', 'act%d', 'pool%d', 'cat%d', 'out' and the gradients 'g:<name>',
    'dz%d'; grads is keyed by parameter name; running by buffer name."""
    T, grads, run, stats = {'image': x}, {}, {}, {}
    by_src = {u['src']: u for u in UPS}

    def write(dst, val):
        name, lo, hi = dst
        if name in CHANNELS:
            if name not in T:
                T[name] = val.new_zeros((val.shape[0], CHANNELS[name]) + tuple(val.shape[2:]))
            T[name][:, lo:hi] = val
        else:
            T[name] = val

    for L in LAYERS:
        i, bn = L['i'], L['bn']
        z = T[f'z{i}'] = conv_fwd(T[L['src']], p[L['conv']])
        st = stats[i] = bn_stats(z, p[bn + 'weight'], p[bn + 'bias'])
        run[bn + 'running_mean'], run[bn + 'running_var'] = running_update(p[bn + 'running_mean'], p[bn + 'running_var'], st['mean'],
                                                                           st['var'], z.shape[2] * z.shape[3])
        a = T[f'act{i}'] = bn_apply(z, st['scale'], st['shift'], fma32)
        write(L['dst'], a)
        if L['pooled']:
            T[L['pooled']] = pool_fwd(a, pooling)
        u = by_src.get(f'act{i}')
        if u:
            write(u['dst'], convt_fwd(a, p[u['prefix'] + 'weight'], p[u['prefix'] + 'bias']))
    O = WIRING['out']
    T['out'] = outconv_fwd(T[O['src']], p[O['weight']], p[O['bias']], pooling)

    T['g:' + O['grad_to']], grads[O['weight']], grads[O['bias']] = outconv_bwd(T[O['src']], p[O['weight']], p[O['bias']], gout, pooling)
    ups_by_cat = {u['dst'][0]: u for u in UPS}
    skip_by_act = {s['act']: s for s in SKIPS}
    for L in reversed(LAYERS):
        i, bn = L['i'], L['bn']
        if f'act{i}' in skip_by_act:                       # both consumers' gradients exist by now: join them
            s = skip_by_act[f'act{i}']
            cat, lo, hi = s['cat']
            T[f'g:act{i}'] = pool_bwd(T[f'act{i}'], T['g:' + cat][:, lo:hi], T['g:' + s['pooled']], pooling)
        dz, grads[bn + 'weight'], grads[bn + 'bias'] = bn_relu_bwd(T[f'g:act{i}'], T[f'z{i}'], stats[i], fma32)
        T[f'dz{i}'] = dz
        grads[L['conv']], dx = conv_bwd(T[L['src']], p[L['conv']], dz, need_dx=L['grad_to'] is not None)
        if L['grad_to']:
            T['g:' + L['grad_to']] = dx
        if L['src'] in ups_by_cat:                         # the concatenation's gradient is there: the Up block's backward
            u = ups_by_cat[L['src']]
            cat, lo, hi = u['dst']
            dw, db, dxu = convt_bwd(T[u['src']], p[u['prefix'] + 'weight'], T['g:' + cat][:, lo:hi])
            grads[u['prefix'] + 'weight'], grads[u['prefix'] + 'bias'], T['g:' + u['grad_to']] = dw, db, dxu
    return T, grads, run
