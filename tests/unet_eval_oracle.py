"""CPU oracle of the layout U-Net in EVAL mode  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

UNet.forward (src/Unet.py:110-119) with every BatchNorm2d normalising from its running statistics
(`F.batch_norm(training=False)`, src/Unet.py:16-21 after .eval()); no buffer is written.  The shape logic (pooling, the
centre padding of Up, the concatenation order) is that of oracle.restatement's `_pool` / `_up`, restated here because
those call the train-mode DoubleConv.

`rounding='bf16'` is the rounding map of the eval kernels (csrc/unet16_conv.hip, EVAL epilogue), which is NOT the train
path's map: there is no stored pre-activation.
  * operands of every convolution / transposed convolution rounded to bf16 (oracle.bf16.conv2d_bf16 / conv_transpose2d_bf16);
  * scale, shift formed in fp32 by the kernel's sequence: invstd = 1 / sqrtf(rv + eps); scale = gamma * invstd;
    shift = fmaf(-rm, scale, beta);  the affine is applied to the UNROUNDED accumulator, ReLU, then ONE rounding on store;
  * pooled tensors (of the rounded activations) and the transposed convolution's output rounded on store;
  * OutConv: fp32 weights, fp32 output.
`zround=True` is the ablation the kernel test uses: the affine applied to a bf16-rounded pre-activation (what the train
path's map would do).
"""
import torch
import torch.nn.functional as F

from oracle import bf16 as B

EPS = 1e-5


def scale_shift(p, prefix, eps=EPS):
    """(scale, shift) in fp32 exactly as the kernel forms them (each step rounded to fp32; the fma through fp64, where the
    product of two fp32 values is exact)."""
    f32 = lambda t: t.detach().to(torch.float32)
    gamma, beta = f32(p[prefix + 'weight']), f32(p[prefix + 'bias'])
    rm, rv = f32(p[prefix + 'running_mean']), f32(p[prefix + 'running_var'])
    invstd = 1.0 / torch.sqrt(rv + torch.tensor(eps, dtype=torch.float32))
    scale = gamma * invstd
    shift = (-rm.double() * scale.double() + beta.double()).to(torch.float32)
    return scale, shift


def affine_relu_rounded(z, scale, shift, zround=False):
    """bf16(relu(fmaf(z, scale, shift))) of a (N,C,H,W) accumulator z, value kept in z's dtype."""
    c = lambda t: t.double()[None, :, None, None]
    zz = B.r(z) if zround else z
    t = zz.double() * c(scale) + c(shift)
    if z.dtype == torch.float32:
        t = t.to(torch.float32)                       # the kernel's fma rounds to fp32 before the bf16 conversion
    return B.r(torch.relu(t)).to(z.dtype)


def conv_bn_relu(p, cprefix, bprefix, x, rounding=None, eps=EPS, zround=False):
    if not rounding:
        z = F.conv2d(x, p[cprefix], None, padding=1)
        return torch.relu(F.batch_norm(z, p[bprefix + 'running_mean'], p[bprefix + 'running_var'], p[bprefix + 'weight'],
                                       p[bprefix + 'bias'], False, 0.0, eps))
    z = B.conv2d_bf16(x, p[cprefix], 1)
    scale, shift = scale_shift(p, bprefix, eps)
    return affine_relu_rounded(z, scale, shift, zround)


def pool(x, pooling, rounding=None):
    y = F.max_pool2d(x, 2) if pooling == 'max' else F.avg_pool2d(x, 2)
    return B.r(y) if rounding else y


def _double_conv(p, prefix, x, rounding):
    x = conv_bn_relu(p, prefix + 'double_conv.0.weight', prefix + 'double_conv.1.', x, rounding)
    return conv_bn_relu(p, prefix + 'double_conv.3.weight', prefix + 'double_conv.4.', x, rounding)


def _up(p, prefix, x1, x2, rounding):
    if rounding:
        x1 = B.r(B.conv_transpose2d_bf16(x1, p[prefix + 'up.weight'], p[prefix + 'up.bias']))
    else:
        x1 = F.conv_transpose2d(x1, p[prefix + 'up.weight'], p[prefix + 'up.bias'], stride=2)
    dy, dx = x2.shape[2] - x1.shape[2], x2.shape[3] - x1.shape[3]
    x1 = F.pad(x1, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])
    return _double_conv(p, prefix + 'conv.', torch.cat([x2, x1], dim=1), rounding)


@torch.no_grad()
def unet_eval_forward(p, x, pooling='max', rounding=None):
    """p: state_dict-like {name: tensor} in the dtype of x (fp32 or fp64).  Accepts (C,H,W) too."""
    if rounding not in (None, 'bf16'):
        raise ValueError(f'unknown rounding {rounding!r}')
    if x.dim() == 3:
        x = x.unsqueeze(0)
    x1 = _double_conv(p, 'inc.', x, rounding)
    x2 = _double_conv(p, 'down1.maxpool_conv.1.', pool(x1, pooling, rounding), rounding)
    x3 = _double_conv(p, 'down2.maxpool_conv.1.', pool(x2, pooling, rounding), rounding)
    x4 = _double_conv(p, 'down3.maxpool_conv.1.', pool(x3, pooling, rounding), rounding)
    y = _up(p, 'up1.', x4, x3, rounding)
    y = _up(p, 'up2.', y, x2, rounding)
    y = _up(p, 'up3.', y, x1, rounding)
    y = F.conv2d(y, p['outc.conv.0.weight'], p['outc.conv.0.bias'])
    return torch.relu(pool(y, pooling))


def cast_state(sd, dtype):
    return {k: (v.detach().cpu().to(dtype).clone() if v.dtype.is_floating_point else v.detach().cpu().clone()) for k, v in sd.items()}
