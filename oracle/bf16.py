"""Rounding primitives of the bf16 math mode for the CPU oracle  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

`restatement.py` with `rounding='bf16'` rounds to bf16 exactly where MMFT_MATH_BF16 rounds and nowhere else; what is left
between that oracle and the kernels is fp32 accumulation order plus the rare ReLU / max-pool decision that a last-bit
difference flips.  Plain torch on the CPU; nothing here imports the product package.

Conversion.  The kernels round fp32 values (v_cvt_pk_bf16_f32: round to nearest, ties to even).  `r(t)` therefore goes
fp64 -> fp32 -> bf16, which is also what torch does for a direct fp64 -> bf16 cast: 1 + 2^-8 + 2^-30 is first rounded to
the fp32 tie 1 + 2^-8 and then to 1.0, where a single fp64 -> bf16 rounding would give 1 + 2^-7.  The double rounding is
chosen on purpose: it is the rounding of the fp32 value the kernel holds (tests/test_oracle_bf16_cpu.py pins both facts).

Primitives (each a torch.autograd.Function with the backward written out):
  r(t)                  round to bf16, value kept in t's dtype; no gradient path of its own
  stored(t)             a tensor the kernels keep in HBM as bf16: rounds the value forward and the incoming gradient backward
  linear_bf16           y = r(x) r(w)^T + b;  dx = r(g) r(w);  dw = r(g)^T r(x);  db = sum g  (the gradient as it arrives)
  conv2d_bf16           the same for a 3x3 / pad-1 convolution without bias
  conv_transpose2d_bf16 the same for the k = 2, s = 2 transposed convolution with bias
Where a kernel's bias gradient sums a rounded gradient the rounding sits upstream, in a `stored` on that gradient's tensor.

Rounding map (paths below the package's csrc/; class = the name `classes()` knows it by, used for ablation):

| where | what is bf16 | kernel line | class |
|---|---|---|---|
| feature MLPs fc_cell_self / fc_net_self (mlp_feat.hip) | X at staging (:231), W1 / W2 fragments (:38, :172-190), the hidden H in LDS (:115-117); backward G (:225), recomputed H and dH as MFMA operands (:262-265). db1 sums the fp32 dH (:262 `dsum += dh` before the pack), db2 the fp32 G (:224 `gsum += v`) | mlp_feat.hip | sweep |
| fc_cell_neigh in the level kernels (mlp2_bf16.hip, rows_outer.hip) | A and the packed W1 / W2 / W2^T / W1^T (ops.pack_bf16, sweep.py:565-566); weight gradients round g and x at staging (rows_outer.hip:7-9) | mlp2_bf16.hip, rows_outer.hip | sweep |
| fc_cell_neigh hidden HN / DHN (sweep.HIDDEN_BF16) | HN and DHN stored as bf16 ONLY when sweep.HIDDEN_BF16 is set, the bf16 weight packs exist, the cell levels >= 2 are one contiguous row range and the attention branch is off (sweep.py:572 `st.hid16`; the whole-sweep entry on DesignBatch-numbered graphs); otherwise they stay fp32 and this class must be left out. Modelled as a `stored` on the hidden tensor. Its only visible effect is db1, which sums the rounded DHN (rows_outer.hip:1 `db[o] = sum_r g[r][o]` of the bf16 DHN rows) | sweep.py:569-573 | hidden |
| gathers, softmax-sum, mean, h, G, PRE, A, LSE, DA | fp32 (hardware exp / log are below bf16 resolution: not modelled) | - | - |
| head: fcn masked projection (fusion.hip) | nothing: fp32 in both modes | - | - |
| head: mlp_fuse, mlp_alpha (GEMM engine) | both operands of every contraction (gemm_bf16.h:32 `v_cvt_pk_bf16_f32`, selected at gemm_engine.h:678); the bias gradient from the fp32 staging registers | gemm_engine.h:678 | head |
| U-Net conv (unet16_conv.hip) | input image at staging (:140), packed weights (:63) | unet16_conv.hip:140, :63 | conv |
| U-Net conv output z | rounded on store (:216); the BatchNorm statistics are of the ROUNDED z (:10-11) | unet16_conv.hip:216 | act (bnstats: statistics of r(z)) |
| BN apply / pool (unet16_ew.hip) | a = relu(fma(z, scale, shift)) rounded (:105, :141); max pool of the rounded values (exact), avg pool = 0.25 * sum of the rounded values, rounded (:109, :154) | unet16_ew.hip:105, :141, :154 | act |
| ConvTranspose (unet16_convt.hip) | operands (packed weights, bf16 input), output rounded into the concatenation buffer (:68) | unet16_convt.hip:68 | conv (operands), act (output) |
| OutConv (unet16_ew.hip:343-) | bf16 activations (:371); weights fp32 (`const float* w`, :350); fp32 output; dx stored as bf16 (:432) | unet16_ew.hip:371, :432 | act, grad |
| U-Net backward | g_i, dz_i, gcat_k, gp_k stored as bf16: conv input gradients (unet16_conv.hip:216, the forward kernel on dz), dz after the whole BN-backward formula (unet16_ew.hip:281), pool backward + skip add in fp32 rounded once (unet16_ew.hip:338), ConvTranspose input gradient (unet16_convt.hip:106). Max pool routes to torch's first maximum of the stored values (unet16_ew.hip:316-321) | see left | grad |

Where two consumers' gradients meet (a skip activation: its concatenation half and its pooled copy) the kernel adds them
in fp32 and rounds once; the oracle puts `stored` on the joined tensor only.
"""
import torch
import torch.nn.functional as F

CLASSES = ('sweep', 'head', 'conv', 'act', 'grad', 'bnstats', 'hidden')


def classes(rounding):
    """None -> frozenset(); 'bf16' -> every class; an iterable of class names -> those (ablation)."""
    if rounding is None:
        return frozenset()
    if rounding == 'bf16':
        return frozenset(CLASSES)
    out = frozenset(rounding)
    bad = out - set(CLASSES)
    if bad:
        raise ValueError(f'unknown rounding classes {sorted(bad)}')
    return out


def r(t):
    """Round to bf16 (ties to even) through fp32, keep t's dtype.  See the module docstring for why through fp32."""
    return t.float().bfloat16().to(t.dtype)


class _Stored(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, value, grad):
        ctx.grad = grad
        return r(x) if value else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (r(g) if ctx.grad else g), None, None


def stored(t, value=True, grad=True):
    """value=False / grad=False switch one direction off (ablation of the 'act' / 'grad' classes)."""
    return _Stored.apply(t, value, grad)


class _LinearBF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        xr, wr = r(x), r(w)
        ctx.save_for_backward(xr, wr)
        ctx.has_b = b is not None
        return F.linear(xr, wr, b)

    @staticmethod
    def backward(ctx, g):
        xr, wr = ctx.saved_tensors
        gr = r(g)
        g2, x2 = gr.reshape(-1, gr.shape[-1]), xr.reshape(-1, xr.shape[-1])
        dx = (g2 @ wr).reshape(xr.shape)
        dw = g2.T @ x2
        db = g.reshape(-1, g.shape[-1]).sum(0) if ctx.has_b else None
        return dx, dw, db


def linear_bf16(x, w, b=None):
    return _LinearBF16.apply(x, w, b)


class _Conv2dBF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, padding):
        xr, wr = r(x), r(w)
        ctx.save_for_backward(xr, wr)
        ctx.padding = padding
        return F.conv2d(xr, wr, None, padding=padding)

    @staticmethod
    def backward(ctx, g):
        xr, wr = ctx.saved_tensors
        gr = r(g)
        dx = torch.nn.grad.conv2d_input(xr.shape, wr, gr, padding=ctx.padding)
        dw = torch.nn.grad.conv2d_weight(xr, wr.shape, gr, padding=ctx.padding)
        return dx, dw, None


def conv2d_bf16(x, w, padding=1):
    return _Conv2dBF16.apply(x, w, padding)


class _ConvT2dBF16(torch.autograd.Function):
    """ConvTranspose2d(k = 2, s = 2): the adjoint of a stride-2 2x2 convolution with the same weight."""

    @staticmethod
    def forward(ctx, x, w, b):
        xr, wr = r(x), r(w)
        ctx.save_for_backward(xr, wr)
        ctx.has_b = b is not None
        return F.conv_transpose2d(xr, wr, b, stride=2)

    @staticmethod
    def backward(ctx, g):
        xr, wr = ctx.saved_tensors
        gr = r(g)
        dx = F.conv2d(gr, wr, None, stride=2)                                     # (N, Ci, h, w)
        # dw[ci, co, a, b] = sum_{n, y, x} x[n, ci, y, x] g[n, co, 2y + a, 2x + b]
        N, Co, H2, W2 = gr.shape
        gq = gr.reshape(N, Co, H2 // 2, 2, W2 // 2, 2)
        dw = torch.einsum('nixy,noxayb->ioab', xr, gq)
        db = g.sum((0, 2, 3)) if ctx.has_b else None
        return dx, dw, db


def conv_transpose2d_bf16(x, w, b=None):
    return _ConvT2dBF16.apply(x, w, b)
