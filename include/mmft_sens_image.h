/* Sensitivity with respect to the layout IMAGE: the two kernels the eval-mode U-Net (mmft_u16_conv3x3_eval of mmft.h, BatchNorm2d
 * from its running statistics, src/Unet.py:16-21 after .eval()) lacks for a DATA gradient - no weight gradient, no BatchNorm
 * parameter gradient.  Everything else of that backward walk is an entry point of mmft.h (mmft_u16_outconv_bwd,
 * mmft_u16_conv3x3 on the mode-1 packs, mmft_u16_convt_dgrad); mmft.unet16.unet_eval_input_grad strings them together.
 *
 * Like include/mmft_report.h, mmft_place.h, mmft_incr.h, mmft_crit.h, mmft_head.h, mmft_crit_sums.h and mmft_sens.h this
 * header holds entry points beyond the generic layer ABI of mmft.h, under its conventions (extern "C", int result, raw device
 * pointers, `int device, void* stream` last, the error codes and mmft_last_error of mmft.h), compiled into the same library,
 * bound by mmft.lib.simg and pinned by a ledger of its own (tests/test_sens_image_cpu.py).
 *
 * mmft_u16_frozen_bwd: the gradient of a = bf16(relu(fmaf(acc, scale, shift))) with respect to acc, where
 *   invstd = 1 / sqrtf(running_var + eps);  scale = gamma * invstd          (fp32, the forward's own sequence)
 * The ReLU mask is read from the STORED activation a (a > 0; a NaN counts as not positive).
 *   gp == NULL  (plain form)    dz[p][c] = bf16(a[p][c] > 0 ? g[p][c] * scale[c] : 0)
 *   gp != NULL  (pooled form)   dz[p][c] = bf16(a[p][c] > 0 ? (g[p][c] + route(gp)[p][c]) * scale[c] : 0)
 *       the layer's output also fed a 2x2 pooling: g is the skip connection's gradient, gp the pooled tensor's, and route is
 *       the rule of mmft_u16_pool_bwd - MMFT_POOL_MAX: the window's gp goes to torch's first maximum of the stored values in
 *       scan order, a NaN wins; MMFT_POOL_AVG: a quarter of it to each pixel.  Sum, product and mask in fp32, ONE rounding.
 * a: bf16, pixel pitch lda elements (a channel slice of a concatenation buffer);  g: bf16, pixel pitch ldg;  gp: bf16 dense
 * [N][H/2][W/2][C];  dz: bf16 dense [N][H][W][C];  gamma, running_var: fp32 [C].  C in {16, 32, 64, 128}.
 *
 * mmft_u16_conv3x3_dgrad_image: the input gradient of the FIRST convolution (Conv2d(3, 16, 3, padding=1, bias=False),
 * src/Unet.py:16), which training never needs:
 *   dx[n][ci][y][x] = sum over co, ky, kx of  bf16(w[co][ci][ky][kx]) * dz1[n][y + 1 - ky][x + 1 - kx][co]     (0 outside)
 * accumulated in fp32 in a fixed order.  dz1: bf16 [N][H][W][16];  w: the layer's fp32 parameter in channels_last memory
 * ([16][3][3][3] = co, ky, kx, ci), rounded to bf16 in the kernel as the forward's weight pack rounds it;  dx: fp32 NCHW
 * [N][3][H][W], every element written, not rounded.  H % 8 == 0, W % 32 == 0, H >= 8.
 *
 * GUARANTEES.  One launch each, no workspace, no atomics, no synchronisation between workgroups: same inputs, same bits.
 * Nothing is written outside dz / dx.  The sizes are judged first: N < 0, C outside the set, lda or ldg below C or not a
 * multiple of 8, H or W not positive (frozen_bwd with gp: not even; dgrad_image: H % 8, W % 32), an unknown pool mode with
 * gp.  N == 0 then returns 0 and looks at no pointer.  Otherwise a null pointer or a pointer that is not 16-byte aligned is
 * refused.  Every refusal is MMFT_ERR_BAD_ARG, made on the host before the device is looked at; nothing is launched. */
#ifndef MMFT_SENS_IMAGE_H
#define MMFT_SENS_IMAGE_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

int mmft_u16_frozen_bwd(const void* a, int lda, const void* g, int ldg, const void* gp, const float* gamma,
                        const float* running_var, float eps, void* dz, int N, int H, int W, int C, int pool_mode,
                        int device, void* stream);

int mmft_u16_conv3x3_dgrad_image(const void* dz1, const float* w, float* dx, int N, int H, int W, int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
