// DATA gradient of the layout U-Net in EVAL mode (bf16 math mode; include/mmft_sens_image.h): the two kernels the backward
// walk of mmft.unet16.unet_eval_input_grad does not find among the training kernels.
//   u16_frozen_bwd*_kernel        backward of the eval epilogue of unet16_conv.hip, a = bf16(relu(fmaf(acc, scale, shift))),
//                                 with the ReLU mask read from the STORED activation; the pooled form also routes the pooled
//                                 tensor's gradient (to u16_pool_argmax of unet16.h, as u16_pool_bwd_kernel of unet16_ew.hip
//                                 does) and adds the skip connection's in the same pass - one rounding, no round trip of g
//   u16_conv3x3_dgrad_image_kernel  input gradient of the 3 -> 16 convolution, fp32 NCHW, from an LDS-resident halo tile
//                                 on the MFMA (the 3 input channels padded to 16 rows)
// No weight gradient, no BatchNorm parameter gradient, no workspace, no atomics: same inputs, same bits.
#include "unet16.h"
#include "../../include/mmft_sens_image.h"

namespace mmft {

// scale of 8 consecutive channels: bn_frozen_scale (unet16.h), the function the eval epilogue of unet16_conv.hip forms it with
__device__ __forceinline__ void frozen_scale8(const float* __restrict__ gamma, const float* __restrict__ rvar, float eps, int c0, float sc[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) sc[j] = bn_frozen_scale(gamma[c0 + j], rvar[c0 + j], eps);
}

struct U16FrozenBwdArgs {
  const u16* a;        // stored activation, pixel pitch lda
  int lda;
  const u16* g;        // gradient at a (plain) / the skip connection's gradient (pooled), pixel pitch ldg
  int ldg;
  const u16* gp;       // [N][H/2][W/2][C] (pooled form only)
  const float* gamma;
  const float* rvar;
  float eps;
  u16* dz;             // [N][H][W][C]
  int N, H, W, C, pool_mode;
};

// plain form; item = (pixel, group of 8 channels).  The grid stride is a multiple of C / 8 (256 is), so a thread keeps its
// channel group and forms its scales once.
__global__ void __launch_bounds__(256) u16_frozen_bwd_kernel(U16FrozenBwdArgs p) {
  const int CG = p.C / 8;
  const long long total = (long long)p.N * p.H * p.W * CG;
  const int cg = threadIdx.x % CG;
  float sc[8];
  frozen_scale8(p.gamma, p.rvar, p.eps, cg * 8, sc);
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
    const long long pix = it / CG;
    float av[8], gv[8];
    unpack8(*reinterpret_cast<const u32x4*>(p.a + pix * p.lda + cg * 8), av);
    unpack8(*reinterpret_cast<const u32x4*>(p.g + pix * p.ldg + cg * 8), gv);
#pragma unroll
    for (int j = 0; j < 8; ++j) gv[j] = av[j] > 0.f ? __fmul_rn(gv[j], sc[j]) : 0.f;
    *reinterpret_cast<u32x4*>(p.dz + pix * p.C + cg * 8) = pack8(gv);
  }
}

// pooled form; item = (2x2 window, group of 8 channels), as u16_pool_bwd_kernel
__global__ void __launch_bounds__(256) u16_frozen_bwd_pool_kernel(U16FrozenBwdArgs p) {
  const int CG = p.C / 8, H2 = p.H / 2, W2 = p.W / 2;
  const long long total = (long long)p.N * H2 * W2 * CG;
  const int cg = threadIdx.x % CG;
  float sc[8];
  frozen_scale8(p.gamma, p.rvar, p.eps, cg * 8, sc);
  for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long long)gridDim.x * 256) {
    const long long win = it / CG;
    const int x2 = (int)(win % W2), y2 = (int)((win / W2) % H2), img = (int)(win / ((long long)W2 * H2));
    const long long p00 = ((long long)img * p.H + 2 * y2) * p.W + 2 * x2;
    float gpv[8];
    unpack8(*reinterpret_cast<const u32x4*>(p.gp + win * p.C + cg * 8), gpv);
    float av[4][8];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      unpack8(*reinterpret_cast<const u32x4*>(p.a + (p00 + (k >> 1) * p.W + (k & 1)) * p.lda + cg * 8), av[k]);
    int arg[8];
    u16_pool_argmax(av, arg);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long pix = p00 + (k >> 1) * p.W + (k & 1);
      float gs[8];
      unpack8(*reinterpret_cast<const u32x4*>(p.g + pix * p.ldg + cg * 8), gs);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float routed = p.pool_mode == MMFT_POOL_MAX ? (arg[j] == k ? gpv[j] : 0.f) : __fmul_rn(0.25f, gpv[j]);
        gs[j] = av[k][j] > 0.f ? __fmul_rn(__fadd_rn(gs[j], routed), sc[j]) : 0.f;
      }
      *reinterpret_cast<u32x4*>(p.dz + pix * p.C + cg * 8) = pack8(gs);
    }
  }
}

// ---------------------------------------------------------------------------------------------- image gradient
// One workgroup of four waves per tile of 8 x 32 pixels (H % 8 == 0, W % 32 == 0: no partial tiles), two rows per wave.
// The tile of dz1 with a one-pixel halo (zero outside the image) lies in LDS as [pixel][16 channels].  Per tap one v_mfma_f32_16x16x16_bf16 contracts the 16
// output channels of 16 neighbouring pixels (B: the natural fragment, lane (r, q) = pixel r, channels 4q .. 4q + 3, one
// 8-byte LDS read) with the tap's weights (A: lane (r, q) = w[co = 4q .. 4q + 3][ci = r], rows ci >= 3 zero, rounded to
// bf16 from the fp32 parameter when the kernel starts): D lane (r, 0) = dx of pixel r, input channels 0 .. 2.  The 9 taps
// accumulate in the order (ky, kx): a fixed order.
constexpr int DG_TH = 8, DG_TW = 32, DG_XR = DG_TH + 2, DG_XC = DG_TW + 2, DG_CO = 16, DG_CI = 3;
constexpr int DG_ITEMS = 2 * DG_XR * DG_XC, DG_LD = (DG_ITEMS + 255) / 256;    // 16-byte pieces of the halo tile, per thread

__global__ void __launch_bounds__(256) u16_conv3x3_dgrad_image_kernel(const u16* __restrict__ dz, const float* __restrict__ w,
                                                                     float* __restrict__ dx, int H, int W, int tiles_x, int tiles_y) {
  __shared__ __attribute__((aligned(16))) u16 xs[DG_XR * DG_XC * DG_CO];
  const int t = threadIdx.x, r = t & 15, q = (t >> 4) & 3, wave = t >> 6;
  const int tile = blockIdx.x;
  const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, img = tile / (tiles_x * tiles_y);
  const int x0 = tx * DG_TW, y0 = ty * DG_TH;
  // the 680 16-byte pieces of the halo tile: every load is issued before the first LDS store
  u32x4 xv[DG_LD];
#pragma unroll
  for (int k = 0; k < DG_LD; ++k) {
    const int it = t + 256 * k, pix = it >> 1, half = it & 1;
    const int yy = y0 + pix / DG_XC - 1, xx = x0 + pix % DG_XC - 1;
    xv[k] = u32x4{0u, 0u, 0u, 0u};
    if (it < DG_ITEMS && yy >= 0 && yy < H && xx >= 0 && xx < W)
      xv[k] = *reinterpret_cast<const u32x4*>(dz + (((long long)img * H + yy) * W + xx) * DG_CO + half * 8);
  }
#pragma unroll
  for (int k = 0; k < DG_LD; ++k) {
    const int it = t + 256 * k;
    if (it < DG_ITEMS) *reinterpret_cast<u32x4*>(xs + it * 8) = xv[k];
  }
  s16x4 wf[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    float f[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < DG_CI) {
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] = w[((4 * q + j) * 9 + tap) * DG_CI + r];      // channels_last memory: [co][ky][kx][ci]
    }
    wf[tap] = pack_bf16x4(f[0], f[1], f[2], f[3]);
  }
  __syncthreads();
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int row = 2 * wave; row < 2 * wave + 2; ++row) {
    f32x4 acc[2] = {zero, zero};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          // dz1[y + 1 - ky][x + 1 - kx] in halo coordinates (+1)
          const int hp = (row + 2 - ky) * DG_XC + s * 16 + r + 2 - kx;
          const s16x4 xf = *reinterpret_cast<const s16x4*>(xs + hp * DG_CO + 4 * q);
          acc[s] = mfma_bf16_k16(wf[ky * 3 + kx], xf, acc[s]);
        }
    if (q == 0) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int ci = 0; ci < DG_CI; ++ci)
          dx[(((long long)img * DG_CI + ci) * H + y0 + row) * W + x0 + s * 16 + r] = acc[s][ci];
    }
  }
}

}  // namespace mmft

using namespace mmft;

extern "C" {

int mmft_u16_frozen_bwd(const void* a, int lda, const void* g, int ldg, const void* gp, const float* gamma,
                        const float* running_var, float eps, void* dz, int N, int H, int W, int C, int pool_mode,
                        int device, void* stream) {
  MMFT_REQUIRE(N >= 0 && H > 0 && W > 0 && (C == 16 || C == 32 || C == 64 || C == 128),
               "u16_frozen_bwd: bad sizes (N >= 0, H, W > 0, C in {16, 32, 64, 128})");
  MMFT_REQUIRE(lda >= C && lda % 8 == 0 && ldg >= C && ldg % 8 == 0, "u16_frozen_bwd: bad sizes (a pixel pitch holds C channels and is a multiple of 8)");
  MMFT_REQUIRE(!gp || (H % 2 == 0 && W % 2 == 0 && (pool_mode == MMFT_POOL_MAX || pool_mode == MMFT_POOL_AVG)),
               "u16_frozen_bwd: bad sizes (the pooled form needs even H, W and a pooling mode)");
  if (N == 0) return MMFT_OK;
  MMFT_REQUIRE(a && g && gamma && running_var && dz, "u16_frozen_bwd: null pointer");
  MMFT_REQUIRE(aligned16(a) && aligned16(g) && aligned16(dz) && (!gp || aligned16(gp)), "u16_frozen_bwd: 16-byte alignment");
  DeviceGuard dg(device);
  U16FrozenBwdArgs p{reinterpret_cast<const u16*>(a), lda, reinterpret_cast<const u16*>(g), ldg, reinterpret_cast<const u16*>(gp),
                     gamma, running_var, eps, reinterpret_cast<u16*>(dz), N, H, W, C, pool_mode};
  const double elems = (double)N * H * W * C;
  if (gp) {
    const long long items = (long long)N * (H / 2) * (W / 2) * (C / 8);
    MMFT_LAUNCH("u16_frozen_bwd_pool_kernel", 2.0 * elems, 2.0 * elems * 3.25, u16_frozen_bwd_pool_kernel, dim3(ew_grid(items)), dim3(256),
                (hipStream_t)stream, p);
  } else {
    const long long items = (long long)N * H * W * (C / 8);
    MMFT_LAUNCH("u16_frozen_bwd_kernel", elems, 2.0 * elems * 3.0, u16_frozen_bwd_kernel, dim3(ew_grid(items)), dim3(256), (hipStream_t)stream, p);
  }
  return check_launch("u16_frozen_bwd");
}

int mmft_u16_conv3x3_dgrad_image(const void* dz1, const float* w, float* dx, int N, int H, int W, int device, void* stream) {
  MMFT_REQUIRE(N >= 0 && H >= DG_TH && H % DG_TH == 0 && W > 0 && W % DG_TW == 0 && (long long)N * (H / DG_TH) * (W / DG_TW) <= 0x7fffffffLL,
               "u16_conv3x3_dgrad_image: bad sizes (N >= 0, H % 8 == 0, W % 32 == 0, H >= 8)");
  if (N == 0) return MMFT_OK;
  MMFT_REQUIRE(dz1 && w && dx, "u16_conv3x3_dgrad_image: null pointer");
  MMFT_REQUIRE(aligned16(dz1) && (reinterpret_cast<uintptr_t>(w) & 3) == 0 && (reinterpret_cast<uintptr_t>(dx) & 3) == 0,
               "u16_conv3x3_dgrad_image: alignment (dz1 16 bytes, w and dx 4)");
  DeviceGuard dg(device);
  const int tiles_x = W / DG_TW, tiles_y = H / DG_TH;
  const double px = (double)N * H * W;
  MMFT_LAUNCH("u16_conv3x3_dgrad_image_kernel", 2.0 * 432.0 * px, 44.0 * px, u16_conv3x3_dgrad_image_kernel, dim3(N * tiles_x * tiles_y), dim3(256),
              (hipStream_t)stream, reinterpret_cast<const u16*>(dz1), w, dx, H, W, tiles_x, tiles_y);
  return check_launch("u16_conv3x3_dgrad_image");
}

}  // extern "C"
