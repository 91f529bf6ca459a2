// Input gradient of the feature MLPs fc_cell_self / fc_net_self (mmft_mlp2_feat_dx_bf16, include/mmft_sens.h), bf16 math
// mode, without a stored hidden tensor: the third kernel of the family in mlp_feat.hip.
//
//   dx[r][0 .. fin) = ((G[r] W2) * relu'(X[r] W1^T + b1)) W1       rows r of a contiguous node range
//
// One kernel reads G (gradient of the MLP's output rows, 512 B per row) and X, recomputes the pre-activation with the
// forward's instruction sequence (tile_layer1 over the same fragments: bitwise the forward's H, so the ReLU mask agrees),
// forms dH = (G W2) * (H > 0) in registers, keeps the 64 x 256 dH tile in LDS as bf16 and contracts it with W1.  Rows are
// independent: no slab, no reduction between workgroups, every output element is written by exactly one lane.  HBM-bound by
// construction (4 (128 + 2 fin) bytes per row against 2 x 256 x (128 + 2 fin) flops).
// Lane layouts are those of mlp_tile_bf16.h: A = weights (lane = output feature, 8 consecutive k), B = row tiles (lane = row,
// 8 consecutive k), D at lane (r16 = lane & 15, q = lane >> 4) = features 4q .. 4q + 3 of row r16.
#include <limits.h>
#include "mlp_tile_bf16.h"
#include "mlp_feat_frag.h"
#include "../../include/mmft_sens.h"

namespace mmft {

struct FeatDxArgs {
  const float* g;
  long long ldg;
  const float* x;
  long long ldx;
  int row0, n, fin;
  const float *w1, *b1, *w2;
  float* dx;
  long long lddx;
};

template <int KS>   // K steps of 32 of the first layer (fin <= 32 KS), as in the forward
__global__ void __launch_bounds__(512) mlp2_feat_dx_kernel(FeatDxArgs a) {
  // NKB 16-column blocks of dx; the 8 waves split the tile's (row block, column block) pairs: wave -> column block
  // wave % NKB, row blocks (wave / NKB) * RPW .. + RPW - 1
  constexpr int BM = 64, RT = BM / 16, KP = KS * 32, XS = KP + 8, GS = L2_D2 + 8, HS = L2_HD + 8, NKB = KP / 16;
  constexpr int RPW = RT * NKB / 8;
  static_assert(RPW >= 1 && RPW * 8 == RT * NKB, "the waves cover the output tile exactly once");
  __shared__ __attribute__((aligned(16))) unsigned short xs[BM * XS];      // X tile  [row][k]
  __shared__ __attribute__((aligned(16))) unsigned short gs[BM * GS];      // G tile  [row][d2]
  __shared__ __attribute__((aligned(16))) unsigned short ds[BM * HS];      // dH tile [row][col]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // weights in registers for the life of the workgroup
  bf16x8 w1f[2][KS], w2tf[2][4], w1tf[8];
  f32x4 b1v[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = wave * 32 + j * 16 + r16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) w1f[j][ks] = mf_w1_frag(a.w1, a.fin, col, ks * 32 + q * 8);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {         // A fragment of W2^T: W2T[col][d2] = w2[d2][col], d2 = 32 ks + 8 q ..
      float v[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) v[t] = a.w2[(long long)(ks * 32 + q * 8 + t) * L2_HD + col];
      w2tf[j][ks] = mf_pack8(v);
    }
    b1v[j] = *reinterpret_cast<const f32x4*>(a.b1 + wave * 32 + j * 16 + q * 4);
  }
  const int kb = wave % NKB, rb0 = (wave / NKB) * RPW;
  const int kout = kb * 16 + r16;            // A fragment of W1^T: W1T[k][col] = w1[col][k], col = 32 ks + 8 q .. (zero beyond fin)
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    float v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = kout < a.fin ? a.w1[(long long)(ks * 32 + q * 8 + t) * a.fin + kout] : 0.f;
    w1tf[ks] = mf_pack8(v);
  }

  const int ntiles = (a.n + BM - 1) / BM;
  // G (four 16-byte groups per thread) and X (BM * KP / 512 scalars) of the workgroup's next tile are requested before
  // this one is multiplied
  constexpr int NGE = BM * L2_D2 / 4 / 512, NXE = BM * KP / 512;
  f32x4 gr[NGE];
  float xr[NXE];
  auto request = [&](int tile) {
    const int m0 = tile * BM;
#pragma unroll
    for (int it = 0; it < NGE; ++it) {
      const int e = tid + it * 512, r = e >> 5, c = (e & 31) * 4;
      gr[it] = m0 + r < a.n ? *reinterpret_cast<const f32x4*>(a.g + (long long)(a.row0 + m0 + r) * a.ldg + c) : zero;
    }
#pragma unroll
    for (int k = 0; k < NXE; ++k) {
      const int e = tid + k * 512, r = e / KP, kk = e % KP;
      xr[k] = (m0 + r < a.n && kk < a.fin) ? a.x[(long long)(a.row0 + m0 + r) * a.ldx + kk] : 0.f;
    }
  };
  if ((int)blockIdx.x < ntiles) request(blockIdx.x);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int m0 = tile * BM;
    // ---- deposit G and X as bf16; rows past the end are zero
#pragma unroll
    for (int it = 0; it < NGE; ++it) {
      const int e = tid + it * 512, r = e >> 5, c = (e & 31) * 4;
      st_bf16x4(gs + r * GS + c, gr[it]);
    }
#pragma unroll
    for (int k = 0; k < NXE; ++k) {
      const int e = tid + k * 512;
      xs[(e / KP) * XS + e % KP] = mf_bf16(xr[k]);
    }
    __syncthreads();
    if (tile + (int)gridDim.x < ntiles) request(tile + gridDim.x);
    // ---- H = X W1^T + b1 (the forward's tile_layer1), dH = (G W2) * (H > 0): hidden columns [32 wave, 32 wave + 32)
    {
      f32x4 acc1[RT][2], acc3[RT][2];
      tile_layer1<KS, RT>(acc1, w1f, xs, XS, r16, q);
      tile_layer1<4, RT>(acc3, w2tf, gs, GS, r16, q);
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          st_bf16x4(ds + (i * 16 + r16) * HS + wave * 32 + j * 16 + q * 4, relu_mask4(acc3[i][j], acc1[i][j] + b1v[j]));
    }
    __syncthreads();
    // ---- dx = dH W1: the wave's column block of its row blocks (K = 256, tile_layer2 over the W1^T fragments)
#pragma unroll
    for (int ii = 0; ii < RPW; ++ii) {
      const int i = rb0 + ii;
      const f32x4 acc = tile_layer2(w1tf, ds, HS, r16, q, i);
      const int m = m0 + i * 16 + r16;
      if (m >= a.n) continue;
      float* out = a.dx + (long long)(a.row0 + m) * a.lddx + kb * 16 + q * 4;
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (kb * 16 + q * 4 + t < a.fin) out[t] = acc[t];
    }
    // the next deposit overwrites xs / gs, last read before the barrier above; the next dH tile is written after the next
    // deposit's barrier, which every wave reaches only after it has read this one
  }
}

}  // namespace mmft

using namespace mmft;

extern "C" int mmft_mlp2_feat_dx_bf16(const float* g, long long ldg, const float* x, long long ldx, int row0, int n, int fin,
                                      const float* w1, const float* b1, const float* w2, float* dx, long long lddx, int device,
                                      void* stream) {
  MMFT_REQUIRE(n >= 0 && row0 >= 0 && row0 <= INT_MAX - n && fin >= 1 && fin <= 64 && ldx >= fin && lddx >= fin && ldg >= L2_D2,
               "mlp2_feat_dx_bf16: bad sizes (fin <= 64)");
  if (n == 0) return MMFT_OK;
  MMFT_REQUIRE(g && x && w1 && b1 && w2 && dx, "mlp2_feat_dx_bf16: null pointer");
  MMFT_REQUIRE(ldg % 4 == 0 && aligned16(g) && aligned16(b1), "mlp2_feat_dx_bf16: g / b1 must be 16-byte aligned");
  DeviceGuard dg(device);
  FeatDxArgs a{g, ldg, x, ldx, row0, n, fin, w1, b1, w2, dx, lddx};
  const double fl = 2.0 * n * (2.0 * fin * L2_HD + (double)L2_HD * L2_D2), by = 4.0 * n * (2.0 * fin + L2_D2);
  int grid = cdiv(n, 64);
  if (grid > 256) grid = 256;                      // one workgroup per CU (230 - 238 VGPRs): each walks tiles of 64 rows
  if (fin <= 32)
    MMFT_LAUNCH("mlp2_feat_dx_kernel", fl, by, mlp2_feat_dx_kernel<1>, dim3(grid), dim3(512), (hipStream_t)stream, a);
  else
    MMFT_LAUNCH("mlp2_feat_dx_kernel", fl, by, mlp2_feat_dx_kernel<2>, dim3(grid), dim3(512), (hipStream_t)stream, a);
  return check_launch("mlp2_feat_dx_bf16");
}
