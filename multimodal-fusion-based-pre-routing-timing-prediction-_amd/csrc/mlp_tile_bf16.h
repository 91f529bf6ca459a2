// The 8-wave bf16 MLP tile shared by the level kernels (mlp2_bf16.hip) and the feature MLPs' forward (mlp_feat.hip):
// rows of a bf16 x tile in LDS -> Linear(K, 256) -> hidden tile in LDS (bf16) -> Linear(256, 128), fp32 accumulate on
// v_mfma_f32_16x16x32_bf16.  Lane layout, for every 16-row block of the tile:
//   lane = (r16 = lane & 15, q = lane >> 4); wave w owns hidden columns [32w, 32w + 32) and output columns [16w, 16w + 16);
//   A fragment (weights, lane = output feature 16-block + r16) and B fragment (row r16 of the block): 8 consecutive k at 8q;
//   result: the lane holds features (16-block) + 4q .. + 3 of row r16.
// Only the arithmetic and the layout live here.  Each kernel keeps its own prologue, gather, row liveness and epilogue
// decisions (bias, mask, add-to-old, which rows are stored), and its own order of loads.
#pragma once
#include "gemm_bf16.h"

namespace mmft {

constexpr int L2_K1 = 128, L2_HD = 256, L2_D2 = 128;
constexpr int L2_XS = L2_K1 + 8, L2_HS = L2_HD + 8;        // LDS row strides in bf16 elements (multiples of 8)

__device__ __forceinline__ f32x4 relu4(f32x4 v) {
  v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f;
  v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f;
  return v;
}
// v where the saved forward activation is positive, else 0 (relu' applied by component)
__device__ __forceinline__ f32x4 relu_mask4(f32x4 v, f32x4 mk) {
  v.x = mk.x > 0.f ? v.x : 0.f; v.y = mk.y > 0.f ? v.y : 0.f;
  v.z = mk.z > 0.f ? v.z : 0.f; v.w = mk.w > 0.f ? v.w : 0.f;
  return v;
}
// four consecutive elements of a bf16 LDS tile (one 8-byte store)
__device__ __forceinline__ void st_bf16x4(unsigned short* p, f32x4 v) {
  const unsigned lo = pack_bf16(v.x, v.y), hi = pack_bf16(v.z, v.w);
  *reinterpret_cast<unsigned long long*>(p) = ((unsigned long long)hi << 32) | lo;
}

// Four consecutive columns of a row of the hidden tensors (fc_cell_neigh's hidden activations HN, their gradients DHN): fp32, or
// - hid16 - bf16 (round to nearest even; `ld` counts elements of the stored type).  Every consumer rounds these values to
// bf16 anyway (MFMA operands of the weight gradients) or only looks at their sign (the ReLU mask), so the bf16 form changes
// no result and halves 2 KB of traffic per row and direction.
__device__ __forceinline__ void hid_store4(float* base, long long off, f32x4 v, int hid16) {
  if (hid16) {
    const unsigned lo = pack_bf16(v.x, v.y), hi = pack_bf16(v.z, v.w);
    *reinterpret_cast<unsigned long long*>(reinterpret_cast<unsigned short*>(base) + off) = ((unsigned long long)hi << 32) | lo;
  } else {
    *reinterpret_cast<f32x4*>(base + off) = v;
  }
}
__device__ __forceinline__ f32x4 hid_load4(const float* base, long long off, int hid16) {
  if (!hid16) return *reinterpret_cast<const f32x4*>(base + off);
  const unsigned long long u = *reinterpret_cast<const unsigned long long*>(reinterpret_cast<const unsigned short*>(base) + off);
  const unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32);
  return f32x4{__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u), __uint_as_float(hi << 16), __uint_as_float(hi & 0xffff0000u)};
}

// The wave's A fragments of the weights, pre-packed bf16 in [n][k] order (mmft_pack_bf16): one 16-byte load each.
// Layer 1: W1 [HD][K1], hidden columns 32 wave + 16 j + r16.
__device__ __forceinline__ void load_w1_frags(bf16x8 (&f)[2][4], const unsigned short* w1, int wave, int r16, int q) {
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      f[j][ks] = *reinterpret_cast<const bf16x8*>(w1 + (long long)(wave * 32 + j * 16 + r16) * L2_K1 + ks * 32 + q * 8);
}
// Layer 2: W2 [D2][HD], output columns 16 wave + r16.
__device__ __forceinline__ void load_w2_frags(bf16x8 (&f)[8], const unsigned short* w2, int wave, int r16, int q) {
#pragma unroll
  for (int ks = 0; ks < 8; ++ks)
    f[ks] = *reinterpret_cast<const bf16x8*>(w2 + (long long)(wave * 16 + r16) * L2_HD + ks * 32 + q * 8);
}

// Layer 1 over RB 16-row blocks of a bf16 tile in LDS (row stride `stride`, K = 32 KS): acc[i][j] = rows 16 i .. of the
// tile times the wave's hidden columns 32 wave + 16 j ..  Blocks i >= nrb (block-uniform) are skipped and stay zero.
template <int KS, int RB>
__device__ __forceinline__ void tile_layer1(f32x4 (&acc)[RB][2], const bf16x8 (&w1f)[2][KS], const unsigned short* xs, int stride,
                                            int r16, int q, int nrb = RB) {
#pragma unroll
  for (int i = 0; i < RB; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      if (i >= nrb) continue;
      const bf16x8 xf = *reinterpret_cast<const bf16x8*>(xs + (i * 16 + r16) * stride + ks * 32 + q * 8);
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1f[j][ks], xf, acc[i][j], 0, 0, 0);
    }
}

// Layer 2 of the 16-row block i of the hidden tile in LDS (row stride `stride`, K = 256): the wave's output columns 16 wave + ..
__device__ __forceinline__ f32x4 tile_layer2(const bf16x8 (&w2f)[8], const unsigned short* hs, int stride, int r16, int q, int i) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    const bf16x8 hf = *reinterpret_cast<const bf16x8*>(hs + (i * 16 + r16) * stride + ks * 32 + q * 8);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2f[ks], hf, acc, 0, 0, 0);
  }
  return acc;
}

}  // namespace mmft
