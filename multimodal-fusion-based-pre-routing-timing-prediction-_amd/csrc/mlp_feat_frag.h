// Fragment helpers of the feature-MLP kernels (mlp_feat.hip: forward and weight gradients; mlp_feat_dx.hip: input gradient):
// fp32 values packed to the bf16 MFMA operand registers of mlp_tile_bf16.h's lane layout.
#pragma once
#include "mlp_tile_bf16.h"

namespace mmft {

__device__ __forceinline__ unsigned short mf_bf16(float v) { return (unsigned short)(pack_bf16(v, 0.f) & 0xffff); }

__device__ __forceinline__ bf16x8 mf_pack8(const float* v) {
  u32x4 p = {pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
  return __builtin_bit_cast(bf16x8, p);
}

// A fragment of W1 [HD][fin] for hidden column `col`, k = k0 .. k0 + 7 (zero beyond fin)
__device__ __forceinline__ bf16x8 mf_w1_frag(const float* __restrict__ w1, int fin, int col, int k0) {
  float v[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) v[t] = k0 + t < fin ? w1[(long long)col * fin + k0 + t] : 0.f;
  return mf_pack8(v);
}

}  // namespace mmft
