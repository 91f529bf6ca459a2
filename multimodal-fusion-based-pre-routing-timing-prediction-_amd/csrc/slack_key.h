// The slack of a batch row and its order-preserving integer key, shared by the timing report (report.hip) and the
// criticality kernels (crit.hip): both headers state ONE rule for slack and validity, this is its one implementation.
#pragma once
#include <hip/hip_runtime.h>

namespace mmft {

// required - pred in one fp32 subtraction; + 0.0f: -0.0 becomes +0.0.  NaN: the row is not valid
__device__ __forceinline__ float slack_of(float required, float pred) { return (required - pred) + 0.0f; }

// unsigned order of the result == numeric order of the floats (-inf lowest, +inf highest); no non-NaN float maps to
// 0xffffffff, which is free to mean "no value"
__device__ __forceinline__ unsigned ordered_bits(float s) {
  const unsigned u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_float(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// a (slack, row) key: ordered_bits(slack) << 32 | row, so the smallest key is the worst slack at the lowest row
typedef unsigned long long slack_u64;
constexpr slack_u64 SLACK_KEY_NONE = ~0ull;   // no valid key has all-ones slack bits (that pattern is a NaN)

}  // namespace mmft
