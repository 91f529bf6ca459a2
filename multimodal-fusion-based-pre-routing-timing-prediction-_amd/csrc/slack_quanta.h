// THE QUANTUM of include/mmft_crit_sums.h as device code, stated once: the criticality sums (crit.hip) and the window search's
// scores (search.hip) add the same integers, and the tests compare both with criticality.reference_quanta bit by bit.
#pragma once
#include <hip/hip_runtime.h>

namespace mmft {

// The quanta of a violating slack s < 0 (-inf included): rint(min(-s, 2^(32 - L)) * 2^L), exactly.  The scaling by a power of
// two is exact in fp32 (it only raises the exponent; a denormal scaled by at most 2^30 rounds to 0 whether or not it is flushed
// first), rintf rounds to nearest even, and below the cap the result is an integer fp32 below 2^32 (at most 2^32 - 256), which
// the conversion to unsigned takes as it is.
__device__ __forceinline__ unsigned long long crit_quanta(float s, int scale_log2, bool& capped) {
  const float m = -s;
  capped = m >= ldexpf(1.f, 32 - scale_log2);
  const unsigned below = (unsigned)rintf(ldexpf(capped ? 0.f : m, scale_log2));    // (never converts a value out of range)
  return capped ? (1ull << 32) : (unsigned long long)below;
}

}  // namespace mmft
