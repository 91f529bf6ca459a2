// THE MOVE RULE and THE WINDOW of include/mmft_search.h as code, stated once.  A pin moved by a displacement is the sum in
// 64 bits saturated to int32; offset w of a window of radius r is the displacement (w / side - r, w % side - r), side =
// 2 r + 1.  The kernels that form overrides (trial_stage_group of trial_row.h for search.hip and refine.hip, swap_rows_kernel)
// and the ones that write the tables (commit_apply_kernel, swap_apply_kernel) move pins by `moved`; search.hip, commit.hip and refine.hip
// decode offsets and refuse radii by the window here: the tests hold them to the same coordinates, and the rule is here.
#pragma once
#include <hip/hip_runtime.h>

namespace mmft {

// a resident coordinate moved by d cells (d a window displacement, or a difference of two resident coordinates:
// |c + d| < 2^33): the sum in 64 bits, saturated to int32
__device__ __forceinline__ int moved(int c, long long d) {
  const long long v = (long long)c + d;
  return v > 2147483647ll ? 2147483647 : (v < -2147483648ll ? (int)-2147483648ll : (int)v);
}

constexpr int WINDOW_RADIUS_MAX = 8;

__host__ __device__ inline int window_side(int radius) { return 2 * radius + 1; }
__host__ __device__ inline int window_cells(int radius) { return window_side(radius) * window_side(radius); }   // W
__host__ __device__ inline int window_centre(int radius) { return 2 * radius * (radius + 1); }                  // the offset of (0, 0)
__host__ __device__ inline void window_offset(int w, int radius, int& dx, int& dy) {
  const int side = window_side(radius);
  dx = w / side - radius;
  dy = w % side - radius;
}

}  // namespace mmft
