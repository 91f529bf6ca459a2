// THE MASK RULE of include/mmft_place.h as device code, stated once: the box of two pins (min / max per axis, lower corner
// clamped to 0, upper to map - 1, empty boxes skipped) ORed into an LDS bitmap, cell (x, y) = bit x * map_y + y.
// path_mask_kernel (prep.hip), placed_fc_fwd_kernel (place.hip), crit_scatter_kernel (crit.hip) and the four rows kernels
// (trial.hip, search.hip, refine.hip, swap.hip: under overrides, through trial_row_write of trial_row.h) build their bitmaps
// with it, pin_move.hip takes the axis arithmetic: the tests compare these kernels bitwise, and the rule they share is here.
#pragma once
#include <hip/hip_runtime.h>

namespace mmft {

constexpr int MASK_MAX_CELLS = 65536;       // a bitmap of 8 KB in LDS

// the maps of the kernels that number the bitmap's 64-cell blocks: a multiple of 64 cells, at most MASK_MAX_CELLS
inline bool mask_map_ok(int map_x, int map_y) {
  return map_x > 0 && map_y > 0 && (long long)map_x * map_y <= MASK_MAX_CELLS && ((long long)map_x * map_y) % 64 == 0;
}

// [lo, hi] of the rule along one axis for two pins at u and v on an axis of `lim` cells; empty when lo > hi
__device__ __forceinline__ void mask_axis_range(int u, int v, int lim, int& lo, int& hi) {
  lo = u < v ? u : v;
  hi = u < v ? v : u;
  lo = lo < 0 ? 0 : lo;
  hi = hi >= lim ? lim - 1 : hi;
}

// The box of the pins (xa, ya) and (xb, yb) into `bits`, by the THREADS threads of the workgroup (tid = this one's index).
// A box row is the contiguous bit range [x * map_y + y1, x * map_y + y2]: whole-word masks, not one LDS atomic per cell
// (boxes of long nets cover thousands of cells).
template <int THREADS>
__device__ __forceinline__ void mask_or_box(unsigned* bits, int xa, int ya, int xb, int yb, int map_x, int map_y, int tid) {
  int x1, x2, y1, y2;
  mask_axis_range(xa, xb, map_x, x1, x2);
  mask_axis_range(ya, yb, map_y, y1, y2);
  const int w = y2 - y1 + 1, hgt = x2 - x1 + 1;
  if (w <= 0 || hgt <= 0) return;
  const int wpr = ((w + 30) >> 5) + 1;                        // words a row's range can touch
  for (int c = tid; c < hgt * wpr; c += THREADS) {
    int row = c / wpr, k = c - row * wpr;
    int lo = (x1 + row) * map_y + y1, hi = lo + w - 1;        // inclusive bit range, inside [0, map_x * map_y) after the clamps
    int word = (lo >> 5) + k;
    if (word > (hi >> 5)) continue;
    int b0 = word == (lo >> 5) ? (lo & 31) : 0;
    int b1 = word == (hi >> 5) ? (hi & 31) : 31;
    unsigned mask = (b1 == 31 ? 0xffffffffu : ((1u << (b1 + 1)) - 1u)) & ~((1u << b0) - 1u);
    atomicOr(&bits[word], mask);
  }
}

// The boxes of path[0 .. len) into `bits` (zeroed by the caller, no barrier needed in between).  The node -> coordinate loads
// of up to THREADS nodes are issued by as many threads at once into pin_x / pin_y [THREADS] (LDS) instead of one dependent
// pair of loads per box; chunks overlap by the node two boxes share.  `len` is the same for every thread: the barriers are
// uniform.  CLAMP: node ids outside [0, n_nodes) read the nearest valid pin instead of memory that is not there.
// The caller's barrier follows.
template <int THREADS, bool CLAMP>
__device__ __forceinline__ void mask_raster_path(unsigned* bits, int* pin_x, int* pin_y, const int* path, int len,
                                                 const int* loc_x, const int* loc_y, int n_nodes, int map_x, int map_y, int tid) {
  for (int j0 = 0; j0 + 1 < len; j0 += THREADS - 1) {
    const int n = len - j0 < THREADS ? len - j0 : THREADS;
    __syncthreads();                                          // bitmap zeroed / the previous chunk's boxes read
    if (tid < n) {
      int a = path[j0 + tid];
      if constexpr (CLAMP) a = a < 0 ? 0 : (a >= n_nodes ? n_nodes - 1 : a);
      pin_x[tid] = loc_x[a];
      pin_y[tid] = loc_y[a];
    }
    __syncthreads();
    for (int j = 0; j + 1 < n; ++j) mask_or_box<THREADS>(bits, pin_x[j], pin_y[j], pin_x[j + 1], pin_y[j + 1], map_x, map_y, tid);
  }
}

// mask_raster_path under a trial move: the nodes mv_node[0 .. n_mv) (LDS, distinct, written by the caller before the call:
// the first barrier below orders those writes) take the coordinates (mv_x[m], mv_y[m]) at EVERY occurrence in the path, every
// other node its own from loc_x / loc_y, which are not written.  The override is applied where a node's coordinates are
// staged, so the boxes go through the same mask_or_box in the same order: with n_mv == 0, or with no moved node on the path,
// the bitmap is mask_raster_path's.
template <int THREADS>
__device__ __forceinline__ void mask_raster_path_moved(unsigned* bits, int* pin_x, int* pin_y, const int* path, int len,
                                                       const int* loc_x, const int* loc_y, const int* mv_node, const int* mv_x,
                                                       const int* mv_y, int n_mv, int map_x, int map_y, int tid) {
  for (int j0 = 0; j0 + 1 < len; j0 += THREADS - 1) {
    const int n = len - j0 < THREADS ? len - j0 : THREADS;
    __syncthreads();                                          // bitmap zeroed, overrides staged / the previous chunk's boxes read
    if (tid < n) {
      const int a = path[j0 + tid];
      int x = loc_x[a], y = loc_y[a];
      for (int m = 0; m < n_mv; ++m) {
        if (mv_node[m] == a) {
          x = mv_x[m];
          y = mv_y[m];
        }
      }
      pin_x[tid] = x;
      pin_y[tid] = y;
    }
    __syncthreads();
    for (int j = 0; j + 1 < n; ++j) mask_or_box<THREADS>(bits, pin_x[j], pin_y[j], pin_x[j + 1], pin_y[j + 1], map_x, map_y, tid);
  }
}

}  // namespace mmft
