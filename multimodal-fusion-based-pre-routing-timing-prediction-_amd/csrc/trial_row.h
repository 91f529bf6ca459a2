// ONE head input row under a set of pin overrides (include/mmft_trial.h): the row's columns around h_cnn copied from the
// resident batch, its mask rasterised with the overrides (mask_raster_path_moved, mask_rule.h) and projected by place_project
// (place_project.h).  The four rows kernels differ in where the overrides come from: trial_rows_kernel (trial.hip) stages a
// candidate's from the caller's tables; search_rows_kernel (search.hip) and refine_rows_kernel (refine.hip) form a group's
// from the resident pins and a window offset by trial_stage_group; swap_rows_kernel (swap.hip) forms two groups' from the
// resident pins and the difference of their anchors, in one pass of its own.  All then call trial_row_write,
// and their entry points refuse and launch through trial_row_check and trial_row_launch: the tests hold the kernels to the
// same bits and the entry points to the same refusals, and the code that makes both is here once.
#pragma once
#include "common.h"
#include "mask_rule.h"
#include "move_rule.h"
#include "place_project.h"

namespace mmft {

constexpr int TRIAL_MOVES = 64;              // overrides of one row, staged behind the bitmap: [3][TRIAL_MOVES] int
inline size_t trial_lds_bytes(int P) { return place_lds_bytes(P) + 3 * TRIAL_MOVES * 4; }

struct TrialRowArgs {
  const int* path_nodes;
  const int* path_lens;
  const int* loc_x;
  const int* loc_y;
  const int* paths;
  const int* foff;
  const float* GP;
  const float* bias;
  const float* x;
  float* xt;
  long long ldx, ldxt;
  int maxlen, map_x, map_y, width, cnn_col, Dout;
};

// where the overrides of a row live in LDS: mv_node, mv_x, mv_y [TRIAL_MOVES] each, behind the bitmap of P cells
struct TrialMoves {
  int* node;
  int* x;
  int* y;
};
__device__ inline TrialMoves trial_moves_lds(const PlaceLds& L, int P) {
  TrialMoves m;
  m.node = reinterpret_cast<int*>(L.bits + (P >> 5));
  m.x = m.node + TRIAL_MOVES;
  m.y = m.x + TRIAL_MOVES;
  return m;
}

// THE STAGING of a group: the pins mv_node[mv_ptr[g] .. mv_ptr[g + 1]) moved by (dx, dy) from where the resident tables have
// them (THE MOVE RULE, move_rule.h), written to the override slots [0, n); n, the group's pins held to TRIAL_MOVES, is
// returned.  Called by all 256 threads; g and n are the same for every thread.
__device__ __forceinline__ int trial_stage_group(const TrialRowArgs& a, const TrialMoves& mv, const int* mv_ptr, const int* mv_node,
                                                 int g, int dx, int dy, int tid) {
  const int m0 = mv_ptr[g];
  const int n = clamp_to(mv_ptr[g + 1] - m0, TRIAL_MOVES);
  if (tid < n) {
    const int node = mv_node[m0 + tid];
    mv.node[tid] = node;
    mv.x[tid] = moved(a.loc_x[node], dx);
    mv.y[tid] = moved(a.loc_y[node], dy);
  }
  return n;
}

// xt[p][0 .. width) from row t of x under the n_mv overrides in `mv` (written by the caller before the call, no barrier
// needed in between: the raster's first barrier orders them).  Called by all 256 threads; n_mv is the same for every thread.
__device__ __forceinline__ void trial_row_write(const TrialRowArgs& a, const PlaceLds& L, const TrialMoves& mv, int n_mv, int t,
                                                long long p, int tid) {
  const int P = a.map_x * a.map_y, words = P >> 5, nblk = P >> 6;
  for (int w = tid; w < words; w += 256) L.bits[w] = 0u;
  // ---- the columns around h_cnn: the row as the resident batch has it
  {
    const float* src = a.x + (long long)t * a.ldx;
    float* dst = a.xt + p * a.ldxt;
    const int rest = a.width - a.Dout;                  // columns [0, cnn_col) and [cnn_col + Dout, width)
    for (int c = tid; c < rest; c += 256) {
      const int col = c < a.cnn_col ? c : c + a.Dout;
      dst[col] = src[col];
    }
  }
  // ---- the union of boxes under the overrides: THE MASK RULE, staged, with the overrides applied at the staging
  const int q = a.paths[t];
  const int* path = a.path_nodes + (long long)q * a.maxlen;
  const int len = a.path_lens[q] < a.maxlen ? a.path_lens[q] : a.maxlen;
  mask_raster_path_moved<256>(L.bits, L.pin_x, L.pin_y, path, len, a.loc_x, a.loc_y, mv.node, mv.x, mv.y, n_mv, a.map_x, a.map_y, tid);
  __syncthreads();
  // ---- the runs numbered and accumulated through the prefix table (place_project.h)
  place_project(L, nblk, a.GP + (long long)(a.foff ? a.foff[t] : 0) * a.Dout, a.bias, a.xt + p * a.ldxt + a.cnn_col, a.Dout, nullptr, tid);
}

// THE LAUNCHER of a rows kernel.  What every rows entry point is called with, in the order of its signature; `entry` starts
// every message.
struct TrialRowCall {
  const char* entry;
  const int* path_nodes;
  const int* path_lens;
  int maxlen;
  const int* loc_x;
  const int* loc_y;
  int map_x, map_y;
  const int* paths;
  const int* f_off;
  const float* GP;
  const float* bias;
  const float* x;
  long long ldx;
  float* xt;
  long long ldxt;
  int width, cnn_col, Dout, S, device;
  void* stream;
};

// the first refusals: the block, the map, the sizes - own_sizes_ok and own_sizes are the entry point's own, as a condition and
// as the words of the message - and the columns.  No pointer is looked at: an empty call returns between this and the launch.
inline int trial_row_check(const TrialRowCall& c, bool own_sizes_ok, const char* own_sizes) {
  MMFT_REQUIRE(c.S == 64, "%s: the prefix block must be 64 cells (one bitmap word per block)", c.entry);
  MMFT_REQUIRE(mask_map_ok(c.map_x, c.map_y), "%s: the map must hold a multiple of 64 cells, at most 65536", c.entry);
  MMFT_REQUIRE(c.Dout >= 4 && c.Dout % 4 == 0 && c.Dout <= 1024 && c.maxlen >= 1 && own_sizes_ok,
               "%s: bad sizes (Dout a multiple of 4 in [4, 1024], maxlen >= 1, %s)", c.entry, own_sizes);
  MMFT_REQUIRE(c.cnn_col >= 0 && c.cnn_col % 4 == 0 && c.ldx % 4 == 0 && c.ldxt % 4 == 0 && (long long)c.cnn_col + c.Dout <= c.width &&
                   c.width <= c.ldx && c.width <= c.ldxt,
               "%s: bad columns (cnn_col, ldx, ldxt multiples of 4, 0 <= cnn_col, cnn_col + Dout <= width <= ldx, ldxt)", c.entry);
  return MMFT_OK;
}

// the last refusals and the launch of Kernel(a) on `grid` workgroups: own_pointers_ok says that none of the kernel's own
// pointers is null; a.row is filled here, the kernel's own fields by the caller.  One DynLdsOnce per kernel.
template <typename Args, void (*Kernel)(Args)>
inline int trial_row_launch(const TrialRowCall& c, const char* kernel_name, Args& a, unsigned grid, bool own_pointers_ok) {
  MMFT_REQUIRE(c.path_nodes && c.path_lens && c.loc_x && c.loc_y && c.paths && c.GP && c.x && c.xt && own_pointers_ok,
               "%s: null pointer", c.entry);
  MMFT_REQUIRE(aligned16(c.GP) && aligned16(c.x) && aligned16(c.xt) && (!c.bias || aligned16(c.bias)), "%s: 16-byte alignment", c.entry);
  DeviceGuard dg(c.device);
  static DynLdsOnce once;
  int arc = ensure_dyn_lds(once, (const void*)Kernel, (int)trial_lds_bytes(MASK_MAX_CELLS), c.entry);
  if (arc) return arc;
  TrialRowArgs& r = a.row;
  r.path_nodes = c.path_nodes; r.path_lens = c.path_lens; r.loc_x = c.loc_x; r.loc_y = c.loc_y; r.paths = c.paths; r.foff = c.f_off;
  r.GP = c.GP; r.bias = c.bias; r.x = c.x; r.xt = c.xt; r.ldx = c.ldx; r.ldxt = c.ldxt;
  r.maxlen = c.maxlen; r.map_x = c.map_x; r.map_y = c.map_y; r.width = c.width; r.cnn_col = c.cnn_col; r.Dout = c.Dout;
  MMFT_LAUNCH_LDS(kernel_name, 0.0, 0.0, Kernel, dim3(grid), dim3(256), trial_lds_bytes(c.map_x * c.map_y), (hipStream_t)c.stream, a);
  return check_launch(c.entry);
}

}  // namespace mmft
