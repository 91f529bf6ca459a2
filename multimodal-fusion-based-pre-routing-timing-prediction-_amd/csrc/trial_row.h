// ONE head input row under a set of pin overrides (include/mmft_trial.h): the row's columns around h_cnn copied from the
// resident batch, its mask rasterised with the overrides (mask_raster_path_moved, mask_rule.h) and projected by place_project
// (place_project.h).  trial_rows_kernel (trial.hip) stages a candidate's overrides from the caller's tables,
// search_rows_kernel (search.hip) forms a group's from the resident pins and a window offset; both then call trial_row_write:
// the tests hold the two kernels to the same bits, and the code that makes those bits is here once.
#pragma once
#include "mask_rule.h"
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

}  // namespace mmft
