// Exact window search of pin-group moves (include/mmft_search.h).
//
// search_rows_kernel: one workgroup per slot (entry e, offset w).  The group's overrides are formed from the resident pins
// and the offset by trial_stage_group (trial_row.h: THE MOVE RULE and THE WINDOW of move_rule.h), staged in LDS where
// trial_rows_kernel stages a candidate's, and the row is written by trial_row_write, the function that kernel calls: the same
// bits, and the tables are never written.
// search_score_kernel: one wave per (group, offset) walks the group's entries and reduces the change of the quanta, of the
// violations, the new NaN rows, the capped rows and the worst (slack, row) key in integers (search_score.h, shared with swap.hip).
// search_best_kernel: one wave per group takes the smallest (dq, |dx| + |dy|, w) key among the eligible offsets.
// search_base_kernel: the design's own sum of quanta, violations and NaN rows, by integer atomics; search_base_launch clears
// the three figures and launches it, for mmft_search_best and for mmft_swap_score (swap.hip).
#include "common.h"
#include "search_score.h"
#include "trial_row.h"
#include "../../include/mmft_search.h"

namespace mmft {

struct SearchRowsArgs {
  TrialRowArgs row;
  const int* grow_row;
  const int* grow_grp;
  const int* mv_ptr;
  const int* mv_node;
  int R, radius, w0;
};

__global__ void __launch_bounds__(256) search_rows_kernel(SearchRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char search_smem[];
  const int P = a.row.map_x * a.row.map_y;
  const PlaceLds L = place_lds(search_smem, P >> 6);
  const TrialMoves mv = trial_moves_lds(L, P);
  const int slot = blockIdx.x, tid = threadIdx.x;
  const int e = slot % a.R, w = a.w0 + slot / a.R;
  int dx, dy;
  window_offset(w, a.radius, dx, dy);
  const int t = a.grow_row[e], g = a.grow_grp[e];
  const int n_mv = trial_stage_group(a.row, mv, a.mv_ptr, a.mv_node, g, dx, dy, tid);
  trial_row_write(a.row, L, mv, n_mv, t, slot, tid);
}

__global__ void __launch_bounds__(256) search_score_kernel(const float* __restrict__ pred_trial, const float* __restrict__ pred_base,
                                                           const float* __restrict__ required, int T,
                                                           const int* __restrict__ grow_ptr, const int* __restrict__ grow_row, int G,
                                                           int R, int W, int w0, int Wc, int scale_log2, long long* __restrict__ dq,
                                                           int* __restrict__ dviol, int* __restrict__ new_nan, int* __restrict__ capped,
                                                           float* __restrict__ worst, int* __restrict__ worst_row) {
  const int lane = threadIdx.x & 63;
  const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);      // the same for the lanes of a wave
  if (item >= (long long)G * Wc) return;
  const int g = (int)(item / Wc), wc = (int)(item - (long long)g * Wc);
  const int e0 = grow_ptr[g], e1 = grow_ptr[g + 1];
  const float* trial = pred_trial + (long long)wc * R;
  SearchAcc acc;
  for (int e = e0 + lane; e < e1; e += 64) search_acc_entry(acc, grow_row[e], T, required, pred_base, trial + e, scale_log2);
  search_acc_wave(acc);
  if (lane == 0) search_acc_store(acc, (long long)g * W + w0 + wc, dq, dviol, new_nan, capped, worst, worst_row);
}

__global__ void __launch_bounds__(256) search_best_kernel(const long long* __restrict__ dq, const int* __restrict__ new_nan, int G,
                                                          int radius, int* __restrict__ best_w, long long* __restrict__ best_dq) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= G) return;
  const int W = window_cells(radius);
  long long bq = 0;
  int bm = 0, bw = -1;                                  // bw == -1: no eligible offset yet
  for (int w = lane; w < W; w += 64) {
    if (new_nan[(long long)g * W + w] != 0) continue;
    const long long q = dq[(long long)g * W + w];
    int dx, dy;
    window_offset(w, radius, dx, dy);
    const int m = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
    if (bw < 0 || q < bq || (q == bq && (m < bm || (m == bm && w < bw)))) {
      bq = q; bm = m; bw = w;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long q = __shfl_xor(bq, o, 64);
    const int m = __shfl_xor(bm, o, 64), w = __shfl_xor(bw, o, 64);
    if (w >= 0 && (bw < 0 || q < bq || (q == bq && (m < bm || (m == bm && w < bw))))) {
      bq = q; bm = m; bw = w;
    }
  }
  if (lane == 0) {
    best_w[g] = bw;
    best_dq[g] = bw < 0 ? 0ll : bq;
  }
}

// base [3] (cleared by search_base_launch) += the three figures; grid-strided over workgroups of 256 threads, a wave's figures
// added by integer atomics
__global__ void __launch_bounds__(256) search_base_kernel(const float* __restrict__ pred_base, const float* __restrict__ required,
                                                          const int* __restrict__ design_rows, int n, int T, int scale_log2,
                                                          slack_u64* __restrict__ base) {
  slack_u64 sum = 0ull;
  int viol = 0, nans = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int r = design_rows[i];
    float s = __uint_as_float(0x7fc00000u);
    if ((unsigned)r < (unsigned)T) s = slack_of(required[r], pred_base[r]);
    if (s != s) {
      ++nans;
    } else if (s < 0.f) {
      bool cap;
      sum += crit_quanta(s, scale_log2, cap);
      ++viol;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    viol += __shfl_xor(viol, o, 64);
    nans += __shfl_xor(nans, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {                        // integer adds: the order of the waves does not show
    if (sum) atomicAdd(base, sum);
    if (viol) atomicAdd(base + 1, (slack_u64)viol);
    if (nans) atomicAdd(base + 2, (slack_u64)nans);
  }
}

int search_base_launch(const char* entry, const char* what, const float* pred_base, const float* required, const int* design_rows,
                       int n, int T, int scale_log2, long long* base, hipStream_t st) {
  hipError_t e = hipMemsetAsync(base, 0, 3 * sizeof(long long), st);
  if (e != hipSuccess) {
    set_error("%s: clearing the base figures failed: %s", entry, hipGetErrorString(e));
    return MMFT_ERR_LAUNCH;
  }
  int grid = cdiv(n, 256);
  grid = grid > 256 ? 256 : grid;
  MMFT_LAUNCH("search_base_kernel", 0.0, 12.0 * n, search_base_kernel, dim3(grid), dim3(256), st, pred_base, required, design_rows, n, T,
              scale_log2, reinterpret_cast<slack_u64*>(base));
  return check_launch(what);
}

}  // namespace mmft

using namespace mmft;

extern "C" {

int mmft_search_rows(const int* path_nodes, const int* path_lens, int maxlen, const int* loc_x, const int* loc_y, int map_x,
                     int map_y, const int* paths, const int* f_off, int T, const int* grow_row, const int* grow_grp, int R,
                     const int* mv_ptr, const int* mv_node, int G, int radius, int w0, int w1, const float* GP, const float* bias,
                     const float* x, long long ldx, float* xt, long long ldxt, int width, int cnn_col, int Dout, int S, int device,
                     void* stream) {
  const TrialRowCall c = {"search_rows", path_nodes, path_lens, maxlen, loc_x, loc_y, map_x, map_y, paths, f_off, GP, bias,
                          x, ldx, xt, ldxt, width, cnn_col, Dout, S, device, stream};
  int rc = trial_row_check(c, T >= 1 && G >= 1 && R >= 0, "T >= 1, G >= 1, R >= 0");
  if (rc) return rc;
  MMFT_REQUIRE(radius >= 1 && radius <= WINDOW_RADIUS_MAX, "search_rows: radius must lie in [1, %d] (got %d)", WINDOW_RADIUS_MAX, radius);
  const int W = window_cells(radius);
  MMFT_REQUIRE(w0 >= 0 && w0 <= w1 && w1 <= W, "search_rows: need 0 <= w0 <= w1 <= %d (got %d, %d)", W, w0, w1);
  MMFT_REQUIRE((long long)R * (w1 - w0) < (1ll << 31), "search_rows: R * (w1 - w0) must stay below 2^31 (got %d * %d)", R, w1 - w0);
  if (R == 0 || w0 == w1) return MMFT_OK;
  SearchRowsArgs a;
  a.grow_row = grow_row; a.grow_grp = grow_grp; a.mv_ptr = mv_ptr; a.mv_node = mv_node; a.R = R; a.radius = radius; a.w0 = w0;
  return trial_row_launch<SearchRowsArgs, search_rows_kernel>(c, "search_rows_kernel", a, (unsigned)(R * (w1 - w0)),
                                                              grow_row && grow_grp && mv_ptr && mv_node);
}

int mmft_search_score(const float* pred_trial, const float* pred_base, const float* required, int T, const int* grow_ptr,
                      const int* grow_row, int G, int R, int radius, int w0, int w1, int scale_log2, long long* dq, int* dviol,
                      int* new_nan, int* capped, float* worst, int* worst_row, int device, void* stream) {
  MMFT_REQUIRE(T >= 1 && T <= (1 << 24) && G >= 1 && R >= 0, "search_score: need 1 <= T <= 2^24, G >= 1, R >= 0 (got T %d, G %d, R %d)", T,
               G, R);
  MMFT_REQUIRE(radius >= 1 && radius <= WINDOW_RADIUS_MAX, "search_score: radius must lie in [1, %d] (got %d)", WINDOW_RADIUS_MAX, radius);
  const int W = window_cells(radius);
  MMFT_REQUIRE(w0 >= 0 && w0 < w1 && w1 <= W, "search_score: need 0 <= w0 < w1 <= %d (got %d, %d)", W, w0, w1);
  MMFT_REQUIRE((long long)R * (w1 - w0) < (1ll << 31), "search_score: R * (w1 - w0) must stay below 2^31 (got %d * %d)", R, w1 - w0);
  MMFT_REQUIRE(scale_log2 >= 0 && scale_log2 <= 30, "search_score: scale_log2 must lie in [0, 30] (got %d)", scale_log2);
  MMFT_REQUIRE(pred_base && required && grow_ptr && dq && dviol && new_nan && capped && worst && worst_row &&
                   ((grow_row && pred_trial) || R == 0),
               "search_score: null pointer");
  MMFT_REQUIRE(aligned8(dq), "search_score: dq must be 8-byte aligned");
  DeviceGuard dg(device);
  const int Wc = w1 - w0;
  const long long items = (long long)G * Wc;
  MMFT_REQUIRE(items <= (1ll << 32), "search_score: G * (w1 - w0) must not exceed 2^32");
  const double alg_bytes = 16.0 * (double)R * Wc + 28.0 * (double)items;
  MMFT_LAUNCH("search_score_kernel", 0.0, alg_bytes, search_score_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), (hipStream_t)stream,
              pred_trial, pred_base, required, T, grow_ptr, grow_row, G, R, W, w0, Wc, scale_log2, dq, dviol, new_nan, capped, worst,
              worst_row);
  return check_launch("search_score");
}

int mmft_search_best(const long long* dq, const int* new_nan, int G, int radius, int* best_w, long long* best_dq,
                     const float* pred_base, const float* required, const int* design_rows, int n, int T, int scale_log2,
                     long long* base, int device, void* stream) {
  MMFT_REQUIRE(G >= 1 && n >= 1 && n <= (1 << 24) && T >= 1 && T <= (1 << 24),
               "search_best: need G >= 1, 1 <= n <= 2^24, 1 <= T <= 2^24 (got G %d, n %d, T %d)", G, n, T);
  MMFT_REQUIRE(radius >= 1 && radius <= WINDOW_RADIUS_MAX, "search_best: radius must lie in [1, %d] (got %d)", WINDOW_RADIUS_MAX, radius);
  MMFT_REQUIRE(scale_log2 >= 0 && scale_log2 <= 30, "search_best: scale_log2 must lie in [0, 30] (got %d)", scale_log2);
  MMFT_REQUIRE(dq && new_nan && best_w && best_dq && pred_base && required && design_rows && base, "search_best: null pointer");
  MMFT_REQUIRE(aligned8(dq) && aligned8(best_dq) && aligned8(base), "search_best: dq, best_dq and base must be 8-byte aligned");
  DeviceGuard dg(device);
  hipStream_t st = (hipStream_t)stream;
  MMFT_LAUNCH("search_best_kernel", 0.0, 0.0, search_best_kernel, dim3((unsigned)((G + 3) / 4)), dim3(256), st, dq, new_nan, G, radius,
              best_w, best_dq);
  int rc = check_launch("search_best");
  if (rc) return rc;
  return search_base_launch("search_best", "search_base", pred_base, required, design_rows, n, T, scale_log2, base, st);
}

}  // extern "C"
