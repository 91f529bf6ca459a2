// Exact window search of pin-group moves (include/mmft_search.h).
//
// search_rows_kernel: one workgroup per slot (entry e, offset w).  The group's overrides are formed from the resident pins
// and the offset - a 64-bit sum saturated to int32 -, staged in LDS where trial_rows_kernel stages a candidate's, and the row
// is written by trial_row_write (trial_row.h), the function that kernel calls: the same bits, and the tables are never written.
// search_score_kernel: one wave per (group, offset) walks the group's entries and reduces the change of the quanta, of the
// violations, the new NaN rows, the capped rows and the worst (slack, row) key in integers (search_score.h, shared with swap.hip).
// search_best_kernel: one wave per group takes the smallest (dq, |dx| + |dy|, w) key among the eligible offsets.
// search_base_kernel: the design's own sum of quanta, violations and NaN rows, by integer atomics (search_score.h).
#include "common.h"
#include "search_score.h"
#include "trial_row.h"
#include "../../include/mmft_search.h"

namespace mmft {

constexpr int SEARCH_MAX_RADIUS = 8;

__host__ __device__ inline int search_side(int radius) { return 2 * radius + 1; }

// a resident coordinate moved by d cells: the sum in 64 bits, saturated to int32
__device__ __forceinline__ int search_moved(int c, int d) {
  const long long v = (long long)c + d;
  return v > 2147483647ll ? 2147483647 : (v < -2147483648ll ? (int)-2147483648ll : (int)v);
}

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
  const int side = search_side(a.radius);
  const int dx = w / side - a.radius, dy = w % side - a.radius;
  const int t = a.grow_row[e], g = a.grow_grp[e];
  const int m0 = a.mv_ptr[g];
  int n_mv = a.mv_ptr[g + 1] - m0;                      // the same for every thread
  n_mv = n_mv < 0 ? 0 : (n_mv > TRIAL_MOVES ? TRIAL_MOVES : n_mv);
  if (tid < n_mv) {
    const int node = a.mv_node[m0 + tid];
    mv.node[tid] = node;
    mv.x[tid] = search_moved(a.row.loc_x[node], dx);
    mv.y[tid] = search_moved(a.row.loc_y[node], dy);
  }
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
  const int side = search_side(radius), W = side * side;
  long long bq = 0;
  int bm = 0, bw = -1;                                  // bw == -1: no eligible offset yet
  for (int w = lane; w < W; w += 64) {
    if (new_nan[(long long)g * W + w] != 0) continue;
    const long long q = dq[(long long)g * W + w];
    const int dx = w / side - radius, dy = w % side - radius;
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

__global__ void __launch_bounds__(256) search_base_kernel(const float* __restrict__ pred_base, const float* __restrict__ required,
                                                          const int* __restrict__ design_rows, int n, int T, int scale_log2,
                                                          search_u64* __restrict__ base) {
  search_base_rows(pred_base, required, design_rows, n, T, scale_log2, base);
}

static bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace mmft

using namespace mmft;

extern "C" {

int mmft_search_rows(const int* path_nodes, const int* path_lens, int maxlen, const int* loc_x, const int* loc_y, int map_x,
                     int map_y, const int* paths, const int* f_off, int T, const int* grow_row, const int* grow_grp, int R,
                     const int* mv_ptr, const int* mv_node, int G, int radius, int w0, int w1, const float* GP, const float* bias,
                     const float* x, long long ldx, float* xt, long long ldxt, int width, int cnn_col, int Dout, int S, int device,
                     void* stream) {
  MMFT_REQUIRE(S == 64, "search_rows: the prefix block must be 64 cells (one bitmap word per block)");
  MMFT_REQUIRE(mask_map_ok(map_x, map_y), "search_rows: the map must hold a multiple of 64 cells, at most 65536");
  MMFT_REQUIRE(Dout >= 4 && Dout % 4 == 0 && Dout <= 1024 && maxlen >= 1 && T >= 1 && G >= 1 && R >= 0,
               "search_rows: bad sizes (Dout a multiple of 4 in [4, 1024], maxlen >= 1, T >= 1, G >= 1, R >= 0)");
  MMFT_REQUIRE(cnn_col >= 0 && cnn_col % 4 == 0 && ldx % 4 == 0 && ldxt % 4 == 0 && (long long)cnn_col + Dout <= width &&
                   width <= ldx && width <= ldxt,
               "search_rows: bad columns (cnn_col, ldx, ldxt multiples of 4, 0 <= cnn_col, cnn_col + Dout <= width <= ldx, ldxt)");
  MMFT_REQUIRE(radius >= 1 && radius <= SEARCH_MAX_RADIUS, "search_rows: radius must lie in [1, %d] (got %d)", SEARCH_MAX_RADIUS, radius);
  const int W = search_side(radius) * search_side(radius);
  MMFT_REQUIRE(w0 >= 0 && w0 <= w1 && w1 <= W, "search_rows: need 0 <= w0 <= w1 <= %d (got %d, %d)", W, w0, w1);
  MMFT_REQUIRE((long long)R * (w1 - w0) < (1ll << 31), "search_rows: R * (w1 - w0) must stay below 2^31 (got %d * %d)", R, w1 - w0);
  if (R == 0 || w0 == w1) return MMFT_OK;
  MMFT_REQUIRE(path_nodes && path_lens && loc_x && loc_y && paths && grow_row && grow_grp && mv_ptr && mv_node && GP && x && xt,
               "search_rows: null pointer");
  MMFT_REQUIRE(aligned16(GP) && aligned16(x) && aligned16(xt) && (!bias || aligned16(bias)), "search_rows: 16-byte alignment");
  DeviceGuard dg(device);
  const int P = map_x * map_y;
  static DynLdsOnce once;
  int arc = ensure_dyn_lds(once, (const void*)search_rows_kernel, (int)trial_lds_bytes(MASK_MAX_CELLS), "search_rows");
  if (arc) return arc;
  SearchRowsArgs a;
  TrialRowArgs& r = a.row;
  r.path_nodes = path_nodes; r.path_lens = path_lens; r.loc_x = loc_x; r.loc_y = loc_y; r.paths = paths; r.foff = f_off;
  r.GP = GP; r.bias = bias; r.x = x; r.xt = xt; r.ldx = ldx; r.ldxt = ldxt;
  r.maxlen = maxlen; r.map_x = map_x; r.map_y = map_y; r.width = width; r.cnn_col = cnn_col; r.Dout = Dout;
  a.grow_row = grow_row; a.grow_grp = grow_grp; a.mv_ptr = mv_ptr; a.mv_node = mv_node; a.R = R; a.radius = radius; a.w0 = w0;
  MMFT_LAUNCH_LDS("search_rows_kernel", 0.0, 0.0, search_rows_kernel, dim3((unsigned)(R * (w1 - w0))), dim3(256), trial_lds_bytes(P),
                  (hipStream_t)stream, a);
  return check_launch("search_rows");
}

int mmft_search_score(const float* pred_trial, const float* pred_base, const float* required, int T, const int* grow_ptr,
                      const int* grow_row, int G, int R, int radius, int w0, int w1, int scale_log2, long long* dq, int* dviol,
                      int* new_nan, int* capped, float* worst, int* worst_row, int device, void* stream) {
  MMFT_REQUIRE(T >= 1 && T <= (1 << 24) && G >= 1 && R >= 0, "search_score: need 1 <= T <= 2^24, G >= 1, R >= 0 (got T %d, G %d, R %d)", T,
               G, R);
  MMFT_REQUIRE(radius >= 1 && radius <= SEARCH_MAX_RADIUS, "search_score: radius must lie in [1, %d] (got %d)", SEARCH_MAX_RADIUS, radius);
  const int W = search_side(radius) * search_side(radius);
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
  MMFT_REQUIRE(radius >= 1 && radius <= SEARCH_MAX_RADIUS, "search_best: radius must lie in [1, %d] (got %d)", SEARCH_MAX_RADIUS, radius);
  MMFT_REQUIRE(scale_log2 >= 0 && scale_log2 <= 30, "search_best: scale_log2 must lie in [0, 30] (got %d)", scale_log2);
  MMFT_REQUIRE(dq && new_nan && best_w && best_dq && pred_base && required && design_rows && base, "search_best: null pointer");
  MMFT_REQUIRE(aligned8(dq) && aligned8(best_dq) && aligned8(base), "search_best: dq, best_dq and base must be 8-byte aligned");
  DeviceGuard dg(device);
  hipStream_t st = (hipStream_t)stream;
  MMFT_LAUNCH("search_best_kernel", 0.0, 0.0, search_best_kernel, dim3((unsigned)((G + 3) / 4)), dim3(256), st, dq, new_nan, G, radius,
              best_w, best_dq);
  int rc = check_launch("search_best");
  if (rc) return rc;
  hipError_t e = hipMemsetAsync(base, 0, 3 * sizeof(long long), st);
  if (e != hipSuccess) {
    set_error("search_best: clearing the base figures failed: %s", hipGetErrorString(e));
    return MMFT_ERR_LAUNCH;
  }
  int grid = cdiv(n, 256);
  grid = grid > 256 ? 256 : grid;
  MMFT_LAUNCH("search_base_kernel", 0.0, 12.0 * n, search_base_kernel, dim3(grid), dim3(256), st, pred_base, required, design_rows, n, T,
              scale_log2, reinterpret_cast<search_u64*>(base));
  return check_launch("search_base");
}

}  // extern "C"
