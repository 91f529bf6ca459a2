// Exact search and commit of cell swaps (include/mmft_swap.h).
//
// swap_rows_kernel: one workgroup per entry.  The overrides of both groups of the entry's pair are formed from the resident
// pins and the difference of the two anchors - in 64 bits, saturated to int32 once, by THE MOVE RULE (move_rule.h) -, staged
// in LDS where search_rows_kernel stages a group's, and the row is written by trial_row_write (trial_row.h), the function
// trial_rows_kernel and search_rows_kernel call: the same bits, and the tables are never written.
// swap_score_kernel: one wave per pair walks the pair's entries with the accumulation of search_score_kernel
// (search_score.h) and writes the six figures and `pick`.  The base figures are search.hip's (search_base_launch).
// swap_apply_kernel: one wave per selected pair writes both groups' pins at their swapped coordinates, by the same rule.
#include "common.h"
#include "search_score.h"
#include "trial_row.h"
#include "../../include/mmft_swap.h"

namespace mmft {

struct SwapRowsArgs {
  TrialRowArgs row;
  const int* prow_row;
  const int* prow_pair;
  const int* pair_a;
  const int* pair_b;
  const int* mv_ptr;
  const int* mv_node;
  int K, G, e0;
};

__global__ void __launch_bounds__(256) swap_rows_kernel(SwapRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char swap_smem[];
  const int P = a.row.map_x * a.row.map_y;
  const PlaceLds L = place_lds(swap_smem, P >> 6);
  const TrialMoves mv = trial_moves_lds(L, P);
  const int slot = blockIdx.x, tid = threadIdx.x;
  const int e = a.e0 + slot;
  const int t = a.prow_row[e], k = a.prow_pair[e];
  int n_a = 0, n_b = 0, m_a = 0, m_b = 0;                 // the same for every thread
  if ((unsigned)k < (unsigned)a.K) {
    const int ga = a.pair_a[k], gb = a.pair_b[k];
    if ((unsigned)ga < (unsigned)a.G && (unsigned)gb < (unsigned)a.G) {
      m_a = a.mv_ptr[ga];
      m_b = a.mv_ptr[gb];
      n_a = a.mv_ptr[ga + 1] - m_a;
      n_b = a.mv_ptr[gb + 1] - m_b;
    }
  }
  if (n_a <= 0 || n_b <= 0) n_a = n_b = 0;                // no anchor: nothing moves
  n_a = n_a > TRIAL_MOVES ? TRIAL_MOVES : n_a;            // group a's pins first, then b's, TRIAL_MOVES in all
  n_b = n_b > TRIAL_MOVES - n_a ? TRIAL_MOVES - n_a : n_b;
  const int n_mv = n_a + n_b;
  // both groups in one pass, not two calls of trial_stage_group: a thread's pin id is fetched while the anchors' dependent
  // loads are under way; behind them (the two-call form) the launches of swap_moves measured 1 - 2 % longer
  if (tid < n_mv) {
    const int A = a.mv_node[m_a], B = a.mv_node[m_b];
    const long long dx = (long long)a.row.loc_x[B] - a.row.loc_x[A], dy = (long long)a.row.loc_y[B] - a.row.loc_y[A];
    const bool first = tid < n_a;
    const int node = first ? a.mv_node[m_a + tid] : a.mv_node[m_b + tid - n_a];
    mv.node[tid] = node;
    mv.x[tid] = moved(a.row.loc_x[node], first ? dx : -dx);
    mv.y[tid] = moved(a.row.loc_y[node], first ? dy : -dy);
  }
  trial_row_write(a.row, L, mv, n_mv, t, slot, tid);
}

__global__ void __launch_bounds__(256) swap_score_kernel(const float* __restrict__ pred_trial, const float* __restrict__ pred_base,
                                                         const float* __restrict__ required, int T,
                                                         const int* __restrict__ prow_ptr, const int* __restrict__ prow_row, int RP,
                                                         int k0, int k1, int scale_log2, long long* __restrict__ dq,
                                                         int* __restrict__ dviol, int* __restrict__ new_nan, int* __restrict__ capped,
                                                         float* __restrict__ worst, int* __restrict__ worst_row, int* __restrict__ pick) {
  const int lane = threadIdx.x & 63;
  const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);      // the same for the lanes of a wave
  if (item >= (long long)k1 - k0) return;
  const int k = k0 + (int)item;
  const int first = clamp_to(prow_ptr[k0], RP);         // where the call's predictions start
  const int e0 = clamp_to(prow_ptr[k], RP), e1 = clamp_to(prow_ptr[k + 1], RP);
  SearchAcc acc;
  for (int e = e0 + lane; e < e1; e += 64)
    if (e >= first) search_acc_entry(acc, prow_row[e], T, required, pred_base, pred_trial + (e - first), scale_log2);
  search_acc_wave(acc);
  if (lane == 0) {
    search_acc_store(acc, k, dq, dviol, new_nan, capped, worst, worst_row);
    pick[k] = acc.nans == 0 ? 0 : -1;
  }
}

__global__ void __launch_bounds__(256) swap_apply_kernel(int* loc_x, int* loc_y, int n_nodes, const int* __restrict__ sel,
                                                         const int* __restrict__ pick, const int* __restrict__ pair_a,
                                                         const int* __restrict__ pair_b, int K, const int* __restrict__ mv_ptr,
                                                         const int* __restrict__ mv_node, int G, int M) {
  const int lane = threadIdx.x & 63;
  const long long k = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);          // the same for the lanes of a wave
  if (k >= K || sel[k] == 0 || pick[k] != 0) return;
  const int ga = pair_a[k], gb = pair_b[k];
  if ((unsigned)ga >= (unsigned)G || (unsigned)gb >= (unsigned)G || ga == gb) return;
  const int a0 = clamp_to(mv_ptr[ga], M), a1 = clamp_to(mv_ptr[ga + 1], M);
  const int b0 = clamp_to(mv_ptr[gb], M), b1 = clamp_to(mv_ptr[gb + 1], M);
  if (a1 <= a0 || b1 <= b0) return;
  const int A = mv_node[a0], B = mv_node[b0];
  if ((unsigned)A >= (unsigned)n_nodes || (unsigned)B >= (unsigned)n_nodes) return;
  // THE ORDER of the anchors' reads and the pins' writes: every lane of this wave - the only writer of the pair's pins -
  // reads both anchors here, and every value a lane stores below is a sum with dx or dy.  A store therefore cannot issue
  // before the four loads have returned to its wave (the wait for them is wave-wide), and the loop below reads no anchor
  // again: only each lane's own pin.
  const long long dx = (long long)loc_x[B] - loc_x[A], dy = (long long)loc_y[B] - loc_y[A];
  const int n_a = a1 - a0, n_mv = n_a + (b1 - b0);
  for (int m = lane; m < n_mv; m += 64) {
    const bool first = m < n_a;
    const int n = first ? mv_node[a0 + m] : mv_node[b0 + m - n_a];
    if ((unsigned)n >= (unsigned)n_nodes) continue;
    loc_x[n] = moved(loc_x[n], first ? dx : -dx);
    loc_y[n] = moved(loc_y[n], first ? dy : -dy);
  }
}

}  // namespace mmft

using namespace mmft;

extern "C" {

int mmft_swap_rows(const int* path_nodes, const int* path_lens, int maxlen, const int* loc_x, const int* loc_y, int map_x, int map_y,
                   const int* paths, const int* f_off, int T, const int* prow_row, const int* prow_pair, int RP, const int* pair_a,
                   const int* pair_b, int K, const int* mv_ptr, const int* mv_node, int G, int e0, int e1, const float* GP,
                   const float* bias, const float* x, long long ldx, float* xt, long long ldxt, int width, int cnn_col, int Dout, int S,
                   int device, void* stream) {
  const TrialRowCall c = {"swap_rows", path_nodes, path_lens, maxlen, loc_x, loc_y, map_x, map_y, paths, f_off, GP, bias,
                          x, ldx, xt, ldxt, width, cnn_col, Dout, S, device, stream};
  int rc = trial_row_check(c, T >= 1 && G >= 1 && K >= 1 && RP >= 0, "T >= 1, G >= 1, K >= 1, RP >= 0");
  if (rc) return rc;
  MMFT_REQUIRE(e0 >= 0 && e0 <= e1 && e1 <= RP, "swap_rows: need 0 <= e0 <= e1 <= RP = %d (got %d, %d)", RP, e0, e1);
  if (e0 == e1) return MMFT_OK;
  SwapRowsArgs a;
  a.prow_row = prow_row; a.prow_pair = prow_pair; a.pair_a = pair_a; a.pair_b = pair_b; a.mv_ptr = mv_ptr; a.mv_node = mv_node;
  a.K = K; a.G = G; a.e0 = e0;
  return trial_row_launch<SwapRowsArgs, swap_rows_kernel>(c, "swap_rows_kernel", a, (unsigned)(e1 - e0),
                                                          prow_row && prow_pair && pair_a && pair_b && mv_ptr && mv_node);
}

int mmft_swap_score(const float* pred_trial, const float* pred_base, const float* required, int T, const int* prow_ptr,
                    const int* prow_row, int K, int RP, int k0, int k1, int scale_log2, long long* dq, int* dviol, int* new_nan,
                    int* capped, float* worst, int* worst_row, int* pick, long long* base, const int* design_rows, int n, int device,
                    void* stream) {
  MMFT_REQUIRE(T >= 1 && T <= (1 << 24) && K >= 1 && RP >= 0, "swap_score: need 1 <= T <= 2^24, K >= 1, 0 <= RP < 2^31 (got T %d, K %d, RP %d)",
               T, K, RP);
  MMFT_REQUIRE(k0 >= 0 && k0 < k1 && k1 <= K, "swap_score: need 0 <= k0 < k1 <= K = %d (got %d, %d)", K, k0, k1);
  MMFT_REQUIRE(scale_log2 >= 0 && scale_log2 <= 30, "swap_score: scale_log2 must lie in [0, 30] (got %d)", scale_log2);
  MMFT_REQUIRE(pred_base && required && prow_ptr && dq && dviol && new_nan && capped && worst && worst_row && pick &&
                   ((prow_row && pred_trial) || RP == 0),
               "swap_score: null pointer");
  MMFT_REQUIRE(aligned8(dq), "swap_score: dq must be 8-byte aligned");
  if (base) {
    MMFT_REQUIRE(n >= 1 && n <= (1 << 24) && design_rows, "swap_score: the base figures need design_rows [n], 1 <= n <= 2^24 (got n %d)", n);
    MMFT_REQUIRE(aligned8(base), "swap_score: base must be 8-byte aligned");
  }
  DeviceGuard dg(device);
  hipStream_t st = (hipStream_t)stream;
  const int items = k1 - k0;
  MMFT_LAUNCH("swap_score_kernel", 0.0, 32.0 * (double)items, swap_score_kernel, dim3((unsigned)(((long long)items + 3) / 4)), dim3(256), st,
              pred_trial, pred_base, required, T, prow_ptr, prow_row, RP, k0, k1, scale_log2, dq, dviol, new_nan, capped, worst, worst_row,
              pick);
  int rc = check_launch("swap_score");
  if (rc || !base) return rc;
  return search_base_launch("swap_score", "swap_base", pred_base, required, design_rows, n, T, scale_log2, base, st);
}

int mmft_swap_apply(int* loc_x, int* loc_y, int n_nodes, const int* sel, const int* pick, const int* pair_a, const int* pair_b, int K,
                    const int* mv_ptr, const int* mv_node, int G, int M, int device, void* stream) {
  MMFT_REQUIRE(n_nodes >= 1 && K >= 1 && G >= 1 && M >= 0, "swap_apply: need n_nodes >= 1, K >= 1, G >= 1, M >= 0 (got %d, %d, %d, %d)", n_nodes,
               K, G, M);
  MMFT_REQUIRE(loc_x && loc_y && sel && pick && pair_a && pair_b && mv_ptr && (mv_node || M == 0), "swap_apply: null pointer");
  if (M == 0) return MMFT_OK;
  DeviceGuard dg(device);
  MMFT_LAUNCH("swap_apply_kernel", 0.0, 0.0, swap_apply_kernel, dim3((unsigned)(((long long)K + 3) / 4)), dim3(256), (hipStream_t)stream,
              loc_x, loc_y, n_nodes, sel, pick, pair_a, pair_b, K, mv_ptr, mv_node, G, M);
  return check_launch("swap_apply");
}

}  // extern "C"
