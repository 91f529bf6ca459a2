// Exact search and commit of cell swaps (include/mmft_swap.h).
//
// swap_rows_kernel: one workgroup per entry.  The overrides of both groups of the entry's pair are formed from the resident
// pins and the two anchors - a 64-bit difference and sum saturated to int32 once -, staged in LDS where search_rows_kernel
// stages a group's, and the row is written by trial_row_write (trial_row.h), the function trial_rows_kernel and
// search_rows_kernel call: the same bits, and the tables are never written.
// swap_score_kernel: one wave per pair walks the pair's entries with the accumulation of search_score_kernel
// (search_score.h) and writes the six figures and `pick`.
// swap_base_kernel: the body of search_base_kernel (search_score.h).
// swap_apply_kernel: one wave per selected pair writes both groups' pins at their swapped coordinates, saturating.
#include "common.h"
#include "search_score.h"
#include "trial_row.h"
#include "../../include/mmft_swap.h"

namespace mmft {

// a resident coordinate moved by d, d a difference of two resident coordinates: the sum in 64 bits (|c + d| < 2^33),
// saturated to int32
__device__ __forceinline__ int swap_moved(int c, long long d) {
  const long long v = (long long)c + d;
  return v > 2147483647ll ? 2147483647 : (v < -2147483648ll ? (int)-2147483648ll : (int)v);
}

__device__ __forceinline__ int swap_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

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
  if (tid < n_mv) {
    const int A = a.mv_node[m_a], B = a.mv_node[m_b];
    const long long dx = (long long)a.row.loc_x[B] - a.row.loc_x[A], dy = (long long)a.row.loc_y[B] - a.row.loc_y[A];
    const bool first = tid < n_a;
    const int node = first ? a.mv_node[m_a + tid] : a.mv_node[m_b + tid - n_a];
    mv.node[tid] = node;
    mv.x[tid] = swap_moved(a.row.loc_x[node], first ? dx : -dx);
    mv.y[tid] = swap_moved(a.row.loc_y[node], first ? dy : -dy);
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
  const int first = swap_clamp(prow_ptr[k0], RP);         // where the call's predictions start
  const int e0 = swap_clamp(prow_ptr[k], RP), e1 = swap_clamp(prow_ptr[k + 1], RP);
  SearchAcc acc;
  for (int e = e0 + lane; e < e1; e += 64)
    if (e >= first) search_acc_entry(acc, prow_row[e], T, required, pred_base, pred_trial + (e - first), scale_log2);
  search_acc_wave(acc);
  if (lane == 0) {
    search_acc_store(acc, k, dq, dviol, new_nan, capped, worst, worst_row);
    pick[k] = acc.nans == 0 ? 0 : -1;
  }
}

__global__ void __launch_bounds__(256) swap_base_kernel(const float* __restrict__ pred_base, const float* __restrict__ required,
                                                        const int* __restrict__ design_rows, int n, int T, int scale_log2,
                                                        search_u64* __restrict__ base) {
  search_base_rows(pred_base, required, design_rows, n, T, scale_log2, base);
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
  const int a0 = swap_clamp(mv_ptr[ga], M), a1 = swap_clamp(mv_ptr[ga + 1], M);
  const int b0 = swap_clamp(mv_ptr[gb], M), b1 = swap_clamp(mv_ptr[gb + 1], M);
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
    loc_x[n] = swap_moved(loc_x[n], first ? dx : -dx);
    loc_y[n] = swap_moved(loc_y[n], first ? dy : -dy);
  }
}

static bool swap_aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace mmft

using namespace mmft;

extern "C" {

int mmft_swap_rows(const int* path_nodes, const int* path_lens, int maxlen, const int* loc_x, const int* loc_y, int map_x, int map_y,
                   const int* paths, const int* f_off, int T, const int* prow_row, const int* prow_pair, int RP, const int* pair_a,
                   const int* pair_b, int K, const int* mv_ptr, const int* mv_node, int G, int e0, int e1, const float* GP,
                   const float* bias, const float* x, long long ldx, float* xt, long long ldxt, int width, int cnn_col, int Dout, int S,
                   int device, void* stream) {
  MMFT_REQUIRE(S == 64, "swap_rows: the prefix block must be 64 cells (one bitmap word per block)");
  MMFT_REQUIRE(mask_map_ok(map_x, map_y), "swap_rows: the map must hold a multiple of 64 cells, at most 65536");
  MMFT_REQUIRE(Dout >= 4 && Dout % 4 == 0 && Dout <= 1024 && maxlen >= 1 && T >= 1 && G >= 1 && K >= 1 && RP >= 0,
               "swap_rows: bad sizes (Dout a multiple of 4 in [4, 1024], maxlen >= 1, T >= 1, G >= 1, K >= 1, RP >= 0)");
  MMFT_REQUIRE(cnn_col >= 0 && cnn_col % 4 == 0 && ldx % 4 == 0 && ldxt % 4 == 0 && (long long)cnn_col + Dout <= width &&
                   width <= ldx && width <= ldxt,
               "swap_rows: bad columns (cnn_col, ldx, ldxt multiples of 4, 0 <= cnn_col, cnn_col + Dout <= width <= ldx, ldxt)");
  MMFT_REQUIRE(e0 >= 0 && e0 <= e1 && e1 <= RP, "swap_rows: need 0 <= e0 <= e1 <= RP = %d (got %d, %d)", RP, e0, e1);
  if (e0 == e1) return MMFT_OK;
  MMFT_REQUIRE(path_nodes && path_lens && loc_x && loc_y && paths && prow_row && prow_pair && pair_a && pair_b && mv_ptr && mv_node &&
                   GP && x && xt,
               "swap_rows: null pointer");
  MMFT_REQUIRE(aligned16(GP) && aligned16(x) && aligned16(xt) && (!bias || aligned16(bias)), "swap_rows: 16-byte alignment");
  DeviceGuard dg(device);
  const int P = map_x * map_y;
  static DynLdsOnce once;
  int arc = ensure_dyn_lds(once, (const void*)swap_rows_kernel, (int)trial_lds_bytes(MASK_MAX_CELLS), "swap_rows");
  if (arc) return arc;
  SwapRowsArgs a;
  TrialRowArgs& r = a.row;
  r.path_nodes = path_nodes; r.path_lens = path_lens; r.loc_x = loc_x; r.loc_y = loc_y; r.paths = paths; r.foff = f_off;
  r.GP = GP; r.bias = bias; r.x = x; r.xt = xt; r.ldx = ldx; r.ldxt = ldxt;
  r.maxlen = maxlen; r.map_x = map_x; r.map_y = map_y; r.width = width; r.cnn_col = cnn_col; r.Dout = Dout;
  a.prow_row = prow_row; a.prow_pair = prow_pair; a.pair_a = pair_a; a.pair_b = pair_b; a.mv_ptr = mv_ptr; a.mv_node = mv_node;
  a.K = K; a.G = G; a.e0 = e0;
  MMFT_LAUNCH_LDS("swap_rows_kernel", 0.0, 0.0, swap_rows_kernel, dim3((unsigned)(e1 - e0)), dim3(256), trial_lds_bytes(P),
                  (hipStream_t)stream, a);
  return check_launch("swap_rows");
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
  MMFT_REQUIRE(swap_aligned8(dq), "swap_score: dq must be 8-byte aligned");
  if (base) {
    MMFT_REQUIRE(n >= 1 && n <= (1 << 24) && design_rows, "swap_score: the base figures need design_rows [n], 1 <= n <= 2^24 (got n %d)", n);
    MMFT_REQUIRE(swap_aligned8(base), "swap_score: base must be 8-byte aligned");
  }
  DeviceGuard dg(device);
  hipStream_t st = (hipStream_t)stream;
  const int items = k1 - k0;
  MMFT_LAUNCH("swap_score_kernel", 0.0, 32.0 * (double)items, swap_score_kernel, dim3((unsigned)(((long long)items + 3) / 4)), dim3(256), st,
              pred_trial, pred_base, required, T, prow_ptr, prow_row, RP, k0, k1, scale_log2, dq, dviol, new_nan, capped, worst, worst_row,
              pick);
  int rc = check_launch("swap_score");
  if (rc || !base) return rc;
  hipError_t e = hipMemsetAsync(base, 0, 3 * sizeof(long long), st);
  if (e != hipSuccess) {
    set_error("swap_score: clearing the base figures failed: %s", hipGetErrorString(e));
    return MMFT_ERR_LAUNCH;
  }
  int grid = cdiv(n, 256);
  grid = grid > 256 ? 256 : grid;
  MMFT_LAUNCH("swap_base_kernel", 0.0, 12.0 * n, swap_base_kernel, dim3(grid), dim3(256), st, pred_base, required, design_rows, n, T,
              scale_log2, reinterpret_cast<search_u64*>(base));
  return check_launch("swap_base");
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
