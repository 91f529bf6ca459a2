// Exact predictions for a batch of trial pin moves (include/mmft_trial.h).
//
// trial_rows_kernel: one workgroup per (row, candidate) pair.  The candidate's overrides are staged in LDS, the row's mask is
// rasterised with them (mask_raster_path_moved, mask_rule.h: the boxes of mask_raster_path, on the same mask_or_box) and
// projected by place_project (place_project.h), the function placed_fc_fwd_kernel calls - the h_cnn columns are that kernel's
// bits on moved tables, and the tables are never written.  The row's other columns are copied.  Everything after the staging
// is trial_row_write (trial_row.h), which search.hip calls too.
// trial_reduce_kernel: one workgroup per candidate walks the design's rows, takes the trial prediction where the candidate has
// a pair and the resident one elsewhere, and reduces counts, the worst (slack, row) key and the fp64 negative sum in one fixed
// tree.
#include "common.h"
#include "slack_key.h"
#include "trial_row.h"
#include "../../include/mmft_trial.h"

namespace mmft {

struct TrialRowsArgs {
  TrialRowArgs row;
  const int* pair_row;
  const int* pair_cand;
  const int* mv_ptr;
  const int* mv_node;
  const int* mv_x;
  const int* mv_y;
};

__global__ void __launch_bounds__(256) trial_rows_kernel(TrialRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char trial_smem[];
  const int P = a.row.map_x * a.row.map_y;
  const PlaceLds L = place_lds(trial_smem, P >> 6);
  const TrialMoves mv = trial_moves_lds(L, P);
  const int p = blockIdx.x, tid = threadIdx.x;
  const int t = a.pair_row[p], k = a.pair_cand[p];
  const int m0 = a.mv_ptr[k];
  int n_mv = a.mv_ptr[k + 1] - m0;                      // the same for every thread
  n_mv = n_mv < 0 ? 0 : (n_mv > TRIAL_MOVES ? TRIAL_MOVES : n_mv);
  if (tid < n_mv) {
    mv.node[tid] = a.mv_node[m0 + tid];
    mv.x[tid] = a.mv_x[m0 + tid];
    mv.y[tid] = a.mv_y[m0 + tid];
  }
  trial_row_write(a.row, L, mv, n_mv, t, p, tid);       // trial_row.h: the copy, the raster under the overrides, the projection
}

typedef unsigned long long trial_u64;
constexpr trial_u64 TRIAL_KEY_NONE = ~0ull;   // no valid key has all-ones slack bits (that pattern is a NaN)

__global__ void __launch_bounds__(256) trial_reduce_kernel(const float* __restrict__ pred_base, const float* __restrict__ pred_trial,
                                                           const float* __restrict__ required, const int* __restrict__ design_rows,
                                                           int n, int T, const int* __restrict__ pair_ptr,
                                                           const int* __restrict__ pair_row, int K, double* __restrict__ summary) {
  __shared__ double s_sum[4];
  __shared__ trial_u64 s_key[4];
  __shared__ int s_cnt[4][3];
  const int k = blockIdx.x, tid = threadIdx.x;
  int p0 = 0, p1 = 0;                                   // the candidate's pairs; entry K, the base, has none
  if (k < K) {
    p0 = pair_ptr[k];
    p1 = pair_ptr[k + 1];
  }
  int nv = 0, nn = 0, nneg = 0;
  double sum = 0.0;
  trial_u64 best = TRIAL_KEY_NONE;
  for (int i = tid; i < n; i += 256) {
    const int r = design_rows[i];
    float s = __uint_as_float(0x7fc00000u);
    if ((unsigned)r < (unsigned)T) {
      float pr = pred_base[r];
      int lo = p0, hi = p1;                             // the first pair of the range whose row is >= r
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pair_row[mid] < r) lo = mid + 1; else hi = mid;
      }
      if (lo < p1 && pair_row[lo] == r) pr = pred_trial[lo];
      s = slack_of(required[r], pr);                    // -0.0 becomes +0.0
    }
    if (s != s) {
      ++nn;
    } else {
      ++nv;
      const trial_u64 key = ((trial_u64)ordered_bits(s) << 32) | (unsigned)r;
      best = key < best ? key : best;
      if (s < 0.f) {
        ++nneg;
        sum += (double)s;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nv += __shfl_xor(nv, o, 64);
    nn += __shfl_xor(nn, o, 64);
    nneg += __shfl_xor(nneg, o, 64);
    sum += __shfl_xor(sum, o, 64);
    const trial_u64 other = __shfl_xor(best, o, 64);
    best = other < best ? other : best;
  }
  if ((tid & 63) == 0) {
    s_cnt[tid >> 6][0] = nv; s_cnt[tid >> 6][1] = nn; s_cnt[tid >> 6][2] = nneg;
    s_sum[tid >> 6] = sum;
    s_key[tid >> 6] = best;
  }
  __syncthreads();
  if (tid == 0) {
    nv = nn = nneg = 0;
    sum = 0.0;
    best = TRIAL_KEY_NONE;
    for (int w = 0; w < 4; ++w) {
      nv += s_cnt[w][0]; nn += s_cnt[w][1]; nneg += s_cnt[w][2];
      sum += s_sum[w];
      best = s_key[w] < best ? s_key[w] : best;
    }
    double* o = summary + (long long)k * 6;
    o[0] = nv; o[1] = nn; o[2] = nneg;
    o[3] = best == TRIAL_KEY_NONE ? (double)__uint_as_float(0x7fc00000u) : (double)ordered_float((unsigned)(best >> 32));
    o[4] = best == TRIAL_KEY_NONE ? -1.0 : (double)(int)(unsigned)(best & 0xffffffffull);
    o[5] = sum;
  }
}

}  // namespace mmft

using namespace mmft;

extern "C" {

int mmft_trial_rows(const int* path_nodes, const int* path_lens, int maxlen, const int* loc_x, const int* loc_y, int map_x,
                    int map_y, const int* paths, const int* f_off, int T, const int* pair_row, const int* pair_cand, int n_pairs,
                    const int* mv_ptr, const int* mv_node, const int* mv_x, const int* mv_y, int K, const float* GP,
                    const float* bias, const float* x, long long ldx, float* xt, long long ldxt, int width, int cnn_col, int Dout,
                    int S, int device, void* stream) {
  MMFT_REQUIRE(S == 64, "trial_rows: the prefix block must be 64 cells (one bitmap word per block)");
  MMFT_REQUIRE(mask_map_ok(map_x, map_y), "trial_rows: the map must hold a multiple of 64 cells, at most 65536");
  MMFT_REQUIRE(Dout >= 4 && Dout % 4 == 0 && Dout <= 1024 && maxlen >= 1 && T >= 1 && K >= 1 && n_pairs >= 0,
               "trial_rows: bad sizes (Dout a multiple of 4 in [4, 1024], maxlen >= 1, T >= 1, K >= 1, n_pairs >= 0)");
  MMFT_REQUIRE(cnn_col >= 0 && cnn_col % 4 == 0 && ldx % 4 == 0 && ldxt % 4 == 0 && (long long)cnn_col + Dout <= width &&
                   width <= ldx && width <= ldxt,
               "trial_rows: bad columns (cnn_col, ldx, ldxt multiples of 4, 0 <= cnn_col, cnn_col + Dout <= width <= ldx, ldxt)");
  if (n_pairs == 0) return MMFT_OK;
  MMFT_REQUIRE(path_nodes && path_lens && loc_x && loc_y && paths && pair_row && pair_cand && mv_ptr && mv_node && mv_x && mv_y &&
                   GP && x && xt,
               "trial_rows: null pointer");
  MMFT_REQUIRE(aligned16(GP) && aligned16(x) && aligned16(xt) && (!bias || aligned16(bias)), "trial_rows: 16-byte alignment");
  DeviceGuard dg(device);
  const int P = map_x * map_y;
  static DynLdsOnce once;
  int arc = ensure_dyn_lds(once, (const void*)trial_rows_kernel, (int)trial_lds_bytes(MASK_MAX_CELLS), "trial_rows");
  if (arc) return arc;
  TrialRowsArgs a;
  TrialRowArgs& r = a.row;
  r.path_nodes = path_nodes; r.path_lens = path_lens; r.loc_x = loc_x; r.loc_y = loc_y; r.paths = paths; r.foff = f_off;
  r.GP = GP; r.bias = bias; r.x = x; r.xt = xt; r.ldx = ldx; r.ldxt = ldxt;
  r.maxlen = maxlen; r.map_x = map_x; r.map_y = map_y; r.width = width; r.cnn_col = cnn_col; r.Dout = Dout;
  a.pair_row = pair_row; a.pair_cand = pair_cand; a.mv_ptr = mv_ptr; a.mv_node = mv_node; a.mv_x = mv_x; a.mv_y = mv_y;
  MMFT_LAUNCH_LDS("trial_rows_kernel", 0.0, 0.0, trial_rows_kernel, dim3(n_pairs), dim3(256), trial_lds_bytes(P), (hipStream_t)stream, a);
  return check_launch("trial_rows");
}

int mmft_trial_reduce(const float* pred_base, const float* pred_trial, const float* required, const int* design_rows, int n, int T,
                      const int* pair_ptr, const int* pair_row, int n_pairs, int K, double* summary, int device, void* stream) {
  MMFT_REQUIRE(n >= 1 && n <= (1 << 24) && T >= 1 && T <= (1 << 24) && K >= 0 && n_pairs >= 0,
               "trial_reduce: need 1 <= n <= 2^24, 1 <= T <= 2^24, K >= 0, n_pairs >= 0 (got n %d, T %d, K %d, n_pairs %d)", n, T, K,
               n_pairs);
  MMFT_REQUIRE(pred_base && required && design_rows && summary && (pair_ptr || K == 0) && ((pair_row && pred_trial) || n_pairs == 0),
               "trial_reduce: null pointer");
  MMFT_REQUIRE((reinterpret_cast<uintptr_t>(summary) & 7) == 0, "trial_reduce: summary must be 8-byte aligned");
  DeviceGuard dg(device);
  const double alg_bytes = (double)(K + 1) * (12.0 * n + 48.0);
  MMFT_LAUNCH("trial_reduce_kernel", 0.0, alg_bytes, trial_reduce_kernel, dim3(K + 1), dim3(256), (hipStream_t)stream, pred_base,
              pred_trial, required, design_rows, n, T, pair_ptr, pair_row, K, summary);
  return check_launch("trial_reduce");
}

}  // extern "C"
