// Exact predictions for a batch of trial pin moves (include/mmft_trial.h).
//
// trial_rows_kernel: one workgroup per (row, candidate) pair.  The candidate's overrides are staged in LDS, the row's mask is
// rasterised with them (mask_raster_path_moved, mask_rule.h: the boxes of mask_raster_path, on the same mask_or_box) and
// projected by place_project (place_project.h), the function placed_fc_fwd_kernel calls - the h_cnn columns are that kernel's
// bits on moved tables, and the tables are never written.  The row's other columns are copied.  Everything after the staging
// is trial_row_write (trial_row.h), which the rows kernels of search.hip, refine.hip and swap.hip call too; the entry point
// refuses and launches through that header's launcher, as theirs do.
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
  const int n_mv = clamp_to(a.mv_ptr[k + 1] - m0, TRIAL_MOVES);      // the same for every thread
  if (tid < n_mv) {
    mv.node[tid] = a.mv_node[m0 + tid];
    mv.x[tid] = a.mv_x[m0 + tid];
    mv.y[tid] = a.mv_y[m0 + tid];
  }
  trial_row_write(a.row, L, mv, n_mv, t, p, tid);       // trial_row.h: the copy, the raster under the overrides, the projection
}

__global__ void __launch_bounds__(256) trial_reduce_kernel(const float* __restrict__ pred_base, const float* __restrict__ pred_trial,
                                                           const float* __restrict__ required, const int* __restrict__ design_rows,
                                                           int n, int T, const int* __restrict__ pair_ptr,
                                                           const int* __restrict__ pair_row, int K, double* __restrict__ summary) {
  __shared__ double s_sum[4];
  __shared__ slack_u64 s_key[4];
  __shared__ int s_cnt[4][3];
  const int k = blockIdx.x, tid = threadIdx.x;
  int p0 = 0, p1 = 0;                                   // the candidate's pairs; entry K, the base, has none
  if (k < K) {
    p0 = pair_ptr[k];
    p1 = pair_ptr[k + 1];
  }
  int nv = 0, nn = 0, nneg = 0;
  double sum = 0.0;
  slack_u64 best = SLACK_KEY_NONE;
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
      const slack_u64 key = ((slack_u64)ordered_bits(s) << 32) | (unsigned)r;
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
    const slack_u64 other = __shfl_xor(best, o, 64);
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
    best = SLACK_KEY_NONE;
    for (int w = 0; w < 4; ++w) {
      nv += s_cnt[w][0]; nn += s_cnt[w][1]; nneg += s_cnt[w][2];
      sum += s_sum[w];
      best = s_key[w] < best ? s_key[w] : best;
    }
    double* o = summary + (long long)k * 6;
    o[0] = nv; o[1] = nn; o[2] = nneg;
    o[3] = best == SLACK_KEY_NONE ? (double)__uint_as_float(0x7fc00000u) : (double)ordered_float((unsigned)(best >> 32));
    o[4] = best == SLACK_KEY_NONE ? -1.0 : (double)(int)(unsigned)(best & 0xffffffffull);
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
  const TrialRowCall c = {"trial_rows", path_nodes, path_lens, maxlen, loc_x, loc_y, map_x, map_y, paths, f_off, GP, bias,
                          x, ldx, xt, ldxt, width, cnn_col, Dout, S, device, stream};
  int rc = trial_row_check(c, T >= 1 && K >= 1 && n_pairs >= 0, "T >= 1, K >= 1, n_pairs >= 0");
  if (rc) return rc;
  if (n_pairs == 0) return MMFT_OK;
  TrialRowsArgs a;
  a.pair_row = pair_row; a.pair_cand = pair_cand; a.mv_ptr = mv_ptr; a.mv_node = mv_node; a.mv_x = mv_x; a.mv_y = mv_y;
  return trial_row_launch<TrialRowsArgs, trial_rows_kernel>(c, "trial_rows_kernel", a, n_pairs,
                                                            pair_row && pair_cand && mv_ptr && mv_node && mv_x && mv_y);
}

int mmft_trial_reduce(const float* pred_base, const float* pred_trial, const float* required, const int* design_rows, int n, int T,
                      const int* pair_ptr, const int* pair_row, int n_pairs, int K, double* summary, int device, void* stream) {
  MMFT_REQUIRE(n >= 1 && n <= (1 << 24) && T >= 1 && T <= (1 << 24) && K >= 0 && n_pairs >= 0,
               "trial_reduce: need 1 <= n <= 2^24, 1 <= T <= 2^24, K >= 0, n_pairs >= 0 (got n %d, T %d, K %d, n_pairs %d)", n, T, K,
               n_pairs);
  MMFT_REQUIRE(pred_base && required && design_rows && summary && (pair_ptr || K == 0) && ((pair_row && pred_trial) || n_pairs == 0),
               "trial_reduce: null pointer");
  MMFT_REQUIRE(aligned8(summary), "trial_reduce: summary must be 8-byte aligned");
  DeviceGuard dg(device);
  const double alg_bytes = (double)(K + 1) * (12.0 * n + 48.0);
  MMFT_LAUNCH("trial_reduce_kernel", 0.0, alg_bytes, trial_reduce_kernel, dim3(K + 1), dim3(256), (hipStream_t)stream, pred_base,
              pred_trial, required, design_rows, n, T, pair_ptr, pair_row, K, summary);
  return check_launch("trial_reduce");
}

}  // extern "C"
