// The score of ONE candidate over its entries, and the design's base figures (include/mmft_search.h): per entry the change of
// the quanta, of the violations, the new NaN rows, the capped rows and the worst (slack, row) key, all in integers; a wave's
// 64 lanes combined by butterflies; one lane's store of the six figures.  search_score_kernel (search.hip) calls it per
// (group, offset), swap_score_kernel (swap.hip) per pair: the tests hold the two to the same definitions, and the code that
// makes those figures is here once.  mmft_search_best and mmft_swap_score form the base figures by search_base_launch.
#pragma once
#include "slack_key.h"
#include "slack_quanta.h"

namespace mmft {

struct SearchAcc {
  long long sum = 0;
  int viol = 0, nans = 0, caps = 0;
  slack_u64 best = SLACK_KEY_NONE;
};

// one entry: row r of pred_base against the candidate's prediction *trial (read only for a row inside [0, T))
__device__ __forceinline__ void search_acc_entry(SearchAcc& a, int r, int T, const float* __restrict__ required,
                                                 const float* __restrict__ pred_base, const float* __restrict__ trial, int scale_log2) {
  if ((unsigned)r >= (unsigned)T) return;
  const float req = required[r];
  const float sb = slack_of(req, pred_base[r]), st = slack_of(req, *trial);
  bool cb = false, ct = false;
  const long long qb = sb < 0.f ? (long long)crit_quanta(sb, scale_log2, cb) : 0ll;
  const long long qt = st < 0.f ? (long long)crit_quanta(st, scale_log2, ct) : 0ll;
  a.sum += qt - qb;
  a.viol += (st < 0.f ? 1 : 0) - (sb < 0.f ? 1 : 0);
  a.caps += (cb || ct) ? 1 : 0;
  if (st != st) {
    a.nans += (sb == sb) ? 1 : 0;
  } else {
    const slack_u64 key = ((slack_u64)ordered_bits(st) << 32) | (unsigned)r;
    a.best = key < a.best ? key : a.best;
  }
}

// the 64 lanes of a wave combined: integer adds and a 64-bit minimum, every lane ends with the same figures
__device__ __forceinline__ void search_acc_wave(SearchAcc& a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.sum += __shfl_xor(a.sum, o, 64);
    a.viol += __shfl_xor(a.viol, o, 64);
    a.nans += __shfl_xor(a.nans, o, 64);
    a.caps += __shfl_xor(a.caps, o, 64);
    const slack_u64 other = __shfl_xor(a.best, o, 64);
    a.best = other < a.best ? other : a.best;
  }
}

// element `at` of the six tables (one lane calls it)
__device__ __forceinline__ void search_acc_store(const SearchAcc& a, long long at, long long* __restrict__ dq, int* __restrict__ dviol,
                                                 int* __restrict__ new_nan, int* __restrict__ capped, float* __restrict__ worst,
                                                 int* __restrict__ worst_row) {
  dq[at] = a.sum;
  dviol[at] = a.viol;
  new_nan[at] = a.nans;
  capped[at] = a.caps;
  worst[at] = a.best == SLACK_KEY_NONE ? __uint_as_float(0x7fc00000u) : ordered_float((unsigned)(a.best >> 32));
  worst_row[at] = a.best == SLACK_KEY_NONE ? -1 : (int)(unsigned)(a.best & 0xffffffffull);
}

// THE BASE FIGURES: base [3] = the sum of q(s_base) over design_rows [n], the violating rows, the NaN rows.  A memset of the
// three int64 and search_base_kernel (search.hip), on `st`; `entry` starts the message if the memset fails, `what` if the launch does
int search_base_launch(const char* entry, const char* what, const float* pred_base, const float* required, const int* design_rows,
                       int n, int T, int scale_log2, long long* base, hipStream_t st);

}  // namespace mmft
