// The score of ONE candidate over its entries, and the design's base figures (include/mmft_search.h): per entry the change of
// the quanta, of the violations, the new NaN rows, the capped rows and the worst (slack, row) key, all in integers; a wave's
// 64 lanes combined by butterflies; one lane's store of the six figures.  search_score_kernel (search.hip) calls it per
// (group, offset), swap_score_kernel (swap.hip) per pair: the tests hold the two to the same definitions, and the code that
// makes those figures is here once.  search_base_rows is the body of search_base_kernel and of swap_base_kernel.
#pragma once
#include "slack_key.h"
#include "slack_quanta.h"

namespace mmft {

typedef unsigned long long search_u64;
constexpr search_u64 SEARCH_KEY_NONE = ~0ull;   // no valid key has all-ones slack bits (that pattern is a NaN)

struct SearchAcc {
  long long sum = 0;
  int viol = 0, nans = 0, caps = 0;
  search_u64 best = SEARCH_KEY_NONE;
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
    const search_u64 key = ((search_u64)ordered_bits(st) << 32) | (unsigned)r;
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
    const search_u64 other = __shfl_xor(a.best, o, 64);
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
  worst[at] = a.best == SEARCH_KEY_NONE ? __uint_as_float(0x7fc00000u) : ordered_float((unsigned)(a.best >> 32));
  worst_row[at] = a.best == SEARCH_KEY_NONE ? -1 : (int)(unsigned)(a.best & 0xffffffffull);
}

// THE BASE FIGURES: base [3] (cleared by the caller) += the sum of q(s_base) over design_rows [n], the violating rows, the NaN
// rows; grid-strided over workgroups of 256 threads, a wave's figures added by integer atomics
__device__ __forceinline__ void search_base_rows(const float* __restrict__ pred_base, const float* __restrict__ required,
                                                 const int* __restrict__ design_rows, int n, int T, int scale_log2,
                                                 search_u64* __restrict__ base) {
  search_u64 sum = 0ull;
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
    if (viol) atomicAdd(base + 1, (search_u64)viol);
    if (nans) atomicAdd(base + 2, (search_u64)nans);
  }
}

}  // namespace mmft
