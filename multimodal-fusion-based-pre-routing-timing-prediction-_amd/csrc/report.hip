// Timing report on the device (include/mmft_report.h): per design WNS, TNS, violation count, the k most critical endpoints
// and a slack histogram, from the predictions and the required times of a batch.
//
// Every valid row becomes ONE 64-bit key, (ordered_bits(slack) << 32) | batch row: unsigned order of the keys is ascending
// (slack, row) order, and because a row appears once the keys of a design are distinct.  "The next worst endpoint" is then
// "the smallest key above the last one taken": k rounds of a block-wide minimum, no marking, no tie handling.  WNS and its
// row are the first key taken.
//
// A design is cut into parts of at most TR_PART rows, one workgroup per part.  A part gathers its rows once, keeps their
// keys in LDS, reduces its counts, its negative sum (fp64; thread-strided, then wave, then LDS in wave order: a fixed tree)
// and its histogram, and selects its own k smallest keys.  A design with one part writes its outputs from there.  A design
// with several parts leaves each part's result in the workspace and counts the part in the design's counter; the part that
// arrives last merges all of them IN PART ORDER (the discipline of level_bwd_pair_kernel, mlp2_bf16.hip): fp64 sums in part
// order, integer counts, and the k smallest of the parts' sorted lists.  Whichever part that is, the bits are the same.
// Nobody waits for anybody, and there are no float atomics.
#include "common.h"
#include "slack_key.h"
#include "../../include/mmft_report.h"

#include <math.h>

namespace {

typedef unsigned long long u64;

constexpr int TR_THREADS = 256;
constexpr int TR_WAVES = TR_THREADS / 64;
constexpr int TR_PART = 4096;                 // rows of one part: 32 KB of keys in LDS
constexpr int TR_KMAX = 64;
constexpr int TR_BINS_MAX = 64;
constexpr u64 KEY_NONE = ~0ull;               // no valid key has all-ones slack bits (that pattern is a NaN)

struct TimingReportArgs {
  const float* pred;
  const float* required;
  const int* design_ptr;
  const int* design_rows;
  int T, B, k, nbins;
  float lo, hi, w;
  double* summary;
  int* worst_row;
  float* worst_slack;
  int* hist;
  int* counters;               // [B], zero when the kernel starts
  char* slots;                 // [B + T / TR_PART] part results of slot_bytes each: keys u64[k], tns, counts int[4], hist int[nbins + 2]
  long long slot_bytes;
};

using mmft::ordered_bits;                     // slack_key.h: unsigned order of the bits == numeric order of the floats
__device__ __forceinline__ float key_slack(u64 key) { return mmft::ordered_float((unsigned)(key >> 32)); }
__device__ __forceinline__ int key_row(u64 key) { return (int)(unsigned)(key & 0xffffffffull); }

__device__ __forceinline__ u64 wave_min(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}

// out[0 .. k): the k smallest of the distinct keys[0 .. n) (KEY_NONE entries are holes) in ascending order, KEY_NONE where
// there are fewer.  All threads of the block call it; keys, out and red are LDS.  red is double-buffered over the rounds, so
// one barrier per round is enough: a round's slots are rewritten two rounds later, behind the next round's barrier.
__device__ void select_smallest(const u64* keys, int n, int k, u64* out, u64 (*red)[TR_WAVES]) {
  const int tid = threadIdx.x;
  u64 last = 0;                                // below every valid key (-inf maps to 0x007fffff in the high word)
  for (int r = 0; r < k; ++r) {
    u64 m = KEY_NONE;
    for (int i = tid; i < n; i += TR_THREADS) {
      const u64 v = keys[i];
      if (v > last && v < m) m = v;
    }
    m = wave_min(m);
    if ((tid & 63) == 0) red[r & 1][tid >> 6] = m;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < TR_WAVES; ++w) {
      const u64 t = red[r & 1][w];
      m = t < m ? t : m;
    }
    if (m == KEY_NONE) {                       // block-uniform: nothing is left, the rest is padding
      for (int j = r + tid; j < k; j += TR_THREADS) out[j] = KEY_NONE;
      break;
    }
    if (tid == 0) out[r] = m;
    last = m;
  }
  __syncthreads();
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void __launch_bounds__(TR_THREADS) timing_report_kernel(TimingReportArgs a) {
  __shared__ u64 s_keys[TR_PART];
  __shared__ u64 s_sel[TR_KMAX];
  __shared__ u64 s_red[2][TR_WAVES];
  __shared__ double s_sum[TR_WAVES];
  __shared__ int s_cnt[TR_WAVES][3];
  __shared__ int s_hist[TR_BINS_MAX + 2];
  __shared__ int s_where[6];                   // design, part, parts, first slot, first row, end row
  __shared__ int s_last;
  const int tid = threadIdx.x, k = a.k, nh = a.nbins ? a.nbins + 2 : 0;

  // which part of which design this workgroup is: parts are numbered design by design (the grid has B + T / TR_PART
  // workgroups, at least as many as there are parts; the others leave).  design_ptr is clamped to a monotone sequence in
  // [0, T], so nothing below can index outside the T rows whatever the table holds
  if (tid == 0) {
    int first = 0, found = -1;
    for (int b = 0; b < a.B; ++b) {
      const int lo = clampi(a.design_ptr[b], 0, a.T), hi = clampi(a.design_ptr[b + 1], lo, a.T);
      const int parts = hi - lo > TR_PART ? (hi - lo + TR_PART - 1) / TR_PART : 1;
      if ((int)blockIdx.x < first + parts) {
        const int part = blockIdx.x - first, r0 = lo + part * TR_PART;
        found = b;
        s_where[1] = part; s_where[2] = parts; s_where[3] = first; s_where[4] = r0; s_where[5] = hi - r0 > TR_PART ? r0 + TR_PART : hi;
        break;
      }
      first += parts;
    }
    s_where[0] = found;
  }
  for (int j = tid; j < TR_BINS_MAX + 2; j += TR_THREADS) s_hist[j] = 0;
  __syncthreads();
  const int b = s_where[0];
  if (b < 0) return;
  const int part = s_where[1], parts = s_where[2], first = s_where[3], r0 = s_where[4], n = s_where[5] - r0;

  // ---- the part's rows: gather, keys into LDS, counts / negative sum / histogram
  int nv = 0, nn = 0, nneg = 0;
  double sum = 0.0;
  for (int i = tid; i < n; i += TR_THREADS) {
    const int r = a.design_rows[r0 + i];
    u64 key = KEY_NONE;
    float s = __uint_as_float(0x7fc00000u);
    if ((unsigned)r < (unsigned)a.T) s = mmft::slack_of(a.required[r], a.pred[r]);  // -0.0 becomes +0.0
    if (s != s) {
      ++nn;
    } else {
      ++nv;
      key = ((u64)ordered_bits(s) << 32) | (unsigned)r;
      if (s < 0.f) {
        ++nneg;
        sum += (double)s;
      }
      if (nh) {
        int bin;
        if (s < a.lo) bin = 0;
        else if (s >= a.hi) bin = a.nbins + 1;
        else {
          const int j = (int)floorf((s - a.lo) / a.w);
          bin = 1 + (j < a.nbins - 1 ? j : a.nbins - 1);
        }
        atomicAdd(&s_hist[bin], 1);
      }
    }
    s_keys[i] = key;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nv += __shfl_xor(nv, o, 64);
    nn += __shfl_xor(nn, o, 64);
    nneg += __shfl_xor(nneg, o, 64);
    sum += __shfl_xor(sum, o, 64);
  }
  if ((tid & 63) == 0) {
    s_cnt[tid >> 6][0] = nv; s_cnt[tid >> 6][1] = nn; s_cnt[tid >> 6][2] = nneg;
    s_sum[tid >> 6] = sum;
  }
  __syncthreads();
  nv = nn = nneg = 0;
  sum = 0.0;
#pragma unroll
  for (int w = 0; w < TR_WAVES; ++w) {
    nv += s_cnt[w][0]; nn += s_cnt[w][1]; nneg += s_cnt[w][2];
    sum += s_sum[w];
  }
  select_smallest(s_keys, n, k, s_sel, s_red);

  if (parts > 1) {
    // ---- publish this part; the last part to arrive merges all of them in part order
    {
      char* slot = a.slots + (long long)(first + part) * a.slot_bytes;
      u64* pk = reinterpret_cast<u64*>(slot);
      int* pc = reinterpret_cast<int*>(slot + 8 * (k + 1));
      for (int j = tid; j < k; j += TR_THREADS) __hip_atomic_store(pk + j, s_sel[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int j = tid; j < nh; j += TR_THREADS) __hip_atomic_store(pc + 4 + j, s_hist[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (tid == 0) {
        __hip_atomic_store(pk + k, (u64)__double_as_longlong(sum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pc + 0, nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pc + 1, nn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(pc + 2, nneg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");          // the part's result is visible before the counter moves
    }
    __syncthreads();
    if (tid == 0) {
      const int old = __hip_atomic_fetch_add(a.counters + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_last = old == parts - 1;
      if (old == parts - 1) __hip_atomic_store(a.counters + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next call
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");            // ... and the other parts are read after it was seen full
    const char* base = a.slots + (long long)first * a.slot_bytes;
    if (tid == 0) {
      nv = nn = nneg = 0;
      sum = 0.0;
      for (int p = 0; p < parts; ++p) {
        const char* slot = base + (long long)p * a.slot_bytes;
        const int* pc = reinterpret_cast<const int*>(slot + 8 * (k + 1));
        nv += __hip_atomic_load(pc + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        nn += __hip_atomic_load(pc + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        nneg += __hip_atomic_load(pc + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sum += __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const u64*>(slot) + k, __ATOMIC_RELAXED,
                                                                  __HIP_MEMORY_SCOPE_AGENT));
      }
    }
    for (int j = tid; j < nh; j += TR_THREADS) {                  // (thread j is the only one that touches s_hist[j] here)
      int c = 0;
      for (int p = 0; p < parts; ++p)
        c += __hip_atomic_load(reinterpret_cast<const int*>(base + (long long)p * a.slot_bytes + 8 * (k + 1)) + 4 + j,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_hist[j] = c;
    }
    // the k smallest of the parts' sorted lists: the running result in s_keys[0 .. k), as many parts' lists behind it as fit
    const int fit = (TR_PART - k) / k;
    for (int j = tid; j < k; j += TR_THREADS) s_keys[j] = KEY_NONE;
    for (int p0 = 0; p0 < parts; p0 += fit) {
      const int np = parts - p0 < fit ? parts - p0 : fit;
      for (int i = tid; i < np * k; i += TR_THREADS)
        s_keys[k + i] = __hip_atomic_load(reinterpret_cast<const u64*>(base + (long long)(p0 + i / k) * a.slot_bytes) + i % k,
                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      select_smallest(s_keys, k + np * k, k, s_sel, s_red);
      for (int j = tid; j < k; j += TR_THREADS) s_keys[j] = s_sel[j];
      __syncthreads();
    }
  }

  // ---- the design's outputs (every element, pads included)
  if (tid == 0) {
    double* o = a.summary + (long long)b * 6;
    const u64 w0 = s_sel[0];
    o[0] = nv; o[1] = nn; o[2] = nneg;
    o[3] = w0 == KEY_NONE ? (double)__uint_as_float(0x7fc00000u) : (double)key_slack(w0);
    o[4] = w0 == KEY_NONE ? -1.0 : (double)key_row(w0);
    o[5] = sum;
  }
  for (int j = tid; j < k; j += TR_THREADS) {
    const u64 key = s_sel[j];
    a.worst_row[(long long)b * k + j] = key == KEY_NONE ? -1 : key_row(key);
    a.worst_slack[(long long)b * k + j] = key == KEY_NONE ? __uint_as_float(0x7f800000u) : key_slack(key);
  }
  for (int j = tid; j < nh; j += TR_THREADS) a.hist[(long long)b * nh + j] = s_hist[j];
}

inline long long align16(long long v) { return (v + 15) & ~15ll; }
inline long long slot_bytes(int k, int nbins) { return (8ll * (k + 1) + 4ll * (4 + (nbins ? nbins + 2 : 0)) + 7) & ~7ll; }
inline bool limits_ok(int T, int B, int k, int nbins) {
  return T >= 1 && T <= (1 << 24) && B >= 1 && k >= 1 && k <= TR_KMAX && nbins >= 0 && nbins <= TR_BINS_MAX;
}

}  // namespace

extern "C" {

long long mmft_timing_report_workspace_bytes(int T, int B, int k, int nbins) {
  if (!limits_ok(T, B, k, nbins)) {
    mmft::set_error("timing_report_workspace_bytes: need 1 <= T <= 2^24, B >= 1, 1 <= k <= %d, 0 <= nbins <= %d (got T %d, B %d, k %d, nbins %d)",
                    TR_KMAX, TR_BINS_MAX, T, B, k, nbins);
    return -1;
  }
  return align16(4ll * B) + ((long long)B + T / TR_PART) * slot_bytes(k, nbins);
}

int mmft_timing_report(const float* pred, const float* required, const int* design_ptr, const int* design_rows,
                       int T, int B, int k, float hist_lo, float hist_hi, int nbins,
                       double* summary, int* worst_row, float* worst_slack, int* hist,
                       void* workspace, long long workspace_bytes, int device, void* stream) {
  MMFT_REQUIRE(limits_ok(T, B, k, nbins),
               "timing_report: need 1 <= T <= 2^24, B >= 1, 1 <= k <= %d, 0 <= nbins <= %d (got T %d, B %d, k %d, nbins %d)",
               TR_KMAX, TR_BINS_MAX, T, B, k, nbins);
  MMFT_REQUIRE(pred && required && design_ptr && design_rows && summary && worst_row && worst_slack && (hist || nbins == 0),
               "timing_report: null pointer");
  MMFT_REQUIRE(nbins == 0 || (isfinite(hist_lo) && isfinite(hist_hi) && hist_lo < hist_hi),
               "timing_report: a histogram needs finite hist_lo < hist_hi (got %g, %g)", (double)hist_lo, (double)hist_hi);
  const long long need = mmft_timing_report_workspace_bytes(T, B, k, nbins);
  MMFT_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && workspace_bytes >= need,
               "timing_report: workspace of %lld bytes, 8-byte aligned, needed (got %lld)", need, workspace_bytes);
  mmft::DeviceGuard dg(device);
  hipStream_t st = (hipStream_t)stream;
  TimingReportArgs a;
  a.pred = pred; a.required = required; a.design_ptr = design_ptr; a.design_rows = design_rows;
  a.T = T; a.B = B; a.k = k; a.nbins = nbins;
  a.lo = hist_lo; a.hi = hist_hi; a.w = nbins ? (hist_hi - hist_lo) / (float)nbins : 1.f;
  a.summary = summary; a.worst_row = worst_row; a.worst_slack = worst_slack; a.hist = hist;
  a.counters = static_cast<int*>(workspace);
  a.slots = static_cast<char*>(workspace) + align16(4ll * B);
  a.slot_bytes = slot_bytes(k, nbins);
  const int grid = B + T / TR_PART;
  if (T > TR_PART) {
    // only then can a design have several parts.  The finisher leaves its counter zero, but the workspace may come with
    // anything in it (a fresh allocation, a launch that was cut short): the counters are zeroed on the stream every call
    hipError_t e = hipMemsetAsync(a.counters, 0, 4ll * B, st);
    if (e != hipSuccess) {
      mmft::set_error("timing_report: hipMemsetAsync: %s", hipGetErrorString(e));
      return MMFT_ERR_LAUNCH;
    }
  }
  const double alg_bytes = 12.0 * T + B * (48.0 + 8.0 * k + 4.0 * (nbins ? nbins + 2 : 0));
  MMFT_LAUNCH("timing_report_kernel", 0.0, alg_bytes, timing_report_kernel, dim3(grid), dim3(TR_THREADS), st, a);
  return mmft::check_launch("timing_report");
}

}  // extern "C"
