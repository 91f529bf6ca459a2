// Timing criticality per pin and per map cell (include/mmft_crit.h): every valid batch row scatters its slack
// into the pins of its path and into the cells of its mask.
//
// A minimum is an unsigned integer atomicMin over an order-preserving key of the slack (slack_key.h, the key of report.hip):
// per pin ONE 64-bit word (key << 32) | batch row, whose minimum is the smallest slack and, on equal slack, the smallest row;
// per cell and per design the 32-bit key alone.  Counts are integer atomic adds.  Integer min and add commute, so the words
// do not depend on the order in which workgroups arrive: no float atomics, same inputs, same bits.
//
// Three launches on one stream:
//   crit_init_kernel     the keyed words (workspace) to "none", the counts (outputs) to zero
//   crit_scatter_kernel  one workgroup of 256 threads per batch row: slack, the pins of the path (<= maxlen 8-byte atomics),
//                        and - with the cell outputs - the row's mask as a bitmap in LDS (mask_raster_path, mask_rule.h: the
//                        function placed_fc_fwd_kernel, place.hip, builds its bitmap with), then one atomic per set bit, a
//                        wave on the 64 consecutive cells of one bitmap block at a time, empty blocks skipped
//                        The designs' minima and row counts come from the first T / 1024 workgroups, each for 1024 rows,
//                        combined in LDS (crit_design_words)
//   crit_decode_kernel   keyed words -> node_slack / node_row / node_crit, cell_slack
//
// The three kernels are templates on SUMS (include/mmft_crit_sums.h, mmft_criticality_sums): <false> is the code above and
// nothing else; <true> also adds, for every violating row, its negative slack as an integer number of quanta (crit_quanta)
// wherever <false> counts the row - 8-byte integer adds into the int64 outputs themselves, beside the 4-byte ones, from the
// same walk over the pins and the same bitmap - and sums the quanta and the saturated rows per design through the LDS
// combine of crit_design_words; its decode kernel forms the shares in one fp64 division each.
#include "common.h"
#include "mask_rule.h"
#include "slack_key.h"
#include "slack_quanta.h"
#include "../../include/mmft_crit.h"
#include "../../include/mmft_crit_sums.h"

namespace mmft {

typedef unsigned long long crit_u64;

constexpr int CRIT_THREADS = 256;
constexpr int CRIT_ROWS = 1024;               // rows whose per-design words one workgroup combines in LDS
constexpr int CRIT_LDS_DESIGNS = 256;         // ... for the designs below this
constexpr int CRIT_MAX_GRID = 8192;           // the init and decode kernels stride over their elements
constexpr crit_u64 CRIT_NONE64 = ~0ull;       // no valid slack has all-ones ordered bits (that pattern is a NaN)
constexpr unsigned CRIT_NONE32 = ~0u;

struct CritArgs {
  const float* pred;
  const float* required;
  const int* path_nodes;
  const int* path_lens;
  const int* loc_x;
  const int* loc_y;
  const int* paths;
  const int* row_design;
  int maxlen, map_x, map_y, P, T, N, B;       // P == 0: no cell outputs
  float* node_slack;
  int* node_row;
  int* node_viol;
  float* node_crit;
  float* cell_slack;
  int* cell_viol;
  int* counts;
  crit_u64* node_key;                         // [N]
  unsigned* design_key;                       // [B]
  unsigned* cell_key;                         // [B][P]
  // SUMS only (include/mmft_crit_sums.h); the sums accumulate in the outputs
  int scale_log2;
  crit_u64* node_nsum;                        // [N]
  crit_u64* cell_nsum;                        // [B][P]
  crit_u64* design_nsum;                      // [B]
  int* saturated;                             // [B]
  float* node_share;
  float* cell_share;
};

// The quanta of a violating slack: crit_quanta (slack_quanta.h), shared with the window search.

template <bool SUMS>
__global__ void __launch_bounds__(CRIT_THREADS) crit_init_kernel(CritArgs a) {
  const long long BP = (long long)a.B * a.P;
  const long long n = a.N > BP ? a.N : BP;    // (2 B <= N or B P is not promised: the design words have a loop of their own)
  const long long step = (long long)gridDim.x * CRIT_THREADS;
  for (long long i = (long long)blockIdx.x * CRIT_THREADS + threadIdx.x; i < n; i += step) {
    if (i < a.N) {
      a.node_key[i] = CRIT_NONE64;
      a.node_viol[i] = 0;
      if constexpr (SUMS) a.node_nsum[i] = 0ull;
    }
    if (i < BP) {
      a.cell_key[i] = CRIT_NONE32;
      a.cell_viol[i] = 0;
      if constexpr (SUMS) a.cell_nsum[i] = 0ull;
    }
  }
  for (long long i = (long long)blockIdx.x * CRIT_THREADS + threadIdx.x; i < a.B; i += step) {
    a.design_key[i] = CRIT_NONE32;
    a.counts[2 * i] = 0;
    a.counts[2 * i + 1] = 0;
    if constexpr (SUMS) {
      a.design_nsum[i] = 0ull;
      a.saturated[i] = 0;
    }
  }
}

// The per-design words of the rows [blockIdx.x * CRIT_ROWS, ... + CRIT_ROWS): valid and NaN counts and the smallest key.  One
// atomic per row on a handful of addresses serialises in L2 (measured: 10 800 rows on 8 designs cost 0.1 ms), so
// the rows meet in LDS first - designs below CRIT_LDS_DESIGNS; the others go to memory directly - and a block sends at most
// three atomics per design.  lds: 3 * CRIT_LDS_DESIGNS words, free again when this returns.
// SUMS: the violating rows' quanta and the saturated rows take the same way - 3 * CRIT_LDS_DESIGNS more words, the sums as
// 8-byte LDS adds (1024 rows of at most 2^32: no overflow) - and a block sends at most two more atomics per design.
template <bool SUMS>
__device__ void crit_design_words(const CritArgs& a, unsigned* lds) {
  const int tid = threadIdx.x;
  unsigned* s_min = lds;
  unsigned* s_valid = lds + CRIT_LDS_DESIGNS;
  unsigned* s_nan = lds + 2 * CRIT_LDS_DESIGNS;
  unsigned* s_sat = lds + 3 * CRIT_LDS_DESIGNS;
  crit_u64* s_sum = reinterpret_cast<crit_u64*>(lds + 4 * CRIT_LDS_DESIGNS);      // (the caller's array is 8-byte aligned)
  for (int d = tid; d < CRIT_LDS_DESIGNS; d += CRIT_THREADS) {
    s_min[d] = CRIT_NONE32;
    s_valid[d] = 0u;
    s_nan[d] = 0u;
    if constexpr (SUMS) {
      s_sat[d] = 0u;
      s_sum[d] = 0ull;
    }
  }
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * CRIT_ROWS;
  for (int i = tid; i < CRIT_ROWS && r0 + i < a.T; i += CRIT_THREADS) {
    const int r = (int)(r0 + i);
    const int b = a.row_design ? a.row_design[r] : 0;
    if ((unsigned)b >= (unsigned)a.B) continue;                            // outside the contract; nothing is indexed by it
    const float s = slack_of(a.required[r], a.pred[r]);
    const bool nan = s != s;
    if (b < CRIT_LDS_DESIGNS) {
      if (nan) {
        atomicAdd(s_nan + b, 1u);
      } else {
        atomicAdd(s_valid + b, 1u);
        atomicMin(s_min + b, ordered_bits(s));
      }
    } else if (nan) {
      atomicAdd(a.counts + 2 * b + 1, 1);
    } else {
      atomicAdd(a.counts + 2 * b, 1);
      atomicMin(a.design_key + b, ordered_bits(s));
    }
    if constexpr (SUMS) {
      if (s < 0.f) {                                                       // (false for a NaN)
        bool capped;
        const crit_u64 q = crit_quanta(s, a.scale_log2, capped);
        if (b < CRIT_LDS_DESIGNS) {
          atomicAdd(s_sum + b, q);
          if (capped) atomicAdd(s_sat + b, 1u);
        } else {
          atomicAdd(a.design_nsum + b, q);
          if (capped) atomicAdd(a.saturated + b, 1);
        }
      }
    }
  }
  __syncthreads();
  for (int d = tid; d < CRIT_LDS_DESIGNS && d < a.B; d += CRIT_THREADS) {
    if (s_valid[d]) {
      atomicAdd(a.counts + 2 * d, (int)s_valid[d]);
      atomicMin(a.design_key + d, s_min[d]);
    }
    if (s_nan[d]) atomicAdd(a.counts + 2 * d + 1, (int)s_nan[d]);
    if constexpr (SUMS) {
      if (s_sum[d]) atomicAdd(a.design_nsum + d, s_sum[d]);
      if (s_sat[d]) atomicAdd(a.saturated + d, (int)s_sat[d]);
    }
  }
  __syncthreads();
}

template <bool SUMS>
__global__ void __launch_bounds__(CRIT_THREADS) crit_scatter_kernel(CritArgs a) {
  __shared__ __attribute__((aligned(8))) unsigned bits[MASK_MAX_CELLS / 32];
  static_assert(6 * CRIT_LDS_DESIGNS <= MASK_MAX_CELLS / 32, "the per-design words borrow the bitmap");
  __shared__ int pin_x[CRIT_THREADS], pin_y[CRIT_THREADS];
  const int t = blockIdx.x, tid = threadIdx.x;
  // the first T / CRIT_ROWS (rounded up) workgroups also carry a slice of the per-design words (the grid has T workgroups)
  if ((long long)blockIdx.x * CRIT_ROWS < a.T) crit_design_words<SUMS>(a, bits);
  const int b = a.row_design ? a.row_design[t] : 0;
  if ((unsigned)b >= (unsigned)a.B) return;                                // (not promised to be checked; nothing is indexed by it)
  const float s = slack_of(a.required[t], a.pred[t]);
  if (s != s) return;                                                      // the same for every thread of the row
  const unsigned key = ordered_bits(s);
  const bool viol = s < 0.f;
  crit_u64 quanta = 0ull;                                                  // SUMS: what a violating row adds wherever it is counted
  if constexpr (SUMS) {
    bool capped;
    if (viol) quanta = crit_quanta(s, a.scale_log2, capped);
  }
  const int q = a.paths[t];
  const int* path = a.path_nodes + (long long)q * a.maxlen;
  const int len = a.path_lens[q] < a.maxlen ? a.path_lens[q] : a.maxlen;   // the same for every thread: the barriers below are uniform
  // ---- the pins: one 64-bit minimum per live position
  const crit_u64 word = ((crit_u64)key << 32) | (unsigned)t;
  for (int j = tid; j < len; j += CRIT_THREADS) {
    const int n = path[j];
    if ((unsigned)n >= (unsigned)a.N) continue;                            // outside the contract; never written through
    atomicMin(a.node_key + n, word);
    if (viol) {
      atomicAdd(a.node_viol + n, 1);
      if constexpr (SUMS) atomicAdd(a.node_nsum + n, quanta);
    }
  }
  if (a.P == 0) return;
  // ---- the mask: THE MASK RULE of mmft_place.h, staged (mask_rule.h); a node id outside the contract is never read through
  const int words = a.P >> 5, nblk = a.P >> 6;
  if (len < 2) return;                                                     // an empty mask
  for (int w = tid; w < words; w += CRIT_THREADS) bits[w] = 0u;
  mask_raster_path<CRIT_THREADS, true>(bits, pin_x, pin_y, path, len, a.loc_x, a.loc_y, a.N, a.map_x, a.map_y, tid);
  __syncthreads();
  // ---- the cells: wave w takes the blocks w, w + 4, ... of 64 consecutive cells, lane l the cell l of the block
  const int lane = tid & 63, wave = tid >> 6;
  unsigned* ck = a.cell_key + (long long)b * a.P;
  int* cv = a.cell_viol + (long long)b * a.P;
  crit_u64* cn = SUMS ? a.cell_nsum + (long long)b * a.P : nullptr;
  for (int blk = wave; blk < nblk; blk += CRIT_THREADS / 64) {
    const unsigned lo = bits[2 * blk], hi = bits[2 * blk + 1];
    if ((lo | hi) == 0u) continue;                                         // wave-uniform
    if (((lane < 32 ? lo : hi) >> (lane & 31)) & 1u) {
      const int c = (blk << 6) + lane;
      atomicMin(ck + c, key);
      if (viol) {
        atomicAdd(cv + c, 1);
        if constexpr (SUMS) atomicAdd(cn + c, quanta);
      }
    }
  }
}

// SUMS: nsum / design_nsum as the header states it - both sums to fp64 (round to nearest), one IEEE fp64 division, to fp32
__device__ __forceinline__ float crit_share(crit_u64 nsum, crit_u64 total) {
  return total == 0ull ? 0.f : (float)((double)(long long)nsum / (double)(long long)total);
}

template <bool SUMS>
__global__ void __launch_bounds__(CRIT_THREADS) crit_decode_kernel(CritArgs a) {
  const long long BP = (long long)a.B * a.P;
  const long long n = a.N > BP ? a.N : BP;
  const long long step = (long long)gridDim.x * CRIT_THREADS;
  const float inf = __uint_as_float(0x7f800000u);
  for (long long i = (long long)blockIdx.x * CRIT_THREADS + threadIdx.x; i < n; i += step) {
    if (i < a.N) {
      const crit_u64 word = a.node_key[i];
      float s = inf, crit = 0.f;
      int row = -1;
      if (word != CRIT_NONE64) {
        s = ordered_float((unsigned)(word >> 32));
        row = (int)(unsigned)(word & 0xffffffffull);
        if (s < 0.f) {
          // the worst slack of the row's design, over all its valid rows: <= s, so negative
          const float w = ordered_float(a.design_key[a.row_design ? a.row_design[row] : 0]);
          crit = s == w ? 1.f : s / w;
        }
      }
      a.node_slack[i] = s;
      a.node_row[i] = row;
      a.node_crit[i] = crit;
      if constexpr (SUMS)
        a.node_share[i] = row < 0 ? 0.f : crit_share(a.node_nsum[i], a.design_nsum[a.row_design ? a.row_design[row] : 0]);
    }
    if (i < BP) {
      const unsigned key = a.cell_key[i];
      a.cell_slack[i] = key == CRIT_NONE32 ? inf : ordered_float(key);
      if constexpr (SUMS) a.cell_share[i] = crit_share(a.cell_nsum[i], a.design_nsum[i / a.P]);
    }
  }
}

inline long long crit_align8(long long v) { return (v + 7) & ~7ll; }
inline bool crit_sizes_ok(int N, int B, int P) {
  return N >= 1 && B >= 1 && (P == 0 || mask_map_ok(P, 1));    // (the cell count alone: a map of P x 1)
}
inline long long crit_workspace_bytes(int N, int B, int P) { return 8ll * N + crit_align8(4ll * B) + 4ll * B * P; }

// The checks both entry points share (`fn` names the caller in the message), then the three launches.  `a` arrives with the
// SUMS fields filled in (or unset, <false> never reads them); everything else is set here.
template <bool SUMS>
int crit_run(const char* fn, CritArgs a, const float* pred, const float* required, const int* path_nodes, const int* path_lens, int maxlen,
             const int* loc_x, const int* loc_y, int map_x, int map_y, const int* paths, const int* row_design, int T, int N, int B,
             float* node_slack, int* node_row, int* node_viol, float* node_crit, float* cell_slack, int* cell_viol, int* counts,
             void* workspace, long long workspace_bytes, int device, void* stream) {
  MMFT_REQUIRE(T >= 1 && T <= (1 << 24) && N >= 1 && B >= 1 && maxlen >= 1,
               "%s: need 1 <= T <= 2^24, N >= 1, B >= 1, maxlen >= 1 (got T %d, N %d, B %d, maxlen %d)", fn, T, N, B, maxlen);
  MMFT_REQUIRE((cell_slack == nullptr) == (cell_viol == nullptr), "%s: cell_slack and cell_viol go together", fn);
  const bool cells = cell_slack != nullptr;
  MMFT_REQUIRE(pred && required && path_nodes && path_lens && paths && node_slack && node_row && node_viol && node_crit && counts &&
                   (!cells || (loc_x && loc_y)),
               "%s: null pointer", fn);
  MMFT_REQUIRE(!cells || mask_map_ok(map_x, map_y),
               "%s: with the cell outputs the map must hold a multiple of 64 cells, at most %d (got %d x %d)", fn, MASK_MAX_CELLS,
               map_x, map_y);
  const int P = cells ? map_x * map_y : 0;
  if constexpr (SUMS) {
    MMFT_REQUIRE(a.scale_log2 >= 0 && a.scale_log2 <= 30, "%s: scale_log2 must lie in [0, 30] (got %d)", fn, a.scale_log2);
    MMFT_REQUIRE((long long)T * maxlen <= (1ll << 30), "%s: T * maxlen must be at most 2^30 for the sums to fit int64 (got %d * %d)", fn, T,
                 maxlen);
    MMFT_REQUIRE(a.node_nsum && a.design_nsum && a.saturated && a.node_share, "%s: null pointer among the sums", fn);
    MMFT_REQUIRE((a.cell_nsum != nullptr) == cells && (a.cell_share != nullptr) == cells,
                 "%s: cell_nsum and cell_share go together, with cell_slack and cell_viol and not without them", fn);
    MMFT_REQUIRE(((reinterpret_cast<uintptr_t>(a.node_nsum) | reinterpret_cast<uintptr_t>(a.cell_nsum) |
                   reinterpret_cast<uintptr_t>(a.design_nsum)) & 7) == 0,
                 "%s: the int64 outputs must be 8-byte aligned", fn);
  }
  const long long need = crit_workspace_bytes(N, B, P);
  MMFT_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && workspace_bytes >= need,
               "%s: workspace of %lld bytes, 8-byte aligned, needed (got %lld)", fn, need, workspace_bytes);
  DeviceGuard dg(device);
  hipStream_t st = (hipStream_t)stream;
  a.pred = pred; a.required = required; a.path_nodes = path_nodes; a.path_lens = path_lens;
  a.loc_x = loc_x; a.loc_y = loc_y; a.paths = paths; a.row_design = row_design;
  a.maxlen = maxlen; a.map_x = cells ? map_x : 0; a.map_y = cells ? map_y : 0; a.P = P; a.T = T; a.N = N; a.B = B;
  a.node_slack = node_slack; a.node_row = node_row; a.node_viol = node_viol; a.node_crit = node_crit;
  a.cell_slack = cell_slack; a.cell_viol = cell_viol; a.counts = counts;
  char* ws = static_cast<char*>(workspace);
  a.node_key = reinterpret_cast<crit_u64*>(ws);
  a.design_key = reinterpret_cast<unsigned*>(ws + 8ll * N);
  a.cell_key = reinterpret_cast<unsigned*>(ws + 8ll * N + crit_align8(4ll * B));
  const long long BP = (long long)B * P;
  const long long elems = N > BP ? N : BP;
  const long long want = (elems + CRIT_THREADS - 1) / CRIT_THREADS;
  const int grid = (int)(want < CRIT_MAX_GRID ? want : CRIT_MAX_GRID);
  const double sweep_bytes = (SUMS ? 20.0 : 12.0) * N + (SUMS ? 16.0 : 8.0) * BP;
  MMFT_LAUNCH(SUMS ? "crit_init_sums_kernel" : "crit_init_kernel", 0.0, sweep_bytes, crit_init_kernel<SUMS>, dim3(grid), dim3(CRIT_THREADS), st, a);
  int rc = check_launch(fn);
  if (rc) return rc;
  MMFT_LAUNCH(SUMS ? "crit_scatter_sums_kernel" : "crit_scatter_kernel", 0.0, 0.0, crit_scatter_kernel<SUMS>, dim3(T), dim3(CRIT_THREADS), st, a);
  rc = check_launch(fn);
  if (rc) return rc;
  MMFT_LAUNCH(SUMS ? "crit_decode_sums_kernel" : "crit_decode_kernel", 0.0, sweep_bytes + (SUMS ? 16.0 : 12.0) * N + (SUMS ? 4.0 : 0.0) * BP,
              crit_decode_kernel<SUMS>, dim3(grid), dim3(CRIT_THREADS), st, a);
  return check_launch(fn);
}

}  // namespace mmft

using namespace mmft;

extern "C" {

long long mmft_criticality_workspace_bytes(int N, int B, int P) {
  if (!crit_sizes_ok(N, B, P)) {
    set_error("criticality_workspace_bytes: need N >= 1, B >= 1, P == 0 or a multiple of 64 up to %d (got N %d, B %d, P %d)",
              MASK_MAX_CELLS, N, B, P);
    return -1;
  }
  return crit_workspace_bytes(N, B, P);
}

int mmft_criticality(const float* pred, const float* required, const int* path_nodes, const int* path_lens, int maxlen,
                     const int* loc_x, const int* loc_y, int map_x, int map_y, const int* paths, const int* row_design, int T,
                     int N, int B, float* node_slack, int* node_row, int* node_viol, float* node_crit, float* cell_slack,
                     int* cell_viol, int* counts, void* workspace, long long workspace_bytes, int device, void* stream) {
  CritArgs a = {};
  return crit_run<false>("criticality", a, pred, required, path_nodes, path_lens, maxlen, loc_x, loc_y, map_x, map_y, paths, row_design, T, N, B,
                         node_slack, node_row, node_viol, node_crit, cell_slack, cell_viol, counts, workspace, workspace_bytes, device, stream);
}

// the sums accumulate in their outputs, so the workspace is the keyed words of mmft_criticality
long long mmft_criticality_sums_workspace_bytes(int N, int B, int P) {
  if (!crit_sizes_ok(N, B, P)) {
    set_error("criticality_sums_workspace_bytes: need N >= 1, B >= 1, P == 0 or a multiple of 64 up to %d (got N %d, B %d, P %d)",
              MASK_MAX_CELLS, N, B, P);
    return -1;
  }
  return crit_workspace_bytes(N, B, P);
}

int mmft_criticality_sums(const float* pred, const float* required, const int* path_nodes, const int* path_lens, int maxlen,
                          const int* loc_x, const int* loc_y, int map_x, int map_y, const int* paths, const int* row_design, int T,
                          int N, int B, float* node_slack, int* node_row, int* node_viol, float* node_crit, float* cell_slack,
                          int* cell_viol, int* counts, int scale_log2, long long* node_nsum, long long* cell_nsum,
                          long long* design_nsum, int* saturated, float* node_share, float* cell_share, void* workspace,
                          long long workspace_bytes, int device, void* stream) {
  CritArgs a = {};
  a.scale_log2 = scale_log2;
  a.node_nsum = reinterpret_cast<crit_u64*>(node_nsum);
  a.cell_nsum = reinterpret_cast<crit_u64*>(cell_nsum);
  a.design_nsum = reinterpret_cast<crit_u64*>(design_nsum);
  a.saturated = saturated; a.node_share = node_share; a.cell_share = cell_share;
  return crit_run<true>("criticality_sums", a, pred, required, path_nodes, path_lens, maxlen, loc_x, loc_y, map_x, map_y, paths, row_design, T, N,
                        B, node_slack, node_row, node_viol, node_crit, cell_slack, cell_viol, counts, workspace, workspace_bytes, device, stream);
}

}  // extern "C"
