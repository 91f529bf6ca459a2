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
//                        and - with the cell outputs - the row's mask as a bitmap in LDS
//                        (the box loop of placed_fc_fwd_kernel, place.hip, restated here: ~35 lines duplicated, so that that
//                        kernel stays byte for byte what it is), then one atomic per set bit, a wave on the 64 consecutive
//                        cells of one bitmap block at a time, empty blocks skipped
//                        The designs' minima and row counts come from the first T / 1024 workgroups, each for 1024 rows,
//                        combined in LDS (crit_design_words)
//   crit_decode_kernel   keyed words -> node_slack / node_row / node_crit, cell_slack
#include "common.h"
#include "slack_key.h"
#include "../../include/mmft_crit.h"

namespace mmft {

typedef unsigned long long crit_u64;

constexpr int CRIT_THREADS = 256;
constexpr int CRIT_MAX_CELLS = 65536;         // bitmap 8 KB in LDS: the limit of mmft_placed_fc_fwd
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
};

__global__ void __launch_bounds__(CRIT_THREADS) crit_init_kernel(CritArgs a) {
  const long long BP = (long long)a.B * a.P;
  const long long n = a.N > BP ? a.N : BP;    // (2 B <= N or B P is not promised: the design words have a loop of their own)
  const long long step = (long long)gridDim.x * CRIT_THREADS;
  for (long long i = (long long)blockIdx.x * CRIT_THREADS + threadIdx.x; i < n; i += step) {
    if (i < a.N) {
      a.node_key[i] = CRIT_NONE64;
      a.node_viol[i] = 0;
    }
    if (i < BP) {
      a.cell_key[i] = CRIT_NONE32;
      a.cell_viol[i] = 0;
    }
  }
  for (long long i = (long long)blockIdx.x * CRIT_THREADS + threadIdx.x; i < a.B; i += step) {
    a.design_key[i] = CRIT_NONE32;
    a.counts[2 * i] = 0;
    a.counts[2 * i + 1] = 0;
  }
}

// The per-design words of the rows [blockIdx.x * CRIT_ROWS, ... + CRIT_ROWS): valid and NaN counts and the smallest key.  One
// atomic per row on a handful of addresses serialises in L2 (measured: 10 800 rows on 8 designs cost 0.1 ms), so
// the rows meet in LDS first - designs below CRIT_LDS_DESIGNS; the others go to memory directly - and a block sends at most
// three atomics per design.  lds: 3 * CRIT_LDS_DESIGNS words, free again when this returns.
__device__ void crit_design_words(const CritArgs& a, unsigned* lds) {
  const int tid = threadIdx.x;
  unsigned* s_min = lds;
  unsigned* s_valid = lds + CRIT_LDS_DESIGNS;
  unsigned* s_nan = lds + 2 * CRIT_LDS_DESIGNS;
  for (int d = tid; d < CRIT_LDS_DESIGNS; d += CRIT_THREADS) {
    s_min[d] = CRIT_NONE32;
    s_valid[d] = 0u;
    s_nan[d] = 0u;
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
  }
  __syncthreads();
  for (int d = tid; d < CRIT_LDS_DESIGNS && d < a.B; d += CRIT_THREADS) {
    if (s_valid[d]) {
      atomicAdd(a.counts + 2 * d, (int)s_valid[d]);
      atomicMin(a.design_key + d, s_min[d]);
    }
    if (s_nan[d]) atomicAdd(a.counts + 2 * d + 1, (int)s_nan[d]);
  }
  __syncthreads();
}

__global__ void __launch_bounds__(CRIT_THREADS) crit_scatter_kernel(CritArgs a) {
  __shared__ unsigned bits[CRIT_MAX_CELLS / 32];
  __shared__ int pin_x[256], pin_y[256];
  const int t = blockIdx.x, tid = threadIdx.x;
  // the first T / CRIT_ROWS (rounded up) workgroups also carry a slice of the per-design words (the grid has T workgroups)
  if ((long long)blockIdx.x * CRIT_ROWS < a.T) crit_design_words(a, bits);
  const int b = a.row_design ? a.row_design[t] : 0;
  if ((unsigned)b >= (unsigned)a.B) return;                                // (not promised to be checked; nothing is indexed by it)
  const float s = slack_of(a.required[t], a.pred[t]);
  if (s != s) return;                                                      // the same for every thread of the row
  const unsigned key = ordered_bits(s);
  const bool viol = s < 0.f;
  const int q = a.paths[t];
  const int* path = a.path_nodes + (long long)q * a.maxlen;
  const int len = a.path_lens[q] < a.maxlen ? a.path_lens[q] : a.maxlen;   // the same for every thread: the barriers below are uniform
  // ---- the pins: one 64-bit minimum per live position
  const crit_u64 word = ((crit_u64)key << 32) | (unsigned)t;
  for (int j = tid; j < len; j += CRIT_THREADS) {
    const int n = path[j];
    if ((unsigned)n >= (unsigned)a.N) continue;                            // outside the contract; never written through
    atomicMin(a.node_key + n, word);
    if (viol) atomicAdd(a.node_viol + n, 1);
  }
  if (a.P == 0) return;
  // ---- the mask: the union of boxes as placed_fc_fwd_kernel (place.hip) builds it - THE MASK RULE of mmft_place.h
  const int map_x = a.map_x, map_y = a.map_y, words = a.P >> 5, nblk = a.P >> 6;
  if (len < 2) return;                                                     // an empty mask
  for (int w = tid; w < words; w += CRIT_THREADS) bits[w] = 0u;
  for (int j0 = 0; j0 + 1 < len; j0 += 255) {                              // chunks overlap by the node two boxes share
    const int n = len - j0 < 256 ? len - j0 : 256;
    __syncthreads();                                                       // bitmap zeroed / the previous chunk's boxes read
    if (tid < n) {
      int p = path[j0 + tid];
      p = p < 0 ? 0 : (p >= a.N ? a.N - 1 : p);                            // outside the contract; never read through
      pin_x[tid] = a.loc_x[p];
      pin_y[tid] = a.loc_y[p];
    }
    __syncthreads();
    for (int j = 0; j + 1 < n; ++j) {
      int xa = pin_x[j], ya = pin_y[j], xb = pin_x[j + 1], yb = pin_y[j + 1];
      int x1 = xa < xb ? xa : xb, x2 = xa < xb ? xb : xa;
      int y1 = ya < yb ? ya : yb, y2 = ya < yb ? yb : ya;
      x1 = x1 < 0 ? 0 : x1;
      y1 = y1 < 0 ? 0 : y1;
      x2 = x2 >= map_x ? map_x - 1 : x2;
      y2 = y2 >= map_y ? map_y - 1 : y2;
      int w = y2 - y1 + 1, hgt = x2 - x1 + 1;
      if (w <= 0 || hgt <= 0) continue;
      // a box row is the contiguous bit range [x * map_y + y1, x * map_y + y2]: whole-word masks, not one atomic per cell
      const int wpr = ((w + 30) >> 5) + 1;                                 // words a row's range can touch
      for (int c = tid; c < hgt * wpr; c += CRIT_THREADS) {
        int row = c / wpr, k = c - row * wpr;
        int lo = (x1 + row) * map_y + y1, hi = lo + w - 1;                 // inclusive bit range, inside [0, P) after the clamps
        int wd = (lo >> 5) + k;
        if (wd > (hi >> 5)) continue;
        int b0 = wd == (lo >> 5) ? (lo & 31) : 0;
        int b1 = wd == (hi >> 5) ? (hi & 31) : 31;
        unsigned mask = (b1 == 31 ? 0xffffffffu : ((1u << (b1 + 1)) - 1u)) & ~((1u << b0) - 1u);
        atomicOr(&bits[wd], mask);
      }
    }
  }
  __syncthreads();
  // ---- the cells: wave w takes the blocks w, w + 4, ... of 64 consecutive cells, lane l the cell l of the block
  const int lane = tid & 63, wave = tid >> 6;
  unsigned* ck = a.cell_key + (long long)b * a.P;
  int* cv = a.cell_viol + (long long)b * a.P;
  for (int blk = wave; blk < nblk; blk += CRIT_THREADS / 64) {
    const unsigned lo = bits[2 * blk], hi = bits[2 * blk + 1];
    if ((lo | hi) == 0u) continue;                                         // wave-uniform
    if (((lane < 32 ? lo : hi) >> (lane & 31)) & 1u) {
      const int c = (blk << 6) + lane;
      atomicMin(ck + c, key);
      if (viol) atomicAdd(cv + c, 1);
    }
  }
}

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
    }
    if (i < BP) {
      const unsigned key = a.cell_key[i];
      a.cell_slack[i] = key == CRIT_NONE32 ? inf : ordered_float(key);
    }
  }
}

inline long long crit_align8(long long v) { return (v + 7) & ~7ll; }
inline bool crit_sizes_ok(int N, int B, int P) {
  return N >= 1 && B >= 1 && (P == 0 || (P > 0 && P % 64 == 0 && P <= CRIT_MAX_CELLS));
}

}  // namespace mmft

using namespace mmft;

extern "C" {

long long mmft_criticality_workspace_bytes(int N, int B, int P) {
  if (!crit_sizes_ok(N, B, P)) {
    set_error("criticality_workspace_bytes: need N >= 1, B >= 1, P == 0 or a multiple of 64 up to %d (got N %d, B %d, P %d)",
              CRIT_MAX_CELLS, N, B, P);
    return -1;
  }
  return 8ll * N + crit_align8(4ll * B) + 4ll * B * P;
}

int mmft_criticality(const float* pred, const float* required, const int* path_nodes, const int* path_lens, int maxlen,
                     const int* loc_x, const int* loc_y, int map_x, int map_y, const int* paths, const int* row_design, int T,
                     int N, int B, float* node_slack, int* node_row, int* node_viol, float* node_crit, float* cell_slack,
                     int* cell_viol, int* counts, void* workspace, long long workspace_bytes, int device, void* stream) {
  MMFT_REQUIRE(T >= 1 && T <= (1 << 24) && N >= 1 && B >= 1 && maxlen >= 1,
               "criticality: need 1 <= T <= 2^24, N >= 1, B >= 1, maxlen >= 1 (got T %d, N %d, B %d, maxlen %d)", T, N, B, maxlen);
  MMFT_REQUIRE((cell_slack == nullptr) == (cell_viol == nullptr), "criticality: cell_slack and cell_viol go together");
  const bool cells = cell_slack != nullptr;
  MMFT_REQUIRE(pred && required && path_nodes && path_lens && paths && node_slack && node_row && node_viol && node_crit && counts &&
                   (!cells || (loc_x && loc_y)),
               "criticality: null pointer");
  MMFT_REQUIRE(!cells || (map_x > 0 && map_y > 0 && (long long)map_x * map_y <= CRIT_MAX_CELLS && ((long long)map_x * map_y) % 64 == 0),
               "criticality: with the cell outputs the map must hold a multiple of 64 cells, at most %d (got %d x %d)", CRIT_MAX_CELLS,
               map_x, map_y);
  const int P = cells ? map_x * map_y : 0;
  const long long need = mmft_criticality_workspace_bytes(N, B, P);
  MMFT_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && workspace_bytes >= need,
               "criticality: workspace of %lld bytes, 8-byte aligned, needed (got %lld)", need, workspace_bytes);
  DeviceGuard dg(device);
  hipStream_t st = (hipStream_t)stream;
  CritArgs a;
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
  const double sweep_bytes = 12.0 * N + 8.0 * BP;
  MMFT_LAUNCH("crit_init_kernel", 0.0, sweep_bytes, crit_init_kernel, dim3(grid), dim3(CRIT_THREADS), st, a);
  int rc = check_launch("criticality (init)");
  if (rc) return rc;
  MMFT_LAUNCH("crit_scatter_kernel", 0.0, 0.0, crit_scatter_kernel, dim3(T), dim3(CRIT_THREADS), st, a);
  rc = check_launch("criticality (scatter)");
  if (rc) return rc;
  MMFT_LAUNCH("crit_decode_kernel", 0.0, sweep_bytes + 12.0 * N, crit_decode_kernel, dim3(grid), dim3(CRIT_THREADS), st, a);
  return check_launch("criticality");
}

}  // extern "C"
