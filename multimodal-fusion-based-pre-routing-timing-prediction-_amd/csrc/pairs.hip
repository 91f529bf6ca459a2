// Near pairs of a search plan's groups and their swap tables (include/mmft_pairs.h).
//
// near_kernel<FILL>: one thread per group a, 256 per workgroup.  The partners b are walked in tiles of 1024 whose anchors,
// sizes and classes the workgroup stages in LDS once - the walk mv_ptr -> mv_node -> loc is made per staged partner, four
// independent chains per thread and tile, never per tested pair -, and the inner loop reads them at one address for the
// whole wave (a broadcast), four tests at a time with their verdicts kept as bits.  The work per a is triangular (b > a):
// workgroup w takes the blocks w and nblk - 1 - w of 256 groups, whose partner counts add up to the same G + 256 for every w.  FILL == false counts, FILL == true writes the pairs
// of a from off[a] on in ascending b: the order of the output is that of the tables.
// scan_kernel: one workgroup of 1024 threads, rounds of 4096 elements; the prefix in wrapping 32-bit words, the total apart
// in 64 bits.
// rows_count_kernel / rows_fill_kernel: one wave per pair.  Each lane takes one row of one list and finds it in the other by
// binary search; shared rows are counted by ballot, and a row's rank in the union is its index plus the other list's rows
// below it less the shared rows before it.
#include "common.h"
#include "../../include/mmft_pairs.h"

namespace mmft {

constexpr int NEAR_BLOCK = 256;        // groups a per workgroup, one per thread
constexpr int NEAR_TILE = 1024;        // partners staged per round: 16 KiB of LDS
constexpr int NEAR_BATCH = 4;         // tests whose LDS reads are issued together
constexpr int NEAR_NONE = 65;          // the size of a group that pairs with nothing: 65 + (any size >= 1) > 64
constexpr int SCAN_BLOCK = 1024;
constexpr int SCAN_ITEMS = 4;

struct NearArgs {
  const int* mv_ptr;
  const int* mv_node;
  const int* loc_x;
  const int* loc_y;
  const int* klass;
  const int* off;
  int* cnt;
  int* pair_a;
  int* pair_b;
  int G, M, n_nodes, reach, K;
};

// the anchor's coordinates, the size and the class of group g; NEAR_NONE as the size of a group that takes part in no pair
__device__ __forceinline__ void near_group(const NearArgs& a, int g, int& x, int& y, int& size, int& klass) {
  x = y = klass = 0;
  size = NEAR_NONE;
  if (g >= a.G) return;
  const int m0 = clamp_to(a.mv_ptr[g], a.M), m1 = clamp_to(a.mv_ptr[g + 1], a.M);
  if (m1 <= m0) return;
  const int A = a.mv_node[m0];
  if ((unsigned)A >= (unsigned)a.n_nodes) return;
  x = a.loc_x[A];
  y = a.loc_y[A];
  size = m1 - m0 > 64 ? NEAR_NONE : m1 - m0;
  klass = a.klass ? a.klass[g] : 0;
}

template <bool FILL>
__global__ void __launch_bounds__(NEAR_BLOCK) near_kernel(NearArgs a) {
  __shared__ int4 s_tile[NEAR_TILE];                    // x, y, size, class of a partner: one 16-byte LDS read per test
  const int tid = threadIdx.x;
  const int nblk = (a.G + NEAR_BLOCK - 1) / NEAR_BLOCK;
  const long long reach = a.reach;
  for (int half = 0; half < 2; ++half) {                // the same for every thread of the workgroup
    const int blk = half == 0 ? (int)blockIdx.x : nblk - 1 - (int)blockIdx.x;
    if (half == 1 && blk <= (int)blockIdx.x) break;     // the middle block of an odd count: done already
    const int first = blk * NEAR_BLOCK, g = first + tid;
    int ax, ay, sa, ka;
    near_group(a, g, ax, ay, sa, ka);
    int n = 0;
    long long pos = FILL && g < a.G ? a.off[g] : 0;
    for (int t0 = first / NEAR_TILE * NEAR_TILE; t0 < a.G; t0 += NEAR_TILE) {
      __syncthreads();                                  // the tile before is read no more
      for (int j = tid; j < NEAR_TILE; j += NEAR_BLOCK) {
        int4 q;
        near_group(a, t0 + j, q.x, q.y, q.z, q.w);
        s_tile[j] = q;
      }
      __syncthreads();
      const int hi = a.G - t0 < NEAR_TILE ? a.G - t0 : NEAR_TILE;
      const int lo = first + 1 > t0 ? first + 1 - t0 : 0;      // no b at or below the block's first a
      for (int j = lo; j < hi; j += NEAR_BATCH) {
        // a batch of tests first, their verdicts as bits, the stores after: every term of a test is formed, none behind a
        // branch on another, so the batch's 16-byte LDS reads (one address per wave and read: a broadcast) go out
        // together - a short-circuit chain waited for the LDS once per term, a store per test once per test
        unsigned hits = 0;
#pragma unroll
        for (int u = 0; u < NEAR_BATCH; ++u) {
          const int jj = j + u;
          const int4 q = s_tile[jj < NEAR_TILE ? jj : NEAR_TILE - 1];
          const long long dx = (long long)ax - q.x, dy = (long long)ay - q.y;
          const long long mx = dx < 0 ? -dx : dx, my = dy < 0 ? -dy : dy;
          const long long d = mx > my ? mx : my;
          const bool near = (jj < hi) & (t0 + jj > g) & (sa + q.z <= 64) & (ka == q.w) & (d >= 1) & (d <= reach);
          hits |= (near ? 1u : 0u) << u;
        }
        if (FILL) {
          while (hits) {                                // ascending b
            const int b = t0 + j + __ffs((int)hits) - 1;
            hits &= hits - 1;
            if ((unsigned long long)pos < (unsigned long long)a.K) {
              a.pair_a[pos] = g;
              a.pair_b[pos] = b;
            }
            ++pos;
          }
        } else {
          n += __popc(hits);
        }
      }
    }
    if (!FILL && g < a.G) a.cnt[g] = n;
  }
}

__global__ void __launch_bounds__(SCAN_BLOCK) scan_kernel(const int* __restrict__ in, int n, int* __restrict__ out,
                                                          long long* __restrict__ total) {
  __shared__ unsigned s_wave[SCAN_BLOCK / 64];
  __shared__ long long s_total[SCAN_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned carry = 0;                                   // the low word of the sum of the rounds before: the same for every thread
  long long mine = 0;                                   // the exact sum of this thread's elements
  for (long long base = 0; base < n; base += SCAN_BLOCK * SCAN_ITEMS) {
    const long long i0 = base + (long long)SCAN_ITEMS * tid;
    unsigned v[SCAN_ITEMS], sum = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      const int w = i0 + j < n ? in[i0 + j] : 0;
      v[j] = (unsigned)w;
      sum += (unsigned)w;
      mine += w;
    }
    unsigned inc = sum;                                 // inclusive over the lanes of the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    unsigned before = carry, round = 0;
#pragma unroll
    for (int w = 0; w < SCAN_BLOCK / 64; ++w) {
      const unsigned s = s_wave[w];
      before += w < wave ? s : 0u;
      round += s;
    }
    unsigned run = before + inc - sum;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
      if (i0 + j < n) out[i0 + j] = (int)run;
      run += v[j];
    }
    carry += round;
    __syncthreads();                                    // s_wave is written again in the next round
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mine += __shfl_down(mine, d);
  if (lane == 0) s_total[wave] = mine;
  __syncthreads();
  if (tid == 0) {
    long long t = 0;
    for (int w = 0; w < SCAN_BLOCK / 64; ++w) t += s_total[w];
    total[0] = t;
    out[n] = (int)carry;
  }
}

// the first index in v[0 .. n) whose element is not below key; v ascending
__device__ __forceinline__ int rows_lower_bound(const int* __restrict__ v, int n, int key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the rows of group g: a group outside [0, G) holds none
__device__ __forceinline__ const int* rows_of_group(const int* __restrict__ grow_ptr, const int* __restrict__ grow_row, int g, int G, int R,
                                                    int& n) {
  n = 0;
  if ((unsigned)g >= (unsigned)G) return grow_row;
  const int r0 = clamp_to(grow_ptr[g], R), r1 = clamp_to(grow_ptr[g + 1], R);
  n = r1 > r0 ? r1 - r0 : 0;
  return grow_row + r0;
}

__global__ void __launch_bounds__(256) rows_count_kernel(const int* __restrict__ pair_a, const int* __restrict__ pair_b, int K,
                                                         const int* __restrict__ grow_ptr, const int* __restrict__ grow_row, int G,
                                                         int R, int* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const long long k = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);        // the same for the lanes of a wave
  if (k >= K) return;
  int na, nb;
  const int* ra = rows_of_group(grow_ptr, grow_row, pair_a[k], G, R, na);
  const int* rb = rows_of_group(grow_ptr, grow_row, pair_b[k], G, R, nb);
  int shared = 0;
  for (int i0 = 0; i0 < na; i0 += 64) {
    const int i = i0 + lane;
    bool both = false;
    if (i < na) {
      const int key = ra[i], at = rows_lower_bound(rb, nb, key);
      both = at < nb && rb[at] == key;
    }
    shared += __popcll(__ballot(both));
  }
  if (lane == 0) cnt[k] = na + nb - shared;
}

struct RowsFillArgs {
  const int* pair_a;
  const int* pair_b;
  const int* prow_ptr;
  const int* grow_ptr;
  const int* grow_row;
  int* prow_row;
  int* prow_pair;
  int* sel_ptr;
  int* sel_row;
  int K, RP, G, R, T;
};

// the rows of `mine` that survive into the union, each at its rank: all of them (KEEP_SHARED, list a) or those the other
// list does not hold (list b)
template <bool KEEP_SHARED>
__device__ __forceinline__ void rows_place(const RowsFillArgs& a, const int* __restrict__ mine, int n_mine, const int* __restrict__ other,
                                           int n_other, int k, int e0, int s0, int slots, int lane) {
  int before = 0;                                       // the shared rows among mine[0 .. i0): the same for the lanes of a wave
  for (int i0 = 0; i0 < n_mine; i0 += 64) {
    const int i = i0 + lane;
    bool both = false;
    int key = 0, at = 0;
    if (i < n_mine) {
      key = mine[i];
      at = rows_lower_bound(other, n_other, key);
      both = at < n_other && other[at] == key;
    }
    const unsigned long long mask = __ballot(both);
    if (i < n_mine && (KEEP_SHARED || !both)) {
      const int rank = i + at - before - __popcll(mask & ((1ull << lane) - 1ull));
      if ((unsigned)rank < (unsigned)slots) {
        a.prow_row[e0 + rank] = key;
        a.prow_pair[e0 + rank] = k;
        a.sel_row[s0 + rank] = key;
      }
    }
    before += __popcll(mask);
  }
}

__global__ void __launch_bounds__(256) rows_fill_kernel(RowsFillArgs a) {
  const int lane = threadIdx.x & 63;
  const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);     // the same for the lanes of a wave
  if (item > a.K) return;
  const int k = (int)item;
  const int e0 = clamp_to(a.prow_ptr[k], a.RP);
  const int s0 = e0 + 2 * k;                            // RP + 2 K < 2^31
  if (lane == 0) a.sel_ptr[k] = s0;
  if (k == a.K) return;                                 // the wave behind the last pair closes sel_ptr
  const int e1 = clamp_to(a.prow_ptr[k + 1], a.RP);
  const int slots = e1 > e0 ? e1 - e0 : 0;
  const int ga = a.pair_a[k], gb = a.pair_b[k];
  int na, nb;
  const int* ra = rows_of_group(a.grow_ptr, a.grow_row, ga, a.G, a.R, na);
  const int* rb = rows_of_group(a.grow_ptr, a.grow_row, gb, a.G, a.R, nb);
  rows_place<true>(a, ra, na, rb, nb, k, e0, s0, slots, lane);
  rows_place<false>(a, rb, nb, ra, na, k, e0, s0, slots, lane);
  if (lane == 0) {
    a.sel_row[s0 + slots] = a.T + ga;
    a.sel_row[s0 + slots + 1] = a.T + gb;
  }
}

static int near_sizes(const char* who, int G, int M, int n_nodes, int reach) {
  MMFT_REQUIRE(G >= 1 && G <= (1 << 24) && M >= 0 && n_nodes >= 1, "%s: need 1 <= G <= 2^24, M >= 0, n_nodes >= 1 (got %d, %d, %d)", who, G, M,
               n_nodes);
  MMFT_REQUIRE(reach >= 1, "%s: reach must be at least 1 (got %d)", who, reach);
  return MMFT_OK;
}

static NearArgs near_args(const int* mv_ptr, const int* mv_node, int G, int M, const int* loc_x, const int* loc_y, int n_nodes,
                          const int* klass, int reach) {
  NearArgs a = {};
  a.mv_ptr = mv_ptr; a.mv_node = mv_node; a.loc_x = loc_x; a.loc_y = loc_y; a.klass = klass;
  a.G = G; a.M = M; a.n_nodes = n_nodes; a.reach = reach;
  return a;
}

static unsigned near_grid(int G) { return (unsigned)((cdiv(G, NEAR_BLOCK) + 1) / 2); }

}  // namespace mmft

using namespace mmft;

extern "C" {

int mmft_pairs_near_count(const int* mv_ptr, const int* mv_node, int G, int M, const int* loc_x, const int* loc_y, int n_nodes,
                          const int* klass, int reach, int* cnt, int device, void* stream) {
  int rc = near_sizes("pairs_near_count", G, M, n_nodes, reach);
  if (rc) return rc;
  MMFT_REQUIRE(mv_ptr && (mv_node || M == 0) && loc_x && loc_y && cnt, "pairs_near_count: null pointer");
  NearArgs a = near_args(mv_ptr, mv_node, G, M, loc_x, loc_y, n_nodes, klass, reach);
  a.cnt = cnt;
  DeviceGuard dg(device);
  MMFT_LAUNCH("pairs_near_count_kernel", 0.0, 16.0 * (double)G, near_kernel<false>, dim3(near_grid(G)), dim3(NEAR_BLOCK), (hipStream_t)stream, a);
  return check_launch("pairs_near_count");
}

int mmft_pairs_scan(const int* in, int n, int* out, long long* total, int device, void* stream) {
  MMFT_REQUIRE(n >= 0, "pairs_scan: n must not be negative (got %d)", n);
  if (n == 0) return MMFT_OK;
  MMFT_REQUIRE(in && out && total, "pairs_scan: null pointer");
  MMFT_REQUIRE(aligned8(total), "pairs_scan: total must be 8-byte aligned");
  const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), o0 = reinterpret_cast<uintptr_t>(out);
  MMFT_REQUIRE(i0 + 4ull * (unsigned)n <= o0 || o0 + 4ull * ((unsigned)n + 1ull) <= i0, "pairs_scan: in and out overlap");
  DeviceGuard dg(device);
  MMFT_LAUNCH("pairs_scan_kernel", 0.0, 8.0 * (double)n, scan_kernel, dim3(1), dim3(SCAN_BLOCK), (hipStream_t)stream, in, n, out, total);
  return check_launch("pairs_scan");
}

int mmft_pairs_near_fill(const int* mv_ptr, const int* mv_node, int G, int M, const int* loc_x, const int* loc_y, int n_nodes,
                         const int* klass, int reach, const int* off, int K, int* pair_a, int* pair_b, int device, void* stream) {
  int rc = near_sizes("pairs_near_fill", G, M, n_nodes, reach);
  if (rc) return rc;
  MMFT_REQUIRE(K >= 0, "pairs_near_fill: K must not be negative (got %d)", K);
  if (K == 0) return MMFT_OK;
  MMFT_REQUIRE(mv_ptr && (mv_node || M == 0) && loc_x && loc_y && off && pair_a && pair_b, "pairs_near_fill: null pointer");
  NearArgs a = near_args(mv_ptr, mv_node, G, M, loc_x, loc_y, n_nodes, klass, reach);
  a.off = off; a.K = K; a.pair_a = pair_a; a.pair_b = pair_b;
  DeviceGuard dg(device);
  MMFT_LAUNCH("pairs_near_fill_kernel", 0.0, 16.0 * (double)G + 8.0 * (double)K, near_kernel<true>, dim3(near_grid(G)), dim3(NEAR_BLOCK),
              (hipStream_t)stream, a);
  return check_launch("pairs_near_fill");
}

int mmft_pairs_rows_count(const int* pair_a, const int* pair_b, int K, const int* grow_ptr, const int* grow_row, int G, int R, int* cnt,
                          int device, void* stream) {
  MMFT_REQUIRE(K >= 0 && G >= 1 && R >= 0, "pairs_rows_count: need K >= 0, G >= 1, R >= 0 (got %d, %d, %d)", K, G, R);
  if (K == 0) return MMFT_OK;
  MMFT_REQUIRE(pair_a && pair_b && grow_ptr && (grow_row || R == 0) && cnt, "pairs_rows_count: null pointer");
  DeviceGuard dg(device);
  MMFT_LAUNCH("pairs_rows_count_kernel", 0.0, 12.0 * (double)K, rows_count_kernel, dim3((unsigned)cdiv(K, 4)), dim3(256), (hipStream_t)stream,
              pair_a, pair_b, K, grow_ptr, grow_row, G, R, cnt);
  return check_launch("pairs_rows_count");
}

int mmft_pairs_rows_fill(const int* pair_a, const int* pair_b, const int* prow_ptr, int K, int RP, const int* grow_ptr, const int* grow_row,
                         int G, int R, int T, int* prow_row, int* prow_pair, int* sel_ptr, int* sel_row, int device, void* stream) {
  MMFT_REQUIRE(K >= 0 && RP >= 0 && G >= 1 && R >= 0 && T >= 1, "pairs_rows_fill: need K >= 0, RP >= 0, G >= 1, R >= 0, T >= 1 (got %d, %d, %d, %d, %d)",
               K, RP, G, R, T);
  MMFT_REQUIRE((long long)RP + 2ll * K < (1ll << 31), "pairs_rows_fill: RP + 2 K = %lld does not stay below 2^31", (long long)RP + 2ll * K);
  MMFT_REQUIRE((long long)T + G <= (1 << 24), "pairs_rows_fill: T + G = %lld rows of the selection exceed 2^24", (long long)T + G);
  if (K == 0) return MMFT_OK;
  MMFT_REQUIRE(pair_a && pair_b && prow_ptr && grow_ptr && (grow_row || R == 0) && ((prow_row && prow_pair) || RP == 0) && sel_ptr && sel_row,
               "pairs_rows_fill: null pointer");
  RowsFillArgs a;
  a.pair_a = pair_a; a.pair_b = pair_b; a.prow_ptr = prow_ptr; a.grow_ptr = grow_ptr; a.grow_row = grow_row;
  a.prow_row = prow_row; a.prow_pair = prow_pair; a.sel_ptr = sel_ptr; a.sel_row = sel_row;
  a.K = K; a.RP = RP; a.G = G; a.R = R; a.T = T;
  DeviceGuard dg(device);
  MMFT_LAUNCH("pairs_rows_fill_kernel", 0.0, 12.0 * (double)K + 12.0 * (double)RP, rows_fill_kernel, dim3((unsigned)cdiv((long long)K + 1, 4)),
              dim3(256), (hipStream_t)stream, a);
  return check_launch("pairs_rows_fill");
}

}  // extern "C"
