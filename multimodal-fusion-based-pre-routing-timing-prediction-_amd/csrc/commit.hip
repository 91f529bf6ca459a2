// Commit a conflict-free set of best moves (include/mmft_commit.h).
//
// commit_select_kernel: ONE workgroup of 1024 threads picks the lexicographically first maximal independent set of the
// candidates under the key (best_dq, g), in rounds.  `sel` is the state on the way (0 dead or no candidate, 1 taken, 2 live);
// the row-owner table lives in global memory and is touched only through relaxed agent-scope atomics (loads and stores that
// go past L1), with every wave's memory operations drained before each barrier.
// commit_apply_kernel: one wave per selected group moves its pins by the group's best offset (THE WINDOW and THE MOVE RULE,
// move_rule.h).
#include "common.h"
#include "move_rule.h"
#include "../../include/mmft_commit.h"

namespace mmft {

constexpr int COMMIT_THREADS = 1024;
constexpr long long COMMIT_NO_BID = 0x7fffffffffffffffll;
constexpr int COMMIT_NO_GROUP = 0x7fffffff;
enum { COMMIT_DEAD = 0, COMMIT_TAKEN = 1, COMMIT_LIVE = 2 };

template <typename V>
__device__ __forceinline__ V commit_ld(const V* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename V>
__device__ __forceinline__ void commit_st(V* p, V v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename V>
__device__ __forceinline__ void commit_min(V* p, V v) {
  (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// every store and atomic of this wave has reached L2 before the wave arrives
__device__ __forceinline__ void commit_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void commit_barrier() {
  commit_drain();
  __syncthreads();
}

// f(r) for every row r in [0, T) among the entries of group g
template <typename F>
__device__ __forceinline__ void commit_rows_of(const int* __restrict__ grow_ptr, const int* __restrict__ grow_row, int g, int R, int T, F f) {
  const int e1 = clamp_to(grow_ptr[g + 1], R);
  for (int e = clamp_to(grow_ptr[g], R); e < e1; ++e) {
    const int r = grow_row[e];
    if ((unsigned)r < (unsigned)T) f(r);
  }
}

__global__ void __launch_bounds__(COMMIT_THREADS) commit_select_kernel(const int* __restrict__ best_w, const long long* __restrict__ best_dq,
                                                                       int G, int centre, const int* __restrict__ grow_ptr,
                                                                       const int* __restrict__ grow_row, int R, int T, long long min_q,
                                                                       int* sel, long long* stats, long long* own_q, int* own_g) {
  __shared__ unsigned long long s_sum[3];                // selected, the sum of their best_dq (two's complement), candidates
  const int tid = threadIdx.x;
  if (tid < 3) s_sum[tid] = 0ull;
  unsigned long long n_sel = 0ull, sum = 0ull, n_cand = 0ull;
  const auto clear = [&](int r) {
    commit_st(own_q + r, COMMIT_NO_BID);
    commit_st(own_g + r, COMMIT_NO_GROUP);
  };
  int live = 0;
  // the candidates, and their rows cleared
  for (int g = tid; g < G; g += COMMIT_THREADS) {
    const int w = best_w[g];
    const bool cand = w >= 0 && w != centre && best_dq[g] <= -min_q;
    commit_st(sel + g, cand ? (int)COMMIT_LIVE : (int)COMMIT_DEAD);
    if (!cand) continue;
    ++n_cand;
    live = 1;
    commit_rows_of(grow_ptr, grow_row, g, R, T, clear);
  }
  int rounds = 0;
  commit_drain();
  // the smallest live key is taken in every round: no more than G rounds (the bound is never the one that ends the loop)
  while (__syncthreads_or(live) && rounds < G) {
    ++rounds;
    // 1. the smallest best_dq among the live candidates of each row
    for (int g = tid; g < G; g += COMMIT_THREADS) {
      if (commit_ld(sel + g) != COMMIT_LIVE) continue;
      const long long q = best_dq[g];
      commit_rows_of(grow_ptr, grow_row, g, R, T, [&](int r) { commit_min(own_q + r, q); });
    }
    commit_barrier();
    // 2. the smallest g among those that hold it
    for (int g = tid; g < G; g += COMMIT_THREADS) {
      if (commit_ld(sel + g) != COMMIT_LIVE) continue;
      const long long q = best_dq[g];
      commit_rows_of(grow_ptr, grow_row, g, R, T, [&](int r) {
        if (commit_ld(own_q + r) == q) commit_min(own_g + r, g);
      });
    }
    commit_barrier();
    // 3. a candidate that owns all its rows is taken
    for (int g = tid; g < G; g += COMMIT_THREADS) {
      if (commit_ld(sel + g) != COMMIT_LIVE) continue;
      int lost = 0;
      commit_rows_of(grow_ptr, grow_row, g, R, T, [&](int r) { lost |= commit_ld(own_g + r) != g; });
      if (!lost) {
        commit_st(sel + g, (int)COMMIT_TAKEN);
        ++n_sel;
        sum += (unsigned long long)best_dq[g];
      }
    }
    commit_barrier();
    // 4. a live candidate that finds a taken owner on one of its rows dies (nobody reads a state but for `taken` here)
    for (int g = tid; g < G; g += COMMIT_THREADS) {
      if (commit_ld(sel + g) != COMMIT_LIVE) continue;
      int hit = 0;
      commit_rows_of(grow_ptr, grow_row, g, R, T, [&](int r) {
        const int o = commit_ld(own_g + r);
        if ((unsigned)o < (unsigned)G) hit |= commit_ld(sel + o) == COMMIT_TAKEN;
      });
      if (hit) commit_st(sel + g, (int)COMMIT_DEAD);
    }
    commit_barrier();
    // 5. the survivors clear their rows for the next round
    live = 0;
    for (int g = tid; g < G; g += COMMIT_THREADS) {
      if (commit_ld(sel + g) != COMMIT_LIVE) continue;
      live = 1;
      commit_rows_of(grow_ptr, grow_row, g, R, T, clear);
    }
    commit_drain();
  }
  // whoever the bound on the rounds left alive (nobody, see above) is not selected
  for (int g = tid; g < G; g += COMMIT_THREADS)
    if (commit_ld(sel + g) == COMMIT_LIVE) commit_st(sel + g, (int)COMMIT_DEAD);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n_sel += __shfl_xor(n_sel, o, 64);
    sum += __shfl_xor(sum, o, 64);
    n_cand += __shfl_xor(n_cand, o, 64);
  }
  if ((tid & 63) == 0) {                                 // integer adds in LDS: the order of the waves does not show
    atomicAdd(&s_sum[0], n_sel);
    atomicAdd(&s_sum[1], sum);
    atomicAdd(&s_sum[2], n_cand);
  }
  __syncthreads();
  if (tid < 3) stats[tid] = (long long)s_sum[tid];
  if (tid == 3) stats[3] = rounds;
}

__global__ void __launch_bounds__(256) commit_apply_kernel(int* __restrict__ loc_x, int* __restrict__ loc_y, int n_nodes,
                                                           const int* __restrict__ sel, const int* __restrict__ best_w, int radius,
                                                           const int* __restrict__ mv_ptr, const int* __restrict__ mv_node, int G, int M) {
  const int lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);          // the same for the lanes of a wave
  if (g >= G || sel[g] == 0) return;
  const int w = best_w[g];
  if (w < 0 || w >= window_cells(radius)) return;
  int dx, dy;
  window_offset(w, radius, dx, dy);
  const int m1 = clamp_to(mv_ptr[g + 1], M);
  for (int m = clamp_to(mv_ptr[g], M) + lane; m < m1; m += 64) {
    const int n = mv_node[m];
    if ((unsigned)n >= (unsigned)n_nodes) continue;
    loc_x[n] = moved(loc_x[n], dx);
    loc_y[n] = moved(loc_y[n], dy);
  }
}

}  // namespace mmft

using namespace mmft;

extern "C" {

int mmft_commit_select(const int* best_w, const long long* best_dq, int G, int radius, const int* grow_ptr, const int* grow_row, int R,
                       int T, long long min_q, int* sel, long long* stats, void* owner, int device, void* stream) {
  MMFT_REQUIRE(G >= 1 && R >= 0 && T >= 1 && T <= (1 << 24), "commit_select: need G >= 1, R >= 0, 1 <= T <= 2^24 (got G %d, R %d, T %d)", G, R,
               T);
  MMFT_REQUIRE(radius >= 1 && radius <= WINDOW_RADIUS_MAX, "commit_select: radius must lie in [1, %d] (got %d)", WINDOW_RADIUS_MAX, radius);
  MMFT_REQUIRE(min_q >= 1, "commit_select: min_q must be at least 1 (got %lld)", min_q);
  MMFT_REQUIRE(best_w && best_dq && grow_ptr && sel && stats && owner && (grow_row || R == 0), "commit_select: null pointer");
  MMFT_REQUIRE(aligned8(best_dq) && aligned8(stats) && aligned8(owner),
               "commit_select: best_dq, stats and owner must be 8-byte aligned");
  DeviceGuard dg(device);
  long long* own_q = static_cast<long long*>(owner);
  int* own_g = reinterpret_cast<int*>(own_q + T);
  MMFT_LAUNCH("commit_select_kernel", 0.0, 0.0, commit_select_kernel, dim3(1), dim3(COMMIT_THREADS), (hipStream_t)stream, best_w, best_dq, G,
              window_centre(radius), grow_ptr, grow_row, R, T, min_q, sel, stats, own_q, own_g);
  return check_launch("commit_select");
}

int mmft_commit_apply(int* loc_x, int* loc_y, int n_nodes, const int* sel, const int* best_w, int radius, const int* mv_ptr,
                      const int* mv_node, int G, int M, int device, void* stream) {
  MMFT_REQUIRE(n_nodes >= 1 && G >= 1 && M >= 0, "commit_apply: need n_nodes >= 1, G >= 1, M >= 0 (got %d, %d, %d)", n_nodes, G, M);
  MMFT_REQUIRE(radius >= 1 && radius <= WINDOW_RADIUS_MAX, "commit_apply: radius must lie in [1, %d] (got %d)", WINDOW_RADIUS_MAX, radius);
  MMFT_REQUIRE(loc_x && loc_y && sel && best_w && mv_ptr && (mv_node || M == 0), "commit_apply: null pointer");
  if (M == 0) return MMFT_OK;
  DeviceGuard dg(device);
  MMFT_LAUNCH("commit_apply_kernel", 0.0, 0.0, commit_apply_kernel, dim3((unsigned)(((long long)G + 3) / 4)), dim3(256), (hipStream_t)stream,
              loc_x, loc_y, n_nodes, sel, best_w, radius, mv_ptr, mv_node, G, M);
  return check_launch("commit_apply");
}

}  // extern "C"
