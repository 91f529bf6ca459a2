// Masked projection straight from a placement (include/mmft_place.h): per batch row the path's mask is rasterised into an
// LDS bitmap from (path nodes, pin coordinates) and projected through the block-prefix table of fc_prefix_kernel, run by
// run, in the order and with the arithmetic of masked_fc_fwd_runs_kernel (fusion.hip) - no CSR and no run table in device memory.
#include "common.h"
#include "mask_rule.h"
#include "../../include/mmft_place.h"

namespace mmft {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long place_u64;

constexpr int PLACE_LIST = 1024;            // masks of up to this many runs (box masks have tens) get a run list in LDS, 4 KB

// Dynamic LDS only (a static array in front of it would move its base off 16 bytes):
//   part [256] f32x4 | list [PLACE_LIST] unsigned | cnt [nblk + 1] int, padded to 16 bytes | red [8] int | pin [2][256] int |
//   bits [P / 32] unsigned                 (at MASK_MAX_CELLS: bitmap 8 KB, block counts 4 KB)
__host__ __device__ inline int place_cnt_slots(int nblk) { return (nblk + 1 + 3) & ~3; }
inline size_t place_lds_bytes(int P) {
  return 256 * sizeof(f32x4) + (size_t)(PLACE_LIST + place_cnt_slots(P >> 6) + 8 + 512) * 4 + (size_t)(P >> 5) * 4;
}

// the 64 cells of a block as one word (from its two bitmap words, read by the caller), and the word's run starts: bit i is set
// where a run starts at cell i of the block
__device__ inline place_u64 place_block(unsigned lo, unsigned hi) { return (place_u64)lo | ((place_u64)hi << 32); }
__device__ inline place_u64 place_starts(place_u64 v) { return v & ~(v << 1); }
// the lowest run among `starts` (not empty) of block word v: its first cell i and its length
__device__ inline void place_first_run(place_u64 v, place_u64 starts, int& i, int& len) {
  i = __ffsll((long long)starts) - 1;
  const place_u64 past = ~(v >> i);                     // its first set bit: the run's length (none: the run fills 64 bits)
  len = past ? __ffsll((long long)past) - 1 : 64;
}

// [s, e] (cells of the design's map) of run r; b is the lane's block cursor, it only moves forward (r ascends per lane).
// cnt[b] = runs in the blocks before b, cnt[nblk] = all runs: block b holds run r when cnt[b] <= r < cnt[b + 1].
__device__ inline void place_locate(const int* cnt, const unsigned* bits, int nblk, int r, int& b, int& s, int& e) {
  int lo = b, hi = nblk - 1;
  while (lo < hi) {                                     // the largest block with cnt[block] <= r
    int mid = (lo + hi + 1) >> 1;
    if (cnt[mid] <= r) lo = mid; else hi = mid - 1;
  }
  b = lo;
  const place_u64 v = place_block(bits[2 * b], bits[2 * b + 1]);
  place_u64 starts = place_starts(v);
  for (int k = r - cnt[b]; k > 0; --k) starts &= starts - 1;
  int i, len;
  place_first_run(v, starts, i, len);
  s = (b << 6) + i;
  e = s + len - 1;
}

// The same from the run list when the mask has one: entry r = start | (length - 1) << 16.
__device__ inline void place_run(const unsigned* list, bool listed, const int* cnt, const unsigned* bits, int nblk, int r, int& b,
                                 int& s, int& e) {
  if (listed) {
    unsigned u = list[r];
    s = (int)(u & 0xffffu);
    e = s + (int)(u >> 16);
  } else {
    place_locate(cnt, bits, nblk, r, b, s, e);
  }
}

__global__ void __launch_bounds__(256) placed_fc_fwd_kernel(const int* __restrict__ path_nodes, const int* __restrict__ path_lens,
                                                            int maxlen, const int* __restrict__ loc_x,
                                                            const int* __restrict__ loc_y, int map_x, int map_y,
                                                            const int* __restrict__ paths, const int* __restrict__ foff,
                                                            const float* __restrict__ GP, const float* __restrict__ bias,
                                                            float* __restrict__ out, long long ldo, int Dout,
                                                            int* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char place_smem[];
  const int P = map_x * map_y, words = P >> 5, nblk = P >> 6;
  f32x4* part = reinterpret_cast<f32x4*>(place_smem);
  unsigned* list = reinterpret_cast<unsigned*>(place_smem + 256 * sizeof(f32x4));
  int* cnt = reinterpret_cast<int*>(list + PLACE_LIST);
  int* red = cnt + place_cnt_slots(nblk);               // [0..4) runs per wave, [4..8) cells per wave
  int* pin_x = red + 8;                                 // coordinates of up to 256 consecutive nodes of the path
  int* pin_y = pin_x + 256;
  unsigned* bits = reinterpret_cast<unsigned*>(pin_y + 256);
  const int t = blockIdx.x, tid = threadIdx.x;
  for (int w = tid; w < words; w += 256) bits[w] = 0u;
  // ---- the union of boxes: THE MASK RULE, staged (mask_rule.h); node ids are not checked here (mmft_place.h)
  const int q = paths[t];
  const int* path = path_nodes + (long long)q * maxlen;
  const int len = path_lens[q] < maxlen ? path_lens[q] : maxlen;        // the same for every thread
  mask_raster_path<256, false>(bits, pin_x, pin_y, path, len, loc_x, loc_y, 0, map_x, map_y, tid);
  __syncthreads();
  // ---- number the runs: per-block counts, exclusive scan over the blocks (thread tid owns `per` consecutive blocks)
  const int per = (nblk + 255) >> 8;
  int mine = 0, cells = 0;
  for (int b = tid * per; b < (tid + 1) * per && b < nblk; ++b) {
    const place_u64 v = place_block(bits[2 * b], bits[2 * b + 1]);
    mine += __popcll(place_starts(v));
    cells += __popcll(v);
  }
  const int lane = tid & 63, wave = tid >> 6;
  int incl = mine;
  for (int o = 1; o < 64; o <<= 1) {
    int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  for (int o = 32; o > 0; o >>= 1) cells += __shfl_xor(cells, o, 64);
  if (lane == 63) red[wave] = incl;
  if (lane == 0) red[4 + wave] = cells;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += red[w];
  const int R = red[0] + red[1] + red[2] + red[3];
  const bool listed = R <= PLACE_LIST;                  // the same for every thread
  {
    int run = base + incl - mine;
    for (int b = tid * per; b < (tid + 1) * per && b < nblk; ++b) {
      const place_u64 v = place_block(bits[2 * b], bits[2 * b + 1]);
      cnt[b] = run;
      const place_u64 starts = place_starts(v);
      if (listed) {                                     // every thread lists the runs of its own blocks, ascending
        for (place_u64 st = starts; st; st &= st - 1) {
          int i, len;
          place_first_run(v, st, i, len);
          list[run++] = (unsigned)((b << 6) + i) | ((unsigned)(len - 1) << 16);
        }
      } else {
        run += __popcll(starts);
      }
    }
    if (tid == 0) {
      cnt[nblk] = R;
      if (stats) {
        stats[2 * (long long)t] = red[4] + red[5] + red[6] + red[7];
        stats[2 * (long long)t + 1] = R;
      }
    }
  }
  __syncthreads();
  // ---- accumulate: the loop of masked_fc_fwd_runs_kernel with (start, end) found in the bitmap instead of a table
  const int groups = Dout >> 2;
  const int J = 256 / groups;
  const int j = tid / groups, c4 = tid - j * groups;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (j < J) {
    const float* gb = GP + (long long)(foff ? foff[t] : 0) * Dout + c4 * 4;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    int r = j, b = 0;
    for (; r + J < R; r += 2 * J) {                  // two runs per trip: their bitmap -> row chains overlap
      int s0, e0, s1, e1;
      place_run(list, listed, cnt, bits, nblk, r, b, s0, e0);
      place_run(list, listed, cnt, bits, nblk, r + J, b, s1, e1);
      f32x4 h0 = *reinterpret_cast<const f32x4*>(gb + (long long)e0 * Dout);
      f32x4 h1 = *reinterpret_cast<const f32x4*>(gb + (long long)e1 * Dout);
      f32x4 l0 = (s0 & 63) ? *reinterpret_cast<const f32x4*>(gb + (long long)(s0 - 1) * Dout) : z;
      f32x4 l1 = (s1 & 63) ? *reinterpret_cast<const f32x4*>(gb + (long long)(s1 - 1) * Dout) : z;
      acc += h0 - l0;
      acc += h1 - l1;
    }
    for (; r < R; r += J) {
      int s, e;
      place_run(list, listed, cnt, bits, nblk, r, b, s, e);
      f32x4 hi = *reinterpret_cast<const f32x4*>(gb + (long long)e * Dout);
      f32x4 lo = (s & 63) ? *reinterpret_cast<const f32x4*>(gb + (long long)(s - 1) * Dout) : z;
      acc += hi - lo;
    }
  }
  part[tid] = acc;
  __syncthreads();
  if (tid < groups) {
    f32x4 sum = bias ? *reinterpret_cast<const f32x4*>(bias + tid * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int jj = 0; jj < J; ++jj) sum += part[jj * groups + tid];
    *reinterpret_cast<f32x4*>(out + (long long)t * ldo + tid * 4) = sum;
  }
}

}  // namespace mmft

using namespace mmft;

extern "C" {

int mmft_placed_fc_fwd(const int* path_nodes, const int* path_lens, int maxlen, const int* loc_x, const int* loc_y, int map_x,
                       int map_y, const int* paths, const int* f_off, int T, const float* GP, const float* bias, float* out,
                       long long ldo, int Dout, int S, int* stats, int device, void* stream) {
  MMFT_REQUIRE(S == 64, "placed_fc_fwd: the prefix block must be 64 cells (one bitmap word per block)");
  MMFT_REQUIRE(mask_map_ok(map_x, map_y), "placed_fc_fwd: the map must hold a multiple of 64 cells, at most 65536");
  MMFT_REQUIRE(Dout >= 4 && Dout % 4 == 0 && Dout <= 1024 && maxlen >= 1 && T >= 0 && ldo >= Dout && ldo % 4 == 0,
               "placed_fc_fwd: bad sizes (Dout a multiple of 4 in [4, 1024], maxlen >= 1, T >= 0, ldo >= Dout and a multiple of 4)");
  MMFT_REQUIRE(path_nodes && path_lens && loc_x && loc_y && paths && GP && out, "placed_fc_fwd: null pointer");
  MMFT_REQUIRE(aligned16(GP) && aligned16(out) && (!bias || aligned16(bias)), "placed_fc_fwd: 16-byte alignment");
  if (T == 0) return MMFT_OK;
  DeviceGuard dg(device);
  const int P = map_x * map_y;
  static DynLdsOnce once;
  int arc = ensure_dyn_lds(once, (const void*)placed_fc_fwd_kernel, (int)place_lds_bytes(MASK_MAX_CELLS), "placed_fc_fwd");
  if (arc) return arc;
  MMFT_LAUNCH_LDS("placed_fc_fwd_kernel", 0.0, 0.0, placed_fc_fwd_kernel, dim3(T), dim3(256), place_lds_bytes(P), (hipStream_t)stream,
                  path_nodes, path_lens, maxlen, loc_x, loc_y, map_x, map_y, paths, f_off, GP, bias, out, ldo, Dout, stats);
  return check_launch("placed_fc_fwd");
}

}  // extern "C"
