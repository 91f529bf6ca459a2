// The masked projection of ONE row from its mask's bitmap in LDS (include/mmft_place.h): the LDS layout, the numbering of the
// runs and the accumulation through the block-prefix table.  placed_fc_fwd_kernel (place.hip) and trial_row_write
// (trial_row.h, the body of the four rows kernels) rasterise their bitmaps differently - the pins as they are, or with a set of
// overrides - and both call place_project for everything after the raster: the tests hold these kernels to the same bits, and
// the code that makes those bits is here once.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace mmft {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long place_u64;

constexpr int PLACE_LIST = 1024;            // masks of up to this many runs (box masks have tens) get a run list in LDS, 4 KB

// Dynamic LDS only (a static array in front of it would move its base off 16 bytes):
//   part [256] f32x4 | list [PLACE_LIST] unsigned | cnt [nblk + 1] int, padded to 16 bytes | red [8] int | pin [2][256] int |
//   bits [P / 32] unsigned                 (at MASK_MAX_CELLS: bitmap 8 KB, block counts 4 KB)
// What a kernel keeps besides (trial_row.h: the overrides of a row) goes behind the bitmap.
__host__ __device__ inline int place_cnt_slots(int nblk) { return (nblk + 1 + 3) & ~3; }
inline size_t place_lds_bytes(int P) {
  return 256 * sizeof(f32x4) + (size_t)(PLACE_LIST + place_cnt_slots(P >> 6) + 8 + 512) * 4 + (size_t)(P >> 5) * 4;
}

struct PlaceLds {
  f32x4* part;
  unsigned* list;
  int* cnt;
  int* red;                                 // [0..4) runs per wave, [4..8) cells per wave
  int* pin_x;                               // coordinates of up to 256 consecutive nodes of the path
  int* pin_y;
  unsigned* bits;
};
__device__ inline PlaceLds place_lds(unsigned char* smem, int nblk) {
  PlaceLds s;
  s.part = reinterpret_cast<f32x4*>(smem);
  s.list = reinterpret_cast<unsigned*>(smem + 256 * sizeof(f32x4));
  s.cnt = reinterpret_cast<int*>(s.list + PLACE_LIST);
  s.red = s.cnt + place_cnt_slots(nblk);
  s.pin_x = s.red + 8;
  s.pin_y = s.pin_x + 256;
  s.bits = reinterpret_cast<unsigned*>(s.pin_y + 256);
  return s;
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

// out_row[0 .. Dout) = bias + sum over the runs [s, e] of the bitmap L.bits (nblk blocks of 64 cells, complete: the caller's
// barrier stands between the raster and this call) of gp[e] - gp[s - 1], gp = the row's design in the block-prefix table.
// Called by all 256 threads of the workgroup (tid = threadIdx.x); stats_row NULL or [2]: cells and runs of the mask.
// Run r is added on entry lane r % J, J = 256 / (Dout / 4), ascending r per lane; the lanes are combined from the bias in the
// order 0 .. J - 1: the bits depend on the bitmap, gp, bias and Dout alone.
__device__ __forceinline__ void place_project(const PlaceLds& L, int nblk, const float* __restrict__ gp, const float* __restrict__ bias,
                                              float* __restrict__ out_row, int Dout, int* __restrict__ stats_row, int tid) {
  f32x4* part = L.part;
  unsigned* list = L.list;
  int* cnt = L.cnt;
  int* red = L.red;
  const unsigned* bits = L.bits;
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
      if (stats_row) {
        stats_row[0] = red[4] + red[5] + red[6] + red[7];
        stats_row[1] = R;
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
    const float* gb = gp + c4 * 4;
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
    *reinterpret_cast<f32x4*>(out_row + tid * 4) = sum;
  }
}

}  // namespace mmft
