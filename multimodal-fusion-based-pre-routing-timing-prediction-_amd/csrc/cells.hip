// The cells that violate now and their search plan (include/mmft_cells.h).
//
// cells_kernel<FILL>: one wave per cell, four per workgroup.  Each wave owns a bitmap of `span` bits in LDS (8 KiB at the
// largest span).  The union of up to 64 ascending row lists of any length is formed in it: the lanes load the cell's pins
// and their list bounds, a wave scan of the lengths numbers the (pin, row) pairs, and the pairs are dealt to the lanes 64 at
// a time - a lane finds the pin of its pair by binary search in the prefix, which the wave keeps in LDS -, so that a list of
// 300 rows is read by five rounds of coalesced loads and not by one lane behind 300 dependent ones.  A row's bit is set with
// an LDS OR: the outcome does not depend on the order.  FILL == false forms the row's slack on the way (a shared row is
// visited once per pin; the minimum and the verdict are idempotent) and counts the bits; FILL == true ranks every set bit by
// the popcount below it - a wave scan per 64 words - and writes the row at that place, so the rows come out ascending.
// The phases are separated by workgroup barriers that every wave reaches, with or without a cell.
#include "common.h"
#include "slack_key.h"
#include "../../include/mmft_cells.h"

namespace mmft {

constexpr int CELLS_WAVES = 4;                                  // cells per workgroup
constexpr int CELLS_WORDS = MMFT_CELLS_MAX_SPAN / 32;           // of a wave's bitmap
constexpr unsigned CELLS_NAN = 0x7fc00000u;                     // the worst of a cell without a valid row

struct CellsArgs {
  const int* cell_ptr;
  const int* cell_node;
  const int* inc_ptr;
  const int* inc_row;
  const float* pred;
  const float* required;
  // count
  int* sel_out;
  int* n_rows;
  int* n_pins;
  float* worst_out;
  // fill
  const int* sel;
  const int* worst;
  const int* sel_off;
  const int* row_off;
  const int* pin_off;
  int* grow_ptr;
  int* grow_row;
  int* grow_grp;
  int* mv_ptr;
  int* mv_node;
  int* group_cell;
  int* group_worst;
  int C, M, N, nnz, T, row_lo, span, use_threshold, G, R, MP;
  float slack_below;
};

template <bool FILL>
__global__ void __launch_bounds__(64 * CELLS_WAVES) cells_kernel(CellsArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned s_bits[CELLS_WAVES][CELLS_WORDS];
  __shared__ long long s_pre[CELLS_WAVES][65];                  // pairs before pin p; [64]: all of them
  __shared__ int s_start[CELLS_WAVES][64];                      // where pin p's list starts in inc_row
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long item = (long long)blockIdx.x * CELLS_WAVES + wave;      // the same for the lanes of a wave
  const int c = item < a.C ? (int)item : a.C;
  unsigned* bits = s_bits[wave];
  const int n_words = (a.span + 31) >> 5;

  // ---- phase A: the cell's pins and their lists; the bitmap cleared
  int m0 = 0, n_pins = 0;
  bool walk = false;                                            // the same for the lanes of a wave
  if (c < a.C) {
    m0 = clamp_to(a.cell_ptr[c], a.M);
    const int m1 = clamp_to(a.cell_ptr[c + 1], a.M);
    n_pins = m1 > m0 ? m1 - m0 : 0;
    walk = n_pins >= 1 && n_pins <= MMFT_CELLS_MAX_PINS && (!FILL || a.sel[c] != 0);
  }
  int node = -1, start = 0, len = 0;
  if (walk && lane < n_pins) {
    node = a.cell_node[m0 + lane];
    if ((unsigned)node < (unsigned)a.N) {
      start = clamp_to(a.inc_ptr[node], a.nnz);
      const int end = clamp_to(a.inc_ptr[node + 1], a.nnz);
      len = end > start ? end - start : 0;
    }
  }
  long long inc = len;                                          // inclusive over the lanes of the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  const long long total = __shfl(inc, 63);
  s_pre[wave][lane] = inc - len;
  if (lane == 63) s_pre[wave][64] = inc;
  s_start[wave][lane] = start;
  if (walk) {
    uint4* b4 = reinterpret_cast<uint4*>(bits);
    for (int w = lane; w < (n_words + 3) >> 2; w += 64) b4[w] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();

  // ---- phase B: the (pin, row) pairs, 64 at a time
  unsigned best = 0xffffffffu;                                  // ordered_bits of the smallest valid slack; all ones: none
  bool below = false;
  int w_lo = n_words, w_hi = -1;                                // the words this lane touched
  if (walk) {
    for (long long t = lane; t < total; t += 64) {
      int lo = 1, hi = 64;                                      // the first p in [1, 64] with pre[p] > t; pre[64] == total > t
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_pre[wave][mid] > t) hi = mid;
        else lo = mid + 1;
      }
      const int p = lo - 1;
      const int r = a.inc_row[s_start[wave][p] + (int)(t - s_pre[wave][p])];
      const unsigned b = (unsigned)r - (unsigned)a.row_lo;
      if (b < (unsigned)a.span) {                               // a row outside the range takes part in nothing
        const int w = (int)(b >> 5);
        atomicOr(&bits[w], 1u << (b & 31u));
        w_lo = w < w_lo ? w : w_lo;
        w_hi = w > w_hi ? w : w_hi;
        if (!FILL) {                                            // row_lo + span <= T: r indexes pred and required
          const float s = slack_of(a.required[r], a.pred[r]);
          if (s == s) {
            const unsigned o = ordered_bits(s);
            best = o < best ? o : best;
            below |= s < a.slack_below;
          }
        }
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {                           // every lane ends with the wave's values
    const int lo_o = __shfl_xor(w_lo, d), hi_o = __shfl_xor(w_hi, d);
    w_lo = lo_o < w_lo ? lo_o : w_lo;
    w_hi = hi_o > w_hi ? hi_o : w_hi;
    if (!FILL) {
      const unsigned o = __shfl_xor(best, d);
      best = o < best ? o : best;
    }
  }
  __syncthreads();

  // ---- phase C: the bits counted (count) or ranked and written (fill)
  if (!FILL) {
    if (c >= a.C) return;
    const bool selected = walk && (!a.use_threshold || __any(below));
    int n = 0;
    if (selected)
      for (int w = w_lo + lane; w <= w_hi; w += 64) n += __popc(bits[w]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
    if (lane == 0) {
      a.sel_out[c] = selected ? 1 : 0;
      a.n_rows[c] = n;
      a.n_pins[c] = selected ? n_pins : 0;
      a.worst_out[c] = best == 0xffffffffu ? __uint_as_float(CELLS_NAN) : ordered_float(best);
    }
    return;
  }
  if (item > a.C) return;
  if (c == a.C) {                                               // the wave behind the last cell closes the pointer tables
    if (lane == 0) {
      a.grow_ptr[a.G] = clamp_to(a.row_off[a.C], a.R);
      a.mv_ptr[a.G] = clamp_to(a.pin_off[a.C], a.MP);
    }
    return;
  }
  if (!walk) return;
  const int g = a.sel_off[c];
  if ((unsigned)g >= (unsigned)a.G) return;                     // (tables that do not match: no place of this cell is inside)
  const int r0 = clamp_to(a.row_off[c], a.R), r1 = clamp_to(a.row_off[c + 1], a.R);
  const int p0 = clamp_to(a.pin_off[c], a.MP);
  const int slots = r1 > r0 ? r1 - r0 : 0;
  if (lane == 0) {
    a.grow_ptr[g] = r0;
    a.mv_ptr[g] = p0;
    a.group_cell[g] = c;
    a.group_worst[g] = a.worst[c];
  }
  if (lane < n_pins && p0 + lane < a.MP) a.mv_node[p0 + lane] = node;
  int before = 0;                                               // the set bits below this round's words: the same for every lane
  for (int w0 = w_lo; w0 <= w_hi; w0 += 64) {
    const int w = w0 + lane;
    unsigned word = w <= w_hi ? bits[w] : 0u;
    const int mine = __popc(word);
    int upto = mine;                                            // inclusive over the lanes of the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(upto, d);
      if (lane >= d) upto += o;
    }
    int rank = before + upto - mine;
    while (word) {                                              // ascending bits: ascending rows
      const int bit = __ffs((int)word) - 1;
      word &= word - 1;
      if (rank < slots) {
        a.grow_row[r0 + rank] = a.row_lo + (w << 5) + bit;
        a.grow_grp[r0 + rank] = g;
      }
      ++rank;
    }
    before += __shfl(upto, 63);
  }
}

static int cells_sizes(const char* who, int C, int M, int N, int nnz, int row_lo, int span) {
  MMFT_REQUIRE(C >= 0 && C <= (1 << 24) && M >= 0 && N >= 1 && nnz >= 0, "%s: need 0 <= C <= 2^24, M >= 0, N >= 1, nnz >= 0 (got %d, %d, %d, %d)", who, C,
               M, N, nnz);
  MMFT_REQUIRE(row_lo >= 0 && span >= 1 && span <= MMFT_CELLS_MAX_SPAN, "%s: need row_lo >= 0 and 1 <= span <= %d (got %d, %d)", who,
               MMFT_CELLS_MAX_SPAN, row_lo, span);
  MMFT_REQUIRE((long long)row_lo + span < (1ll << 31), "%s: row_lo + span = %lld does not stay below 2^31", who, (long long)row_lo + span);
  return MMFT_OK;
}

}  // namespace mmft

using namespace mmft;

extern "C" {

int mmft_cells_count(const int* cell_ptr, const int* cell_node, int C, int M, const int* inc_ptr, const int* inc_row, int N, int nnz,
                     const float* pred, const float* required, int T, int row_lo, int span, int use_threshold, float slack_below, int* sel,
                     int* n_rows, int* n_pins, float* worst, int device, void* stream) {
  int rc = cells_sizes("cells_count", C, M, N, nnz, row_lo, span);
  if (rc) return rc;
  MMFT_REQUIRE(T >= 1 && (long long)row_lo + span <= T, "cells_count: the row range [%d, %d + %d) does not lie within the %d rows", row_lo, row_lo,
               span, T);
  MMFT_REQUIRE(use_threshold == 0 || use_threshold == 1, "cells_count: use_threshold must be 0 or 1 (got %d)", use_threshold);
  MMFT_REQUIRE(!use_threshold || slack_below == slack_below, "cells_count: slack_below is NaN");
  if (C == 0) return MMFT_OK;
  MMFT_REQUIRE(cell_ptr && (cell_node || M == 0) && inc_ptr && (inc_row || nnz == 0) && pred && required && sel && n_rows && n_pins && worst,
               "cells_count: null pointer");
  CellsArgs a = {};
  a.cell_ptr = cell_ptr; a.cell_node = cell_node; a.inc_ptr = inc_ptr; a.inc_row = inc_row; a.pred = pred; a.required = required;
  a.sel_out = sel; a.n_rows = n_rows; a.n_pins = n_pins; a.worst_out = worst;
  a.C = C; a.M = M; a.N = N; a.nnz = nnz; a.T = T; a.row_lo = row_lo; a.span = span;
  a.use_threshold = use_threshold; a.slack_below = use_threshold ? slack_below : 0.f;
  DeviceGuard dg(device);
  MMFT_LAUNCH("cells_count_kernel", 0.0, 24.0 * (double)C + 8.0 * (double)M, cells_kernel<false>, dim3((unsigned)cdiv(C, CELLS_WAVES)),
              dim3(64 * CELLS_WAVES), (hipStream_t)stream, a);
  return check_launch("cells_count");
}

int mmft_cells_fill(const int* cell_ptr, const int* cell_node, int C, int M, const int* inc_ptr, const int* inc_row, int N, int nnz, int row_lo,
                    int span, const int* sel, const float* worst, const int* sel_off, const int* row_off, const int* pin_off, int G, int R, int MP,
                    int* grow_ptr, int* grow_row, int* grow_grp, int* mv_ptr, int* mv_node, int* group_cell, int* group_worst, int device,
                    void* stream) {
  int rc = cells_sizes("cells_fill", C, M, N, nnz, row_lo, span);
  if (rc) return rc;
  MMFT_REQUIRE(C >= 1 && G >= 0 && R >= 0 && MP >= 0 && G <= C, "cells_fill: need C >= 1, 0 <= G <= C, R >= 0, MP >= 0 (got %d, %d, %d, %d)", C, G, R, MP);
  if (G == 0) return MMFT_OK;
  MMFT_REQUIRE(cell_ptr && (cell_node || M == 0) && inc_ptr && (inc_row || nnz == 0) && sel && worst && sel_off && row_off && pin_off && grow_ptr &&
                   ((grow_row && grow_grp) || R == 0) && mv_ptr && (mv_node || MP == 0) && group_cell && group_worst,
               "cells_fill: null pointer");
  CellsArgs a = {};
  a.cell_ptr = cell_ptr; a.cell_node = cell_node; a.inc_ptr = inc_ptr; a.inc_row = inc_row;
  a.sel = sel; a.worst = reinterpret_cast<const int*>(worst); a.sel_off = sel_off; a.row_off = row_off; a.pin_off = pin_off;
  a.grow_ptr = grow_ptr; a.grow_row = grow_row; a.grow_grp = grow_grp; a.mv_ptr = mv_ptr; a.mv_node = mv_node;
  a.group_cell = group_cell; a.group_worst = group_worst;
  a.C = C; a.M = M; a.N = N; a.nnz = nnz; a.row_lo = row_lo; a.span = span; a.G = G; a.R = R; a.MP = MP;
  DeviceGuard dg(device);
  MMFT_LAUNCH("cells_fill_kernel", 0.0, 24.0 * (double)C + 8.0 * (double)R + 4.0 * (double)MP, cells_kernel<true>,
              dim3((unsigned)cdiv((long long)C + 1, CELLS_WAVES)), dim3(64 * CELLS_WAVES), (hipStream_t)stream, a);
  return check_launch("cells_fill");
}

}  // extern "C"
