// Discrete pin sensitivity (include/mmft_sens_pins.h): per batch row and (first-occurrence position, direction) the change of
// g[t] . h_cnn[t] when that pin moves one map cell, from the line segments its adjacent boxes gain and lose - no bitmap - and
// the per-pin sums of those rows over a static incidence CSR.  The box arithmetic is the mask rule of include/mmft_place.h,
// per axis mask_axis_range (mask_rule.h) - the function the bitmap kernels build their boxes from.
#include "common.h"
#include "mask_rule.h"
#include "../../include/mmft_sens_pins.h"

namespace mmft {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PMOVE_MAX_LEN = 1024;         // nodes of a row staged in LDS: 3 x 4 KB ints + 1 KB flags, next to 4 KB of g

// Is the cell at (pm, pf) - moving axis, fixed axis - inside the box of the node pair (k, k + 1), pin n displaced by delta along
// the moving axis (delta == 0: the box as it is)?
__device__ inline bool pm_in_box(const int* cm, const int* cf, const int* node, int k, int n, int delta, int lim_m, int lim_f,
                                 int pm, int pf) {
  int lo, hi;
  mask_axis_range(cm[k] + (node[k] == n ? delta : 0), cm[k + 1] + (node[k + 1] == n ? delta : 0), lim_m, lo, hi);
  if (pm < lo || pm > hi) return false;
  mask_axis_range(cf[k], cf[k + 1], lim_f, lo, hi);
  return pf >= lo && pf <= hi;
}

// G lanes share a candidate cell (the boxes to test it against, then the 16-byte pieces of its wT row), 64 / G cells per pass
template <int G>
__device__ inline void pin_move_items(const int* sx, const int* sy, const int* snode, const unsigned char* sfirst,
                                      const float* sg, int len, int map_x, int map_y, const float* __restrict__ fb,
                                      const float* __restrict__ wT, int Dout, float* __restrict__ out_row) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lig = lane & (G - 1), grp = lane / G;
  constexpr int NG = 64 / G;
  const int groups = Dout >> 2;
  const f32x4* sg4 = reinterpret_cast<const f32x4*>(sg);
  for (int it = wave; it < len * 4; it += 4) {                         // wave-uniform from here to the store
    const int j = it >> 2, d = it & 3;
    if (!sfirst[j]) continue;
    const int n = snode[j], delta = (d & 1) ? -1 : 1;
    const int* cm = d < 2 ? sx : sy;                                   // the axis the pin moves along, and the other one
    const int* cf = d < 2 ? sy : sx;
    const int lim_m = d < 2 ? map_x : map_y, lim_f = d < 2 ? map_y : map_x;
    float acc = 0.f;
    for (int k = 0; k + 1 < len; ++k) {
      const bool mk = snode[k] == n, mk1 = snode[k + 1] == n;
      if (!mk && !mk1) continue;                                       // a box the pin does not touch
      int f1, f2, a1, a2, b1, b2;
      mask_axis_range(cf[k], cf[k + 1], lim_f, f1, f2);
      if (f1 > f2) continue;                                           // empty before and after
      mask_axis_range(cm[k], cm[k + 1], lim_m, a1, a2);                       // as it is
      mask_axis_range(cm[k] + (mk ? delta : 0), cm[k + 1] + (mk1 ? delta : 0), lim_m, b1, b2);      // moved
      const int L = f2 - f1 + 1;
      // the two ranges differ by at most one line at each end: gained lines are among {b1, b2}, lost ones among {a1, a2}
      for (int s = 0; s < 4; ++s) {
        const bool add = s < 2;
        const int v = s == 0 ? b1 : s == 1 ? b2 : s == 2 ? a1 : a2;
        bool ok;
        if (add) ok = b1 <= b2 && (s == 0 || b2 != b1) && !(a1 <= a2 && v >= a1 && v <= a2);
        else     ok = a1 <= a2 && (s == 2 || a2 != a1) && !(b1 <= b2 && v >= b1 && v <= b2);
        if (!ok) continue;
        for (int base = 0; base < L; base += NG) {
          const int idx = base + grp;
          const bool active = idx < L;
          const int pf = f1 + idx;
          // a gained cell counts when no box holds it now and no earlier box of the pin gains it too; a lost cell counts when
          // no box holds it after the move and no earlier box of the pin loses it too
          int cov = 0;
          if (active) {
            for (int kk = lig; kk + 1 < len; kk += G) {
              bool in = pm_in_box(cm, cf, snode, kk, n, add ? 0 : delta, lim_m, lim_f, v, pf);
              if (kk < k) in = in || pm_in_box(cm, cf, snode, kk, n, add ? delta : 0, lim_m, lim_f, v, pf);
              cov |= in ? 1 : 0;
            }
          }
          for (int o = 1; o < G; o <<= 1) cov |= __shfl_xor(cov, o, 64);
          const bool counts = active && !cov;
          float part = 0.f;
          int cell = 0;
          if (counts) {
            cell = d < 2 ? v * map_y + pf : pf * map_y + v;            // inside [0, P): v and pf are clamped ranges' members
            const float* wr = wT + (long long)cell * Dout;
            for (int k4 = lig; k4 < groups; k4 += G) {
              const f32x4 w = *reinterpret_cast<const f32x4*>(wr + k4 * 4);
              const f32x4 gg = sg4[k4];
              part = fmaf(gg.x, w.x, part);
              part = fmaf(gg.y, w.y, part);
              part = fmaf(gg.z, w.z, part);
              part = fmaf(gg.w, w.w, part);
            }
          }
          for (int o = 1; o < G; o <<= 1) part += __shfl_xor(part, o, 64);
          if (counts) {
            const float sc = part * fb[cell];
            acc += add ? sc : -sc;
          }
        }
      }
    }
    for (int o = G; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);     // the groups' sums, in a fixed order
    if (lane == 0) out_row[it] = acc;
  }
}

__global__ void __launch_bounds__(256) pin_move_rows_kernel(const int* __restrict__ path_nodes, const int* __restrict__ path_lens,
                                                            int maxlen, const int* __restrict__ loc_x,
                                                            const int* __restrict__ loc_y, int map_x, int map_y,
                                                            const int* __restrict__ paths, const int* __restrict__ foff,
                                                            const float* __restrict__ feat, const float* __restrict__ wT, int Dout,
                                                            const float* __restrict__ g, long long ldg,
                                                            float* __restrict__ row_move) {
  __shared__ __attribute__((aligned(16))) float sg[1024];
  __shared__ int sx[PMOVE_MAX_LEN], sy[PMOVE_MAX_LEN], snode[PMOVE_MAX_LEN];
  __shared__ unsigned char sfirst[PMOVE_MAX_LEN];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int q = paths[t];
  const int* path = path_nodes + (long long)q * maxlen;
  int len = path_lens[q] < maxlen ? path_lens[q] : maxlen;             // the same for every thread
  len = len < 0 ? 0 : len;
  // coordinates saturated to [-2, map + 1]: the rule gives the same boxes for them, with the pin displaced or not, and the
  // displacement cannot overflow
  for (int j = tid; j < len; j += 256) {
    const int a = path[j];
    int x = loc_x[a], y = loc_y[a];
    x = x < -2 ? -2 : (x > map_x + 1 ? map_x + 1 : x);
    y = y < -2 ? -2 : (y > map_y + 1 ? map_y + 1 : y);
    snode[j] = a;
    sx[j] = x;
    sy[j] = y;
  }
  for (int k = tid; k < Dout; k += 256) sg[k] = g[(long long)t * ldg + k];
  __syncthreads();
  for (int j = tid; j < len; j += 256) {
    const int a = snode[j];
    unsigned char first = 1;
    for (int i = 0; i < j; ++i) first = snode[i] == a ? 0 : first;
    sfirst[j] = first;
  }
  __syncthreads();
  float* out_row = row_move + (long long)t * maxlen * 4;
  // every element is written exactly once: the zeros here, the live first occurrences by their wave below
  for (int i = tid; i < maxlen * 4; i += 256) {
    const int j = i >> 2;
    if (j >= len || !sfirst[j]) out_row[i] = 0.f;
  }
  const float* fb = feat + (foff ? foff[t] : 0);
  const int groups = Dout >> 2;
  if (groups >= 8)      pin_move_items<8>(sx, sy, snode, sfirst, sg, len, map_x, map_y, fb, wT, Dout, out_row);
  else if (groups >= 3) pin_move_items<4>(sx, sy, snode, sfirst, sg, len, map_x, map_y, fb, wT, Dout, out_row);
  else if (groups == 2) pin_move_items<2>(sx, sy, snode, sfirst, sg, len, map_x, map_y, fb, wT, Dout, out_row);
  else                  pin_move_items<1>(sx, sy, snode, sfirst, sg, len, map_x, map_y, fb, wT, Dout, out_row);
}

__global__ void __launch_bounds__(256) pin_move_sum_kernel(const float* __restrict__ row_move, long long slots,
                                                           const int* __restrict__ inc_ptr, const int* __restrict__ inc_slot,
                                                           long long nnz, int N, float* __restrict__ pin_move) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;       // (pin, direction)
  if (i >= 4LL * N) return;
  const int n = (int)(i >> 2), d = (int)(i & 3);
  float acc = 0.f;
  const long long e1 = inc_ptr[n + 1];
  for (long long e = inc_ptr[n]; e < e1; ++e) {
    if (e < 0 || e >= nnz) continue;
    const long long s = inc_slot[e];
    if (s >= 0 && s < slots) acc += row_move[s * 4 + d];
  }
  pin_move[i] = acc;
}

}  // namespace mmft

using namespace mmft;

extern "C" {

int mmft_pin_move_rows(const int* path_nodes, const int* path_lens, int maxlen, const int* loc_x, const int* loc_y, int map_x,
                       int map_y, const int* paths, const int* f_off, int T, const float* feat, const float* wT, int Dout,
                       const float* g, long long ldg, float* row_move, int device, void* stream) {
  MMFT_REQUIRE(mask_map_ok(map_x, map_y), "pin_move_rows: the map must hold a multiple of 64 cells, at most 65536");
  MMFT_REQUIRE(Dout >= 4 && Dout % 4 == 0 && Dout <= 1024 && maxlen >= 1 && maxlen <= PMOVE_MAX_LEN && T >= 0 && ldg >= Dout &&
                   ldg % 4 == 0,
               "pin_move_rows: bad sizes (Dout a multiple of 4 in [4, 1024], maxlen in [1, 1024], T >= 0, ldg >= Dout and a "
               "multiple of 4)");
  if (T == 0) return MMFT_OK;
  MMFT_REQUIRE(path_nodes && path_lens && loc_x && loc_y && paths && feat && wT && g && row_move, "pin_move_rows: null pointer");
  MMFT_REQUIRE(aligned16(feat) && aligned16(wT) && aligned16(g), "pin_move_rows: 16-byte alignment of feat, wT and g");
  DeviceGuard dg(device);
  MMFT_LAUNCH("pin_move_rows_kernel", 0.0, 0.0, pin_move_rows_kernel, dim3(T), dim3(256), (hipStream_t)stream, path_nodes, path_lens,
              maxlen, loc_x, loc_y, map_x, map_y, paths, f_off, feat, wT, Dout, g, ldg, row_move);
  return check_launch("pin_move_rows");
}

int mmft_pin_move_sum(const float* row_move, long long slots, const int* inc_ptr, const int* inc_slot, long long nnz, int N,
                      float* pin_move, int device, void* stream) {
  MMFT_REQUIRE(N >= 0 && N < (1 << 29) && slots >= 0 && slots < (1LL << 29) && nnz >= 0 && nnz < (1LL << 31),
               "pin_move_sum: bad sizes (0 <= N < 2^29, 0 <= slots < 2^29, 0 <= nnz < 2^31)");
  if (N == 0) return MMFT_OK;
  MMFT_REQUIRE(inc_ptr && pin_move && (nnz == 0 || (inc_slot && row_move)), "pin_move_sum: null pointer");
  MMFT_REQUIRE(aligned16(row_move) && aligned16(pin_move), "pin_move_sum: 16-byte alignment of row_move and pin_move");
  DeviceGuard dg(device);
  MMFT_LAUNCH("pin_move_sum_kernel", 0.0, 0.0, pin_move_sum_kernel, dim3(cdiv(4LL * N, 256)), dim3(256), (hipStream_t)stream, row_move,
              slots, inc_ptr, inc_slot, nnz, N, pin_move);
  return check_launch("pin_move_sum");
}

}  // extern "C"
