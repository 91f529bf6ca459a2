// Patch the kept head rows after a commit (include/mmft_refine.h).
//
// refine_rows_kernel: one workgroup per entry e.  A selected entry forms its group's overrides from the resident pins and the
// offset best_w[g] by trial_stage_group (trial_row.h), the call search_rows_kernel makes, and writes the row by
// trial_row_write, the function search_rows_kernel and trial_rows_kernel call: the same bits.  Every other entry copies its
// row of x.
// refine_patch_kernel: one wave per selected entry copies the h_cnn columns of its row of xt into x and its prediction into
// pred, with plain vector stores: the selected groups share no row.
#include "common.h"
#include "trial_row.h"
#include "../../include/mmft_refine.h"

namespace mmft {

// the offset of entry e's group if the group is selected, else -1; the same for every thread that asks about one entry
__device__ __forceinline__ int refine_offset(const int* __restrict__ sel, const int* __restrict__ best_w, int g, int G, int W) {
  if ((unsigned)g >= (unsigned)G || sel[g] == 0) return -1;
  const int w = best_w[g];
  return w >= 0 && w < W ? w : -1;
}

struct RefineRowsArgs {
  TrialRowArgs row;
  const int* grow_row;
  const int* grow_grp;
  const int* mv_ptr;
  const int* mv_node;
  const int* sel;
  const int* best_w;
  int G, T, radius;
};

__global__ void __launch_bounds__(256) refine_rows_kernel(RefineRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char refine_smem[];
  const int e = blockIdx.x, tid = threadIdx.x;
  const int t = a.grow_row[e], g = a.grow_grp[e];
  const bool inside = (unsigned)t < (unsigned)a.T && (unsigned)g < (unsigned)a.G;
  const int w = inside ? refine_offset(a.sel, a.best_w, g, a.G, window_cells(a.radius)) : -1;
  if (w < 0) {                                          // the same for every thread: the row as the resident batch has it
    float* dst = a.row.xt + (long long)e * a.row.ldxt;
    const float* src = a.row.x + (long long)(inside ? t : 0) * a.row.ldx;
    const int quads = a.row.width >> 2;                 // rows of x and xt start on 16 bytes
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int c = tid; c < quads; c += 256)
      reinterpret_cast<f32x4*>(dst)[c] = inside ? reinterpret_cast<const f32x4*>(src)[c] : z;
    for (int c = 4 * quads + tid; c < a.row.width; c += 256) dst[c] = inside ? src[c] : 0.f;
    return;
  }
  const int P = a.row.map_x * a.row.map_y;
  const PlaceLds L = place_lds(refine_smem, P >> 6);
  const TrialMoves mv = trial_moves_lds(L, P);
  int dx, dy;
  window_offset(w, a.radius, dx, dy);
  const int n_mv = trial_stage_group(a.row, mv, a.mv_ptr, a.mv_node, g, dx, dy, tid);
  trial_row_write(a.row, L, mv, n_mv, t, e, tid);
}

__global__ void __launch_bounds__(256) refine_patch_kernel(float* __restrict__ x, long long ldx, float* __restrict__ pred, int T,
                                                           const float* __restrict__ xt, long long ldxt,
                                                           const float* __restrict__ pred_t, const int* __restrict__ sel,
                                                           const int* __restrict__ best_w, int W, const int* __restrict__ grow_row,
                                                           const int* __restrict__ grow_grp, int R, int G, int cnn_col, int Dout,
                                                           unsigned long long* __restrict__ stats) {
  __shared__ int s_count[8];                            // [0..4) patched per wave, [4..8) skipped per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int quads = Dout >> 2;
  int patched = 0, skipped = 0;                         // the same for the lanes of a wave
  for (long long e = (long long)blockIdx.x * 4 + wave; e < R; e += (long long)gridDim.x * 4) {
    if (refine_offset(sel, best_w, grow_grp[e], G, W) < 0) continue;
    const int r = grow_row[e];
    if ((unsigned)r >= (unsigned)T) {
      ++skipped;
      continue;
    }
    const f32x4* src = reinterpret_cast<const f32x4*>(xt + e * ldxt + cnn_col);
    f32x4* dst = reinterpret_cast<f32x4*>(x + (long long)r * ldx + cnn_col);
    for (int c = lane; c < quads; c += 64) dst[c] = src[c];
    if (lane == 0) pred[r] = pred_t[e];
    ++patched;
  }
  if (lane == 0) {
    s_count[wave] = patched;
    s_count[4 + wave] = skipped;
  }
  __syncthreads();
  if (threadIdx.x < 2) {                                // integer adds: the order of the workgroups does not show
    const int* c = s_count + 4 * threadIdx.x;
    const int n = c[0] + c[1] + c[2] + c[3];
    if (n) atomicAdd(stats + threadIdx.x, (unsigned long long)n);
  }
}

}  // namespace mmft

using namespace mmft;

extern "C" {

int mmft_refine_rows(const int* path_nodes, const int* path_lens, int maxlen, const int* loc_x, const int* loc_y, int map_x,
                     int map_y, const int* paths, const int* f_off, int T, const int* grow_row, const int* grow_grp, int R,
                     const int* mv_ptr, const int* mv_node, int G, const int* sel, const int* best_w, int radius, const float* GP,
                     const float* bias, const float* x, long long ldx, float* xt, long long ldxt, int width, int cnn_col, int Dout,
                     int S, int device, void* stream) {
  const TrialRowCall c = {"refine_rows", path_nodes, path_lens, maxlen, loc_x, loc_y, map_x, map_y, paths, f_off, GP, bias,
                          x, ldx, xt, ldxt, width, cnn_col, Dout, S, device, stream};
  int rc = trial_row_check(c, T >= 1 && T <= (1 << 24) && G >= 1 && R >= 0, "1 <= T <= 2^24, G >= 1, R >= 0");
  if (rc) return rc;
  MMFT_REQUIRE(radius >= 1 && radius <= WINDOW_RADIUS_MAX, "refine_rows: radius must lie in [1, %d] (got %d)", WINDOW_RADIUS_MAX, radius);
  if (R == 0) return MMFT_OK;
  RefineRowsArgs a;
  a.grow_row = grow_row; a.grow_grp = grow_grp; a.mv_ptr = mv_ptr; a.mv_node = mv_node; a.sel = sel; a.best_w = best_w;
  a.G = G; a.T = T; a.radius = radius;
  return trial_row_launch<RefineRowsArgs, refine_rows_kernel>(c, "refine_rows_kernel", a, (unsigned)R,
                                                              grow_row && grow_grp && mv_ptr && mv_node && sel && best_w);
}

int mmft_refine_patch(float* x, long long ldx, float* pred, int T, const float* xt, long long ldxt, const float* pred_t, const int* sel,
                      const int* best_w, int radius, const int* grow_row, const int* grow_grp, int R, int G, int cnn_col, int Dout,
                      long long* stats, int device, void* stream) {
  MMFT_REQUIRE(T >= 1 && T <= (1 << 24) && G >= 1 && R >= 0, "refine_patch: need 1 <= T <= 2^24, G >= 1, R >= 0 (got T %d, G %d, R %d)", T, G, R);
  MMFT_REQUIRE(radius >= 1 && radius <= WINDOW_RADIUS_MAX, "refine_patch: radius must lie in [1, %d] (got %d)", WINDOW_RADIUS_MAX, radius);
  MMFT_REQUIRE(Dout >= 4 && Dout % 4 == 0 && Dout <= 1024 && cnn_col >= 0 && cnn_col % 4 == 0 && ldx % 4 == 0 && ldxt % 4 == 0 &&
                   (long long)cnn_col + Dout <= ldx && (long long)cnn_col + Dout <= ldxt,
               "refine_patch: bad columns (Dout a multiple of 4 in [4, 1024], cnn_col, ldx, ldxt multiples of 4, 0 <= cnn_col, "
               "cnn_col + Dout <= ldx, ldxt)");
  MMFT_REQUIRE(x && pred && sel && best_w && stats && ((grow_row && grow_grp && xt && pred_t) || R == 0), "refine_patch: null pointer");
  MMFT_REQUIRE(aligned16(x) && (!xt || aligned16(xt)), "refine_patch: x and xt must be 16-byte aligned");
  MMFT_REQUIRE(aligned8(stats), "refine_patch: stats must be 8-byte aligned");
  DeviceGuard dg(device);
  hipStream_t st = (hipStream_t)stream;
  hipError_t err = hipMemsetAsync(stats, 0, 2 * sizeof(long long), st);
  if (err != hipSuccess) {
    set_error("refine_patch: clearing the counts failed: %s", hipGetErrorString(err));
    return MMFT_ERR_LAUNCH;
  }
  if (R == 0) return MMFT_OK;
  int grid = cdiv(R, 4);
  grid = grid > 2048 ? 2048 : grid;
  MMFT_LAUNCH("refine_patch_kernel", 0.0, 8.0 * (double)R * Dout, refine_patch_kernel, dim3(grid), dim3(256), st, x, ldx, pred, T, xt, ldxt,
              pred_t, sel, best_w, window_cells(radius), grow_row, grow_grp, R, G, cnn_col, Dout, reinterpret_cast<unsigned long long*>(stats));
  return check_launch("refine_patch");
}

}  // extern "C"
