// Incremental re-prediction (include/mmft_incr.h): which rows of the resident h are stale after a feature edit.
// Byte flags and row copies - index work, latency-bound, no MFMA.  The masked feature MLP, the third entry point of that
// header, is an instantiation of mlp2_feat_fwd_kernel (mlp_feat.hip).
#include "common.h"
#include "../../include/mmft_incr.h"

namespace mmft {

// ---------------------------------------------------------------------------------------------- fan-out cone
// One step of the forward closure, pulled: a node of the level is marked if it is a seed or an in-neighbour is marked - the
// mirror of cone_step_kernel (prep.hip), which pushes marks down.  The in-neighbours lie in lower levels, which this launch
// only reads; mark[v] has one writer, its own thread.
__global__ void __launch_bounds__(256) fanout_step_kernel(const int* __restrict__ rows, int row0, int n,
                                                          const int* __restrict__ p0, const int* __restrict__ i0,
                                                          const int* __restrict__ p1, const int* __restrict__ i1,
                                                          const unsigned char* __restrict__ within, unsigned char* mark) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int v = rows ? rows[i] : row0 + i;
  if (within && !within[v]) {
    if (mark[v]) mark[v] = 0;
    return;
  }
  if (mark[v]) return;
  bool m = false;
  for (int e = p0[v]; e < p0[v + 1] && !m; ++e) m = mark[i0[e]] != 0;
  if (p1)
    for (int e = p1[v]; e < p1[v + 1] && !m; ++e) m = mark[i1[e]] != 0;
  if (m) mark[v] = 1;
}

// ---------------------------------------------------------------------------------------------- rows that really changed
// G = 2^LG lanes per row (the smallest power of two >= width), 64 / G rows per wave: lane j of a group reads element j of the
// old and of the new row, stores the new one, and the group's bits of the wave's ballot say whether the row changed.
__global__ void __launch_bounds__(256) update_rows_diff_kernel(float* __restrict__ dst, long long ldd, const int* __restrict__ idx,
                                                               int row0, int n, int width, int LG,
                                                               const float* __restrict__ src, long long lds,
                                                               unsigned char* __restrict__ seed) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int G = 1 << LG, j = (int)(t & (G - 1));
  const long long i = t >> LG;
  bool diff = false;
  int target = -1;
  if (i < n) {
    target = idx ? idx[i] : row0 + (int)i;
    if (j < width) {
      unsigned* d = reinterpret_cast<unsigned*>(dst + (long long)target * ldd + j);
      const unsigned was = *d, now = *reinterpret_cast<const unsigned*>(src + i * lds + j);
      diff = was != now;
      *d = now;
    }
  }
  const unsigned long long b = __ballot(diff);
  const int lane = threadIdx.x & 63, g0 = lane & ~(G - 1);
  const unsigned long long mine = (b >> g0) & (G == 64 ? ~0ull : ((1ull << G) - 1));
  if (j == 0 && target >= 0 && mine) seed[target] = 1;
}

}  // namespace mmft

using namespace mmft;

extern "C" {

int mmft_fanout_cone_step(const int* rows, int row0, int n, const int* in_indptr0, const int* in_indices0,
                          const int* in_indptr1, const int* in_indices1, const unsigned char* within, unsigned char* mark,
                          int device, void* stream) {
  MMFT_REQUIRE(n >= 0 && row0 >= 0, "fanout_cone_step: bad sizes");
  if (n == 0) return MMFT_OK;
  MMFT_REQUIRE(in_indptr0 && in_indices0 && mark, "fanout_cone_step: null pointer");
  MMFT_REQUIRE((in_indptr1 == nullptr) == (in_indices1 == nullptr), "fanout_cone_step: second CSR needs both arrays");
  DeviceGuard dg(device);
  MMFT_LAUNCH("fanout_step_kernel", 0.0, 0.0, fanout_step_kernel, dim3(cdiv(n, 256)), dim3(256), (hipStream_t)stream, rows, row0,
              n, in_indptr0, in_indices0, in_indptr1, in_indices1, within, mark);
  return check_launch("fanout_cone_step");
}

int mmft_update_rows_diff(float* dst, long long ldd, const int* idx, int row0, int n, int width, const float* src,
                          long long lds, unsigned char* seed, int device, void* stream) {
  MMFT_REQUIRE(n >= 0 && row0 >= 0 && width >= 1 && width <= 64 && ldd >= width && lds >= width,
               "update_rows_diff: bad sizes (1 <= width <= 64, pitches >= width)");
  MMFT_REQUIRE((long long)row0 + n <= 0x7fffffffll, "update_rows_diff: row range beyond 2^31");
  if (n == 0) return MMFT_OK;
  MMFT_REQUIRE(dst && src && seed, "update_rows_diff: null pointer");
  DeviceGuard dg(device);
  int LG = 0;
  while ((1 << LG) < width) ++LG;
  MMFT_LAUNCH("update_rows_diff_kernel", 0.0, 12.0 * n * width, update_rows_diff_kernel, dim3(cdiv((long long)n << LG, 256)),
              dim3(256), (hipStream_t)stream, dst, ldd, idx, row0, n, width, LG, src, lds, seed);
  return check_launch("update_rows_diff");
}

}  // extern "C"
