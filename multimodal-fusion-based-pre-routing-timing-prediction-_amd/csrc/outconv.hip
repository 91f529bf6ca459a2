// OutConv of the layout U-Net in one kernel per direction (src/Unet.py:71-82): 1x1 convolution to ONE channel (bias),
// 2x2 pooling, ReLU.
//
// As separate operators the head of the U-Net was a GEMM with N = 1 (a 16-wide tile for one column), a pooling and an
// activation kernel forward, and five launches backward - two of them implicit GEMMs with one input / one output channel
// (50 and 63 us at 8 x 256 x 256 x 16).  The whole thing is a dot product per pixel: HBM-bound, 33 MB in, 0.5 MB out.
//   forward : out[n][y][x] = relu(pool_{2x2}(b + sum_c w[c] x[n][2y + dy][2x + dx][c]))
//   backward: g_p = dL/dout routed through the ReLU and the pooling window (torch's argmax rule: the first maximum in
//             scan order, NaN wins), dx[p][c] = g_p w[c], dw[c] = sum_p g_p x[p][c], db = sum_p g_p.
// Nothing is saved between the two: the backward recomputes the pixel values from x (it needs the argmax anyway).
// A wave covers 32 pixels of an even row (lanes 0-31) and the 32 pixels below them (lanes 32-63): every lane's load is
// Ci contiguous elements, a window's four values meet through three lane exchanges.  The arithmetic is plain fp32 in both
// math modes (the layer is 32 flops per pixel).  Weight-gradient partials: one slab per workgroup, added in a fixed order.
//
// ONE kernel family for both storage forms of x / dx: T = float (cnn.py, Ci 16 / 32) and T = u16 (bf16 bits: UNet16Fn and
// the eval path, Ci 16).  The element type enters through oc_load / oc_store and sizeof(T) only, so on inputs that bf16
// represents the two forms agree bit for bit (tests/test_unet16_gpu.py::test_outconv_bf16_form_is_the_fp32_form).
#include <type_traits>
#include "unet16.h"

namespace mmft {

template <typename T>
struct OutConvArgs {
  const T* x;          // [N][H][W][Ci]
  const float* w;      // [Ci]
  const float* bias;   // [1] or null
  const float* gout;   // [N][H/2][W/2]       (backward)
  float* out;          // [N][H/2][W/2]       (forward)
  T* dx;               // [N][H][W][Ci]       (backward)
  float* slabs;        // [gridDim.x][Ci + 1] (backward)
  int N, H, W, mode;
  long long items;     // N * (H / 2) * (W / 32), set by the launcher
};

// a pixel's Ci values as floats and back: 16-byte accesses of 4 floats / 8 bf16 (dx is rounded to nearest even)
template <int CI>
__device__ __forceinline__ void oc_load(const float* p, float v[CI]) {
#pragma unroll
  for (int c = 0; c < CI; c += 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[c + j] = t[j];
  }
}
template <int CI>
__device__ __forceinline__ void oc_load(const u16* p, float v[CI]) {
#pragma unroll
  for (int c = 0; c < CI; c += 8) unpack8(*reinterpret_cast<const u32x4*>(p + c), v + c);
}
template <int CI>
__device__ __forceinline__ void oc_store(float* p, const float v[CI]) {
#pragma unroll
  for (int c = 0; c < CI; c += 4) *reinterpret_cast<f32x4*>(p + c) = f32x4{v[c], v[c + 1], v[c + 2], v[c + 3]};
}
template <int CI>
__device__ __forceinline__ void oc_store(u16* p, const float v[CI]) {
#pragma unroll
  for (int c = 0; c < CI; c += 8) *reinterpret_cast<u32x4*>(p + c) = pack8(v + c);
}

// this lane's pixel (xv, pix), its place in the window (me) and the pooled value / argmax of the window
template <typename T, int CI>
__device__ __forceinline__ void oc_window(const OutConvArgs<T>& a, long long item, int lane, float xv[CI], float& pooled,
                                          int& arg, int& me, long long& pix, long long& opix) {
  const int wx = a.W / 32;
  const int xb = (int)(item % wx);
  const long long rp = item / wx;                    // n * (H / 2) + y2
  const int y2 = (int)(rp % (a.H / 2));
  const long long n = rp / (a.H / 2);
  const int rowbit = lane >> 5, xx = xb * 32 + (lane & 31);
  pix = (n * a.H + 2 * y2 + rowbit) * a.W + xx;
  opix = rp * (a.W / 2) + (xx >> 1);
  oc_load<CI>(a.x + pix * CI, xv);
  float v = a.bias ? a.bias[0] : 0.f;
#pragma unroll
  for (int c = 0; c < CI; ++c) v = __fmaf_rn(xv[c], a.w[c], v);
  me = rowbit * 2 + (xx & 1);
  const float vx = __shfl_xor(v, 1, 64), vy = __shfl_xor(v, 32, 64), vd = __shfl_xor(v, 33, 64);
  // window values in scan order (0,0) (0,1) (1,0) (1,1), by selects (me differs from lane to lane)
  float q[4];
  q[0] = me == 0 ? v : me == 1 ? vx : me == 2 ? vy : vd;
  q[1] = me == 1 ? v : me == 0 ? vx : me == 3 ? vy : vd;
  q[2] = me == 2 ? v : me == 3 ? vx : me == 0 ? vy : vd;
  q[3] = me == 3 ? v : me == 2 ? vx : me == 1 ? vy : vd;
  if (a.mode == MMFT_POOL_MAX) {
    float m = q[0];
    arg = 0;
#pragma unroll
    for (int j = 1; j < 4; ++j)
      if (q[j] > m || q[j] != q[j]) {               // torch: take val if (val > max) || isnan(val)
        m = q[j];
        arg = j;
      }
    pooled = m;
  } else {
    pooled = (q[0] + q[1] + q[2] + q[3]) * 0.25f;
    arg = -1;
  }
}

template <typename T, int CI>
__global__ void __launch_bounds__(256) outconv_fwd_kernel(OutConvArgs<T> a) {
  const int lane = threadIdx.x & 63;
  for (long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); item < a.items; item += (long long)gridDim.x * 4) {
    float xv[CI], pooled;
    int arg, me;
    long long pix, opix;
    oc_window<T, CI>(a, item, lane, xv, pooled, arg, me, pix, opix);
    if (me == 0) a.out[opix] = pooled > 0.f ? pooled : 0.f;
  }
}

template <typename T, int CI>
__global__ void __launch_bounds__(256) outconv_bwd_kernel(OutConvArgs<T> a) {
  __shared__ float red[4][CI + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc[CI + 1];
#pragma unroll
  for (int c = 0; c <= CI; ++c) acc[c] = 0.f;
  for (long long item = (long long)blockIdx.x * 4 + wave; item < a.items; item += (long long)gridDim.x * 4) {
    float xv[CI], pooled;
    int arg, me;
    long long pix, opix;
    oc_window<T, CI>(a, item, lane, xv, pooled, arg, me, pix, opix);
    float g = a.gout[opix];
    if (!(pooled > 0.f)) g = 0.f;                                       // ReLU (mask from the output, as ActFn)
    g = a.mode == MMFT_POOL_MAX ? (me == arg ? g : 0.f) : g * 0.25f;
    float d[CI];
#pragma unroll
    for (int c = 0; c < CI; ++c) {
      d[c] = a.w[c] * g;
      acc[c] = __fmaf_rn(g, xv[c], acc[c]);
    }
    acc[CI] += g;
    oc_store<CI>(a.dx + pix * CI, d);
  }
  // wave sums (butterfly: every lane ends with the total), then the four waves in order
#pragma unroll
  for (int c = 0; c <= CI; ++c) {
    float v = acc[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wave][c] = v;
  }
  __syncthreads();
  if (threadIdx.x <= CI)
    a.slabs[(long long)blockIdx.x * (CI + 1) + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// dw[c] / db = sum of the slabs, fixed order: 8 partial sums per element combined through LDS
__global__ void __launch_bounds__(512) outconv_reduce_kernel(const float* __restrict__ slabs, int nslab, int CI,
                                                             float* __restrict__ dw, float* __restrict__ db, int accumulate) {
  __shared__ float part[8][64];
  const int e = threadIdx.x & 63, p = threadIdx.x >> 6;
  float s = 0.f;
  if (e <= CI)
    for (int b = p; b < nslab; b += 8) s += slabs[(long long)b * (CI + 1) + e];
  part[p][e] = s;
  __syncthreads();
  if (p == 0 && e <= CI) {
    float t = 0.f;
    for (int k = 0; k < 8; ++k) t += part[k][e];
    float* dst = e < CI ? dw + e : db;
    if (dst) *dst = accumulate ? *dst + t : t;
  }
}

// names of the bf16-storage form (entry points in messages, kernels in the profiler) carry the family's u16_ prefix
#define OC_NAME(T, s) (std::is_same<T, u16>::value ? "u16_" s : s)

template <typename T>
static inline bool outconv_ok(int H, int W, int Ci) {
  return (Ci == 16 || (Ci == 32 && std::is_same<T, float>::value)) && H % 2 == 0 && W % 32 == 0;
}

static inline long long outconv_items(int N, int H, int W) { return (long long)N * (H / 2) * (W / 32); }

static inline int outconv_grid(long long items) {
  long long g = (items + 3) / 4;
  if (g > 1024) g = 1024;
  return (int)(g < 1 ? 1 : g);
}

// one slab of Ci + 1 floats per workgroup: [dw[Ci] | db]
static inline long long outconv_slab_bytes(int N, int H, int W, int Ci) {
  return (long long)outconv_grid(outconv_items(N, H, W)) * (Ci + 1) * 4;
}

// w is read element by element; the fp32 entry points have always asked for an aligned one, the bf16 ones never
template <typename T>
static inline bool outconv_w_ok(const float* w) { return std::is_same<T, u16>::value || aligned16(w); }

template <typename T>
static int launch_outconv_fwd(OutConvArgs<T> a, int Ci, int device, void* stream) {
  const char* what = OC_NAME(T, "outconv_fwd");
  MMFT_REQUIRE(a.x && a.w && a.out && a.N > 0 && (a.mode == MMFT_POOL_MAX || a.mode == MMFT_POOL_AVG), "%s: bad arguments", what);
  MMFT_REQUIRE(outconv_ok<T>(a.H, a.W, Ci), "%s: needs Ci = 16 (fp32 form: or 32), even H, W %% 32 == 0", what);
  MMFT_REQUIRE(aligned16(a.x) && outconv_w_ok<T>(a.w), "%s: x / w must be 16-byte aligned", what);
  DeviceGuard dg(device);
  a.items = outconv_items(a.N, a.H, a.W);
  const dim3 grid(outconv_grid(a.items));
  const double px = 1.0 * a.N * a.H * a.W, flops = 2.0 * px * Ci, by = sizeof(T) * px * Ci + px;
  if (Ci == 16)
    MMFT_LAUNCH(OC_NAME(T, "outconv_fwd_kernel"), flops, by, (outconv_fwd_kernel<T, 16>), grid, dim3(256), (hipStream_t)stream, a);
  else if constexpr (std::is_same<T, float>::value)
    MMFT_LAUNCH(OC_NAME(T, "outconv_fwd_kernel"), flops, by, (outconv_fwd_kernel<T, 32>), grid, dim3(256), (hipStream_t)stream, a);
  return check_launch(what);
}

// dw == NULL: no reduction, the slabs stay in a.slabs
template <typename T>
static int launch_outconv_bwd(OutConvArgs<T> a, int Ci, long long workspace_bytes, float* dw, float* db, int accumulate,
                              int device, void* stream) {
  const char* what = OC_NAME(T, "outconv_bwd");
  MMFT_REQUIRE(a.x && a.w && a.gout && a.dx && a.N > 0 && (a.mode == MMFT_POOL_MAX || a.mode == MMFT_POOL_AVG), "%s: bad arguments", what);
  MMFT_REQUIRE(outconv_ok<T>(a.H, a.W, Ci), "%s: needs Ci = 16 (fp32 form: or 32), even H, W %% 32 == 0", what);
  MMFT_REQUIRE(aligned16(a.x) && outconv_w_ok<T>(a.w) && aligned16(a.dx), "%s: x / w / dx must be 16-byte aligned", what);
  MMFT_REQUIRE(a.slabs && workspace_bytes >= outconv_slab_bytes(a.N, a.H, a.W, Ci), "%s: workspace too small", what);
  DeviceGuard dg(device);
  hipStream_t st = (hipStream_t)stream;
  a.items = outconv_items(a.N, a.H, a.W);
  const int grid = outconv_grid(a.items);
  const double px = 1.0 * a.N * a.H * a.W, flops = 4.0 * px * Ci, by = 2.0 * sizeof(T) * px * Ci + px;
  if (Ci == 16)
    MMFT_LAUNCH(OC_NAME(T, "outconv_bwd_kernel"), flops, by, (outconv_bwd_kernel<T, 16>), dim3(grid), dim3(256), st, a);
  else if constexpr (std::is_same<T, float>::value)
    MMFT_LAUNCH(OC_NAME(T, "outconv_bwd_kernel"), flops, by, (outconv_bwd_kernel<T, 32>), dim3(grid), dim3(256), st, a);
  int rc = check_launch(what);
  if (rc || !dw) return rc;
  hipLaunchKernelGGL(outconv_reduce_kernel, dim3(1), dim3(512), 0, st, a.slabs, grid, Ci, dw, db, accumulate ? 1 : 0);
  return check_launch(OC_NAME(T, "outconv_reduce"));
}

}  // namespace mmft

using namespace mmft;

extern "C" {

int mmft_outconv_supported(int H, int W, int Ci) { return outconv_ok<float>(H, W, Ci) ? 1 : 0; }

int mmft_outconv_fwd(const float* x, const float* w, const float* bias, float* out, int Nimg, int H, int W, int Ci, int mode,
                     int device, void* stream) {
  return launch_outconv_fwd(OutConvArgs<float>{x, w, bias, nullptr, out, nullptr, nullptr, Nimg, H, W, mode, 0}, Ci, device, stream);
}

long long mmft_outconv_bwd_workspace_bytes(int Nimg, int H, int W, int Ci) {
  return Nimg > 0 && outconv_ok<float>(H, W, Ci) ? outconv_slab_bytes(Nimg, H, W, Ci) : 0;
}

int mmft_outconv_bwd(const float* x, const float* w, const float* bias, const float* gout, float* dx, float* dw, float* db,
                     int accumulate, int Nimg, int H, int W, int Ci, int mode, float* workspace, long long workspace_bytes,
                     int device, void* stream) {
  MMFT_REQUIRE(dw, "outconv_bwd: bad arguments");          // this form always reduces
  return launch_outconv_bwd(OutConvArgs<float>{x, w, bias, gout, nullptr, dx, workspace, Nimg, H, W, mode, 0}, Ci, workspace_bytes,
                            dw, db, accumulate, device, stream);
}

int mmft_u16_outconv_fwd(const void* x, const float* w, const float* bias, float* out, int N, int H, int W, int mode, int device,
                         void* stream) {
  return launch_outconv_fwd(OutConvArgs<u16>{reinterpret_cast<const u16*>(x), w, bias, nullptr, out, nullptr, nullptr, N, H, W, mode, 0},
                            16, device, stream);
}

long long mmft_u16_outconv_bwd_workspace_bytes(int N, int H, int W) { return outconv_slab_bytes(N, H, W, 16); }

int mmft_u16_outconv_bwd_slabs(int N, int H, int W) { return outconv_grid(outconv_items(N, H, W)); }

/* dw == NULL: the slabs stay in `workspace` for mmft_slab_reduce_batch */
int mmft_u16_outconv_bwd(const void* x, const float* w, const float* bias, const float* gout, void* dx, float* dw, float* db,
                         int accumulate, int N, int H, int W, int mode, float* workspace, long long workspace_bytes, int device,
                         void* stream) {
  return launch_outconv_bwd(OutConvArgs<u16>{reinterpret_cast<const u16*>(x), w, bias, gout, nullptr, reinterpret_cast<u16*>(dx),
                                             workspace, N, H, W, mode, 0},
                            16, workspace_bytes, dw, db, accumulate, device, stream);
}

}  // extern "C"
