// The fusion head's mlp_fuse, MLP(288, 576, 1) over the T sampled endpoints of a batch (src/model.py:267,291), bf16 math mode:
// forward and backward as three fused kernels (include/mmft_head.h) in place of ten launches of the generic layer path.
//
// The head runs alone between the join of the step's two streams and the start of the reverse sweep: one small
// kernel at a time on an otherwise idle chip, so launches and passes over memory come off the wall clock in full.  The generic
// path writes a fp32 hidden tensor (25 MB, read three times) and a fp32 hidden gradient made by a rank-1 "GEMM" (25 MB, read
// three times).  Here the only tensor between forward and backward is r(h) in bf16 (12 MB); the hidden gradient
//   g1[t][j] = [r(h)[t][j] > 0] * r(dpred[t]) * r(w2[j])          (an exact fp32 product of two bf16 values)
// is recomputed where it is consumed and never stored.  The ReLU mask is read from r(h), not from h: the two differ only
// where h is an fp32 denormal (it rounds to a bf16 denormal or to zero; the MFMA flushes such operands anyway).
//
//   head_mlp_fwd_kernel<KEEP>   64 rows per workgroup (T = 10 800: 169 workgroups, one round on 256 CUs), 12 waves x 3 hidden
//                               16-blocks.  x tile -> LDS as bf16; W1 [576][288] is already the [n][k] order of an A fragment:
//                               read as fp32 from L2 two k-steps ahead and rounded in registers (no pack, no extra launch).
//                               r(h) is stored once (KEEP) and pred = r(h) . r(w2) + b2 is reduced lane -> wave -> LDS in a
//                               fixed order.  KEEP = false is the same instruction stream without the stores.
//   head_mlp_bwd_dx_kernel      same tiling.  g1 -> LDS as bf16 from r(h), dpred, w2; dx = r(g1) r(W1) with A fragments from
//                               the transposed bf16 pack of W1 made by this call; db1 / dW2 / db2 partial rows per workgroup.
//   head_mlp_wgrad_kernel       dW1 = r(g1)^T r(x): the pattern of rows_outer.hip (32-row chunks in natural layout in LDS,
//                               ds_read_b64_tr_b16 operands), 192 x 96 output tiles x row shares, one slab per workgroup.
// All partial results are added by ONE slab_reduce_batch launch in its fixed order.  No atomics, no cross-workgroup
// synchronisation; every global access is predicated on row < T.
#include "mlp_tile_bf16.h"
#include "tr_read.h"
#include "unet16.h"
#include "../../include/mmft_head.h"

namespace mmft {

constexpr int HM_IN = 288, HM_HD = 576;
constexpr int HM_ROWS = 64;                          // rows per workgroup (forward, dx)
constexpr int HM_WAVES = 12, HM_THREADS = 64 * HM_WAVES;
constexpr int HM_PX = HM_IN + 8, HM_PG = HM_HD + 8;  // LDS row pitches in bf16 elements (16-byte rows, conflict-free b128 reads)
constexpr int HM_KS1 = HM_IN / 32, HM_KS2 = HM_HD / 32;
constexpr int HM_PART = 2 * HM_HD + 4;               // partial row of a dx workgroup: [db1 576 | dW2 576 | db2, 3 unused]
constexpr int HM_STAGE = HM_HD / 8;                  // dx staging: 72 column groups of 8 ...
constexpr int HM_RL = 8;                             // ... x 8 row lanes = 576 staging threads

// weight gradient
constexpr int HW_JT = 192, HW_IT = 96, HW_KT = 32;   // output tile (hidden x in), rows per chunk
constexpr int HW_TILES = (HM_HD / HW_JT) * (HM_IN / HW_IT);
constexpr int HW_PG = HW_JT + 16, HW_PX = HW_IT + 16;   // 8 x odd dwords: conflict-free transposed reads (tr_read.h)
constexpr int HW_MAX_SHARES = 28;                    // 9 tiles x at most 28 row shares (T = 10 800: 26 shares, 234 workgroups)

__device__ __forceinline__ float round_bf16(float v) { return bf2f(f2bf(v)); }
__device__ __forceinline__ bf16x8 as_bf16x8(u32x4 v) { return __builtin_bit_cast(bf16x8, v); }

struct HeadFwdArgs {
  const float* x;
  long long ldx;
  const float *w1, *b1, *w2, *b2;
  u16* hid;
  float* pred;
  long long T;
};

template <bool KEEP>
__global__ void __launch_bounds__(HM_THREADS) head_mlp_fwd_kernel(HeadFwdArgs a) {
  __shared__ __attribute__((aligned(16))) u16 xs[HM_ROWS * HM_PX];
  __shared__ float red[HM_WAVES][HM_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, q = lane >> 4;
  const long long t0 = (long long)blockIdx.x * HM_ROWS;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // A fragments: hidden unit 48 wave + 16 c + r16, k = 32 ks + 8 q .. + 7 - two 16-byte fp32 loads each, two k-steps ahead
  const float* wrow[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) wrow[c] = a.w1 + (long long)(wave * 48 + c * 16 + r16) * HM_IN + q * 8;
  f32x4 wr[2][3][2];
  auto wload = [&](int slot, int ks) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      wr[slot][c][0] = *reinterpret_cast<const f32x4*>(wrow[c] + ks * 32);
      wr[slot][c][1] = *reinterpret_cast<const f32x4*>(wrow[c] + ks * 32 + 4);
    }
  };
  wload(0, 0);
  wload(1, 1);

  // the x tile: fp32 -> bf16, 16-byte loads, 8-byte LDS stores; rows at and beyond T are zeros
  constexpr int XI = HM_ROWS * (HM_IN / 4) / HM_THREADS;
  static_assert(HM_ROWS * (HM_IN / 4) % HM_THREADS == 0, "staging granularity");
  f32x4 xr[XI];
#pragma unroll
  for (int k = 0; k < XI; ++k) {
    const int it = tid + k * HM_THREADS, row = it / (HM_IN / 4), c4 = it % (HM_IN / 4);
    xr[k] = t0 + row < a.T ? *reinterpret_cast<const f32x4*>(a.x + (t0 + row) * a.ldx + c4 * 4) : zero;
  }
#pragma unroll
  for (int k = 0; k < XI; ++k) {
    const int it = tid + k * HM_THREADS, row = it / (HM_IN / 4), c4 = it % (HM_IN / 4);
    *reinterpret_cast<s16x4*>(xs + row * HM_PX + c4 * 4) = pack_bf16x4(xr[k]);
  }
  __syncthreads();

  f32x4 acc[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[i][c] = zero;
#pragma unroll
  for (int ks = 0; ks < HM_KS1; ++ks) {
    bf16x8 af[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x4 lo = wr[ks & 1][c][0], hi = wr[ks & 1][c][1];
      af[c] = as_bf16x8(u32x4{pack_bf16(lo.x, lo.y), pack_bf16(lo.z, lo.w), pack_bf16(hi.x, hi.y), pack_bf16(hi.z, hi.w)});
    }
    if (ks + 2 < HM_KS1) wload(ks & 1, ks + 2);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bf16x8 xf = *reinterpret_cast<const bf16x8*>(xs + (i * 16 + r16) * HM_PX + ks * 32 + q * 8);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[c], xf, acc[i][c], 0, 0, 0);
    }
  }

  // the lane holds hidden units f0 .. f0 + 3 of row 16 i + r16: bias, ReLU, ONE rounding to bf16 - what is stored is what the
  // second layer multiplies.  pred: units in ascending order per lane, then q (lanes +16, +32), then the 12 waves in order.
  float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int f0 = wave * 48 + c * 16 + q * 4;
    const f32x4 b1v = *reinterpret_cast<const f32x4*>(a.b1 + f0), w2v = *reinterpret_cast<const f32x4*>(a.w2 + f0);
    const float w2r[4] = {round_bf16(w2v.x), round_bf16(w2v.y), round_bf16(w2v.z), round_bf16(w2v.w)};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4 v = relu4(acc[i][c] + b1v);
      const unsigned lo = pack_bf16(v.x, v.y), hi = pack_bf16(v.z, v.w);
      const long long t = t0 + i * 16 + r16;
      if (KEEP && t < a.T) *reinterpret_cast<u32x2*>(a.hid + t * HM_HD + f0) = u32x2{lo, hi};
      p[i] += __uint_as_float(lo << 16) * w2r[0];
      p[i] += __uint_as_float(lo & 0xffff0000u) * w2r[1];
      p[i] += __uint_as_float(hi << 16) * w2r[2];
      p[i] += __uint_as_float(hi & 0xffff0000u) * w2r[3];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p[i] += __shfl_xor(p[i], 16);
    p[i] += __shfl_xor(p[i], 32);
    if (q == 0) red[wave][i * 16 + r16] = p[i];
  }
  __syncthreads();
  if (tid < HM_ROWS && t0 + tid < a.T) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < HM_WAVES; ++w) s += red[w][tid];
    a.pred[t0 + tid] = s + a.b2[0];
  }
}

// w1t[i][j] (bf16) = w1[j][i]: the [n][k] order of dx = g1 W1 (n = input feature, k = hidden unit).  Indexed by the
// destination (coalesced stores); the strided reads of the 660 KB weight hit L2.
__global__ void __launch_bounds__(256) head_mlp_pack_w1t_kernel(const float* __restrict__ w1, u16* __restrict__ w1t) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < HM_IN * HM_HD) {
    const int i = idx / HM_HD, j = idx - i * HM_HD;
    w1t[idx] = (u16)f2bf(w1[j * HM_IN + i]);
  }
}

struct HeadDxArgs {
  const float* dpred;
  const u16* hid;
  const u16* w1t;
  const float* w2;
  float* dx;          // NULL: only the partial rows
  long long lddx;
  float* part;        // [gridDim.x][HM_PART]
  long long T;
};

constexpr int HM_DX_LDS = HM_ROWS * HM_PG * 2 + HM_RL * 2 * HM_HD * 4 + HM_ROWS * 4;

__global__ void __launch_bounds__(HM_THREADS) head_mlp_bwd_dx_kernel(HeadDxArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hm_smem[];
  u16* gs = reinterpret_cast<u16*>(hm_smem);                                             // [64][HM_PG] r(g1)
  float* colp = reinterpret_cast<float*>(hm_smem + HM_ROWS * HM_PG * 2);                 // [8 row lanes][db1 576 | dW2 576]
  float* dps = colp + HM_RL * 2 * HM_HD;                                                 // [64] dpred of the tile
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, q = lane >> 4;
  const long long t0 = (long long)blockIdx.x * HM_ROWS;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // A fragments of dx: input feature 48 cgp + 16 c + r16, k = hidden unit 32 ks + 8 q .. + 7 (one 16-byte load of the pack),
  // two k-steps ahead; wave = (row half rg, column group cgp)
  const int cgp = wave % 6, rg = wave / 6;
  const u16* wrow[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) wrow[c] = a.w1t + (long long)(cgp * 48 + c * 16 + r16) * HM_HD + q * 8;
  bf16x8 wa[3][3];
  auto wload = [&](int slot, int ks) {
#pragma unroll
    for (int c = 0; c < 3; ++c) wa[slot][c] = *reinterpret_cast<const bf16x8*>(wrow[c] + ks * 32);
  };
  if (a.dx) {
    wload(0, 0);
    wload(1, 1);
  }

  if (tid < HM_ROWS) dps[tid] = t0 + tid < a.T ? a.dpred[t0 + tid] : 0.f;
  __syncthreads();

  // g1 of the tile: thread = (8 hidden units cg, row lane rl), rows rl, rl + 8, ..; its column sums stay in registers
  if (tid < HM_STAGE * HM_RL) {
    const int cg = tid % HM_STAGE, rl = tid / HM_STAGE;
    const f32x4 wlo = *reinterpret_cast<const f32x4*>(a.w2 + cg * 8), whi = *reinterpret_cast<const f32x4*>(a.w2 + cg * 8 + 4);
    const float w2r[8] = {round_bf16(wlo.x), round_bf16(wlo.y), round_bf16(wlo.z), round_bf16(wlo.w),
                          round_bf16(whi.x), round_bf16(whi.y), round_bf16(whi.z), round_bf16(whi.w)};
    u32x4 hv[HM_ROWS / HM_RL];
#pragma unroll
    for (int rr = 0; rr < HM_ROWS / HM_RL; ++rr) {
      const long long t = t0 + rl + HM_RL * rr;
      hv[rr] = t < a.T ? *reinterpret_cast<const u32x4*>(a.hid + t * HM_HD + cg * 8) : u32x4{0u, 0u, 0u, 0u};
    }
    // the thread's 8 rows are added as a balanced tree (a binary counter over rr: lv[k] holds a finished sum of 2^k rows),
    // not as a chain: the column sums keep the error of a pairwise sum
    static_assert(HM_ROWS / HM_RL == 8, "three tree levels");
    float sb0[8], sb1[8], sb2[8], sw0[8], sw1[8], sw2[8];
#pragma unroll
    for (int rr = 0; rr < HM_ROWS / HM_RL; ++rr) {
      const int row = rl + HM_RL * rr;
      const float dpr = round_bf16(dps[row]);
      float h[8], g[8];
      unpack8(hv[rr], h);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        g[e] = h[e] > 0.f ? dpr * w2r[e] : 0.f;
        float vb = g[e], vw = dpr * h[e];
        if ((rr & 1) == 0) {
          sb0[e] = vb; sw0[e] = vw;
        } else {
          vb = sb0[e] + vb; vw = sw0[e] + vw;
          if ((rr & 2) == 0) {
            sb1[e] = vb; sw1[e] = vw;
          } else {
            vb = sb1[e] + vb; vw = sw1[e] + vw;
            if ((rr & 4) == 0) {
              sb2[e] = vb; sw2[e] = vw;
            } else {
              sb2[e] = sb2[e] + vb; sw2[e] = sw2[e] + vw;
            }
          }
        }
      }
      *reinterpret_cast<u32x4*>(gs + row * HM_PG + cg * 8) = pack8(g);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      colp[rl * 2 * HM_HD + cg * 8 + e] = sb2[e];
      colp[rl * 2 * HM_HD + HM_HD + cg * 8 + e] = sw2[e];
    }
  }
  __syncthreads();

  // partial rows: the 8 row lanes and - db2 - the tile's 64 dpred, both as balanced trees in a fixed order
  float* part = a.part + (long long)blockIdx.x * HM_PART;
  for (int j = tid; j < 2 * HM_HD; j += HM_THREADS) {
    const float* c = colp + j;
    constexpr int S = 2 * HM_HD;
    part[j] = ((c[0] + c[S]) + (c[2 * S] + c[3 * S])) + ((c[4 * S] + c[5 * S]) + (c[6 * S] + c[7 * S]));
  }
  if (wave == HM_WAVES - 1) {
    float s = dps[lane];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
    if (lane == 0) part[2 * HM_HD] = s;
  }
  if (!a.dx) return;

  f32x4 acc[2][3];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[b][c] = zero;
#pragma unroll
  for (int ks = 0; ks < HM_KS2; ++ks) {
    if (ks + 2 < HM_KS2) wload((ks + 2) % 3, ks + 2);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const bf16x8 gf = *reinterpret_cast<const bf16x8*>(gs + ((rg * 2 + b) * 16 + r16) * HM_PG + ks * 32 + q * 8);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[b][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[ks % 3][c], gf, acc[b][c], 0, 0, 0);
    }
  }
  // the lane holds input features 48 cgp + 16 c + 4 q .. + 3 of row 16 (2 rg + b) + r16
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const long long t = t0 + (rg * 2 + b) * 16 + r16;
    if (t < a.T) {
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(a.dx + t * a.lddx + cgp * 48 + c * 16 + q * 4) = acc[b][c];
    }
  }
}

struct HeadWgradArgs {
  const float* dpred;
  const u16* hid;
  const float* w2;
  const float* x;
  long long ldx;
  float* slabs;       // [shares][576][288]: workgroup (tile, share) writes its 192 x 96 block of slab `share`
  long long T;
  int chunks, cps;    // 32-row chunks in all, chunks per share
};

__global__ void __launch_bounds__(256) head_mlp_wgrad_kernel(HeadWgradArgs a) {
  constexpr int MW = HW_JT / 32, NW = HW_IT / 32;                    // 16-blocks per wave: 4 waves as 2 x 2
  constexpr int GG = HW_JT / 4, XG = HW_IT / 4;                      // 4-element items per row
  constexpr int NG = HW_KT * GG / 256, NX = HW_KT * XG / 256;
  static_assert(HW_KT * GG % 256 == 0 && HW_KT * XG % 256 == 0 && (3 * 256) % GG == 0 && NG % 3 == 0, "staging granularity");
  __shared__ __attribute__((aligned(16))) u16 gs[HW_KT * HW_PG];
  __shared__ __attribute__((aligned(16))) u16 xs[HW_KT * HW_PX];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int tile = blockIdx.x % HW_TILES, share = blockIdx.x / HW_TILES;
  const int j0 = (tile / (HM_IN / HW_IT)) * HW_JT, i0 = (tile % (HM_IN / HW_IT)) * HW_IT;
  const int c_begin = share * a.cps, c_end = c_begin + a.cps < a.chunks ? c_begin + a.cps : a.chunks;
  const int tr_row = tr_lane_row(lane), tr_col = tr_lane_col(lane);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[MW][NW];
#pragma unroll
  for (int i = 0; i < MW; ++i)
#pragma unroll
    for (int j = 0; j < NW; ++j) acc[i][j] = zero;
  // item k of a thread lies in column group (tid + 256 k) % 48, which repeats every three items
  float w2r[3][4];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(a.w2 + j0 + ((tid + 256 * m) % GG) * 4);
    w2r[m][0] = round_bf16(v.x); w2r[m][1] = round_bf16(v.y); w2r[m][2] = round_bf16(v.z); w2r[m][3] = round_bf16(v.w);
  }
  u32x2 hr[NG];
  float dpk[NG];
  f32x4 xr[NX];
  auto request = [&](int chunk) {
    const long long r0 = (long long)chunk * HW_KT;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
      const int it = tid + k * 256, col = (it % GG) * 4, row = it / GG;
      const bool ok = r0 + row < a.T;
      hr[k] = ok ? *reinterpret_cast<const u32x2*>(a.hid + (r0 + row) * HM_HD + j0 + col) : u32x2{0u, 0u};
      dpk[k] = ok ? a.dpred[r0 + row] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      const int it = tid + k * 256, col = (it % XG) * 4, row = it / XG;
      xr[k] = r0 + row < a.T ? *reinterpret_cast<const f32x4*>(a.x + (r0 + row) * a.ldx + i0 + col) : zero;
    }
  };
  auto deposit = [&]() {
#pragma unroll
    for (int k = 0; k < NG; ++k) {
      const int it = tid + k * 256, col = (it % GG) * 4, row = it / GG;
      const float dpr = round_bf16(dpk[k]);
      float h[4];
      unpack4(hr[k], h);
      const f32x4 g = {h[0] > 0.f ? dpr * w2r[k % 3][0] : 0.f, h[1] > 0.f ? dpr * w2r[k % 3][1] : 0.f,
                       h[2] > 0.f ? dpr * w2r[k % 3][2] : 0.f, h[3] > 0.f ? dpr * w2r[k % 3][3] : 0.f};
      *reinterpret_cast<s16x4*>(gs + row * HW_PG + col) = pack_bf16x4(g);
    }
#pragma unroll
    for (int k = 0; k < NX; ++k) {
      const int it = tid + k * 256, col = (it % XG) * 4, row = it / XG;
      *reinterpret_cast<s16x4*>(xs + row * HW_PX + col) = pack_bf16x4(xr[k]);
    }
  };
  if (c_begin < c_end) request(c_begin);
  for (int chunk = c_begin; chunk < c_end; ++chunk) {
    deposit();
    __syncthreads();
    if (chunk + 1 < c_end) request(chunk + 1);
    tr_bf16x8 af[MW];
#pragma unroll
    for (int i = 0; i < MW; ++i) af[i] = tr_read_pair(gs + tr_row * HW_PG + (wm * MW + i) * 16 + tr_col, 16 * HW_PG);
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const tr_bf16x8 bfr = tr_read_pair(xs + tr_row * HW_PX + (wn * NW + j) * 16 + tr_col, 16 * HW_PX);
#pragma unroll
      for (int i = 0; i < MW; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr, acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  // acc[i][j][e] at lane (r, q) = dW1[j0 + 16 (wm MW + i) + 4 q + e][i0 + 16 (wn NW + j) + r]; a share without chunks writes zeros
  const int r = lane & 15, q = lane >> 4;
  float* slab = a.slabs + (long long)share * (HM_HD * HM_IN);
#pragma unroll
  for (int i = 0; i < MW; ++i)
#pragma unroll
    for (int j = 0; j < NW; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        slab[(long long)(j0 + (wm * MW + i) * 16 + 4 * q + e) * HM_IN + i0 + (wn * NW + j) * 16 + r] = acc[i][j][e];
}

// row shares of the weight gradient: at least four 32-row chunks per slab, at most HW_MAX_SHARES, no empty share
static inline int head_shares(long long T, int* chunks_out, int* cps_out) {
  const int chunks = (int)((T + HW_KT - 1) / HW_KT);
  int shares = chunks / 4;
  if (shares > HW_MAX_SHARES) shares = HW_MAX_SHARES;
  if (shares < 1) shares = 1;
  const int cps = (chunks + shares - 1) / shares;
  if (chunks_out) *chunks_out = chunks;
  if (cps_out) *cps_out = cps;
  return (chunks + cps - 1) / cps;
}

constexpr long long HM_PACK_FLOATS = (long long)HM_IN * HM_HD / 2;          // the bf16 pack, counted in floats
static inline long long head_tiles(long long T) { return (T + HM_ROWS - 1) / HM_ROWS; }
constexpr long long HM_MAX_T = 1ll << 24;

}  // namespace mmft

using namespace mmft;

extern "C" {

long long mmft_head_mlp_supported(int in, int hidden, int out) { return (in == HM_IN && hidden == HM_HD && out == 1) ? 1 : 0; }

/* [W1^T bf16 pack | partial rows of the dx workgroups | dW1 slabs], in bytes; -1 outside 1 <= T <= 2^24 */
long long mmft_head_mlp_workspace_bytes(long long T) {
  if (T <= 0 || T > HM_MAX_T) {
    set_error("head_mlp_workspace_bytes: T must be in [1, 2^24] (got %lld)", T);
    return -1;
  }
  return 4 * (HM_PACK_FLOATS + head_tiles(T) * HM_PART + (long long)head_shares(T, nullptr, nullptr) * HM_HD * HM_IN);
}

int mmft_head_mlp_fwd(const float* x, long long ldx, const float* w1, const float* b1, const float* w2, const float* b2,
                      void* hid, float* pred, long long T, int in, int hidden, int out, int device, void* stream) {
  MMFT_REQUIRE(x && w1 && b1 && w2 && b2 && pred, "head_mlp_fwd: null pointer");
  MMFT_REQUIRE(T > 0 && T <= HM_MAX_T, "head_mlp_fwd: T must be in [1, 2^24] (got %lld)", T);
  MMFT_REQUIRE(mmft_head_mlp_supported(in, hidden, out), "head_mlp_fwd: (in, hidden, out) must be (288, 576, 1), got (%d, %d, %d)",
               in, hidden, out);
  MMFT_REQUIRE(ldx >= HM_IN && ldx % 4 == 0 && aligned16(x) && aligned16(w1) && aligned16(b1) && aligned16(w2) && (!hid || aligned16(hid)),
               "head_mlp_fwd: rows must be 16-byte aligned");
  DeviceGuard dg(device);
  hipStream_t st = (hipStream_t)stream;
  HeadFwdArgs a{x, ldx, w1, b1, w2, b2, (u16*)hid, pred, T};
  const int grid = (int)head_tiles(T);
  const double fl = 2.0 * T * HM_HD * (HM_IN + 1.0), wby = 4.0 * HM_HD * (HM_IN + 2.0);
  if (hid) {
    MMFT_LAUNCH("head_mlp_fwd_kernel<keep>", fl, T * (4.0 * HM_IN + 2.0 * HM_HD + 4.0) + wby, head_mlp_fwd_kernel<true>, dim3(grid),
                dim3(HM_THREADS), st, a);
  } else {
    MMFT_LAUNCH("head_mlp_fwd_kernel<nokeep>", fl, T * (4.0 * HM_IN + 4.0) + wby, head_mlp_fwd_kernel<false>, dim3(grid),
                dim3(HM_THREADS), st, a);
  }
  return check_launch("head_mlp_fwd");
}

int mmft_head_mlp_bwd(const float* dpred, const void* hid, const float* x, long long ldx, const float* w1, const float* w2,
                      float* dx, long long lddx, float* dw1, float* db1, float* dw2, float* db2,
                      long long T, int in, int hidden, int out, int accumulate,
                      void* workspace, long long workspace_bytes, int device, void* stream) {
  MMFT_REQUIRE(dpred && hid && x && w1 && w2 && dw1 && db1 && dw2 && db2, "head_mlp_bwd: null pointer");
  MMFT_REQUIRE(T > 0 && T <= HM_MAX_T, "head_mlp_bwd: T must be in [1, 2^24] (got %lld)", T);
  MMFT_REQUIRE(mmft_head_mlp_supported(in, hidden, out), "head_mlp_bwd: (in, hidden, out) must be (288, 576, 1), got (%d, %d, %d)",
               in, hidden, out);
  MMFT_REQUIRE(ldx >= HM_IN && ldx % 4 == 0 && aligned16(x) && aligned16(hid) && aligned16(w1) && aligned16(w2) && aligned16(dw1) &&
                   aligned16(db1) && aligned16(dw2) && (!dx || (lddx >= HM_IN && lddx % 4 == 0 && aligned16(dx))),
               "head_mlp_bwd: rows must be 16-byte aligned");
  MMFT_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= mmft_head_mlp_workspace_bytes(T),
               "head_mlp_bwd: workspace too small (%lld bytes given)", workspace_bytes);
  DeviceGuard dg(device);
  hipStream_t st = (hipStream_t)stream;
  static DynLdsOnce once;
  int rc = ensure_dyn_lds(once, reinterpret_cast<const void*>(&head_mlp_bwd_dx_kernel), HM_DX_LDS, "head_mlp_bwd");
  if (rc) return rc;
  const int tiles = (int)head_tiles(T);
  int chunks, cps;
  const int shares = head_shares(T, &chunks, &cps);
  float* ws = (float*)workspace;
  u16* w1t = (u16*)ws;
  float* part = ws + HM_PACK_FLOATS;
  float* slabs = part + (long long)tiles * HM_PART;

  MMFT_LAUNCH("head_mlp_pack_w1t_kernel", 0.0, 6.0 * HM_IN * HM_HD, head_mlp_pack_w1t_kernel, dim3(cdiv(HM_IN * HM_HD, 256)), dim3(256), st,
              w1, w1t);
  rc = check_launch("head_mlp_bwd (pack)");
  if (rc) return rc;
  HeadDxArgs da{dpred, (const u16*)hid, w1t, w2, dx, lddx, part, T};
  MMFT_LAUNCH_LDS("head_mlp_bwd_dx_kernel", (dx ? 2.0 * T * HM_HD * HM_IN : 0.0) + 4.0 * T * HM_HD,
                  T * (2.0 * HM_HD + 4.0 + (dx ? 4.0 * HM_IN : 0.0)) + 2.0 * HM_IN * HM_HD + 4.0 * tiles * HM_PART, head_mlp_bwd_dx_kernel,
                  dim3(tiles), dim3(HM_THREADS), HM_DX_LDS, st, da);
  rc = check_launch("head_mlp_bwd (dx)");
  if (rc) return rc;
  HeadWgradArgs wa{dpred, (const u16*)hid, w2, x, ldx, slabs, T, chunks, cps};
  MMFT_LAUNCH("head_mlp_wgrad_kernel", 2.0 * T * HM_HD * HM_IN,
              T * ((HM_IN / HW_IT) * 2.0 * HM_HD + (HM_HD / HW_JT) * 4.0 * HM_IN) + 4.0 * shares * HM_HD * HM_IN, head_mlp_wgrad_kernel,
              dim3(HW_TILES * shares), dim3(256), st, wa);
  rc = check_launch("head_mlp_bwd (wgrad)");
  if (rc) return rc;
  const SlabSeg segs[4] = {{slabs, dw1, (long long)HM_HD * HM_IN, shares, HM_HD * HM_IN, 1, accumulate},
                           {part, db1, HM_PART, tiles, HM_HD, 1, accumulate},
                           {part + HM_HD, dw2, HM_PART, tiles, HM_HD, 1, accumulate},
                           {part + 2 * HM_HD, db2, HM_PART, tiles, 1, 1, accumulate}};
  return launch_slab_reduce_batch(segs, 4, st);
}

}  // extern "C"
