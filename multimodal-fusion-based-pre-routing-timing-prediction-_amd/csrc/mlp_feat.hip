// The feature MLPs of the sweep, fc_cell_self / fc_net_self (Linear(fin, 256) - ReLU - Linear(256, 128) over ALL cell /
// net nodes, src/model.py:48-51,66-67,148-153,186-189), bf16 math mode, WITHOUT storing the hidden activations.
//
// As two GEMMs per MLP the hidden tensor H (rows x 256 fp32 = 268 MB per MLP at config B) was written once and read three
// times per step (second forward GEMM, weight gradient of layer 2, fused first-layer gradients): 4 x 111 us forward,
// 2 x (120 + 103) us backward, all of it HBM time.  fin is 36 / 2: recomputing H costs 1-5 % of the MLP's flops, so
//   * forward  (mmft_mlp2_feat_fwd_bf16): one kernel per MLP reads X, keeps the 64 x 256 hidden tile in LDS as bf16 and
//     writes only the output rows; its MASKED instantiation (mmft_mlp2_feat_fwd_bf16_masked) does so for flagged rows only;
//   * backward (mmft_mlp2_feat_bwd_bf16): one kernel per MLP reads G (gradient of the output rows) and X, recomputes
//     H = relu(X W1^T + b1) with the forward's instruction sequence (bitwise the forward's H, so the ReLU mask agrees),
//     forms dH = (G W2) * (H > 0) in registers and accumulates all four gradients
//         dW2 += G^T H,  db2 += sum G,  dW1 += dH^T X,  db1 += sum dH
//     in MFMA accumulators across the 32-row tiles of a persistent workgroup (the contractions over rows take their
//     operands from transposed bf16 copies of the tile in LDS); one slab per workgroup, summed in a fixed order.
// Lane layouts are those of mlp_tile_bf16.h: A = weights / transposed tiles (lane = output feature, 8 consecutive k),
// B = row tiles (lane = row or feature, 8 consecutive k), D[m][n] at lane (n = lane & 15, q = lane >> 4) = rows 4q..4q+3.
#include <stdlib.h>
#include "mlp_tile_bf16.h"
#include "mlp_feat_frag.h"        // mf_bf16, mf_pack8, mf_w1_frag (shared with mlp_feat_dx.hip)
#include "tr_read.h"
#include "../../include/mmft_incr.h"

namespace mmft {

int launch_slab_reduce(const float* slabs, int splits, long long elems, float* out, int accumulate, hipStream_t st);

struct FeatFwdArgs {
  const float* x;
  long long ldx;
  int row0, n, fin;
  const float *w1, *b1, *w2, *b2;
  float* out;
  long long ldout;
  int relu_out;
  const unsigned char* active;   // MASKED only: one flag per node
};

// MASKED (mmft_mlp2_feat_fwd_bf16_masked, include/mmft_incr.h): only rows whose flag is set are stored.  Every wave reads the
// 64 flags of a tile itself and takes the ballot: the same 64 bits in all eight waves (nobody writes the flags while the kernel
// runs), so the choice of the tiles that run is uniform over the workgroup and every barrier below is reached by all of it.
// A tile without a flag costs that one load.  The tiles that run are computed exactly as by MASKED = false - rows are
// independent in both GEMMs - and only the store is predicated.
// The unmasked form asks for four waves per SIMD - two workgroups resident per CU, 128 registers: KS = 2 takes 140 when left
// alone (one workgroup per CU), KS = 1 fits anyway.  The masked form keeps the default bounds: held to 128 registers its
// KS = 2 instantiation would go through scratch.
template <int KS, bool MASKED>   // K steps of 32 for the first layer (fin <= 32 KS)
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(MASKED ? 2 : 4, MASKED ? 8 : 4)))
mlp2_feat_fwd_kernel(FeatFwdArgs a) {
  constexpr int BM = 64, RT = BM / 16, XS = KS * 32 + 8, HS = L2_HD + 8;
  __shared__ __attribute__((aligned(16))) unsigned short xs[BM * XS];
  __shared__ __attribute__((aligned(16))) unsigned short hs[BM * HS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int ntiles = (a.n + BM - 1) / BM;
  // the first tile at or after t (in this workgroup's stride) that runs, and its rows' flags
  auto next_tile = [&](int t, unsigned long long& flags) -> int {
    if constexpr (MASKED) {
      for (; t < ntiles; t += (int)gridDim.x) {
        const int m = t * BM + lane;
        flags = __ballot(m < a.n && a.active[a.row0 + m] != 0);
        if (flags) break;
      }
    }
    return t;
  };
  unsigned long long flags = ~0ull;
  int tile = next_tile(blockIdx.x, flags);
  if constexpr (MASKED) {
    if (tile >= ntiles) return;      // nothing to do here: not worth the weights
  }
  bf16x8 w1f[2][KS], w2f[8];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) w1f[j][ks] = mf_w1_frag(a.w1, a.fin, wave * 32 + j * 16 + r16, ks * 32 + q * 8);
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) w2f[ks] = mf_pack8(a.w2 + (long long)(wave * 16 + r16) * L2_HD + ks * 32 + q * 8);
  const int nn2 = wave * 16 + q * 4;
  const f32x4 b2v = *reinterpret_cast<const f32x4*>(a.b2 + nn2);
  f32x4 b1v[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) b1v[j] = *reinterpret_cast<const f32x4*>(a.b1 + wave * 32 + j * 16 + q * 4);
  // The weights (164 KB of fp32) are fetched ONCE per workgroup: the grid is a few workgroups per CU and each walks
  // tiles of 64 rows; the X elements of the next tile that runs are requested before this one is multiplied.
  constexpr int NXE = BM * KS * 32 / 512;
  float xr[NXE];
  auto request = [&](int tile) {
#pragma unroll
    for (int k = 0; k < NXE; ++k) {
      const int e = tid + k * 512, r = e / (KS * 32), kk = e % (KS * 32);
      const int m = tile * BM + r;
      xr[k] = (m < a.n && kk < a.fin) ? a.x[(long long)(a.row0 + m) * a.ldx + kk] : 0.f;
    }
  };
  if (tile < ntiles) request(tile);
  while (tile < ntiles) {
    const int m0 = tile * BM;
#pragma unroll
    for (int k = 0; k < NXE; ++k) {
      const int e = tid + k * 512;
      xs[(e / (KS * 32)) * XS + e % (KS * 32)] = mf_bf16(xr[k]);
    }
    __syncthreads();
    unsigned long long nflags = ~0ull;
    const int nxt = next_tile(tile + (int)gridDim.x, nflags);
    if (nxt < ntiles) request(nxt);
    f32x4 acc1[RT][2];
    tile_layer1<KS, RT>(acc1, w1f, xs, XS, r16, q);
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) st_bf16x4(hs + (i * 16 + r16) * HS + wave * 32 + j * 16 + q * 4, relu4(acc1[i][j] + b1v[j]));
    __syncthreads();
    f32x4 acc2[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) acc2[i] = tile_layer2(w2f, hs, HS, r16, q, i);
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const int m = m0 + i * 16 + r16;
      if (m >= a.n) continue;
      if constexpr (MASKED) {
        if (!((flags >> (i * 16 + r16)) & 1)) continue;
      }
      f32x4 v = acc2[i] + b2v;
      if (a.relu_out) v = relu4(v);
      *reinterpret_cast<f32x4*>(a.out + (long long)(a.row0 + m) * a.ldout + nn2) = v;
    }
    // the next deposit overwrites xs (last read before the barrier above) and the next epilogue hs (last read here)
    __syncthreads();
    tile = nxt;
    flags = nflags;
  }
}

struct FeatBwdArgs {
  const float* g;
  long long ldg;
  const float* x;
  long long ldx;
  int row0, n, fin;
  const float *w1, *b1, *w2;
  float* slabs;        // [gridDim.x][slab]: dw1 [HD][fin] | db1 [HD] | dw2 [D2][HD] | db2 [D2]
  long long slab;
};

constexpr int FEAT_BWD_WS = L2_D2 + 8;      // pitch of the W2^T image in LDS (bf16 elements; 17 x 16 bytes)
// whether mlp2_feat_bwd_kernel<KS, .> keeps W2^T in LDS (68 KB) instead of 32 registers per lane
template <int KS>
constexpr bool feat_bwd_w2_lds() { return KS == 2; }

// KB: the 16-column blocks of dW1 that hold a column below fin, ceil(fin / 16) - the launcher's choice, KS = ceil(KB / 2).
// A block entirely at or beyond fin would accumulate zeros that are never stored.
template <int KS, int KB>
__global__ void __launch_bounds__(512) mlp2_feat_bwd_kernel(FeatBwdArgs a) {
  // every tile lives in LDS in its natural [row][column] layout; the contractions over the tile's rows read their operands
  // with the hardware-transposed read (tr_read.h) - pitches of 16 x odd elements
  constexpr int BM = 32, KP = KS * 32, XS = KP + 16, GS = L2_D2 + 16, HS = L2_HD + 16, WS = FEAT_BWD_WS;
  static_assert(KB >= 2 * KS - 1 && KB <= 2 * KS, "KB = ceil(fin / 16) with 32 (KS - 1) < fin <= 32 KS");
  extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
  unsigned short* xs = lds;                       // X tile  [row][k]
  unsigned short* gs = xs + BM * XS;              // G tile  [row][d2]
  unsigned short* hs = gs + BM * GS;              // H tile  [row][col]
  unsigned short* ds = hs + BM * HS;              // dH tile [row][col]
  unsigned short* w2s = ds + BM * HS;             // W2^T    [col][d2], written once
  f32x4(*gred)[32] = reinterpret_cast<f32x4(*)[32]>(hs);      // end of the kernel only (16 x 32 x 16 B <= hs)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, q = lane >> 4;
  const int trr = tr_lane_row(lane), trc = tr_lane_col(lane);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // W1 in registers for the life of the workgroup, and for KS = 1 the A fragments of W2^T (W2T[col][d2] = w2[d2][col],
  // d2 = 32 ks + 8 q ..) too.  With KS = 2 those 32 registers left the tile loop none for the next tile's loads, which then
  // went through scratch one at a time: there W2^T stays in LDS as bf16 and a fragment is one 16-byte read in the dH phase.
  // (KS = 1 has the room, and reading its fragments from LDS cost it 11 us per launch: feat_bwd_w2_lds.)
  constexpr bool W2LDS = feat_bwd_w2_lds<KS>();
  bf16x8 w1f[2][KS], w2tf[W2LDS ? 1 : 2][W2LDS ? 1 : 4];
  f32x4 b1v[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = wave * 32 + j * 16 + r16;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) w1f[j][ks] = mf_w1_frag(a.w1, a.fin, col, ks * 32 + q * 8);
    if constexpr (!W2LDS) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        float v[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) v[t] = a.w2[(long long)(ks * 32 + q * 8 + t) * L2_HD + col];
        w2tf[j][ks] = mf_pack8(v);
      }
    }
    b1v[j] = *reinterpret_cast<const f32x4*>(a.b1 + wave * 32 + j * 16 + q * 4);
  }
  if constexpr (W2LDS) {
    // w2s[col * WS + d2] = bf16(w2[d2][col]): a thread packs 8 consecutive d2 of one column (loads coalesced over the columns)
#pragma unroll
    for (int k = 0; k < L2_D2 / 16; ++k) {
      const int col = tid & (L2_HD - 1), d0 = ((tid >> 8) + 2 * k) * 8;
      float v[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) v[t] = a.w2[(d0 + t) * L2_HD + col];
      *reinterpret_cast<bf16x8*>(w2s + col * WS + d0) = mf_pack8(v);
    }
  }
  f32x4 dw2[2][8], dw1[2][KB], dsum[2], gsum = zero;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    dsum[j] = zero;
#pragma unroll
    for (int d = 0; d < 8; ++d) dw2[j][d] = zero;
#pragma unroll
    for (int k = 0; k < KB; ++k) dw1[j][k] = zero;
  }

  const int ntiles = (a.n + BM - 1) / BM;
  // G (two 16-byte groups per thread) and X (BM * KP / 512 scalars) of tile t + 1 are requested before tile t is multiplied.
  // request() only loads: every lane reads an element of the tile (row clamped to the last row of the range, column to
  // fin - 1) and keeps the raw value; what lies past the end becomes zero where the registers are deposited, an iteration
  // later.  A select at the load makes the compiler branch around each load and wait for it on the spot.  The tile's bases
  // are uniform (64-bit, scalar registers); a lane adds a 32-bit element offset of at most 32 rows (the launcher checks).
  constexpr int NXE = BM * KP / 512;
  f32x4 gr[2];
  float xr[NXE];
  auto request = [&](int tile) {
    const int m0 = tile * BM, rlast = a.n - 1 - m0, klast = a.fin - 1;
    const float* gt = a.g + (long long)(a.row0 + m0) * a.ldg;
    const float* xt = a.x + (long long)(a.row0 + m0) * a.ldx;
    const unsigned ldg = (unsigned)a.ldg, ldx = (unsigned)a.ldx;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int e = tid + it * 512, r = e >> 5, c = (e & 31) * 4;
      gr[it] = *reinterpret_cast<const f32x4*>(gt + ((unsigned)min(r, rlast) * ldg + (unsigned)c));
    }
#pragma unroll
    for (int k = 0; k < NXE; ++k) {
      const int e = tid + k * 512, r = e / KP, kk = e % KP;
      xr[k] = xt[(unsigned)min(r, rlast) * ldx + (unsigned)min(kk, klast)];
    }
  };
  if ((int)blockIdx.x < ntiles) request(blockIdx.x);
  if constexpr (W2LDS) __syncthreads();       // W2^T is in LDS
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // ---- deposit G and X; rows past the end and columns past fin are zero
    const int nrow = a.n - tile * BM;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int e = tid + it * 512, r = e >> 5, c = (e & 31) * 4;          // (row, 4 consecutive d2): c is the same for both
      const f32x4 v = r < nrow ? gr[it] : zero;
      gsum += v;
      const unsigned lo = pack_bf16(v.x, v.y), hi = pack_bf16(v.z, v.w);
      *reinterpret_cast<unsigned long long*>(gs + r * GS + c) = ((unsigned long long)hi << 32) | lo;
    }
#pragma unroll
    for (int k = 0; k < NXE; ++k) {
      const int e = tid + k * 512, r = e / KP, kk = e % KP;
      xs[r * XS + kk] = mf_bf16((r < nrow && kk < a.fin) ? xr[k] : 0.f);
    }
    __syncthreads();
    if (tile + (int)gridDim.x < ntiles) request(tile + gridDim.x);
    __syncthreads();
    // ---- H = relu(X W1^T + b1), dH = (G W2) * (H > 0): hidden columns [32 wave, 32 wave + 32) of the 32 rows
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      f32x4 acc1[2] = {zero, zero}, acc3[2] = {zero, zero};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 xf = *reinterpret_cast<const bf16x8*>(xs + (i * 16 + r16) * XS + ks * 32 + q * 8);
#pragma unroll
        for (int j = 0; j < 2; ++j) acc1[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1f[j][ks], xf, acc1[j], 0, 0, 0);
      }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 gf = *reinterpret_cast<const bf16x8*>(gs + (i * 16 + r16) * GS + ks * 32 + q * 8);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          bf16x8 wf;
          if constexpr (W2LDS) wf = *reinterpret_cast<const bf16x8*>(w2s + (wave * 32 + j * 16 + r16) * WS + ks * 32 + q * 8);
          else wf = w2tf[j][ks];
          acc3[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, gf, acc3[j], 0, 0, 0);
        }
      }
      const int m = i * 16 + r16;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int nn = wave * 32 + j * 16 + q * 4;
        f32x4 hv = acc1[j] + b1v[j], dh = acc3[j];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          hv[t] = hv[t] > 0.f ? hv[t] : 0.f;
          dh[t] = hv[t] > 0.f ? dh[t] : 0.f;
        }
        dsum[j] += dh;
        const unsigned hl = pack_bf16(hv.x, hv.y), hh = pack_bf16(hv.z, hv.w);
        const unsigned dl = pack_bf16(dh.x, dh.y), dhh = pack_bf16(dh.z, dh.w);
        *reinterpret_cast<unsigned long long*>(hs + m * HS + nn) = ((unsigned long long)hh << 32) | hl;
        *reinterpret_cast<unsigned long long*>(ds + m * HS + nn) = ((unsigned long long)dhh << 32) | dl;
      }
    }
    __syncthreads();
    // ---- contractions over the tile's 32 rows (one K step): dW2^T[col][d2] += H^T G, dW1^T[col][k] += dH^T X
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col0 = wave * 32 + j * 16;
      const bf16x8 hf = __builtin_bit_cast(bf16x8, tr_read_pair(hs + trr * HS + col0 + trc, 16 * HS));
      const bf16x8 df = __builtin_bit_cast(bf16x8, tr_read_pair(ds + trr * HS + col0 + trc, 16 * HS));
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const bf16x8 gf = __builtin_bit_cast(bf16x8, tr_read_pair(gs + trr * GS + d * 16 + trc, 16 * GS));
        dw2[j][d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hf, gf, dw2[j][d], 0, 0, 0);
      }
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        const bf16x8 xf = __builtin_bit_cast(bf16x8, tr_read_pair(xs + trr * XS + k * 16 + trc, 16 * XS));
        dw1[j][k] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df, xf, dw1[j][k], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // ---- the workgroup's slab
  float* sl = a.slabs + (long long)blockIdx.x * a.slab;
  float* s_dw1 = sl;
  float* s_db1 = s_dw1 + (long long)L2_HD * a.fin;
  float* s_dw2 = s_db1 + L2_HD;
  float* s_db2 = s_dw2 + (long long)L2_D2 * L2_HD;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int colq = wave * 32 + j * 16 + q * 4;           // D[m = col][n]: lane (n = r16, q) holds cols colq .. colq + 3
#pragma unroll
    for (int d = 0; d < 8; ++d) *reinterpret_cast<f32x4*>(s_dw2 + (long long)(d * 16 + r16) * L2_HD + colq) = dw2[j][d];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const int kk = k * 16 + r16;
      if (kk < a.fin) {
#pragma unroll
        for (int t = 0; t < 4; ++t) s_dw1[(long long)(colq + t) * a.fin + kk] = dw1[j][k][t];
      }
    }
    // db1: sum over the 16 row lanes (rows live on r16), fixed butterfly order
    f32x4 v = dsum[j];
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] += __shfl_xor(v[t], o, 64);
    }
    if (r16 == 0) *reinterpret_cast<f32x4*>(s_db1 + colq) = v;
  }
  // db2: thread t summed d2 group (t & 31) over its rows; 16 threads share a group
  __syncthreads();
  gred[tid >> 5][tid & 31] = gsum;
  __syncthreads();
  if (tid < 32) {
    f32x4 v = gred[0][tid];
    for (int p = 1; p < 16; ++p) v += gred[p][tid];
    *reinterpret_cast<f32x4*>(s_db2 + tid * 4) = v;
  }
}

template <int KS>
constexpr int feat_bwd_lds() {
  constexpr int BM = 32, KP = KS * 32, XS = KP + 16, GS = L2_D2 + 16, HS = L2_HD + 16;
  return (BM * XS + BM * GS + 2 * BM * HS + (feat_bwd_w2_lds<KS>() ? L2_HD * FEAT_BWD_WS : 0)) * 2;      // 46 / 116 KB
}

static inline long long feat_slab(int fin) { return (long long)L2_HD * fin + L2_HD + (long long)L2_D2 * L2_HD + L2_D2; }
// One workgroup per CU (230 - 248 VGPRs; KS = 2: 116 KB of LDS) - on 192 of the 256 CUs: the two launches close the reverse
// sweep on its side stream while the U-Net's backward, the stream that finishes last, still runs on the main one; a grid that
// takes every CU stalls it.  Measured on the replayed config-B step (ms) when the launches took 2 x 118 us: 256 -> 3.37,
// 224 -> 3.28, 192 -> 3.23, 160 -> 3.26, 128 -> 3.29; again at 112 + 84 us, each value alternated with 192 (three pairs):
// 160 -> 2.905 2.905 2.891 (192: 2.886 2.889 2.895), 224 -> 2.943 2.938 2.929 (2.920 2.936 2.906), 256 -> 3.007 2.999 3.064
// (2.928 2.999 2.906).  MMFT_FEAT_BWD_GRID overrides (read once).
static inline int feat_bwd_grid(int n) {
  int tiles = cdiv(n, 32);
  static int cap = getenv("MMFT_FEAT_BWD_GRID") ? atoi(getenv("MMFT_FEAT_BWD_GRID")) : 192;
  if (cap < 1) cap = 1;
  return tiles < cap ? (tiles < 1 ? 1 : tiles) : cap;
}

}  // namespace mmft

using namespace mmft;

static int feat_fwd_launch(const char* what, const float* x, long long ldx, int row0, int n, int fin, const float* w1,
                           const float* b1, const float* w2, const float* b2, float* out, long long ldout, int relu_out,
                           const unsigned char* active, int device, void* stream) {
  MMFT_REQUIRE(x && w1 && b1 && w2 && b2 && out, "%s: null pointer", what);
  MMFT_REQUIRE(n >= 0 && row0 >= 0 && fin >= 1 && fin <= 64 && ldx >= fin, "%s: bad sizes (fin <= 64)", what);
  MMFT_REQUIRE(ldout % 4 == 0 && aligned16(out) && aligned16(w2) && aligned16(b1) && aligned16(b2),
               "%s: out / w2 / biases must be 16-byte aligned", what);
  if (n == 0) return MMFT_OK;
  DeviceGuard dg(device);
  FeatFwdArgs a{x, ldx, row0, n, fin, w1, b1, w2, b2, out, ldout, relu_out, active};
  const double fl = 2.0 * n * ((double)fin * L2_HD + (double)L2_HD * L2_D2), by = 4.0 * n * ((double)fin + L2_D2);
  int grid = cdiv(n, 64);
  // Two workgroups are resident per CU (8 waves of <= 128 registers each, 38 / 42 KB of LDS; the masked KS = 2 form: one), so
  // 512 fill the chip at once.  The grid was 768 when the unmasked KS = 2 form held one workgroup per CU (140 registers);
  // per launch at config B (us): cells 72.7 -> 56.6 (66.7 with the grid alone, 66.1 with the registers alone), nets
  // 58.1 -> 48.4.  The masked form keeps its 768 (not measured).  MMFT_FEAT_FWD_GRID overrides both (read once).
  static int env_cap = getenv("MMFT_FEAT_FWD_GRID") ? atoi(getenv("MMFT_FEAT_FWD_GRID")) : 0;
  const int cap = env_cap >= 1 ? env_cap : active ? 768 : 512;
  if (grid > cap) grid = cap;
  // (flops / bytes of the masked form: the upper bound, every flag set - the flags live on the device)
  if (active) {
    if (fin <= 32)
      MMFT_LAUNCH("mlp2_feat_fwd_masked_kernel", fl, by, (mlp2_feat_fwd_kernel<1, true>), dim3(grid), dim3(512), (hipStream_t)stream, a);
    else
      MMFT_LAUNCH("mlp2_feat_fwd_masked_kernel", fl, by, (mlp2_feat_fwd_kernel<2, true>), dim3(grid), dim3(512), (hipStream_t)stream, a);
  } else if (fin <= 32)
    MMFT_LAUNCH("mlp2_feat_fwd_kernel", fl, by, (mlp2_feat_fwd_kernel<1, false>), dim3(grid), dim3(512), (hipStream_t)stream, a);
  else
    MMFT_LAUNCH("mlp2_feat_fwd_kernel", fl, by, (mlp2_feat_fwd_kernel<2, false>), dim3(grid), dim3(512), (hipStream_t)stream, a);
  return check_launch(what);
}

extern "C" int mmft_mlp2_feat_fwd_bf16(const float* x, long long ldx, int row0, int n, int fin, const float* w1, const float* b1,
                                       const float* w2, const float* b2, float* out, long long ldout, int relu_out, int device,
                                       void* stream) {
  return feat_fwd_launch("mlp2_feat_fwd_bf16", x, ldx, row0, n, fin, w1, b1, w2, b2, out, ldout, relu_out, nullptr, device, stream);
}

extern "C" int mmft_mlp2_feat_fwd_bf16_masked(const float* x, long long ldx, int row0, int n, int fin, const float* w1,
                                              const float* b1, const float* w2, const float* b2, float* out, long long ldout,
                                              int relu_out, const unsigned char* active, int device, void* stream) {
  MMFT_REQUIRE(active, "mlp2_feat_fwd_bf16_masked: null pointer (active)");
  return feat_fwd_launch("mlp2_feat_fwd_bf16_masked", x, ldx, row0, n, fin, w1, b1, w2, b2, out, ldout, relu_out, active, device,
                         stream);
}

template <int KS, int KB>
static int feat_bwd_launch(const FeatBwdArgs& a, int grid, double fl, double by, hipStream_t st) {
  static DynLdsOnce once;
  int rc = ensure_dyn_lds(once, reinterpret_cast<const void*>(&mlp2_feat_bwd_kernel<KS, KB>), feat_bwd_lds<KS>(), "mlp2_feat_bwd_bf16");
  if (rc) return rc;
  MMFT_LAUNCH_LDS("mlp2_feat_bwd_kernel", fl, by, (mlp2_feat_bwd_kernel<KS, KB>), dim3(grid), dim3(512), feat_bwd_lds<KS>(), st, a);
  return check_launch("mlp2_feat_bwd_bf16");
}

extern "C" long long mmft_mlp2_feat_bwd_workspace_bytes(int n, int fin) {
  if (n <= 0 || fin < 1 || fin > 64) return 0;
  return (long long)feat_bwd_grid(n) * feat_slab(fin) * 4;
}

extern "C" int mmft_mlp2_feat_bwd_bf16(const float* g, long long ldg, const float* x, long long ldx, int row0, int n, int fin,
                                       const float* w1, const float* b1, const float* w2, float* dw1, float* db1, float* dw2,
                                       float* db2, int accumulate, float* workspace, long long workspace_bytes, int device,
                                       void* stream) {
  MMFT_REQUIRE(g && x && w1 && b1 && w2 && dw1 && db1 && dw2 && db2, "mlp2_feat_bwd_bf16: null pointer");
  MMFT_REQUIRE(n > 0 && row0 >= 0 && fin >= 1 && fin <= 64 && ldx >= fin && ldg >= L2_D2, "mlp2_feat_bwd_bf16: bad sizes (fin <= 64)");
  MMFT_REQUIRE(ldg % 4 == 0 && aligned16(g) && aligned16(b1), "mlp2_feat_bwd_bf16: g / b1 must be 16-byte aligned");
  // a lane addresses its element of a 32-row tile with a 32-bit offset from the tile's base
  MMFT_REQUIRE(ldx < (1ll << 31) / 32 && ldg < (1ll << 31) / 32, "mlp2_feat_bwd_bf16: 32 rows of x / g must fit 31 bits");
  MMFT_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= mmft_mlp2_feat_bwd_workspace_bytes(n, fin),
               "mlp2_feat_bwd_bf16: workspace too small");
  DeviceGuard dg(device);
  hipStream_t st = (hipStream_t)stream;
  const int grid = feat_bwd_grid(n);
  const long long slab = feat_slab(fin);
  FeatBwdArgs a{g, ldg, x, ldx, row0, n, fin, w1, b1, w2, workspace, slab};
  const double fl = 2.0 * n * (2.0 * fin * L2_HD + 2.0 * L2_HD * L2_D2), by = 4.0 * n * ((double)fin + L2_D2);
  int rc = fin <= 16   ? feat_bwd_launch<1, 1>(a, grid, fl, by, st)
           : fin <= 32 ? feat_bwd_launch<1, 2>(a, grid, fl, by, st)
           : fin <= 48 ? feat_bwd_launch<2, 3>(a, grid, fl, by, st)
                       : feat_bwd_launch<2, 4>(a, grid, fl, by, st);
  if (rc) return rc;
  // The four gradients are the four segments of a slab.  In FlatAdam's gradient buffer they are neighbours in exactly that
  // order (weight, bias, weight, bias of one MLP), so ONE parallel slab reduction finishes all of them.
  if (db1 == dw1 + (long long)L2_HD * fin && dw2 == db1 + L2_HD && db2 == dw2 + (long long)L2_D2 * L2_HD && aligned16(dw1))
    return launch_slab_reduce(workspace, grid, slab, dw1, accumulate, st);
  // scattered outputs: the same four reductions as one batched launch - per element the summation order of the joined form,
  // so the gradients do not depend on where the caller's (or the allocator's) tensors happen to lie
  const long long o1 = (long long)L2_HD * fin, o2 = o1 + L2_HD, o3 = o2 + (long long)L2_D2 * L2_HD;
  const SlabSeg segs[4] = {{workspace, dw1, slab, grid, (int)o1, 1, accumulate ? 1 : 0},
                           {workspace + o1, db1, slab, grid, L2_HD, 1, accumulate ? 1 : 0},
                           {workspace + o2, dw2, slab, grid, L2_D2 * L2_HD, 1, accumulate ? 1 : 0},
                           {workspace + o3, db2, slab, grid, L2_D2, 1, accumulate ? 1 : 0}};
  return launch_slab_reduce_batch(segs, 4, st);
}
