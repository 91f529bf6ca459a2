// Masked projection straight from a placement (include/mmft_place.h): per batch row the path's mask is rasterised into an
// LDS bitmap from (path nodes, pin coordinates) and projected through the block-prefix table of fc_prefix_kernel, run by
// run, in the order and with the arithmetic of masked_fc_fwd_runs_kernel (fusion.hip) - no CSR and no run table in device memory.
#include "common.h"
#include "mask_rule.h"
#include "place_project.h"
#include "../../include/mmft_place.h"

namespace mmft {

__global__ void __launch_bounds__(256) placed_fc_fwd_kernel(const int* __restrict__ path_nodes, const int* __restrict__ path_lens,
                                                            int maxlen, const int* __restrict__ loc_x,
                                                            const int* __restrict__ loc_y, int map_x, int map_y,
                                                            const int* __restrict__ paths, const int* __restrict__ foff,
                                                            const float* __restrict__ GP, const float* __restrict__ bias,
                                                            float* __restrict__ out, long long ldo, int Dout,
                                                            int* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char place_smem[];
  const int P = map_x * map_y, words = P >> 5, nblk = P >> 6;
  const PlaceLds L = place_lds(place_smem, nblk);
  const int t = blockIdx.x, tid = threadIdx.x;
  for (int w = tid; w < words; w += 256) L.bits[w] = 0u;
  // ---- the union of boxes: THE MASK RULE, staged (mask_rule.h); node ids are not checked here (mmft_place.h)
  const int q = paths[t];
  const int* path = path_nodes + (long long)q * maxlen;
  const int len = path_lens[q] < maxlen ? path_lens[q] : maxlen;        // the same for every thread
  mask_raster_path<256, false>(L.bits, L.pin_x, L.pin_y, path, len, loc_x, loc_y, 0, map_x, map_y, tid);
  __syncthreads();
  // ---- the runs numbered and accumulated through the prefix table (place_project.h)
  place_project(L, nblk, GP + (long long)(foff ? foff[t] : 0) * Dout, bias, out + (long long)t * ldo, Dout,
                stats ? stats + 2 * (long long)t : nullptr, tid);
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
