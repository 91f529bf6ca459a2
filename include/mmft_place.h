/* Path masks that follow a moving placement: the masked projection straight from (path nodes, pin coordinates).
 *
 * Like include/mmft_report.h this header holds what the reference's loops do not have, under the conventions of mmft.h
 * (extern "C", int results, raw device pointers, `int device, void* stream` last, the error codes and mmft_last_error of
 * mmft.h), compiled into the same library, bound by mmft.lib.place and pinned by a ledger of its own
 * (tests/test_place_cpu.py).
 *
 * THE MASK RULE (the rule of path_mask_kernel in csrc/prep.hip, reference src/verilog_parser_asap7.py:1302-1369; stated
 * here once, restated in numpy by mmft.placement.rasterize_host; its device code is csrc/mask_rule.h, which every kernel
 * that builds a mask or moves a pin of one calls: prep.hip, place.hip, crit.hip, pin_move.hip, trial.hip, search.hip):
 *
 *   The mask of path q over a map_x x map_y map is the union, over the consecutive node pairs (path[j], path[j + 1]) with
 *   j + 1 < min(path_lens[q], maxlen), of the boxes [min x, max x] x [min y, max y] of the two pins' map cells, where
 *     - the lower corner is clamped to 0 and the upper corner to map_x - 1 / map_y - 1,
 *     - a box that is empty after clamping (both pins outside the map on the same side) is skipped,
 *     - cell (x, y) is column x * map_y + y, a cell covered by several boxes counts once,
 *     - a path of fewer than two nodes has an empty mask; entries of a row at and beyond its length are never read.
 *
 * The RUNS of a mask are its maximal groups of consecutive columns that do not cross a multiple of S = 64 (the prefix block of
 * mmft_masked_fc_prefix), numbered in ascending column order: the groups of consecutive ones of the 64-bit words of the
 * mask's bitmap.
 */
#ifndef MMFT_PLACE_H
#define MMFT_PLACE_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[t][0 .. Dout) = bias + sum over the runs [s, e] of the mask of path paths[t] of GP[f_off[t] + e] - GP[f_off[t] + s - 1]
 * (GP[.. + e] alone where s is a multiple of S), for t in [0, T): what mmft_masked_fc_fwd_runs computes from a run table,
 * computed from the path's nodes and the pins' current coordinates instead.  No CSR, no run table, no host work: every
 * table has a static size, so a captured graph follows the pins.
 *
 *   path_nodes [num_paths][maxlen], path_lens [num_paths]   node ids index loc_x / loc_y; they are NOT checked on the device
 *                                      (mmft.placement validates them once).  loc_x / loc_y may hold any int: clamped.
 *   paths [T], f_off [T] or NULL (all 0)   batch rows: path id and the row's offset into GP (design index * P)
 *   GP                                 the block-prefix table of mmft_masked_fc_prefix with block size S
 *   bias [Dout] or NULL, out [T][ldo]  ldo >= Dout, a multiple of 4
 *   stats NULL or [T][2] int           cells and runs of each row's mask
 *
 * One workgroup of 256 threads per batch row: the mask as a bitmap in LDS, the runs numbered by a scan over the per-block
 * counts popc(v & ~(v << 1)), then accumulated exactly as masked_fc_fwd_runs_kernel does (run r on entry lane r % J,
 * J = 256 / (Dout / 4), ascending r per lane, lanes combined from the bias in the order 0 .. J - 1): `out` is BITWISE what
 * mmft_masked_fc_fwd_runs gives on the run table of the same masks.  Every element of out[0 .. T) (and of stats) is written
 * by every call; same inputs, same bits.
 *
 * S == 64; P = map_x * map_y a multiple of 64, <= 65536; Dout a multiple of 4 in [4, 1024]; maxlen >= 1; T >= 0; GP, out and
 * bias 16-byte aligned; no null pointer but f_off, bias, stats.  Anything else is MMFT_ERR_BAD_ARG and nothing is launched. */
int mmft_placed_fc_fwd(const int* path_nodes, const int* path_lens, int maxlen,
                       const int* loc_x, const int* loc_y, int map_x, int map_y,
                       const int* paths, const int* f_off, int T,
                       const float* GP, const float* bias, float* out, long long ldo, int Dout, int S,
                       int* stats,
                       int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
