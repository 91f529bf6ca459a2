/* Sensitivity: the change of the weighted predictions when ONE pin moves by ONE map cell - the third thing a physical-design
 * loop can change, next to the features (include/mmft_sens.h) and the layout image (include/mmft_sens_image.h).  A pin is not
 * differentiable through box masks (it moves a path's mask by whole cells), so this is a DISCRETE sensitivity.
 *
 * Like the other extension headers it holds entry points beyond the generic layer ABI of mmft.h, under its conventions
 * (extern "C", int result, raw device pointers, `int device, void* stream` last, the error codes and mmft_last_error of mmft.h),
 * compiled into the same library, bound by mmft.lib.pmove and pinned by a ledger of its own (tests/test_pin_move_cpu.py).
 *
 * THE QUANTITY.  For a batch row t let q = paths[t] be its path, b its design (f_off[t] = b * P), g[t][0 .. Dout) the gradient
 * of J = sum_r w_r pred_r at the masked projection h_cnn[t], W = fcn.weight [Dout][P] (wT [P][Dout] its transpose).  The score
 * of map cell c for row t is
 *
 *     s_t(c) = feat[f_off[t] + c] * sum_k g[t][k] * W[k][c]                    (the bias of fcn cancels)
 *
 * M_t is the mask of path q under the current pins, by THE MASK RULE of include/mmft_place.h.  M_t^{n,d} is the mask by the
 * same rule after pin n ALONE is displaced by d - 0: x + 1, 1: x - 1, 2: y + 1, 3: y - 1 -, at ALL of its occurrences in the
 * row, BEFORE the rule clamps.  Coordinates may be any int32; the +-1 never overflows (a pin that far outside the map changes
 * nothing).  With M = M_t, M' = M_t^{n,d}, n = the pin at position j of the row:
 *
 *     row_move[t][j][d] = sum over c in M' \ M of s_t(c)  -  sum over c in M \ M' of s_t(c)
 *                            for the live positions j < min(path_lens[q], maxlen) that are the FIRST occurrence of their pin in
 *                            the row; exactly 0.0f at every other position (later occurrences, padding), for every d
 *     pin_move[n][d]    = sum of row_move[t][j][d] over the (t, j) first-occurrence pairs that hold pin n, in ascending (t, j);
 *                            0 for a pin on no row
 *
 * pin_move[n][d] is the first-order change of J when pin n moves one map cell in direction d: EXACT IN THE MASK (the set
 * differences under the rule - clamping, boxes that vanish or appear at the map's edge, cells kept alive by another box of the
 * path) and LINEAR IN THE HEAD (the change of h_cnn is contracted with g).  It is not a prediction of the moved design.
 */
#ifndef MMFT_SENS_PINS_H
#define MMFT_SENS_PINS_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* row_move [T][maxlen][4] as defined above.
 *
 *   path_nodes [num_paths][maxlen], path_lens [num_paths], loc_x / loc_y   the tables of mmft_placed_fc_fwd (mmft_place.h);
 *                                      node ids are NOT checked on the device
 *   paths [T], f_off [T] or NULL (all 0)   batch rows: path id and the row's offset into feat
 *   feat [B * P], wT [P][Dout]         the feature map and the transposed fcn weight
 *   g [T][ldg]                         ldg >= Dout: g may be a column slice of a wider gradient
 *
 * One workgroup of 256 threads per batch row; the row's nodes, coordinates and g[t] are staged in LDS.  A (first-occurrence
 * position, direction) pair is one wave's work item.  No bitmap: the boxes adjacent to an occurrence of the pin each propose at
 * most two added and two removed line segments; a proposed cell is tested against the row's boxes from the staged coordinates
 * and counted once, at the first box that proposes it.  s_t(c) is one Dout-long dot product with row c of wT.  Every sum runs
 * in a fixed order: no atomics, no workspace; every element of row_move[0 .. T) is written exactly once by every call; same
 * inputs, same bits.
 *
 * P = map_x * map_y a multiple of 64, <= 65536; Dout a multiple of 4 in [4, 1024]; 1 <= maxlen <= 1024 (the LDS staging);
 * T >= 0 (T == 0 returns 0 and looks at no pointer); ldg >= Dout, a multiple of 4; g, wT, feat 16-byte aligned; no null pointer
 * but f_off.  Anything else is MMFT_ERR_BAD_ARG, judged on the host before the device is looked at, and nothing is launched. */
int mmft_pin_move_rows(const int* path_nodes, const int* path_lens, int maxlen,
                       const int* loc_x, const int* loc_y, int map_x, int map_y,
                       const int* paths, const int* f_off, int T,
                       const float* feat, const float* wT, int Dout, const float* g, long long ldg,
                       float* row_move,
                       int device, void* stream);

/* pin_move [N][4] as defined above, from row_move [slots][4], slots = T * maxlen, and the static incidence CSR of the
 * selection: inc_slot[inc_ptr[n] .. inc_ptr[n + 1]) are the slots t * maxlen + j at which pin n occurs first in a row,
 * ascending (mmft.placement.pin_incidence builds it once per selection).  One thread per (pin, direction) sums in CSR order: no
 * float atomics; every element of pin_move is written by every call.  The tables are not trusted with addresses: an entry
 * index outside [0, nnz) (nnz = the length of inc_slot) and a slot outside [0, slots) are skipped, never read.
 * N >= 0 (N == 0 returns 0 and looks at no pointer), 0 <= slots < 2^29, 0 <= nnz < 2^31, N < 2^29; no null pointer (inc_slot
 * and row_move may be null when nnz == 0); row_move and pin_move 16-byte aligned.  Anything else is MMFT_ERR_BAD_ARG, judged
 * on the host before the device is looked at, and nothing is launched. */
int mmft_pin_move_sum(const float* row_move, long long slots, const int* inc_ptr, const int* inc_slot, long long nnz, int N,
                      float* pin_move,
                      int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
