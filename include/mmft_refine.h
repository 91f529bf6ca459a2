/* Patch the kept head rows after a commit, so that the next search needs no predict().
 *
 * mmft_commit_select (mmft_commit.h) leaves sel [G]; a group g is SELECTED here iff sel[g] != 0 and 0 <= best_w[g] < W.  A pin
 * feeds only the path masks, so the move of a selected group changes only the rows grow_row[e] of its entries, and on those
 * rows only the h_cnn columns of the head's input x and the prediction.  mmft_refine_rows recomputes exactly those rows from
 * the pins BEFORE they are moved - the code of mmft_search_rows at the one offset best_w[g] -, mmft_head_mlp_fwd (mmft_head.h,
 * hid == NULL, as it stands) turns them into predictions, and mmft_refine_patch writes both into the kept x and pred: what
 * the next predict() on the moved pins would write, bit for bit.
 *
 * THE ORDER of a patched commit, all on one stream: the launches of the search, mmft_commit_select, mmft_refine_rows, the
 * head over xt [R] into pred_t [R], mmft_refine_patch, and LAST mmft_commit_apply: the rows kernel reads the resident pins.
 *
 * Like include/mmft_commit.h this header holds entry points beyond mmft.h, under its conventions (extern "C", int results, raw
 * device pointers, `int device, void* stream` last, the error codes and mmft_last_error of mmft.h), compiled into the same
 * library.  It is bound by mmft.refine.abi - an accessor of its own, outside the table of mmft.lib - and pinned by a ledger of
 * its own (tests/test_refine_cpu.py).  Every entry point validates every argument on the host before the device is looked
 * at; anything outside its limits is MMFT_ERR_BAD_ARG and nothing is launched.  The window (radius, offset w -> (dx, dy), the
 * CENTRE, sat32), the groups and the entries are those of mmft_search.h.
 */
#ifndef MMFT_REFINE_H
#define MMFT_REFINE_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* xt[e][0 .. width) for every entry e in [0, R), slot e:
 *
 *   e SELECTED (its group g = grow_grp[e] is)   BITWISE the row mmft_search_rows writes for (e, w = best_w[g]): the group's
 *                                               overrides are formed from the resident pins and the offset, staged in LDS, and
 *                                               from there on the kernel runs the code of mmft_search_rows / mmft_trial_rows
 *   every other e                               a bitwise copy of x[grow_row[e]][0 .. width)
 *   grow_row[e] outside [0, T) or grow_grp[e] outside [0, G)   zeros: nothing outside the tables is read
 *
 * so every element of xt[0 .. R)[0 .. width) is written once per call; nothing beyond `width` in a row and no row beyond
 * R is.  sel, best_w and radius are read on the device: no host table depends on a selection.  loc_x / loc_y are read, never
 * written.  One workgroup of 256 threads per entry; no atomics in global memory, no workspace; same inputs, same bits.
 *
 *   path_nodes .. mv_node, G, GP .. S   as in mmft_search_rows, with its limits; and T <= 2^24
 *   sel [G], best_w [G]                 as mmft_commit_select and mmft_search_best wrote them
 *   xt [R][ldxt]
 *
 * R == 0 returns 0 once the sizes are in order and looks at no pointer. */
int mmft_refine_rows(const int* path_nodes, const int* path_lens, int maxlen,
                     const int* loc_x, const int* loc_y, int map_x, int map_y,
                     const int* paths, const int* f_off, int T,
                     const int* grow_row, const int* grow_grp, int R,
                     const int* mv_ptr, const int* mv_node, int G,
                     const int* sel, const int* best_w, int radius,
                     const float* GP, const float* bias,
                     const float* x, long long ldx, float* xt, long long ldxt,
                     int width, int cnn_col, int Dout, int S,
                     int device, void* stream);

/* For every SELECTED entry e whose row r = grow_row[e] lies in [0, T):
 *
 *   x[r][cnn_col .. cnn_col + Dout) = xt[e][cnn_col .. cnn_col + Dout)        pred[r] = pred_t[e]
 *
 * and stats [2] int64 = the entries patched, the selected entries skipped because their row lies outside [0, T).  Nothing
 * else is written: the columns of x outside h_cnn, the rows of unselected groups and every word past T keep their bits.
 *
 * The kernel RELIES on the selected groups sharing no row - mmft_commit_select guarantees it, and inside a group every row
 * occurs once -: no two entries write one row, so plain vector stores do, without atomics on x or pred; a sel of another
 * origin whose groups share a row would race on it.  One wave per entry; the two counts are integer sums (a memset and one
 * integer atomic per workgroup, whose result does not depend on the order): same inputs, same bits.  An entry whose group
 * lies outside [0, G) is not selected.
 *
 * 1 <= T <= 2^24, R >= 0, G >= 1, 1 <= radius <= 8, Dout a multiple of 4 in [4, 1024], cnn_col, ldx and ldxt multiples of 4,
 * 0 <= cnn_col, cnn_col + Dout <= ldx and ldxt; x and xt 16-byte aligned, stats 8-byte aligned; grow_row, grow_grp, xt and
 * pred_t may be NULL when R == 0 (stats is zeroed all the same); no other null pointer. */
int mmft_refine_patch(float* x, long long ldx, float* pred, int T,
                      const float* xt, long long ldxt, const float* pred_t,
                      const int* sel, const int* best_w, int radius,
                      const int* grow_row, const int* grow_grp, int R, int G,
                      int cnn_col, int Dout, long long* stats,
                      int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
