/* Exact window search of pin-group moves on the device.
 *
 * A GROUP g is a set of at most 64 distinct pins that move rigidly together - mv_node[mv_ptr[g] .. mv_ptr[g + 1]), node ids
 * in the tables' numbering.  With a RADIUS r in [1, 8] the WINDOW holds W = (2 r + 1)^2 OFFSETS; offset w stands for
 * (dx, dy) = (w / (2 r + 1) - r, w % (2 r + 1) - r), x the first map axis (cell (x, y) = bit x * map_y + y), so the CENTRE
 * w = 2 r (r + 1) is the zero move.  Under CANDIDATE (g, w) pin n of group g sits at (sat32(loc_x[n] + dx), sat32(loc_y[n] +
 * dy)): the sum formed in 64 bits and saturated to int32 (THE MASK RULE of mmft_place.h clamps it anyway); every other pin
 * where loc_x / loc_y have it.  loc_x / loc_y are read, never written.
 *
 * The rows of `pred` a group can change are those whose path holds one of its pins: ENTRIES e in [grow_ptr[g],
 * grow_ptr[g + 1]), rows grow_row[e] ascending and each once inside a group, grow_grp[e] == g; R entries in all.  The window
 * is enumerated on the device; a call covers the offsets [w0, w1), and the head input row and the prediction of entry e
 * under offset w live at SLOT (w - w0) * R + e.
 *
 * Like include/mmft_trial.h this header holds entry points beyond mmft.h, under its conventions (extern "C", int results, raw
 * device pointers, `int device, void* stream` last, the error codes and mmft_last_error of mmft.h), compiled into the same
 * library.  It is bound by mmft.search.abi - an accessor of its own, outside the table of mmft.lib - and pinned by a ledger of
 * its own (tests/test_search_cpu.py).  Every entry point validates every argument on the host before the device is looked
 * at; anything outside its limits is MMFT_ERR_BAD_ARG and nothing is launched.
 *
 * The head forward over the slots' rows, between mmft_search_rows and mmft_search_score, is mmft_head_mlp_fwd (mmft_head.h)
 * with hid == NULL, as it stands.
 */
#ifndef MMFT_SEARCH_H
#define MMFT_SEARCH_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* xt[slot][0 .. width) for every entry e in [0, R) and offset w in [w0, w1): the head's input row of row grow_row[e] under
 * candidate (grow_grp[e], w).
 *
 * CONTRACT: the row is BITWISE the row mmft_trial_rows writes for the pair (grow_row[e], an explicit candidate that holds the
 * group's pins at the candidate's coordinates).  The overrides are formed on the device, staged in LDS where
 * trial_rows_kernel stages a candidate's, and the two kernels then run the same code (the copy of the columns around h_cnn,
 * mask_raster_path_moved, place_project).
 *
 *   path_nodes .. f_off, GP, bias, x, ldx, xt, ldxt, width, cnn_col, Dout, S   as in mmft_trial_rows, with its limits
 *   grow_row, grow_grp [R]             rows in [0, T), groups in [0, G): NOT checked on the device (mmft.search builds them)
 *   mv_ptr [G + 1], mv_node [mv_ptr[G]]   the groups' pins, CSR; at most 64 per group (the kernel reads no more than 64)
 *   xt [(w1 - w0) * R][ldxt]
 *
 * One workgroup of 256 threads per slot, one offset per workgroup: a workgroup that served several offsets of an entry
 * could reuse the staged path ids, the resident coordinates and the copied columns, but the raster and the projection -
 * most of its time - are per offset anyway; not built, not measured.  Every element of xt[0 .. (w1 - w0) * R)[0 .. width) is
 * written once per call; nothing beyond `width` in a row and no row beyond the last slot is written; no atomics in global
 * memory, no workspace; same inputs, same bits.
 *
 * The limits of mmft_trial_rows (K >= 1 reads G >= 1, n_pairs >= 0 reads R >= 0), and: 1 <= radius <= 8, 0 <= w0 <= w1 <= W,
 * (long long)R * (w1 - w0) < 2^31.  R == 0 or w0 == w1 returns 0 once the sizes are in order and looks at no pointer. */
int mmft_search_rows(const int* path_nodes, const int* path_lens, int maxlen,
                     const int* loc_x, const int* loc_y, int map_x, int map_y,
                     const int* paths, const int* f_off, int T,
                     const int* grow_row, const int* grow_grp, int R,
                     const int* mv_ptr, const int* mv_node, int G,
                     int radius, int w0, int w1,
                     const float* GP, const float* bias,
                     const float* x, long long ldx, float* xt, long long ldxt,
                     int width, int cnn_col, int Dout, int S,
                     int device, void* stream);

/* The slices [g][w0 .. w1) of six tables [G][W], from the slots' predictions pred_trial [(w1 - w0) * R]:
 *
 *   slack                  the rule of mmft_report.h: required[r] - pred in one fp32 subtraction, -0.0 canonicalised to +0.0;
 *                          s_base from pred_base[r], s_trial from the slot's pred_trial, r = grow_row[e]
 *   q(s)                   THE QUANTUM of mmft_crit_sums.h at scale_log2: 0 for a slack that does not violate (s < 0 is
 *                          false), a NaN slack included; the cap 2^32 from -s >= 2^(32 - scale_log2) on
 *   dq[g][w]        int64  the sum over the group's entries of q(s_trial) - q(s_base): -dq * 2^-scale_log2 is the candidate's
 *                          TNS gain up to half a quantum per row; negative is an improvement
 *   dviol[g][w]     int    the sum of [s_trial < 0] - [s_base < 0]
 *   new_nan[g][w]   int    the entries whose s_trial is NaN where s_base is not; a candidate is ELIGIBLE iff this is 0
 *   capped[g][w]    int    the entries whose trial or base quantum is the cap
 *   worst[g][w]     fp32   the smallest valid (not NaN) s_trial among the group's entries, worst_row[g][w] the row that holds
 *                          it (the smallest row on equal slack); no valid s_trial: NaN and -1
 *
 * A group without entries gets zeros, a NaN worst and a worst_row of -1.  An entry whose row lies outside [0, T) takes part
 * in nothing.  One wave of 64 lanes per (group, offset), four per workgroup; the accumulators are integers only - int64 and
 * int32 adds and a 64-bit minimum over (ordered slack bits, row) keys -, so the result does not depend on the order; no float
 * atomics, no atomics at all, no workspace.  Every element of the slices is written by every call; nothing outside them is.
 *
 * 1 <= T <= 2^24, G >= 1, R >= 0, 1 <= radius <= 8, 0 <= w0 < w1 <= W, (long long)R * (w1 - w0) < 2^31, 0 <= scale_log2 <= 30;
 * dq 8-byte aligned; grow_row and pred_trial may be NULL when R == 0; no other null pointer. */
int mmft_search_score(const float* pred_trial, const float* pred_base, const float* required, int T,
                      const int* grow_ptr, const int* grow_row, int G, int R,
                      int radius, int w0, int w1, int scale_log2,
                      long long* dq, int* dviol, int* new_nan, int* capped, float* worst, int* worst_row,
                      int device, void* stream);

/* best_w [G], best_dq [G]: per group the ELIGIBLE offset (new_nan[g][w] == 0) with the smallest key (dq[g][w], |dx| + |dy|, w),
 * compared lexicographically, and its dq.  The centre of a table mmft_search_score wrote is eligible with dq == 0, so
 * best_dq <= 0 there; a group with no eligible offset (tables of another origin) gets best_w -1 and best_dq 0.  One wave per
 * group; integer comparisons only.
 *
 * THE BASE FIGURES come from this entry point too, by one small launch of their own (a memset and a kernel of integer
 * atomics, whose sums do not depend on the order): base [3] int64 = the sum of q(s_base) over design_rows [n] (the design's
 * rows of pred_base; a row outside [0, T) counts like a NaN row), the number of violating rows, the number of NaN rows.
 *
 * G >= 1, 1 <= radius <= 8, 1 <= n <= 2^24, 1 <= T <= 2^24, 0 <= scale_log2 <= 30; best_dq and base 8-byte aligned; no null
 * pointer. */
int mmft_search_best(const long long* dq, const int* new_nan, int G, int radius,
                     int* best_w, long long* best_dq,
                     const float* pred_base, const float* required, const int* design_rows, int n, int T, int scale_log2,
                     long long* base,
                     int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
