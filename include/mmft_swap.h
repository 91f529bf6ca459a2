/* Exact search and commit of cell swaps on the device.
 *
 * The GROUPS are those of a search plan (mmft_search.h): group g holds the pins mv_node[mv_ptr[g] .. mv_ptr[g + 1]), at most 64,
 * node ids in the tables' numbering, and its ENTRIES are the rows grow_row[grow_ptr[g] .. grow_ptr[g + 1]).  The ANCHOR of a
 * group is its first pin, mv_node[mv_ptr[g]]: the caller orders a cell's pins so that the first one stands for the cell's
 * position.  A PAIR k is (pair_a[k], pair_b[k]), two distinct non-empty groups that hold no more than 64 pins together.
 *
 * Under SWAP k, with A and B the anchors of a = pair_a[k] and b = pair_b[k], every pin n of group a sits at
 * sat32(loc[n] + (loc[B] - loc[A])) and every pin n of group b at sat32(loc[n] + (loc[A] - loc[B])), per axis: the difference
 * and the sum formed in 64 bits and saturated to int32 once, at the end, as mmft_search.h states its own sum (THE MASK RULE of
 * mmft_place.h clamps it anyway); every other pin where loc_x / loc_y have it.  The two cells exchange their anchors'
 * positions and each keeps its pins' offsets from its own anchor.  The anchors are read on the device at call time: the
 * tables stay valid while the placement moves.
 *
 * The ENTRIES of pair k are the ascending union, each row once, of the entries of a and of b: prow_row[e], prow_pair[e] == k,
 * for e in [prow_ptr[k], prow_ptr[k + 1]); RP entries in all.  A row that holds pins of both groups gets the overrides of
 * both.
 *
 * Like include/mmft_search.h this header holds entry points beyond mmft.h, under its conventions (extern "C", int results, raw
 * device pointers, `int device, void* stream` last, the error codes and mmft_last_error of mmft.h), compiled into the same
 * library.  It is bound by mmft.swap.abi - an accessor of its own, outside the table of mmft.lib - and pinned by a ledger of
 * its own (tests/test_swap_cpu.py).  Every entry point validates every argument on the host before the device is looked
 * at; anything outside its limits is MMFT_ERR_BAD_ARG and nothing is launched.
 *
 * The head forward over the entries' rows, between mmft_swap_rows and mmft_swap_score, is mmft_head_mlp_fwd (mmft_head.h) with
 * hid == NULL, as it stands.  THE SELECTION of a conflict-free set of swaps is mmft_commit_select (mmft_commit.h), as it
 * stands, with the pairs as its groups: best_w = pick, radius = 1 (the centre there is 4, so pick 0 is "not the centre" and
 * -1 "no eligible offset"), best_dq = dq, G = K, and as its entry table a SELECT TABLE - per pair its entries' rows followed
 * by two pseudo-rows, T + pair_a[k] and T + pair_b[k] - over T + (the number of groups) rows.  Two swaps then conflict iff
 * they share a row or a group, also when the shared group holds no row.  Swaps that share no row and no group cannot see each
 * other: applied together, the design's sum changes by exactly the sum of their dq (the argument of mmft_commit.h).
 */
#ifndef MMFT_SWAP_H
#define MMFT_SWAP_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* xt[e - e0][0 .. width) for every entry e in [e0, e1): the head's input row of row prow_row[e] under swap prow_pair[e].
 *
 * CONTRACT: the row is BITWISE the row mmft_trial_rows writes for the pair (prow_row[e], an explicit candidate that holds the
 * pins of a, then those of b, at the swapped coordinates).  The overrides of both groups are formed on the device from the
 * resident pins and the two anchors - group a's first, then b's, no more than 64 in all -, staged in LDS where
 * search_rows_kernel stages a group's, and the kernel then runs the code of mmft_trial_rows and mmft_search_rows
 * (trial_row_write: the copy of the columns around h_cnn, mask_raster_path_moved, place_project).
 *
 *   path_nodes .. f_off, GP, bias, x, ldx, xt, ldxt, width, cnn_col, Dout, S   as in mmft_trial_rows, with its limits
 *   prow_row, prow_pair [RP]           rows in [0, T), pairs in [0, K): NOT checked on the device (mmft.swap builds them)
 *   pair_a, pair_b [K]                 groups in [0, G); a pair with a group outside it or an empty group moves nothing
 *   mv_ptr [G + 1], mv_node [mv_ptr[G]]   the groups' pins, CSR, as in mmft_search_rows
 *   xt [e1 - e0][ldxt]
 *
 * One workgroup of 256 threads per entry.  Every element of xt[0 .. e1 - e0)[0 .. width) is written once per call; nothing
 * beyond `width` in a row and no row beyond slot e1 - e0 - 1 is written; loc_x / loc_y are read, never written; no atomics, no
 * workspace; same inputs, same bits.  Dynamic LDS as mmft_search_rows.
 *
 * The limits of mmft_search_rows (its G reads G >= 1, its R reads RP >= 0), K >= 1 and 0 <= e0 <= e1 <= RP.  e0 == e1 returns 0
 * once the sizes are in order and looks at no pointer. */
int mmft_swap_rows(const int* path_nodes, const int* path_lens, int maxlen,
                   const int* loc_x, const int* loc_y, int map_x, int map_y,
                   const int* paths, const int* f_off, int T,
                   const int* prow_row, const int* prow_pair, int RP,
                   const int* pair_a, const int* pair_b, int K,
                   const int* mv_ptr, const int* mv_node, int G,
                   int e0, int e1,
                   const float* GP, const float* bias,
                   const float* x, long long ldx, float* xt, long long ldxt,
                   int width, int cnn_col, int Dout, int S,
                   int device, void* stream);

/* The slices [k0, k1) of six tables [K] and of pick [K], from the predictions of the pairs' entries: that of entry e lies at
 * pred_trial[e - prow_ptr[k0]] (prow_ptr[k0] is read on the device).
 *
 *   dq (int64), dviol, new_nan, capped, worst (fp32), worst_row   the definitions of mmft_search_score word for word, a pair's
 *                          entries in the place of a group's under one offset: s_base from pred_base[r], s_trial from the
 *                          entry's prediction, r = prow_row[e]; the per-entry accumulation is one piece of device code
 *                          (csrc/search_score.h) that both kernels call
 *   pick[k]         int    0 where the pair is ELIGIBLE (new_nan[k] == 0), -1 otherwise
 *
 * A pair without entries gets zeros, a NaN worst, a worst_row of -1 and pick 0.  An entry whose row lies outside [0, T) takes
 * part in nothing.  One wave of 64 lanes per pair, four per workgroup; the accumulators are integers only, no atomics, no
 * workspace.  Every element of the slices is written by every call; nothing outside them is.
 *
 * base != NULL: it also writes THE BASE FIGURES of mmft_search_best - base [3] int64 = the sum of q(s_base) over
 * design_rows [n], the number of violating rows, the number of NaN rows - by a launch of their own (a memset and the kernel
 * of integer atomics mmft_search_best runs).  base == NULL: design_rows and n are not looked at.
 *
 * 1 <= T <= 2^24, K >= 1, 0 <= RP < 2^31, 0 <= k0 < k1 <= K, 0 <= scale_log2 <= 30; with base 1 <= n <= 2^24 and design_rows not
 * NULL; dq and base 8-byte aligned; prow_row and pred_trial may be NULL when RP == 0; no other null pointer. */
int mmft_swap_score(const float* pred_trial, const float* pred_base, const float* required, int T,
                    const int* prow_ptr, const int* prow_row, int K, int RP,
                    int k0, int k1, int scale_log2,
                    long long* dq, int* dviol, int* new_nan, int* capped, float* worst, int* worst_row, int* pick,
                    long long* base, const int* design_rows, int n,
                    int device, void* stream);

/* For every pair k with sel[k] != 0 and pick[k] == 0: the pins of both groups written at their swapped coordinates, saturating,
 * into loc_x / loc_y.  The addresses stay, so a replayed graph sees the move.
 *
 * Both anchors' coordinates are read before any pin of the pair is written (the anchors are pins of the pair).  The kernel
 * RELIES on the selected pairs sharing no group - two selected pairs that held one group would race on its pins -, which the
 * selection over the select table guarantees, and on the groups holding distinct pins (mmft.commit.check_plan).  A pair with
 * a group outside [0, G), with a == b, with an empty group or with an anchor outside [0, n_nodes) is skipped whole; a node id
 * outside [0, n_nodes) is skipped; no other element of loc_x / loc_y is written.  Entries of mv_ptr are clamped to [0, M].
 * One wave per pair, four per workgroup; no atomics, no workspace.
 *
 * n_nodes >= 1, K >= 1, G >= 1, M >= 0; mv_node may be NULL when M == 0; no other null pointer. */
int mmft_swap_apply(int* loc_x, int* loc_y, int n_nodes,
                    const int* sel, const int* pick,
                    const int* pair_a, const int* pair_b, int K,
                    const int* mv_ptr, const int* mv_node, int G, int M,
                    int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
