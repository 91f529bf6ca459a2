/* Exact predictions for a batch of trial pin moves.
 *
 * A pin's coordinates feed the path masks and nothing else, so the prediction under a trial move differs from the resident
 * one only on the rows whose path holds a moved pin, and on those rows only in the h_cnn columns of the head's input.  A
 * CANDIDATE is a set of pins that move together; a PAIR p is (row t = pair_row[p], candidate k = pair_cand[p]): row t of the
 * resident batch, re-projected with candidate k's pins where the candidate puts them.  The pairs of a candidate are
 * consecutive, pair_ptr[k] .. pair_ptr[k + 1], and ascend by row.
 *
 * Like include/mmft_report.h and mmft_place.h this header holds entry points beyond mmft.h, under its conventions
 * (extern "C", int results, raw device pointers, `int device, void* stream` last, the error codes and mmft_last_error of
 * mmft.h), compiled into the same library.  It is bound by mmft.trial.abi - an accessor of its own, outside the table of
 * mmft.lib - and pinned by a ledger of its own (tests/test_trial_cpu.py).
 *
 * The head forward over the pairs' rows is mmft_head_mlp_fwd (mmft_head.h) with hid == NULL, as it stands.
 */
#ifndef MMFT_TRIAL_H
#define MMFT_TRIAL_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* xt[p][0 .. width) for p in [0, n_pairs): the head's input row of pair p.
 *
 *   xt[p][cnn_col .. cnn_col + Dout)   bias + the masked projection of path paths[t] (THE MASK RULE and the RUNS of
 *                                      mmft_place.h) through GP at offset f_off[t], with the pins mv_node[m] at (mv_x[m], mv_y[m])
 *                                      for m in [mv_ptr[k], mv_ptr[k + 1]) - at EVERY occurrence of such a node in the row - and
 *                                      every other pin where loc_x / loc_y have it: BITWISE the row mmft_placed_fc_fwd gives
 *                                      on copies of loc_x / loc_y with the candidate written in (the two kernels share the code
 *                                      of the raster's boxes, the run numbering and the accumulation)
 *   every other column below width     copied from x[t]
 *
 *   path_nodes, path_lens, maxlen, loc_x, loc_y, map_x, map_y, paths [T], f_off [T] or NULL, GP, bias or NULL
 *                                      as in mmft_placed_fc_fwd; loc_x / loc_y are read, never written
 *   pair_row, pair_cand [n_pairs]      rows in [0, T), candidates in [0, K): NOT checked on the device (mmft.trial builds them)
 *   mv_ptr [K + 1], mv_node, mv_x, mv_y [mv_ptr[K]]   the candidates' moves, CSR; node ids in the tables' numbering, distinct inside
 *                                      a candidate, at most 64 per candidate (the kernel reads no more than 64); any int
 *                                      coordinate: clamped by the rule
 *   x [T][ldx], xt [n_pairs][ldxt]     fp32, 16-byte aligned
 *
 * One workgroup of 256 threads per pair; the overrides are staged in LDS and applied where the raster stages a node's
 * coordinates.  Every element of xt[0 .. n_pairs)[0 .. width) is written once per call; nothing beyond `width` in a row and no
 * row at or beyond n_pairs is written; no atomics in global memory, no workspace; same inputs, same bits.
 *
 * S == 64; P = map_x * map_y a multiple of 64, <= 65536; Dout a multiple of 4 in [4, 1024]; cnn_col, ldx, ldxt multiples of
 * 4; 0 <= cnn_col, cnn_col + Dout <= width <= ldx, ldxt; maxlen >= 1; T >= 1; K >= 1; n_pairs >= 0; GP, x, xt and bias 16-byte
 * aligned; no null pointer but f_off and bias.  Anything else is MMFT_ERR_BAD_ARG, refused on the host before the device is
 * looked at, and nothing is launched.  n_pairs == 0 returns 0 once the sizes are in order and looks at no pointer. */
int mmft_trial_rows(const int* path_nodes, const int* path_lens, int maxlen,
                    const int* loc_x, const int* loc_y, int map_x, int map_y,
                    const int* paths, const int* f_off, int T,
                    const int* pair_row, const int* pair_cand, int n_pairs,
                    const int* mv_ptr, const int* mv_node, const int* mv_x, const int* mv_y, int K,
                    const float* GP, const float* bias,
                    const float* x, long long ldx, float* xt, long long ldxt,
                    int width, int cnn_col, int Dout, int S,
                    int device, void* stream);

/* summary [K + 1][6] double: one design's timing figures under each candidate, and (entry K) on the pins as they are.
 *
 *   design_rows [n]                    the design's rows of pred_base, ascending (a row outside [0, T) counts like a NaN row)
 *   pred(r) under candidate k          pred_trial[p] where pair_row[p] == r for a p in [pair_ptr[k], pair_ptr[k + 1]) - found by
 *                                      binary search, the range ascends by row -, pred_base[r] otherwise; entry K: pred_base[r]
 *   slack                              the rule of mmft_report.h: required[r] - pred(r) in one fp32 subtraction, -0.0
 *                                      canonicalised to +0.0; a NaN slack is counted in n_nan and takes part in nothing else; a
 *                                      row VIOLATES when slack < 0
 *   summary[k]                         n_valid, n_nan, n_violating, wns, wns_row, tns - wns the smallest valid slack, wns_row the
 *                                      row that holds it (the smallest row on equal slack); n_valid == 0: wns NaN, wns_row -1, tns 0
 *   tns                                the fp64 sum of the violating slacks IN THIS ORDER: thread j of 256 adds its rows
 *                                      design_rows[j], [j + 256], ... in ascending order to 0.0; the 64 threads of a wave
 *                                      combine by s = s + s(lane ^ o) for o = 32, 16, 8, 4, 2, 1; the four waves are added in
 *                                      the order 0, 1, 2, 3 to 0.0.  (mmft.trial.reduce_host restates it.)
 *
 * One workgroup of 256 threads per entry; no float atomics, no workspace; every element of summary is written by every call;
 * same inputs, same bits.
 *
 * 1 <= n <= 2^24, 1 <= T <= 2^24, K >= 0, n_pairs >= 0; pair_ptr, pair_row and pred_trial may be NULL when n_pairs == 0 and
 * K == 0 (only the base is formed); pair_ptr not NULL when K > 0; pair_row and pred_trial not NULL when n_pairs > 0; summary
 * 8-byte aligned; no other null pointer.  Anything else is MMFT_ERR_BAD_ARG and nothing is launched. */
int mmft_trial_reduce(const float* pred_base, const float* pred_trial, const float* required,
                      const int* design_rows, int n, int T,
                      const int* pair_ptr, const int* pair_row, int n_pairs, int K,
                      double* summary,
                      int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
