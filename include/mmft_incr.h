/* Incremental re-prediction: after an edit of a few feature rows only their transitive fan-out can change h, so the next
 * sweep runs over that cone alone.
 *
 * Like include/mmft_report.h and include/mmft_place.h this header holds what the reference's loops do not have, under the
 * conventions of mmft.h (extern "C", int results, raw device pointers, `int device, void* stream` last, the error codes and
 * mmft_last_error of mmft.h), compiled into the same library, bound by mmft.lib.incr and pinned by a ledger of its own
 * (tests/test_incr_cpu.py).
 *
 * The three entry points are the three pieces a resident h needs (mmft.infer.Predictor(incremental=True)):
 *   mmft_update_rows_diff            writes new feature rows and flags the rows that really changed (the SEEDS),
 *   mmft_fanout_cone_step            one level of seeds -> everything they can influence (the DIRTY rows),
 *   mmft_mlp2_feat_fwd_bf16_masked   the feature MLPs over the flagged rows only;
 * the level kernels of mmft.h already take the flags as `active`.
 */
#ifndef MMFT_INCR_H
#define MMFT_INCR_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One level of the FORWARD closure, in pull form - the mirror of mmft_fanin_cone_step.  For every node v of rows[0..n) (or
 * row0 + i when rows is NULL):
 *     mark[v] = (mark[v] != 0 or mark[u] != 0 for an in-neighbour u of v in either CSR) and (within == NULL or within[v] != 0)
 * The second CSR may be NULL (both arrays).  within (optional): a node with within[v] == 0 is never marked, and a mark it
 * carried is cleared - the result is intersected with the fan-in cone the sweep is restricted to.  Called for the levels
 * 1 .. L - 1 in ascending order after the seeds were set, it leaves mark = 1 exactly on the seeds and on every node they can
 * influence.  No atomics: only the thread that owns v writes mark[v], and the in-neighbours of a level's nodes lie in lower
 * levels, which this launch does not write - the result does not depend on scheduling.  n == 0 launches nothing. */
int mmft_fanout_cone_step(const int* rows, int row0, int n, const int* in_indptr0, const int* in_indices0,
                          const int* in_indptr1, const int* in_indices1, const unsigned char* within, unsigned char* mark,
                          int device, void* stream);

/* dst[t(i)][0 .. width) = src[i][0 .. width) for i in [0, n), t(i) = idx[i], or row0 + i when idx is NULL; and
 * seed[t(i)] = 1 where any of the row's elements differs BITWISE from what dst held (compared as 32-bit integers: a NaN
 * replaced by the same NaN is no change, -0.0 over 0.0 is one).  A flag is never cleared.  One pass: old and new row are
 * read once, compared, the new one stored.
 *   dst [.][ldd], src [n][lds]: fp32, ldd, lds >= width, 1 <= width <= 64; seed: one byte per row of dst
 *   idx: DISTINCT rows of dst (the host checks that; with a duplicate the row's final content and flag depend on scheduling);
 *        the device does not range-check idx or row0 + n. */
int mmft_update_rows_diff(float* dst, long long ldd, const int* idx, int row0, int n, int width, const float* src,
                          long long lds, unsigned char* seed, int device, void* stream);

/* mmft_mlp2_feat_fwd_bf16 (mmft.h) over the rows whose flag is set: out[row0 + m] is written, with bitwise the value the
 * unmasked entry point stores, where active[row0 + m] != 0 and is left untouched elsewhere.  active: one byte per NODE
 * (indexed like x and out), not NULL.  A tile of 64 rows without a flag requests no x and runs no MFMA; a workgroup none of
 * whose tiles holds a flag exits before it fetches the weights. */
int mmft_mlp2_feat_fwd_bf16_masked(const float* x, long long ldx, int row0, int n, int fin, const float* w1, const float* b1,
                                   const float* w2, const float* b2, float* out, long long ldout, int relu_out,
                                   const unsigned char* active, int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
