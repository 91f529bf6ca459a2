/* Extensions of libmmft_hip.so beyond the reference's hot path.
 *
 * include/mmft.h declares what the reference's training and evaluation loops need; its entry points are pinned one by one
 * by the kernel-level ledger of tests/test_host_cpu.py.  What the reference does not have lives here, under the same
 * conventions (extern "C", int / long long results, raw device pointers, `int device, void* stream` last, the error codes
 * and mmft_last_error of mmft.h), compiled into the same library, bound by mmft.lib.ext and pinned by a ledger of its own
 * (tests/test_report_cpu.py).
 */
#ifndef MMFT_REPORT_H
#define MMFT_REPORT_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Timing report of a batch of designs, on the device: per design the worst and the total negative slack, the number of
 * violating endpoints, the k most critical endpoints and (optionally) a slack histogram.
 *
 *   slack[t] = required[t] - pred[t]   one fp32 subtraction, -0.0 canonicalised to +0.0; a row VIOLATES when slack < 0 (the
 *                                      rule of mmft_eval_sums).  A row whose slack is NaN is counted in n_nan and takes part
 *                                      in nothing else; +-inf are ordinary values.
 *   design_ptr [B + 1], design_rows [T]   the batch rows of design b are design_rows[design_ptr[b] .. design_ptr[b + 1]); a
 *                                      design may be empty.  (A row index outside [0, T) is counted like a NaN row.)
 *   summary [B][6] double              n_valid, n_nan, n_violating, wns, wns_row, tns: wns the smallest slack of the valid
 *                                      rows and wns_row the batch row that holds it (the smallest row on equal slack), tns
 *                                      the fp64 sum of the violating slacks; n_valid == 0: wns NaN, wns_row -1, tns 0.
 *   worst_row, worst_slack [B][k]      the design's min(k, n_valid) valid rows in ascending (slack, row) order, the rest
 *                                      padded with -1 / +inf.
 *   hist [B][nbins + 2] int            w = (hist_hi - hist_lo) / nbins in fp32: bin 0 counts valid slacks < hist_lo, bin
 *                                      nbins + 1 those >= hist_hi, bin 1 + min(nbins - 1, (int)floorf((slack - hist_lo) / w))
 *                                      the others.  nbins == 0: no histogram, hist may be NULL, hist_lo / hist_hi are ignored.
 *
 * 1 <= k <= 64, 0 <= nbins <= 64 (hist_lo < hist_hi, both finite, when nbins > 0), B >= 1, 1 <= T <= 2^24; anything else is
 * MMFT_ERR_BAD_ARG and nothing is launched.  Every element of every output is written by every call.  The result does not
 * depend on the order in which workgroups run: same inputs, same bits.
 *
 * workspace (8-byte aligned, at least mmft_timing_report_workspace_bytes(T, B, k, nbins) bytes; -1 for arguments outside
 * the limits) holds one arrival counter per design and the partial results of designs with more than 4096 rows.  Its
 * contents need not survive between calls and may be anything before one. */
long long mmft_timing_report_workspace_bytes(int T, int B, int k, int nbins);
int mmft_timing_report(const float* pred, const float* required, const int* design_ptr, const int* design_rows,
                       int T, int B, int k, float hist_lo, float hist_hi, int nbins,
                       double* summary, int* worst_row, float* worst_slack, int* hist,
                       void* workspace, long long workspace_bytes, int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
