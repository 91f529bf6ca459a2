/* Sensitivity: the gradient of the feature MLPs fc_cell_self / fc_net_self - Linear(fin, 256) - ReLU - Linear(256, 128),
 * src/model.py:48-51 - with respect to their INPUT rows, bf16 math mode, without a stored hidden tensor.  It is the last hop
 * of mmft.sensitivity.Sensitivity: after the reverse netlist sweep G holds, for every cell and net row, the gradient at the
 * output of its feature MLP; this entry point carries it to cell_feat / net_feat.
 *
 * Like include/mmft_report.h, mmft_place.h, mmft_incr.h, mmft_crit.h, mmft_head.h and mmft_crit_sums.h this header holds an
 * entry point beyond the generic layer ABI of mmft.h, under its conventions (extern "C", int result, raw device pointers,
 * `int device, void* stream` last, the error codes and mmft_last_error of mmft.h), compiled into the same library, bound by
 * mmft.lib.sens and pinned by a ledger of its own (tests/test_sens_cpu.py).
 *
 * THE ARITHMETIC, for the rows r = row0 .. row0 + n - 1 of the node-indexed g [N][ldg >= 128] and x [N][ldx >= fin]; r()
 * rounds to bf16 (nearest even), every sum is fp32 - the rounding map of "feature MLPs" in oracle/bf16.py, its
 * dx = r(g) r(w) applied twice:
 *   h    = r(x[r]) r(W1)^T + b1          recomputed with the forward kernel's instruction sequence: the ReLU mask [h > 0]
 *                                        is bitwise the forward's
 *   dh   = (r(g[r]) r(W2)) [h > 0]
 *   dx[r][0 .. fin) = r(dh) r(W1)
 * W1 [256][fin], b1 [256], W2 [128][256] fp32, contiguous; dx fp32 [N][lddx >= fin].  1 <= fin <= 64.
 *
 * GUARANTEES.  Nothing is written outside rows row0 .. row0 + n - 1 or at a column >= fin; no row outside the range is
 * read.  One launch, no workspace, no atomics, no synchronisation between workgroups: same inputs, same bits.  n == 0
 * returns 0 and looks at no pointer.  Anything else outside the limits - a null pointer, n < 0, row0 < 0, row0 + n beyond
 * int, fin outside [1, 64], ldx < fin, lddx < fin, ldg < 128, ldg not a multiple of 4, g or b1 not 16-byte aligned -
 * is MMFT_ERR_BAD_ARG, checked on the host before the device is looked at, and nothing is launched. */
#ifndef MMFT_SENS_H
#define MMFT_SENS_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

int mmft_mlp2_feat_dx_bf16(const float* g, long long ldg, const float* x, long long ldx, int row0, int n, int fin,
                           const float* w1, const float* b1, const float* w2, float* dx, long long lddx,
                           int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
