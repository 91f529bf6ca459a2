/* The fusion head's mlp_fuse - MLP(288, 576, 1) over the T sampled endpoints of a batch (src/model.py:267,291) - forward
 * and backward as three fused kernels, bf16 math mode.
 *
 * Like include/mmft_report.h, mmft_place.h, mmft_incr.h and mmft_crit.h this header holds entry points beyond the generic
 * layer ABI of mmft.h, under its conventions (extern "C", int / long long results, raw device pointers, `int device, void*
 * stream` last, the error codes and mmft_last_error of mmft.h), compiled into the same library, bound by mmft.lib.head and
 * pinned by a ledger of its own (tests/test_head_mlp_cpu.py).
 *
 * THE ARITHMETIC is the rounding map of bf16 math mode for "head: mlp_fuse" (oracle/bf16.py): r() rounds to bf16 (nearest
 * even), both operands of every contraction are rounded, every sum is fp32, bias gradients come from the fp32 gradient.
 *   y1   = r(x) r(W1)^T + b1                       h    = relu(y1)              pred = r(h) r(w2) + b2
 *   dh   = r(dpred) r(w2)      (exact in fp32)     g1   = dh [r(h) > 0]
 *   dx   = r(g1) r(W1)                             dW1  = r(g1)^T r(x)          db1  = sum_t g1
 *   dW2  = r(dpred)^T r(h)                         db2  = sum_t dpred
 * The only stored activation is r(h), bf16 [T][576]; the ReLU mask is read from it (it differs from [h > 0] only where h
 * is an fp32 denormal, which rounds to a bf16 denormal or to zero).
 *
 * SHAPES.  (in, hidden, out) = (288, 576, 1) only - mmft_head_mlp_supported is 1 for it and 0 for everything else.
 * x [T][ldx >= 288] and dx [T][lddx >= 288] fp32 with 16-byte aligned rows (ldx, lddx multiples of 4); w1 [576][288], b1
 * [576], w2 [576], b2 [1], dw1 [576][288], db1 [576], dw2 [576], db2 [1] fp32, contiguous, 16-byte aligned (b2 / db2: 4);
 * hid [T][576] bf16, contiguous, 16-byte aligned; pred, dpred [T] fp32.
 *
 * mmft_head_mlp_fwd: pred and - hid != NULL - hid.  hid == NULL (no gradient wanted) stores nothing else and gives
 * bitwise the same pred.  One launch.
 * mmft_head_mlp_bwd: dx (NULL: not wanted) and the four parameter gradients, stored (accumulate == 0) or added to what
 * the sinks hold (accumulate != 0).  Four launches: the transposed bf16 pack of w1 (made in this call, from the weights
 * of this call), the dx kernel with its per-workgroup partial rows of db1 / dW2 / db2, the dW1 kernel (one slab per
 * workgroup), one fixed-order reduction of all slabs.  workspace: 16-byte aligned, at least
 * mmft_head_mlp_workspace_bytes(T) bytes (-1 for T <= 0); may hold anything before the call.
 *
 * GUARANTEES.  No row at or beyond T is read or written; no atomics, no synchronisation between workgroups; same inputs,
 * same bits.  Anything outside the limits above is MMFT_ERR_BAD_ARG, checked on the host before the device is looked at,
 * and nothing is launched. */
#ifndef MMFT_HEAD_H
#define MMFT_HEAD_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

long long mmft_head_mlp_supported(int in, int hidden, int out);
long long mmft_head_mlp_workspace_bytes(long long T);
int mmft_head_mlp_fwd(const float* x, long long ldx, const float* w1, const float* b1, const float* w2, const float* b2,
                      void* hid, float* pred, long long T, int in, int hidden, int out, int device, void* stream);
int mmft_head_mlp_bwd(const float* dpred, const void* hid, const float* x, long long ldx, const float* w1, const float* w2,
                      float* dx, long long lddx, float* dw1, float* db1, float* dw2, float* db2,
                      long long T, int in, int hidden, int out, int accumulate,
                      void* workspace, long long workspace_bytes, int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
