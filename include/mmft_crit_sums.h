/* Negative-slack sums and TNS shares per pin and per map cell, on the device: next to the worst slack and the count of
 * violating paths of include/mmft_crit.h, how much negative slack flows through a pin or a cell, and which part of its
 * design's TNS that is - what a timing-driven placer weights nets and regions by.
 *
 * Like include/mmft_crit.h this header holds what the reference's loops do not have, under the conventions of mmft.h
 * (extern "C", int / long long results, raw device pointers, `int device, void* stream` last, the error codes and
 * mmft_last_error of mmft.h), compiled into the same library (csrc/crit.hip: the same three kernels, instantiated with the
 * sums), bound by mmft.lib.csum and pinned by a ledger of its own (tests/test_crit_sums_cpu.py).
 *
 * mmft_criticality_sums takes the arguments of mmft_criticality, with their meaning, rules and limits (SLACK AND VALIDITY,
 * ROWS, PER PIN, PER MAP CELL, counts: include/mmft_crit.h), and writes its seven outputs bitwise as mmft_criticality does.
 * One rasterisation per row serves the minima, the counts and the sums.
 *
 * THE QUANTUM.  A float sum depends on the order of its terms; an integer sum does not.  With scale_log2 in [0, 30], a valid
 * row that violates (slack < 0) contributes
 *     q = rint(min(-slack, 2^(32 - scale_log2)) * 2^scale_log2),
 *   computed exactly - the scaling by a power of two is exact, the rounding is to nearest, ties to even - so 0 <= q <= 2^32 in
 *   units of 2^-scale_log2.  A row with -slack >= 2^(32 - scale_log2), -inf included, contributes q = 2^32, the cap, and is
 *   SATURATED.  Rows that do not violate and NaN rows contribute nothing.
 *
 * THE SUMS (int64; 64-bit integer adds, which commute and associate: no float atomics, same inputs, same bits)
 *   node_nsum[n]      [N]     the sum of q over the (violating valid row, live position) pairs that hold pin n - the pairs
 *                             node_viol counts, so a pin repeated inside one row counts once per position
 *   cell_nsum[b][c]   [B][P]  the sum of q over the violating valid rows of design b whose mask covers c - the rows cell_viol
 *                             counts: once per row.  Given together with cell_share, and only with cell_slack / cell_viol
 *   design_nsum[b]    [B]     the sum of q over ALL violating valid rows of design b, rows with empty paths included:
 *                             -design_nsum[b] / 2^scale_log2 is the design's TNS up to half a quantum per row
 *   saturated[b]      [B] int the number of saturated rows of design b
 *
 * THE SHARES (fp32)
 *   node_share[n]     [N]     0 when node_row[n] == -1 or design_nsum[d] == 0, d = row_design[node_row[n]]; otherwise
 *                             (float)((double)node_nsum[n] / (double)design_nsum[d]): both conversions to fp64 and the
 *                             conversion to fp32 round to nearest, the division is one IEEE fp64 division.  Above 1 only for
 *                             a pin repeated inside a row
 *   cell_share[b][c]  [B][P]  the same from cell_nsum[b][c] and design_nsum[b]; 0 when design_nsum[b] == 0
 *
 * GUARANTEES: those of include/mmft_crit.h.  Every element of every output is written by every call; the outputs and the
 * workspace may hold anything before one.  Three launches.
 *
 * workspace: 8-byte aligned, at least mmft_criticality_sums_workspace_bytes(N, B, P) bytes (P = 0 without the cell outputs;
 * -1 for arguments outside the limits).  The sums accumulate in their outputs; the workspace holds the keyed words.
 *
 * LIMITS.  Those of mmft_criticality, and: 0 <= scale_log2 <= 30; (long long)T * maxlen <= 2^30, so that every sum is at most
 * 2^62; no null pointer among node_nsum, design_nsum, saturated, node_share; cell_nsum and cell_share both given with the cell
 * outputs and both NULL without them; the int64 outputs 8-byte aligned.  Anything else is MMFT_ERR_BAD_ARG and nothing is
 * launched. */
#ifndef MMFT_CRIT_SUMS_H
#define MMFT_CRIT_SUMS_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

long long mmft_criticality_sums_workspace_bytes(int N, int B, int P);
int mmft_criticality_sums(const float* pred, const float* required,
                          const int* path_nodes, const int* path_lens, int maxlen,
                          const int* loc_x, const int* loc_y, int map_x, int map_y,
                          const int* paths, const int* row_design, int T, int N, int B,
                          float* node_slack, int* node_row, int* node_viol, float* node_crit,
                          float* cell_slack, int* cell_viol,
                          int* counts,
                          int scale_log2,
                          long long* node_nsum, long long* cell_nsum, long long* design_nsum, int* saturated,
                          float* node_share, float* cell_share,
                          void* workspace, long long workspace_bytes, int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
