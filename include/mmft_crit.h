/* Timing criticality per pin and per map cell, on the device: what a timing-driven placer or sizer turns into net weights
 * and into regions to spread, from the predictions of a batch and the tables the masks that follow a placement already hold.
 *
 * Like include/mmft_report.h and include/mmft_place.h this header holds what the reference's loops do not have, under the
 * conventions of mmft.h (extern "C", int / long long results, raw device pointers, `int device, void* stream` last, the error
 * codes and mmft_last_error of mmft.h), compiled into the same library, bound by mmft.lib.crit and pinned by a ledger of its
 * own (tests/test_crit_cpu.py).
 *
 * SLACK AND VALIDITY (exactly the rule of mmft_timing_report, include/mmft_report.h; one helper, csrc/slack_key.h, forms the
 * slack and its ordered key for both):
 *   slack[t] = required[t] - pred[t], one fp32 subtraction, -0.0 canonicalised to +0.0.  Row t is VALID unless its slack is
 *   NaN and VIOLATES when slack < 0; +-inf are ordinary values.  NaN rows are counted in counts[b][1] and take part in nothing
 *   else.
 *
 * ROWS.  paths[t] is the row of path_nodes / path_lens that batch row t predicts; row_design[t] in [0, B) is the row's
 * design, NULL: every row belongs to design 0.  The LIVE entries of path q are those at j < min(path_lens[q], maxlen);
 * entries at and beyond that are never read (the clipping of mmft_place.h).  Node ids are NOT checked on the device
 * (mmft.placement validates them once) but must lie in [0, N); a row_design outside [0, B) is not checked either.
 *
 * PER PIN n in [0, N), in the numbering of path_nodes (the caller's: node offset of the design + the design's own id):
 *   node_slack[n]  the smallest slack over the valid rows that hold n among their live entries; +inf if there is none
 *   node_row[n]    the smallest such batch row t among those with that slack; -1 if there is none
 *   node_viol[n]   the number of (violating valid row, live position) pairs that hold n.  A traced path visits a pin once, so
 *                  this is the number of violating paths through the pin; a pin repeated inside one row counts once per
 *                  position
 *   node_crit[n]   0 when node_row[n] == -1 or node_slack[n] >= 0.  Otherwise let w be the smallest slack over ALL valid rows
 *                  of design row_design[node_row[n]] - rows with empty or one-pin paths included, so w <= node_slack[n] < 0:
 *                  1 when node_slack[n] == w (this covers -inf), else node_slack[n] / w in one fp32 division (IEEE, correctly
 *                  rounded).  In [0, 1].
 *   A path of one live entry contributes to the pin outputs (its endpoint) and has an empty mask.
 *
 * PER MAP CELL, when cell_slack / cell_viol are given (both or neither).  The mask of a row is THE MASK RULE of
 * include/mmft_place.h for path paths[t], evaluated from the pins' CURRENT coordinates loc_x / loc_y; cell c = x * map_y + y.
 *   cell_slack[b][c]  the smallest slack over the valid rows of design b whose mask covers c; +inf if there is none
 *   cell_viol[b][c]   the number of violating valid rows of design b whose mask covers c (a mask is a set: once per row)
 *   P = map_x * map_y must then be a multiple of 64 and at most 65536, the limits of mmft_placed_fc_fwd.  Without the cell
 *   outputs map_x, map_y, loc_x and loc_y are ignored and may be 0 / NULL.
 *
 * counts [B][2] int: per design the number of valid rows and of NaN rows.
 *
 * GUARANTEES.  Every element of every output is written by every call; the outputs and the workspace may hold anything
 * before one.  The result does not depend on the order in which workgroups run: same inputs, same bits.  There are no float
 * atomics: a minimum is an unsigned integer minimum over an order-preserving key of the slack - a 64-bit (key << 32 | row)
 * word per pin, which settles the row with the slack, 32 bits per cell and per design - and the counts are integer adds.
 * Three launches: the keyed words are initialised, the rows scatter into them, the words are decoded into the outputs.
 *
 * workspace: 8-byte aligned, at least mmft_criticality_workspace_bytes(N, B, P) bytes (P = 0 without the cell outputs; -1
 * for arguments outside the limits); it holds the keyed words (8 N + 4 B + 4 B P bytes, rounded up).
 *
 * LIMITS.  1 <= T <= 2^24, N >= 1, B >= 1, maxlen >= 1; no null pointer but row_design, the cell outputs and, without them,
 * loc_x / loc_y.  Anything else is MMFT_ERR_BAD_ARG and nothing is launched. */
#ifndef MMFT_CRIT_H
#define MMFT_CRIT_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

long long mmft_criticality_workspace_bytes(int N, int B, int P);
int mmft_criticality(const float* pred, const float* required,
                     const int* path_nodes, const int* path_lens, int maxlen,
                     const int* loc_x, const int* loc_y, int map_x, int map_y,
                     const int* paths, const int* row_design, int T, int N, int B,
                     float* node_slack, int* node_row, int* node_viol, float* node_crit,
                     float* cell_slack, int* cell_viol,
                     int* counts,
                     void* workspace, long long workspace_bytes, int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
