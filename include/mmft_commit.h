/* Commit a conflict-free set of best moves on the device.
 *
 * mmft_search_best (mmft_search.h) leaves, per pin group g, the best offset best_w[g] of its window and the change best_dq[g]
 * of the design's negative-slack sum under that move taken ALONE, in the integer quanta of mmft_crit_sums.h.  A pin feeds only
 * the path masks, so a move changes only the rows whose path holds one of the group's pins: the plan's ENTRIES grow_row[e], e
 * in [grow_ptr[g], grow_ptr[g + 1]).  Two groups that share no row and no pin cannot see each other's moves: applied together,
 * each row changes exactly as under its own group's move alone, and the design's sum changes by exactly the sum of their
 * best_dq.  mmft_commit_select picks such a set; mmft_commit_apply writes its pins.
 *
 * Like include/mmft_search.h this header holds entry points beyond mmft.h, under its conventions (extern "C", int results, raw
 * device pointers, `int device, void* stream` last, the error codes and mmft_last_error of mmft.h), compiled into the same
 * library.  It is bound by mmft.commit.abi - an accessor of its own, outside the table of mmft.lib - and pinned by a ledger of
 * its own (tests/test_commit_cpu.py).  Every entry point validates every argument on the host before the device is looked
 * at; anything outside its limits is MMFT_ERR_BAD_ARG and nothing is launched.  The window (radius, offset w -> (dx, dy), the
 * CENTRE, sat32) is that of mmft_search.h.
 */
#ifndef MMFT_COMMIT_H
#define MMFT_COMMIT_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* THE ROW-OWNER TABLE of mmft_commit_select: per row of [0, T) one int64 (the smallest bid) and, behind all of those, one
 * int32 (the group that made it); 8-byte aligned.  The kernel initialises what it reads: no memset is expected. */
#define MMFT_COMMIT_OWNER_BYTES(T) (12ll * (long long)(T))

/* sel [G] (0 / 1) and stats [4] from best_w [G], best_dq [G] as mmft_search_best wrote them.
 *
 *   CANDIDATE   best_w[g] >= 0, best_w[g] != the centre 2 r (r + 1), best_dq[g] <= -min_q
 *   CONFLICT    two groups that share a row of grow_row; an entry whose row lies outside [0, T) conflicts with nothing
 *   sel         the lexicographically first maximal independent set of the candidates under the key (best_dq[g], g)
 *               ascending: visit the candidates in key order, take a group iff none of its rows belongs to a group already
 *               taken.  A candidate without entries is always taken
 *   stats       int64: the number selected, the sum of their best_dq, the number of candidates, the rounds the kernel ran
 *
 * ONE launch of ONE workgroup of 1024 threads, a thread per group (strided), rounds separated by workgroup barriers.  In a
 * round every live candidate bids for its rows in `owner` by two integer minima - best_dq first, then g among the groups
 * that hold that minimum -; a candidate that owns all its rows is taken; every live candidate that finds a taken owner on
 * one of its rows dies; the survivors clear their rows.  The smallest live key always owns its rows, so a round settles
 * at least one candidate: at most G rounds, five barriers each, no spin, no grid barrier, no flag between workgroups, no
 * float atomics; the result does not depend on the order in which threads arrive - same inputs, same bits.  The rounds are
 * the length of the longest chain of candidates in which each is beaten only by its predecessor: one on a clique, G / 2 on a
 * path whose keys increase along it.  The cost is latency, rounds times barriers.
 *
 * sel is written in full and used as the kernel's state on the way; stats in full; owner [MMFT_COMMIT_OWNER_BYTES(T)] is
 * scratch.  Nothing else is written.  Entries of grow_ptr are clamped to [0, R].
 *
 * G >= 1, 1 <= radius <= 8, R >= 0, 1 <= T <= 2^24, min_q >= 1; best_dq, stats and owner 8-byte aligned; grow_row may be NULL
 * when R == 0; no other null pointer. */
int mmft_commit_select(const int* best_w, const long long* best_dq, int G, int radius,
                       const int* grow_ptr, const int* grow_row, int R, int T, long long min_q,
                       int* sel, long long* stats, void* owner,
                       int device, void* stream);

/* For every group g with sel[g] != 0 and 0 <= best_w[g] < W, and every pin n in mv_node[mv_ptr[g] .. mv_ptr[g + 1]):
 * loc_x[n] = sat32(loc_x[n] + dx), loc_y[n] = sat32(loc_y[n] + dy), (dx, dy) the offset of best_w[g]; the sums are formed in 64
 * bits and saturated, as mmft_search.h states it.  The pins of different groups are DISTINCT: the kernel relies on it (two
 * groups that held one pin would race), mmft.commit.check_plan guarantees it.  A node id outside [0, n_nodes) is skipped; no
 * other element of loc_x / loc_y is written; the addresses stay, so a replayed graph sees the move.  Entries of mv_ptr are
 * clamped to [0, M].  One wave per group, four per workgroup; no atomics, no workspace.
 *
 * n_nodes >= 1, G >= 1, M >= 0, 1 <= radius <= 8; mv_node may be NULL when M == 0; no other null pointer. */
int mmft_commit_apply(int* loc_x, int* loc_y, int n_nodes,
                      const int* sel, const int* best_w, int radius,
                      const int* mv_ptr, const int* mv_node, int G, int M,
                      int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
