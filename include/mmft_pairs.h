/* Near pairs of a search plan's groups and their swap tables, built on the device.
 *
 * A placer swaps a cell with cells NEAR it, and who is near changes with every commit.  The entry points below form, from the
 * resident pins as they are at call time, the pairs of a swap plan (mmft_swap.h) and every table that goes with them, so that
 * no host table arithmetic stands between a commit and the next search.
 *
 * The GROUPS are those of a search plan (mmft_search.h): group g holds the pins mv_node[mv_ptr[g] .. mv_ptr[g + 1]), node ids
 * in the tables' numbering, and its rows are grow_row[grow_ptr[g] .. grow_ptr[g + 1]).  The ANCHOR of a group is its first pin,
 * as in mmft_swap.h; (Ax_g, Ay_g) are loc_x / loc_y of the anchor, in map cells (mmft_place.h).
 *
 * THE RULE.  Groups a < b form a NEAR PAIR iff all of these hold:
 *   - both are non-empty and both anchors lie in [0, n_nodes);
 *   - size[a] + size[b] <= 64, the limit of mmft_swap_rows;
 *   - klass[a] == klass[b] where a class table is given (a placer may only swap cells of one footprint); klass == NULL is
 *     one class;
 *   - 1 <= max(|Ax_a - Ax_b|, |Ay_a - Ay_b|) <= reach, the differences formed in 64 bits: one pin may sit at INT32_MAX and
 *     another at INT32_MIN, and a 32-bit difference would wrap.
 * Anchors that coincide are no pair: their swap is the zero move.  The pairs are listed in ascending (a, b), each unordered
 * pair once, K in all.  mmft.pairs.near_pairs_host restates the rule in numpy.
 *
 * THE TABLES are those of mmft.swap.pair_tables on these pairs, in the layout a swap plan keeps in one int32 buffer:
 * pair_a [K] | pair_b [K] | prow_ptr [K + 1] | prow_row [RP] | prow_pair [RP] | sel_ptr [K + 1] | sel_row [RP + 2 K], with the
 * entries of a pair and THE SELECT TABLE as mmft_swap.h defines them.
 *
 * THE ORDER of a build, all on one stream: mmft_pairs_near_count, mmft_pairs_scan (the caller reads K), mmft_pairs_near_fill,
 * mmft_pairs_rows_count, mmft_pairs_scan into prow_ptr (the caller reads RP), mmft_pairs_rows_fill.  Count, then scan, then
 * fill: where a pair or an entry lands depends on the tables alone, never on the scheduling - a slot counter of atomics would
 * number the pairs differently from run to run, and mmft_commit_select breaks ties by k.
 *
 * Like include/mmft_swap.h this header holds entry points beyond mmft.h, under its conventions (extern "C", int results, raw
 * device pointers, `int device, void* stream` last, the error codes and mmft_last_error of mmft.h), compiled into the same
 * library.  It is bound by mmft.pairs.abi - an accessor of its own, outside the table of mmft.lib - and pinned by a ledger of
 * its own (tests/test_pairs_cpu.py).  Every entry point validates every argument on the host before the device is looked
 * at; anything outside its limits is MMFT_ERR_BAD_ARG and nothing is launched.  No entry point allocates or synchronises;
 * integer code only, no atomics, no workspace; same inputs, same bits.
 */
#ifndef MMFT_PAIRS_H
#define MMFT_PAIRS_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cnt[a], a in [0, G) = the number of groups b > a that form a near pair with a under THE RULE.
 *
 *   mv_ptr [G + 1], mv_node [M]    the groups' pins, CSR; entries of mv_ptr are clamped to [0, M]
 *   loc_x, loc_y [n_nodes]         the resident pins: read, never written
 *   klass [G] or NULL              the class of each group
 *   cnt [G]                        every element is written by every call; nothing else is
 *
 * A group of more than 64 pins pairs with nothing.  One thread per a, 256 per workgroup; the anchors, sizes and classes of
 * 1024 partners at a time are staged in LDS once per workgroup, so the walk mv_ptr -> mv_node -> loc is made once per
 * staged partner and never per tested pair.
 *
 * 1 <= G <= 2^24, M >= 0, n_nodes >= 1, 1 <= reach; mv_node may be NULL when M == 0; klass may be NULL; no other null pointer. */
int mmft_pairs_near_count(const int* mv_ptr, const int* mv_node, int G, int M,
                          const int* loc_x, const int* loc_y, int n_nodes,
                          const int* klass, int reach, int* cnt,
                          int device, void* stream);

/* The exclusive prefix sum of in [n] into out [n + 1], and the total as int64:
 *
 *   total[0]       the sum of in[0 .. n), every element taken as the signed int it is, formed exactly in 64 bits
 *   out[i]         i in [0, n]: the LOW 32 BITS of the exact sum of in[0 .. i), as an int (two's complement).  While the
 *                  exact sums stay within int32 these ARE the sums; past that they wrap, and out[n] is the low word of total.
 *
 * The caller reads total before it trusts an offset of out.  One workgroup of 1024 threads walks the array in rounds of 4096
 * elements; in and out may not overlap.
 *
 * n >= 0; total 8-byte aligned; no null pointer.  n == 0 returns 0, writes nothing and looks at no pointer. */
int mmft_pairs_scan(const int* in, int n, int* out, long long* total,
                    int device, void* stream);

/* pair_a [K], pair_b [K]: the near pairs in ascending (a, b).  The pairs of group a take the slots off[a] .. off[a + 1), in
 * ascending b, off [G + 1] being the scanned counts of mmft_pairs_near_count on the SAME tables, pins, klass and reach.
 *
 * A slot outside [0, K) is not written (tables that changed between the count and the fill cannot make the kernel write out
 * of bounds); with matching inputs every element of both arrays is written once and nothing else is.  The kernel is that of
 * mmft_pairs_near_count.
 *
 * The limits of mmft_pairs_near_count, K >= 0, and off, pair_a, pair_b not NULL.  K == 0 returns 0 once the sizes are in order
 * and looks at no pointer. */
int mmft_pairs_near_fill(const int* mv_ptr, const int* mv_node, int G, int M,
                         const int* loc_x, const int* loc_y, int n_nodes,
                         const int* klass, int reach,
                         const int* off, int K, int* pair_a, int* pair_b,
                         int device, void* stream);

/* cnt[k], k in [0, K) = the size of the ascending union, each row once, of the rows of groups pair_a[k] and pair_b[k].
 *
 * The kernel RELIES on a group's rows being ascending with each row once - mmft.search.plan_tables guarantees it -: it counts
 * the rows of a that a binary search finds among those of b.  A group outside [0, G) holds no row; entries of grow_ptr are
 * clamped to [0, R].  One wave per pair, four per workgroup: a group's row list can hold hundreds of rows, which one thread
 * would walk behind one dependent load after another, while the 64 lanes of a wave each search for one row at a time.
 *
 * K >= 0, G >= 1, R >= 0; grow_row may be NULL when R == 0; no other null pointer.  K == 0 returns 0 once the sizes are in
 * order and looks at no pointer. */
int mmft_pairs_rows_count(const int* pair_a, const int* pair_b, int K,
                          const int* grow_ptr, const int* grow_row, int G, int R,
                          int* cnt,
                          int device, void* stream);

/* From prow_ptr [K + 1], the scanned counts of mmft_pairs_rows_count on the same pairs and plan (RP = prow_ptr[K]):
 *
 *   prow_row [RP], prow_pair [RP]   the entries of pair k, e in [prow_ptr[k], prow_ptr[k + 1]): the ascending union of its two
 *                                   groups' rows, and k
 *   sel_ptr [K + 1]                 prow_ptr[k] + 2 k
 *   sel_row [RP + 2 K]              THE SELECT TABLE: a pair's rows followed by T + pair_a[k] and T + pair_b[k]
 *
 * Every element of the four is written once per call and nothing else is.  An entry's place is its rank in the union -
 * its index in its own list plus the rows of the other list below it, less the shared rows counted already -, found by
 * binary search; the kernel RELIES on ascending rows, each once per group, as mmft_pairs_rows_count does.  A rank outside the
 * pair's slots is not written; entries of prow_ptr are clamped to [0, RP].  One wave per pair, four per workgroup.
 *
 * K >= 0, RP >= 0, RP + 2 K < 2^31, G >= 1, R >= 0, T >= 1, T + G <= 2^24 (the rows of the selection); grow_row, prow_row and
 * prow_pair may be NULL when their size is 0; no other null pointer.  K == 0 returns 0 once the sizes are in order and looks at
 * no pointer. */
int mmft_pairs_rows_fill(const int* pair_a, const int* pair_b, const int* prow_ptr, int K, int RP,
                         const int* grow_ptr, const int* grow_row, int G, int R, int T,
                         int* prow_row, int* prow_pair, int* sel_ptr, int* sel_row,
                         int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
