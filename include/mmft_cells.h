/* The cells that violate now and their search plan, built on the device.
 *
 * A timing-driven placer does not search a fixed set of cells: after every commit it searches the cells that lie on violating
 * paths NOW.  The entry points below select, from the kept predictions as they are at call time, the cells of a cell set that
 * have a row below a slack threshold, and build every table of a search plan (mmft_search.h) for exactly those cells, so that
 * neither a download nor host table arithmetic stands between a patched commit and the next search.
 *
 * THE INPUTS.
 *   - a CELL SET of one design: cell_ptr [C + 1], cell_node [M], CSR; cell c holds the pins cell_node[cell_ptr[c] ..
 *     cell_ptr[c + 1]), node ids in the tables' numbering;
 *   - the static INCIDENCE of the selection: inc_ptr [N + 1], inc_row [nnz]; pin n lies on the rows inc_row[inc_ptr[n] ..
 *     inc_ptr[n + 1]) of pred, ascending, each once (mmft.trial.rows_of_pin);
 *   - the kept pred [T] and required [T], fp32;
 *   - the design's ROW RANGE row_lo, span: its rows lie in [row_lo, row_lo + span);
 *   - slack_below, an fp32 threshold, or none (use_threshold == 0).
 *
 * THE RULE.  The ROWS OF A CELL are the ascending union, each row once, of its pins' incidence rows that lie in
 * [row_lo, row_lo + span); a row outside that range takes part in nothing, in the count and in the fill alike, and so does a
 * pin outside [0, N).  The SLACK of row r is s = (required[r] - pred[r]) + 0.0f, the rule of mmft_report.h: one fp32
 * subtraction, and -0.0 becomes +0.0.  Cell c is SELECTED iff it holds 1 .. 64 pins and
 *   - no threshold is given, or
 *   - one of its rows has a slack that is not NaN and satisfies s < slack_below; the compare is strict and in fp32.
 * So a slack of -0.0 does not violate at threshold 0; a cell without pins, with more than 64, or - under a threshold -
 * without a row or with NaN rows only is not selected.  The WORST of a cell of 1 .. 64 pins is the smallest non-NaN slack among
 * its rows, NaN (0x7fc00000) where there is none and for a cell of another size.  mmft.cells.count_host / critical_host
 * restate the rule in numpy.
 *
 * THE OUTPUT.  The selected cells, in ascending cell order, are the G groups of a search plan:
 *   grow_ptr [G + 1] | grow_row [R] | grow_grp [R] | mv_ptr [G + 1] | mv_node [MP]
 * word for word what mmft.search.plan_tables gives for those cells - grow_row lists ALL rows of a selected cell, not only the
 * violating ones: the search scores every row a move can change -, and behind them group_cell [G], the cell of each group,
 * and group_worst [G], the fp32 bits of its worst.
 *
 * THE ORDER of a build, all on one stream: mmft_cells_count; mmft_pairs_scan (mmft_pairs.h, as it stands) three times, over
 * sel, n_rows and n_pins, into sel_off, row_off, pin_off [C + 1] and an int64 [3] of totals G, R, MP, which the caller reads
 * before it trusts an offset; mmft_cells_fill.  Count, then scan, then fill: where a group, an entry or a pin lands depends on
 * the tables alone, never on the scheduling.
 *
 * Like include/mmft_pairs.h this header holds entry points beyond mmft.h, under its conventions (extern "C", int results, raw
 * device pointers, `int device, void* stream` last, the error codes and mmft_last_error of mmft.h), compiled into the same
 * library.  It is bound by mmft.cells.abi - an accessor of its own, outside the table of mmft.lib - and pinned by a ledger of
 * its own (tests/test_cells_cpu.py).  Every entry point validates every argument on the host before the device is looked at;
 * anything outside its limits is MMFT_ERR_BAD_ARG and nothing is launched.  No entry point allocates or synchronises or uses a
 * global atomic; integer code plus one fp32 subtraction, addition and compare per visited row; no workspace; same inputs, same
 * bits.
 */
#ifndef MMFT_CELLS_H
#define MMFT_CELLS_H

#include "mmft.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MMFT_CELLS_MAX_SPAN 65536      /* rows of a design's range: a bitmap of 8 KiB per wave */
#define MMFT_CELLS_MAX_PINS 64         /* pins of a cell that can be selected: the limit of a search plan's group */

/* Per cell c in [0, C), under THE RULE:
 *
 *   sel[c]       1 where the cell is selected, else 0
 *   n_rows[c]    the number of its rows where selected, else 0
 *   n_pins[c]    the number of its pins where selected, else 0
 *   worst[c]     its worst
 *
 * Every element of the four is written by every call; nothing else is.  Entries of cell_ptr are clamped to [0, M], those of
 * inc_ptr to [0, nnz].  One wave per cell, four per workgroup; per wave a bitmap of span bits in LDS.  The (pin, row) pairs of
 * a cell are numbered through a prefix sum of its pins' list lengths and dealt to the lanes 64 at a time, so a list of
 * hundreds of rows is spread over the wave; a lane finds its pair's pin by binary search in the prefix, sets the row's bit with
 * an LDS OR - the bits are the same in every schedule - and forms the row's slack.  A row that several pins share is visited
 * once per pin: the minimum and the verdict do not change by it.  n_rows is a popcount over the words that were touched.
 *
 * C >= 0, M >= 0, N >= 1, nnz >= 0, T >= 1, row_lo >= 0, 1 <= span <= MMFT_CELLS_MAX_SPAN, row_lo + span <= T; use_threshold 0
 * or 1; slack_below not NaN where it is used; cell_node may be NULL when M == 0 and inc_row when nnz == 0; no other null
 * pointer.  C == 0 returns 0 once the sizes are in order and looks at no pointer. */
int mmft_cells_count(const int* cell_ptr, const int* cell_node, int C, int M,
                     const int* inc_ptr, const int* inc_row, int N, int nnz,
                     const float* pred, const float* required, int T, int row_lo, int span,
                     int use_threshold, float slack_below,
                     int* sel, int* n_rows, int* n_pins, float* worst,
                     int device, void* stream);

/* The tables of THE OUTPUT from sel and worst as mmft_cells_count wrote them on the SAME cell set, incidence and row range,
 * and sel_off, row_off, pin_off [C + 1], the scans of its sel, n_rows and n_pins (G = sel_off[C], R = row_off[C],
 * MP = pin_off[C]).  For every selected cell c, with g = sel_off[c]:
 *
 *   grow_row, grow_grp    its rows, ascending, from row_off[c] on, and g beside each
 *   grow_ptr[g]           row_off[c]
 *   mv_ptr[g]             pin_off[c]
 *   mv_node               its pins from pin_off[c] on, in the cell's own order
 *   group_cell[g]         c
 *   group_worst[g]        the bits of worst[c]
 *
 * and the closing grow_ptr[G] = row_off[C], mv_ptr[G] = pin_off[C].  With matching inputs every element of the seven is
 * written once per call and nothing else is.  The kernel rebuilds the cell's bitmap as mmft_cells_count does; a row's place is
 * the number of set bits below it, so the rows come out ascending.  A place outside its table is not written (tables that
 * changed between the count and the fill cannot make the kernel write out of bounds): a group outside [0, G), an entry
 * outside the cell's own row_off[c] .. row_off[c + 1) or outside [0, R), a pin outside [0, MP).  Offsets read from the tables
 * are clamped to their table's size.  Integer code only.  One wave per cell, four per workgroup, and one more wave that
 * closes the two pointer tables.
 *
 * The limits of mmft_cells_count on C, M, N, nnz, row_lo, span (row_lo + span < 2^31); C >= 1; G >= 0, R >= 0, MP >= 0;
 * G <= C; grow_row / grow_grp may be NULL when R == 0, mv_node when MP == 0, cell_node when M == 0, inc_row when nnz == 0; no
 * other null pointer.  G == 0 returns 0 once the sizes are in order, looks at no pointer and writes nothing. */
int mmft_cells_fill(const int* cell_ptr, const int* cell_node, int C, int M,
                    const int* inc_ptr, const int* inc_row, int N, int nnz, int row_lo, int span,
                    const int* sel, const float* worst, const int* sel_off, const int* row_off, const int* pin_off,
                    int G, int R, int MP,
                    int* grow_ptr, int* grow_row, int* grow_grp, int* mv_ptr, int* mv_node, int* group_cell, int* group_worst,
                    int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
