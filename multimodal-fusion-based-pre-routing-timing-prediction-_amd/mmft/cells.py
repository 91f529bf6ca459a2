"""The cells that violate now and their search plan, built on the device (include/mmft_cells.h).

A timing-driven placer does not search a fixed set of cells: after every commit it searches the cells that lie on violating
paths now.  Predictor.cell_set validates and uploads a design's cells once; Predictor.critical_plan selects, from the kept
predictions as they are at call time - fresh after predict() and after a patched commit -, the cells with a row below a slack
threshold and builds their search plan on the device; Predictor.refine_cells puts a loop on top that re-targets every pass.

    check_threshold / check_cells     host validation of critical_plan's arguments
    restrict / count_host / critical_host / plan_host / words
                                      THE RULE of the header restated in numpy, and the tables and words a build must equal
    CellSet / cell_set                a design's cells on the device; the incidence, uploaded once per TrialState
    build / critical_plan             the five launches and the one size read of a plan; what Predictor.critical_plan delegates to
    refine_cells                      what Predictor.refine_cells delegates to

The entry points are bound by `abi`, an accessor of this module: the table of mmft.lib's accessors is pinned by its own ledger
and is not touched here.
"""
import math

import numpy as np
import torch

from . import commit as CM
from . import lib
from . import pairs as PR
from . import search as SE
from . import trial as TR
from .report import reference_slack

abi = lib.Header('mmft_cells.h')         # the cells that violate now: their count, and the tables of their search plan
abi_decls = abi.decls

MAX_SPAN = 65536                         # MMFT_CELLS_MAX_SPAN: a bitmap of 8 KiB per wave
MAX_PINS = TR.MAX_MOVES                  # MMFT_CELLS_MAX_PINS
NAN_BITS = 0x7fc00000                    # the worst of a cell without a valid row


# ------------------------------------------------------------------------------------------------ host validation
def check_threshold(slack_below, who='critical_plan'):
    """None for None (no threshold), else the threshold rounded to fp32 as a Python float; ValueError for a bool, something
    that is no number and a NaN."""
    if slack_below is None:
        return None
    if isinstance(slack_below, bool) or not isinstance(slack_below, (int, float, np.integer, np.floating)):
        raise ValueError(f'{who}: slack_below must be a number or None, got {slack_below!r}')
    with np.errstate(over='ignore'):
        thr = float(np.float32(slack_below))
    if math.isnan(thr):
        raise ValueError(f'{who}: slack_below must not be NaN')
    return thr


def check_cells(p, cells, who='critical_plan'):
    """RuntimeError without trials=True, TypeError for something that is no cell set, ValueError for one of another Predictor."""
    if getattr(p, '_trial', None) is None:
        raise RuntimeError(f'Predictor.{who}(): built without trials=True')
    if not isinstance(cells, CellSet):
        raise TypeError(f'{who}: cells must come from cell_set(), got {type(cells).__name__}')
    if cells.owner is not p:
        raise ValueError(f'{who}: the cell set belongs to another Predictor')


# ------------------------------------------------------------------------------------------------ the rule on the host
def restrict(rows_of_pin, row_lo, span):
    """(ptr, rows) of the incidence with every row outside [row_lo, row_lo + span) taken out: such a row takes part in
    nothing."""
    ptr, rows = (np.asarray(v, dtype=np.int64) for v in rows_of_pin)
    keep = (rows >= int(row_lo)) & (rows < int(row_lo) + int(span))
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    return before[ptr], rows[keep]


def count_host(rows_of_pin, node_off, pins, cell_ptr, pred, required, row_lo, span, slack_below):
    """(sel bool [C], n_rows int64 [C], n_pins int64 [C], worst fp32 [C]) of mmft_cells_count in numpy: THE RULE of
    include/mmft_cells.h.  pins: the design's own node ids, + node_off in the tables' numbering; slack_below None: no
    threshold.  A pin outside the incidence lies on no row."""
    ptr, rows = restrict(rows_of_pin, row_lo, span)
    pins, cell_ptr = np.asarray(pins, dtype=np.int64), np.asarray(cell_ptr, dtype=np.int64)
    pred, required = np.asarray(pred, dtype=np.float32).reshape(-1), np.asarray(required, dtype=np.float32).reshape(-1)
    C, size = cell_ptr.shape[0] - 1, np.diff(cell_ptr)
    ok = (size >= 1) & (size <= MAX_PINS)
    cell_of = np.repeat(np.arange(C, dtype=np.int64), size)
    node = pins + int(node_off)
    walked = ok[cell_of] & (node >= 0) & (node < ptr.shape[0] - 1)           # a cell of another size is not walked at all
    sub_ptr = np.concatenate([[0], np.cumsum(np.bincount(cell_of[walked], minlength=C))]).astype(np.int64)
    u_ptr, u_row, u_cell = TR.expand_candidates((ptr, rows), node_off, pins[walked], sub_ptr)
    s = reference_slack(pred[u_row], required[u_row])
    valid = ~np.isnan(s)
    least = np.full(C, np.inf, dtype=np.float32)
    np.minimum.at(least, u_cell[valid], s[valid])
    has = np.bincount(u_cell[valid], minlength=C) > 0
    worst = np.where(has, least, np.float32(np.nan)).astype(np.float32)
    if slack_below is None:
        sel = ok.copy()
    else:
        with np.errstate(invalid='ignore'):
            below = valid & (s < np.float32(slack_below))                    # strict, in fp32
        sel = ok & (np.bincount(u_cell[below], minlength=C) > 0)
    return sel, np.where(sel, np.diff(u_ptr), 0).astype(np.int64), np.where(sel, size, 0).astype(np.int64), worst


def critical_host(rows_of_pin, node_off, pins, cell_ptr, pred, required, row_lo, span, slack_below):
    """(cells int64 [G], worst fp32 [G]): the selected cells in ascending order and the smallest non-NaN slack among the rows of
    each, NaN where there is none."""
    sel, _, _, worst = count_host(rows_of_pin, node_off, pins, cell_ptr, pred, required, row_lo, span, slack_below)
    return np.flatnonzero(sel).astype(np.int64), worst[sel]


def pins_of(pins, cell_ptr, cells):
    """(pins int64 [M'], group_ptr int64 [G + 1]) of the cells `cells` as groups, one after another."""
    pins, cell_ptr, cells = (np.asarray(v, dtype=np.int64) for v in (pins, cell_ptr, cells))
    size = cell_ptr[cells + 1] - cell_ptr[cells]
    group_ptr = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
    flat = np.arange(int(group_ptr[-1]), dtype=np.int64) - np.repeat(group_ptr[:-1] - cell_ptr[cells], size)
    return pins[flat], group_ptr


def plan_host(rows_of_pin, node_off, pins, cell_ptr, cells, row_lo, span):
    """The five tables (int64) of search.plan_tables for the cells `cells`, on the incidence inside the row range."""
    sub, group_ptr = pins_of(pins, cell_ptr, cells)
    return SE.plan_tables(restrict(rows_of_pin, row_lo, span), node_off, sub, group_ptr)


def words(tables, cells, worst):
    """The int32 words of a build: grow_ptr | grow_row | grow_grp | mv_ptr | mv_node | group_cell | group_worst (fp32 bits)."""
    parts = [np.asarray(v).astype(np.int32) for v in tables] + [np.asarray(cells).astype(np.int32)]
    return np.concatenate(parts + [np.ascontiguousarray(worst, dtype=np.float32).view(np.int32)])


# ------------------------------------------------------------------------------------------------ the Predictor's side
class CellSet:
    """What cell_set returns: C cells of design i - pins (int64 [M], the design's own numbering) and cell_ptr (int64 [C + 1]) on
    the host and, in ONE int32 buffer on the device, cell_ptr | cell_node (the tables' numbering) -, and the design's row
    range row_lo, span.  No pin belongs to two cells.  Valid for the life of its Predictor, and its alone."""

    def __init__(self, owner, i, pins, cell_ptr, node_off, row_lo, span, device):
        self.owner, self.i, self.node_off = owner, int(i), int(node_off)
        self.pins, self.cell_ptr = pins, cell_ptr
        self.C, self.M = cell_ptr.shape[0] - 1, pins.shape[0]
        self.row_lo, self.span = int(row_lo), int(span)
        self.ints = torch.from_numpy(np.concatenate([cell_ptr, pins + self.node_off]).astype(np.int32)).to(device)
        self.dev = [self.ints[:self.C + 1], self.ints[self.C + 1:]]


def check_distinct(pins, cell_ptr, who='cell_set'):
    """ValueError where a pin belongs to two cells, naming the first such pin (in the order of `pins`) and the two cells."""
    _, first, count = np.unique(pins, return_index=True, return_counts=True)
    if (count > 1).any():
        pin = pins[first[count > 1].min()]
        at = np.flatnonzero(pins == pin)[:2]
        cell = np.searchsorted(cell_ptr, at, side='right') - 1
        raise ValueError(f'{who}: pin {int(pin)} belongs to cells {int(cell[0])} and {int(cell[1])}; the cells of a set must hold distinct pins')


def cell_set(p, i, pins, cell_ptr=None):
    """Predictor.cell_set: see there."""
    if getattr(p, '_trial', None) is None:
        raise RuntimeError('Predictor.cell_set(): built without trials=True')
    p._check_design(i, 'cell_set')
    rows = np.flatnonzero(np.asarray(p.slack.design) == int(i))              # the rows of p.slack.rows_of(i), on the host
    if rows.size == 0:
        raise ValueError(f'cell_set: design {i} has no selected path')
    placed = p._placed
    off = int(placed.node_off[i])
    pins, cell_ptr = TR.check_pin_sets(int(placed.node_off[i + 1]) - off, pins, cell_ptr, who='cell_set', ptr_name='cell_ptr', unit='cell',
                                       item='pins')
    if cell_ptr.shape[0] < 2:
        raise ValueError('cell_set: no cell')
    check_distinct(pins, cell_ptr)
    return CellSet(p, i, pins, cell_ptr, off, rows.min(), rows.max() - rows.min() + 1, p.device)


def incidence(p):
    """(inc_ptr int32 [N + 1], inc_row int32 [nnz]) on the device: TrialState.rows_of_pin, uploaded once per TrialState on
    first use."""
    st = p._trial
    dev = getattr(st, 'incidence_dev', None)
    if dev is None:
        ptr, rows = st.rows_of_pin
        if rows.shape[0] >= 2 ** 31:
            raise ValueError(f'critical_plan: the incidence holds {rows.shape[0]} entries, which do not stay below 2^31')
        dev = st.incidence_dev = (torch.from_numpy(np.asarray(ptr).astype(np.int32)).to(p.device),
                                  torch.from_numpy(np.asarray(rows).astype(np.int32)).to(p.device))
    return dev


def build(p, cells, thr, max_groups, who='critical_plan', timed=None):
    """The launches of a plan on the current stream with the one size read between them: (buf, G, R, MP) - the int32 buffer in
    SearchPlan's layout with group_cell and group_worst behind it -, or None where no cell is selected.  thr: None or the
    fp32 threshold.  `timed`: a callable that is handed each part as a function (tools/bench_placement.py times them apart)."""
    run = timed if timed is not None else (lambda name, fn: fn())
    dev, kept = p.device, p._trial.kept
    pred, required = kept['pred'], p.slack.required
    if pred.dtype != torch.float32 or not pred.is_contiguous() or required.dtype != torch.float32 or not required.is_contiguous():
        raise ValueError(f'{who}: the kept predictions and the required times must be contiguous fp32')
    T = pred.numel()
    if cells.span > MAX_SPAN:
        raise ValueError(f'{who}: the rows of design {cells.i} span {cells.span}, at most {MAX_SPAN} are supported on the device '
                         '(cells.critical_host and search_plan remain)')
    if cells.row_lo + cells.span > T or required.numel() != T:
        raise ValueError(f'{who}: the cell set\'s rows [{cells.row_lo}, {cells.row_lo + cells.span}) do not lie within the {T} kept predictions')
    inc_ptr, inc_row = incidence(p)
    N, nnz, C, M = inc_ptr.numel() - 1, inc_row.numel(), cells.C, cells.M
    d_cptr, d_cnode = cells.dev[0], cells.dev[1] if M else None
    d_irow = inc_row if nnz else None
    work = torch.empty(7 * C + 3, dtype=torch.int32, device=dev)          # sel | n_rows | n_pins | worst | three offset tables [C + 1]
    total = torch.empty(3, dtype=torch.int64, device=dev)                 # G, R, MP
    sel, n_rows, n_pins, worst = (work[k * C:(k + 1) * C] for k in range(4))
    offs = [work[4 * C + k * (C + 1):4 * C + (k + 1) * (C + 1)] for k in range(3)]
    run('count', lambda: abi('mmft_cells_count', d_cptr, d_cnode, C, M, inc_ptr, d_irow, N, nnz, pred, required, T, cells.row_lo, cells.span,
                             0 if thr is None else 1, 0.0 if thr is None else thr, sel, n_rows, n_pins, worst.view(torch.float32), *lib.stream_args(work)))

    def scans():
        for k, counts in enumerate((sel, n_rows, n_pins)):
            PR.abi('mmft_pairs_scan', counts, C, offs[k], total[k:k + 1], *lib.stream_args(work))
    run('scan', scans)
    sizes = []
    run('read', lambda: sizes.extend(total.tolist()))                     # 24 bytes: the one size read
    G, R, MP = (int(v) for v in sizes)
    if G == 0:
        return None
    if G > int(max_groups):
        raise ValueError(f'{who}: G = {G} selected cells exceed max_groups = {max_groups}')
    if R >= 2 ** 31 or MP >= 2 ** 31:
        raise ValueError(f'{who}: {R} entries and {MP} pins do not stay below 2^31')
    cuts = np.concatenate([[0], np.cumsum([G + 1, R, R, G + 1, MP, G, G])])
    buf = torch.empty(int(cuts[-1]), dtype=torch.int32, device=dev)
    t = [buf[cuts[j]:cuts[j + 1]] for j in range(7)]
    run('fill', lambda: abi('mmft_cells_fill', d_cptr, d_cnode, C, M, inc_ptr, d_irow, N, nnz, cells.row_lo, cells.span, sel,
                            worst.view(torch.float32), offs[0], offs[1], offs[2], G, R, MP, t[0], t[1] if R else None, t[2] if R else None, t[3],
                            t[4] if MP else None, t[5], t[6], *lib.stream_args(work)))
    return buf, G, R, MP


def check_max_groups(max_groups, who='critical_plan'):
    if isinstance(max_groups, bool) or not isinstance(max_groups, (int, np.integer)) or max_groups < 1:
        raise ValueError(f'{who}: max_groups must be an integer of at least 1, got {max_groups!r}')
    return int(max_groups)


def critical_plan(p, cells, slack_below=0.0, max_groups=1 << 20, who='critical_plan', timed=None):
    """Predictor.critical_plan: see there."""
    check_cells(p, cells, who)
    thr = check_threshold(slack_below, who)
    max_groups = check_max_groups(max_groups, who)
    TR.check_state(p, who, 'the number of selected cells is read on the host per call')
    made = build(p, cells, thr, max_groups, who, timed)
    if made is None:
        return None
    run = timed if timed is not None else (lambda name, fn: fn())
    box = []
    run('decode', lambda: box.append(SE.SearchPlan.from_device(p, cells.i, *made, node_off=cells.node_off, pins_distinct=True)))
    plan, G = box[0], made[1]                                             # (the one copy back brought the cells and their worst too)
    plan.cell, plan.worst = plan.tail[:G].astype(np.int64), plan.tail[G:2 * G].view(np.float32).copy()
    return plan


def refine_cells(p, cells, radius=1, passes=4, slack_below=0.0, patch=True, **kw):
    """Predictor.refine_cells: see there."""
    if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or passes < 1:
        raise ValueError(f'refine_cells: passes must be an integer of at least 1, got {passes!r}')
    if not kw.get('apply', True):
        raise ValueError('refine_cells: every pass applies its moves (apply=False is commit_moves\' alone)')
    check_cells(p, cells, 'refine_cells')
    check_threshold(slack_below, 'refine_cells')
    TR.check_state(p, 'refine_cells', 'every pass reads the number of selected cells on the host')
    out = []
    for _ in range(int(passes)):
        plan = critical_plan(p, cells, slack_below, who='refine_cells')
        if plan is None:                                     # no cell violates: a normal end
            break
        out.append(CM.commit_moves(p, plan, radius, patch=bool(patch), **kw))
        out[-1]['cell'] = plan.cell
        if not patch:
            p.predict()                                      # the truth of the pass, and what the next one reads
        if out[-1]['n_selected'] == 0:
            break
    if patch:
        p.predict()                                          # the static output, report() and criticality() are current again
    return out
