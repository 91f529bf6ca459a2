"""Exact window search of pin-group moves on the device (include/mmft_search.h).

For a group of pins that move rigidly together - a cell - a placer asks which displacement within a small window is best, and
by how much.  Predictor(placement=True, trials=True).search_plan builds, once, the static tables of a set of groups (the rows
each group can change, from the incidence trial.TrialState keeps); search_moves enumerates the window on the device, scores
every (group, offset) candidate by the change of the quanta on its affected rows only, and returns the whole score table and
the best offset per group - without writing the placement, h or anything predict() returns.

    offsets / centre / moved_coords   the window: offset w -> (dx, dy), the zero move, the saturating add
    check_groups / check_call         host validation of search_plan's and search_moves' arguments
    plan_tables                       the tables of a plan from the incidence, through trial.expand_candidates
    tables_host / score_host          mmft_search_score, and with it mmft_search_best, restated in numpy
    prepare / launch / fetch          the three stages of a call (refusals and buffers, the launches, one copy back);
                                      search_moves runs them one after another, tools/bench_placement.py times them apart

The entry points are bound by `abi`, an accessor of this module: the table of mmft.lib's accessors is pinned by its own ledger
and is not touched here.
"""
import numpy as np
import torch

from . import lib
from . import trial as TR
from .criticality import reference_quanta
from .report import reference_slack

abi = lib.Header('mmft_search.h')        # window search: rows under a group's offset, per-candidate scores, the best offset
abi_decls = abi.decls

MAX_RADIUS = 8
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
TABLES = ('dq', 'dviol', 'new_nan', 'capped', 'worst', 'worst_row')


# ------------------------------------------------------------------------------------------------ the window
def centre(radius):
    """The offset of the zero move."""
    return 2 * int(radius) * (int(radius) + 1)


def offsets(radius):
    """(dx int32 [W], dy int32 [W]), W = (2 r + 1)^2: offset w stands for (w // (2 r + 1) - r, w % (2 r + 1) - r); x is the
    first map axis."""
    r = int(radius)
    if not 1 <= r <= MAX_RADIUS:
        raise ValueError(f'search_moves: radius must lie in [1, {MAX_RADIUS}], got {radius}')
    w = np.arange((2 * r + 1) ** 2, dtype=np.int64)
    return (w // (2 * r + 1) - r).astype(np.int32), (w % (2 * r + 1) - r).astype(np.int32)


def moved_coords(loc, d):
    """int32 sat32(loc + d): the sum formed in 64 bits, saturated to int32 - where a pin at `loc` sits under an offset d."""
    v = np.asarray(loc).astype(np.int64) + np.asarray(d).astype(np.int64)
    return np.clip(v, I32_MIN, I32_MAX).astype(np.int32)


# ------------------------------------------------------------------------------------------------ host validation
def check_groups(n_nodes, pins, group_ptr=None):
    """(pins int64 [M], group_ptr int64 [G + 1]) or an exception: trial.check_moves' validation with the coordinates left out -
    TypeError for a wrong type or dtype, IndexError for a pin outside [0, n_nodes), ValueError for shapes, a group_ptr that does
    not start at 0 / decreases / does not end at M, a group of more than trial.MAX_MOVES pins, a pin twice in one group."""
    return TR.check_pin_sets(n_nodes, pins, group_ptr, who='search_plan', ptr_name='group_ptr', unit='group', item='pins')


def check_call(R, radius=1, scale_log2=20, max_rows=65536, who='search_moves'):
    """(W, Wc) of a search_moves call over a plan of R entries - the offsets of the window and of one chunk - or ValueError: a
    radius outside [1, 8], a scale_log2 outside [0, 30], max_rows < 1, R * W >= 2^31.  `who`: the caller the messages name."""
    for name, v in (('radius', radius), ('scale_log2', scale_log2), ('max_rows', max_rows)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f'{who}: {name} must be an integer, got {v!r}')
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f'{who}: radius must lie in [1, {MAX_RADIUS}], got {radius}')
    if not 0 <= scale_log2 <= 30:
        raise ValueError(f'{who}: scale_log2 must lie in [0, 30], got {scale_log2}')
    if max_rows < 1:
        raise ValueError(f'{who}: max_rows must be at least 1, got {max_rows}')
    W = (2 * int(radius) + 1) ** 2
    if int(R) * W >= 2 ** 31:
        raise ValueError(f'{who}: {R} entries times {W} offsets do not stay below 2^31')
    return W, min(W, max(1, int(max_rows) // max(int(R), 1)))


# ------------------------------------------------------------------------------------------------ the plan
def plan_tables(rows_of_pin, node_off, pins, group_ptr):
    """(grow_ptr int64 [G + 1], grow_row int64 [R], grow_grp int64 [R], mv_ptr int64 [G + 1], mv_node int64 [M]): per group the
    ascending union of its pins' rows, the group of each entry, and the groups' pins in the tables' numbering -
    trial.expand_candidates with the groups as candidates."""
    grow_ptr, grow_row, grow_grp = TR.expand_candidates(rows_of_pin, node_off, pins, group_ptr)
    return grow_ptr, grow_row, grow_grp, np.asarray(group_ptr, dtype=np.int64), np.asarray(pins, dtype=np.int64) + int(node_off)


class SearchPlan:
    """What search_plan returns: design i's groups as host tables and, in ONE int32 buffer on the device, grow_ptr, grow_row,
    grow_grp, mv_ptr, mv_node.  Valid for the life of its Predictor: the incidence is static, and pin moves do not change it."""

    def __init__(self, owner, i, tables, device, node_off=0):
        self.owner, self.i, self.node_off = owner, int(i), int(node_off)
        self.pins_distinct = None                            # commit.check_plan's verdict, made once: None, True or its message
        self.grow_ptr, self.grow_row, self.grow_grp, self.mv_ptr, self.mv_node = tables
        self.G, self.R, self.M = self.mv_ptr.shape[0] - 1, self.grow_row.shape[0], self.mv_node.shape[0]
        sizes = [a.shape[0] for a in tables]
        self.ints = torch.from_numpy(np.concatenate([a.astype(np.int32) for a in tables])).to(device)
        cuts = np.concatenate([[0], np.cumsum(sizes)])
        self.dev = [self.ints[cuts[j]:cuts[j + 1]] for j in range(len(tables))]

    @classmethod
    def from_device(cls, owner, i, buf, G, R, M, node_off=0, pins_distinct=None):
        """The plan of tables that were built on the device (mmft.cells): `buf` is an int32 buffer that starts with the five
        tables in the layout above and may hold more words behind them.  The host tables are decoded from ONE copy of it;
        `ints` and `dev` are views of it, and `tail` holds the words behind the tables as that copy brought them (int32)."""
        self = cls.__new__(cls)
        self.owner, self.i, self.node_off, self.pins_distinct = owner, int(i), int(node_off), pins_distinct
        self.G, self.R, self.M = int(G), int(R), int(M)
        cuts = np.concatenate([[0], np.cumsum([self.G + 1, self.R, self.R, self.G + 1, self.M])])
        assert buf.dtype == torch.int32 and buf.dim() == 1 and buf.numel() >= cuts[-1]
        self.ints = buf[:cuts[-1]]
        self.dev = [buf[cuts[j]:cuts[j + 1]] for j in range(5)]
        words = buf.cpu().numpy()
        host = words[:cuts[-1]].astype(np.int64)
        self.grow_ptr, self.grow_row, self.grow_grp, self.mv_ptr, self.mv_node = [host[cuts[j]:cuts[j + 1]] for j in range(5)]
        self.tail = words[cuts[-1]:]
        return self


def search_plan(p, i, pins, group_ptr=None):
    """Predictor.search_plan: see there."""
    st = getattr(p, '_trial', None)
    if st is None:
        raise RuntimeError('Predictor.search_plan(): built without trials=True')
    p._check_design(i, 'search_plan')
    if p.slack.rows_of(i).numel() == 0:
        raise ValueError(f'search_plan: design {i} has no selected path')
    placed = p._placed
    off = int(placed.node_off[i])
    pins, group_ptr = check_groups(int(placed.node_off[i + 1]) - off, pins, group_ptr)
    if group_ptr.shape[0] < 2:
        raise ValueError('search_plan: no group')
    return SearchPlan(p, i, plan_tables(st.rows_of_pin, off, pins, group_ptr), p.device, node_off=off)


# ------------------------------------------------------------------------------------------------ the scores on the host
def _ordered_bits(s):
    """slack_key.h: the unsigned order of the result is the numeric order of the fp32 values."""
    u = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def best_host(dq, new_nan, radius, scale_log2=20):
    """best_w, best_dx, best_dy (int32 [G]), best_dq (int64 [G]), best_gain (float64 [G]): per group the eligible offset
    (new_nan == 0) with the smallest key (dq, |dx| + |dy|, w); no eligible offset: -1, and zeros."""
    dx, dy = offsets(radius)
    man = np.abs(dx.astype(np.int64)) + np.abs(dy.astype(np.int64))
    G = dq.shape[0]
    best_w, best_dq = np.full(G, -1, dtype=np.int32), np.zeros(G, dtype=np.int64)
    for g in range(G):
        ok = np.flatnonzero(new_nan[g] == 0)
        if ok.size:
            w = ok[np.lexsort((ok, man[ok], dq[g, ok]))[0]]
            best_w[g], best_dq[g] = w, dq[g, w]
    found = best_w >= 0
    at = np.where(found, best_w, 0)
    return dict(best_w=best_w, best_dx=np.where(found, dx[at], 0).astype(np.int32), best_dy=np.where(found, dy[at], 0).astype(np.int32),
                best_dq=best_dq, best_gain=(-best_dq).astype(np.float64) * 2.0 ** -int(scale_log2))


def tables_host(pred_base, required, grow_ptr, grow_row, pred_trial, scale_log2=20):
    """The six tables [G, W] of mmft_search_score from host arrays, in numpy: pred_trial fp32 [W, R] - row grow_row[e] under
    candidate w of its group -, the slack rule of mmft_report.h (reference_slack), THE QUANTUM (reference_quanta), the smallest
    row on equal worst slack.  An entry whose row lies outside pred_base takes part in nothing.  mmft.swap scores its pairs
    with it too (W == 1, a pair's entries as a group's): the definitions are stated once."""
    pred_base, required = np.asarray(pred_base, dtype=np.float32), np.asarray(required, dtype=np.float32)
    grow_ptr, grow_row = np.asarray(grow_ptr, dtype=np.int64), np.asarray(grow_row, dtype=np.int64)
    G, R, T = grow_ptr.shape[0] - 1, grow_row.shape[0], pred_base.shape[0]
    pred_trial = np.asarray(pred_trial, dtype=np.float32)
    pred_trial = pred_trial if pred_trial.ndim == 2 else pred_trial.reshape(1, R)       # [R]: one candidate per group
    W = pred_trial.shape[0]
    inside = (grow_row >= 0) & (grow_row < T)
    safe = np.where(inside, grow_row, 0)
    sb = reference_slack(pred_base[safe], required[safe])                   # [R]
    st = reference_slack(pred_trial, required[safe][None, :])               # [W, R]
    qb, cb = reference_quanta(sb, scale_log2)
    qt, ct = reference_quanta(st.reshape(-1), scale_log2)
    qt, ct = qt.reshape(W, R), ct.reshape(W, R)
    with np.errstate(invalid='ignore'):
        terms = dict(dq=np.where(inside, qt - qb[None, :], 0).astype(np.int64),
                     dviol=np.where(inside, (st < 0).astype(np.int64) - (sb < 0).astype(np.int64)[None, :], 0),
                     new_nan=(inside & np.isnan(st) & ~np.isnan(sb)[None, :]).astype(np.int64),
                     capped=(inside & (ct | cb[None, :])).astype(np.int64))
    out = {}
    for name, v in terms.items():                                           # per group: a difference of prefix sums, exact
        run = np.concatenate([np.zeros((W, 1), dtype=np.int64), np.cumsum(v, axis=1)], axis=1)
        out[name] = (run[:, grow_ptr[1:]] - run[:, grow_ptr[:-1]]).T.astype(np.int64 if name == 'dq' else np.int32)
    key = (_ordered_bits(st).astype(np.uint64) << np.uint64(32)) | (safe.astype(np.uint64) & np.uint64(0xffffffff))[None, :]
    key = np.where(inside & ~np.isnan(st), key, np.uint64(2 ** 64 - 1))
    worst, worst_row = np.full((G, W), np.nan, dtype=np.float32), np.full((G, W), -1, dtype=np.int32)
    for g in range(G):
        a, b = int(grow_ptr[g]), int(grow_ptr[g + 1])
        if b > a:
            at = a + np.argmin(key[:, a:b], axis=1)
            found = key[np.arange(W), at] != np.uint64(2 ** 64 - 1)
            worst[g] = np.where(found, st[np.arange(W), at], np.float32(np.nan))
            worst_row[g] = np.where(found, grow_row[at], -1)
    out['worst'], out['worst_row'] = worst, worst_row
    return out


def score_host(pred_base, required, grow_ptr, grow_row, pred_trial, radius, scale_log2=20):
    """Every table of mmft_search_score and the best of mmft_search_best from host arrays, in numpy: pred_trial fp32 [W, R] - row
    grow_row[e] under offset w -, the slack rule of mmft_report.h (reference_slack), THE QUANTUM (reference_quanta), the
    smallest row on equal worst slack.  An entry whose row lies outside pred_base takes part in nothing."""
    W, R = offsets(radius)[0].shape[0], np.asarray(grow_row).shape[0]
    out = tables_host(pred_base, required, grow_ptr, grow_row, np.asarray(pred_trial, dtype=np.float32).reshape(W, R), scale_log2)
    out.update(best_host(out['dq'], out['new_nan'], radius, scale_log2))
    return out


def base_host(pred_base, required, design_rows, scale_log2=20):
    """dict(nsum, violations, n_nan) of a design's rows on the pins as they are: the sum of the rows' quanta, the rows that
    violate, the NaN rows (a row outside pred_base counts like one)."""
    pred_base, required = np.asarray(pred_base, dtype=np.float32), np.asarray(required, dtype=np.float32)
    rows = np.asarray(design_rows, dtype=np.int64)
    inside = (rows >= 0) & (rows < pred_base.shape[0])
    safe = np.where(inside, rows, 0)
    s = np.where(inside, reference_slack(pred_base[safe], required[safe]), np.float32(np.nan)).astype(np.float32)
    q, _ = reference_quanta(s, scale_log2)
    with np.errstate(invalid='ignore'):
        return dict(nsum=int(q.sum()), violations=int((s < 0).sum()), n_nan=int(np.isnan(s).sum()))


# ------------------------------------------------------------------------------------------------ the Predictor's side
def prepare(p, plan, radius=1, scale_log2=20, max_rows=65536, who='search_moves', extra=0):
    """Stage 1, host: state and mode refusals, validation, the call's output buffer.  No host table is built and nothing is
    uploaded: the plan holds the tables.  Returns the call `launch` takes.  `who`: the caller the messages name; `extra`:
    int64 words behind the tables in the same buffer, for a caller that returns more in the same copy (mmft.commit)."""
    TR.check_state(p, who, 'the chunks of the window are launched from the host per call')
    if not isinstance(plan, SearchPlan):
        raise TypeError(f'{who}: plan must come from search_plan(), got {type(plan).__name__}')
    if plan.owner is not p:
        raise ValueError(f'{who}: the plan belongs to another Predictor')
    W, Wc = check_call(plan.R, radius, scale_log2, max_rows, who)
    G = plan.G
    # ONE buffer for everything that goes back: int64 [dq G W | best_dq G | base 3], then int32 [5 tables G W | best_w G]
    n64, n32 = G * W + G + 3, 5 * G * W + G
    raw = torch.empty(n64 + (n32 + 1) // 2 + int(extra), dtype=torch.int64, device=p.device)
    return dict(plan=plan, radius=int(radius), scale_log2=int(scale_log2), W=W, Wc=Wc, raw=raw, n64=n64, tail=n64 + (n32 + 1) // 2)


def _views(raw, G, W, n64):
    """The tables inside the call's buffer (torch tensor or numpy array alike)."""
    i64, i32 = raw[:n64], raw[n64:].view(torch.int32 if torch.is_tensor(raw) else np.int32)
    f32 = torch.float32 if torch.is_tensor(raw) else np.float32
    GW = G * W
    return dict(dq=i64[:GW], best_dq=i64[GW:GW + G], base=i64[GW + G:GW + G + 3], dviol=i32[:GW], new_nan=i32[GW:2 * GW],
                capped=i32[2 * GW:3 * GW], worst=i32[3 * GW:4 * GW].view(f32), worst_row=i32[4 * GW:5 * GW], best_w=i32[5 * GW:5 * GW + G])


def launch(p, call):
    """Stage 2, device, on the current stream: per chunk of Wc offsets mmft_search_rows over its slots, mmft_head_mlp_fwd over
    their rows and mmft_search_score; mmft_search_best (with the base figures) once at the end.  Writes buffers of its own
    only.  Returns the call."""
    plan, placed, b, kept = call['plan'], p._placed, p.batch, p._trial.kept
    x, GP, pred = kept['x'], kept['GP'], kept['pred']
    d_gptr, d_grow, d_ggrp, d_mptr, d_node = plan.dev
    fcn, mods = p.pmodel.fcn, list(p.pmodel.mlp_fuse.layers)
    width, Dout, T = x.shape[1], fcn.weight.shape[0], pred.numel()
    G, R, W, Wc, radius, scale = plan.G, plan.R, call['W'], call['Wc'], call['radius'], call['scale_log2']
    v = _views(call['raw'], G, W, call['n64'])
    xt = torch.empty((Wc * R, width), dtype=torch.float32, device=p.device) if R else None
    pred_t = torch.empty(Wc * R, dtype=torch.float32, device=p.device) if R else None
    for w0 in range(0, W, Wc):
        w1 = min(W, w0 + Wc)
        if R:
            abi('mmft_search_rows', placed.nodes, placed.lens, placed.maxlen, placed.loc_x, placed.loc_y, placed.map_x, placed.map_y,
                p._sel.paths, p._sel.feat_off if b.B > 1 else None, T, d_grow, d_ggrp, R, d_mptr, d_node, G, radius, w0, w1,
                GP, fcn.bias, x, x.stride(0), xt, width, width, kept['cnn_col'], Dout, b.masks.run_block, *lib.stream_args(x))
            lib.head('mmft_head_mlp_fwd', xt, width, mods[0].weight, mods[0].bias, mods[2].weight, mods[2].bias, None, pred_t,
                     (w1 - w0) * R, mods[0].weight.shape[1], mods[0].weight.shape[0], 1, *lib.stream_args(x))
        abi('mmft_search_score', pred_t, pred.reshape(-1), p.slack.required, T, d_gptr, d_grow if R else None, G, R, radius, w0, w1,
            scale, v['dq'], v['dviol'], v['new_nan'], v['capped'], v['worst'], v['worst_row'], *lib.stream_args(x))
    rows = p.slack.rows_of(plan.i)
    abi('mmft_search_best', v['dq'], v['new_nan'], G, radius, v['best_w'], v['best_dq'], pred.reshape(-1), p.slack.required, rows,
        rows.numel(), T, scale, v['base'], *lib.stream_args(x))
    call['xt'] = xt
    return call


def fetch(call):
    """Stage 3: ONE device -> host copy (kept as call['host']), decoded.  The result of search_moves."""
    plan, W, radius = call['plan'], call['W'], call['radius']
    G = plan.G
    host = call['host'] = call['raw'].cpu().numpy()
    v = _views(host, G, W, call['n64'])
    res = {k: v[k].reshape(G, W).copy() for k in TABLES}
    dx, dy = offsets(radius)
    best_w, best_dq = v['best_w'].copy(), v['best_dq'].copy()
    at = np.where(best_w >= 0, best_w, centre(radius))
    res.update(best_w=best_w, best_dx=dx[at].copy(), best_dy=dy[at].copy(), best_dq=best_dq,
               best_gain=(-best_dq).astype(np.float64) * 2.0 ** -call['scale_log2'])
    res['base'] = dict(nsum=int(v['base'][0]), violations=int(v['base'][1]), n_nan=int(v['base'][2]))
    res['grow_ptr'], res['rows'] = plan.grow_ptr, plan.grow_row
    return res


def search_moves(p, plan, radius=1, scale_log2=20, max_rows=65536):
    """Predictor.search_moves: see there."""
    return fetch(launch(p, prepare(p, plan, radius, scale_log2, max_rows)))
