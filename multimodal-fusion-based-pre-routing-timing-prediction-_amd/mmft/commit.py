"""Commit a conflict-free set of best moves on the device (include/mmft_commit.h).

search_moves tells a placer the best displacement of each pin group taken alone.  A pin feeds only the path masks, so a move
changes only the rows whose path holds one of the group's pins - the plan's entries.  Two groups that share no row and no pin
cannot see each other's moves: applied together, each row changes exactly as under its own group's move alone, and the
design's sum of negative-slack quanta changes by exactly the sum of their best_dq.  Predictor.commit_moves runs the search,
selects such a set on the device - the lexicographically first maximal independent set under the key (best_dq, g) - and moves
its pins in place; the next predict() is the truth of the prediction it returns.

    select_host / apply_host          mmft_commit_select and mmft_commit_apply restated in numpy
    check_plan                        the groups of a plan hold distinct pins, or ValueError; decided once per plan
    min_quanta                        min_gain as a threshold in quanta
    prepare / launch / fetch          the three stages of a call, built on those of mmft.search: its launches, then select
                                      and apply on the same stream, everything in ONE buffer and one copy back
    commit_moves / refine_moves       what the Predictor's methods of those names delegate to

patch=True (mmft.refine, include/mmft_refine.h) puts three launches between select and apply that write the selected entries'
rows into the kept head state, so that the next search needs no predict(); refine_moves(resident=True) enqueues all its
passes that way and copies their results back once.

The entry points are bound by `abi`, an accessor of this module: the table of mmft.lib's accessors is pinned by its own ledger
and is not touched here.
"""
import math

import numpy as np
import torch

from . import lib
from . import refine as RF
from . import search as SE

abi = lib.Header('mmft_commit.h')        # a conflict-free set of best moves: its selection, the write of its pins
abi_decls = abi.decls

MAX_T = 1 << 24


def owner_bytes(T):
    """MMFT_COMMIT_OWNER_BYTES of the header: the row-owner table of mmft_commit_select."""
    return 12 * int(T)


# ------------------------------------------------------------------------------------------------ the kernels on the host
def select_host(best_w, best_dq, radius, grow_ptr, grow_row, T, min_q):
    """(sel int32 [G], (selected, sum of their best_dq, candidates)): the candidates - best_w >= 0, not the centre, best_dq <=
    -min_q - visited in the order of the key (best_dq, g); a group is taken iff none of its rows belongs to a group already
    taken.  An entry whose row lies outside [0, T) conflicts with nothing."""
    best_w, best_dq = np.asarray(best_w, dtype=np.int64), np.asarray(best_dq, dtype=np.int64)
    grow_ptr, grow_row = np.asarray(grow_ptr, dtype=np.int64), np.asarray(grow_row, dtype=np.int64)
    if int(min_q) < 1:
        raise ValueError(f'select_host: min_q must be at least 1, got {min_q}')
    G, c = best_w.shape[0], SE.centre(radius)
    SE.offsets(radius)                                       # (its refusal of a radius outside [1, 8])
    cand = np.flatnonzero((best_w >= 0) & (best_w != c) & (best_dq <= -int(min_q)))
    order = cand[np.lexsort((cand, best_dq[cand]))]
    owned = np.zeros(int(T), dtype=bool)
    sel = np.zeros(G, dtype=np.int32)
    for g in order:
        rows = grow_row[grow_ptr[g]:grow_ptr[g + 1]]
        rows = rows[(rows >= 0) & (rows < int(T))]
        if not owned[rows].any():
            owned[rows] = True
            sel[g] = 1
    return sel, (int(sel.sum()), int(best_dq[sel != 0].sum()), int(cand.shape[0]))


def apply_host(loc_x, loc_y, sel, best_w, radius, mv_ptr, mv_node):
    """(loc_x, loc_y) int32 copies with the pins of every group g, sel[g] != 0 and 0 <= best_w[g] < W, moved by the offset of
    best_w[g], saturating (search.moved_coords); a node id outside the arrays is skipped."""
    x, y = np.array(loc_x, dtype=np.int32), np.array(loc_y, dtype=np.int32)
    dx, dy = SE.offsets(radius)
    sel, best_w = np.asarray(sel), np.asarray(best_w, dtype=np.int64)
    mv_ptr, mv_node = np.asarray(mv_ptr, dtype=np.int64), np.asarray(mv_node, dtype=np.int64)
    for g in np.flatnonzero((sel != 0) & (best_w >= 0) & (best_w < dx.shape[0])):
        n = mv_node[mv_ptr[g]:mv_ptr[g + 1]]
        n = n[(n >= 0) & (n < x.shape[0])]
        x[n], y[n] = SE.moved_coords(x[n], dx[best_w[g]]), SE.moved_coords(y[n], dy[best_w[g]])
    return x, y


# ------------------------------------------------------------------------------------------------ host validation
def check_plan(plan):
    """ValueError unless the groups of `plan` hold distinct pins, naming the first pin (in the order of the plan's pins, the
    design's own numbering) that a second group holds.  Two such groups would both move it, and their moves could not be
    scored apart.  Decided once per plan and remembered on it; search_plan and search_moves keep accepting such plans."""
    verdict = getattr(plan, 'pins_distinct', None)
    if verdict is None:
        verdict = True
        node = np.asarray(plan.mv_node, dtype=np.int64)
        _, first, count = np.unique(node, return_index=True, return_counts=True)
        if (count > 1).any():
            grp = np.searchsorted(np.asarray(plan.mv_ptr, dtype=np.int64), np.arange(node.shape[0]), side='right') - 1
            pin = node[first[count > 1].min()]                   # the shared pin that comes first
            at = np.flatnonzero(node == pin)[:2]
            verdict = (f'commit_moves: pin {int(pin) - int(getattr(plan, "node_off", 0))} of design {plan.i} belongs to groups '
                       f'{int(grp[at[0]])} and {int(grp[at[1]])}; groups that are committed together must hold distinct pins')
        plan.pins_distinct = verdict
    if verdict is not True:
        raise ValueError(verdict)


def min_quanta(min_gain, scale_log2=20):
    """max(1, ceil(min_gain * 2^scale_log2)): the smallest improvement, in quanta, that makes a group a candidate.  ValueError
    for a gain that is negative, NaN or infinite, or whose quanta do not fit in 62 bits."""
    if isinstance(min_gain, bool) or not isinstance(min_gain, (int, float, np.integer, np.floating)):
        raise ValueError(f'commit_moves: min_gain must be a number, got {min_gain!r}')
    gain = float(min_gain)
    if not math.isfinite(gain) or gain < 0:
        raise ValueError(f'commit_moves: min_gain must be finite and not negative, got {min_gain!r}')
    try:
        q = max(1, math.ceil(math.ldexp(gain, int(scale_log2))))       # a power of two scales a double exactly
    except OverflowError:
        q = 2 ** 1024
    if q >= 2 ** 62:
        raise ValueError(f'commit_moves: min_gain {min_gain!r} is {q} quanta of 2^-{scale_log2}, which do not fit in 62 bits')
    return q


# ------------------------------------------------------------------------------------------------ the Predictor's side
def prepare(p, plan, radius=1, scale_log2=20, max_rows=65536, min_gain=0.0, apply=True, patch=False):
    """Stage 1, host: search.prepare's refusals under this caller's name, check_plan, min_quanta; the search's buffer with
    room behind its tables for stats [4] int64 and sel [G] int32 - and, patch=True, the two counts of mmft_refine_patch behind
    those.  Returns the call `launch` takes."""
    if patch and not apply:
        raise ValueError('commit_moves: patch=True writes the rows of the moved pins into the kept state; it needs apply=True')
    G = getattr(plan, 'G', 0)
    call = SE.prepare(p, plan, radius, scale_log2, max_rows, who='commit_moves', extra=4 + (G + 1) // 2 + (2 if patch else 0))
    check_plan(plan)
    call['min_q'], call['apply'], call['patch'] = min_quanta(min_gain, scale_log2), bool(apply), bool(patch)
    if patch:
        if not p._trial.kept['pred'].is_contiguous():
            raise ValueError('commit_moves: patch=True writes the kept predictions in place; they are not contiguous')
        call['scratch'] = RF.scratch(p, plan)
    owner = getattr(plan, 'commit_owner', None)              # scratch over the rows, kept with the plan
    T = p._trial.kept['pred'].numel()
    if owner is None or owner.numel() * 8 < owner_bytes(T):
        owner = plan.commit_owner = torch.empty((owner_bytes(T) + 7) // 8, dtype=torch.int64, device=p.device)
    call['owner'] = owner
    return call


def _tail(raw, tail, G):
    """stats [4] int64 and sel [G] int32 behind the search's tables (torch tensor or numpy array alike)."""
    return raw[tail:tail + 4], raw[tail + 4:].view(torch.int32 if torch.is_tensor(raw) else np.int32)[:G]


def _patch_stats(raw, tail, G):
    """The counts [2] int64 of mmft_refine_patch behind sel, in the buffer of a patch=True call."""
    at = tail + 4 + (G + 1) // 2
    return raw[at:at + 2]


def launch(p, call, timed=None):
    """Stage 2, device, on the current stream: search.launch, then mmft_commit_select on its best_w / best_dq and - apply=True -
    mmft_commit_apply on the resident pins, after which the trial state is stale as after update().  patch=True: refine.launch
    (rows, head, patch) between the two - the rows kernel reads the pins before apply moves them - and the trial state
    stays fresh.  Returns the call.  `timed`: a callable that is handed each part as a function (tools/bench_placement.py
    times them apart)."""
    run = timed if timed is not None else (lambda name, fn: fn())
    run('search', lambda: SE.launch(p, call))
    plan, placed = call['plan'], p._placed
    G, W = plan.G, call['W']
    v = SE._views(call['raw'], G, W, call['n64'])
    stats, sel = _tail(call['raw'], call['tail'], G)
    d_gptr, d_grow, _, d_mptr, d_node = plan.dev
    T = p._trial.kept['pred'].numel()
    run('select', lambda: abi('mmft_commit_select', v['best_w'], v['best_dq'], G, call['radius'], d_gptr, d_grow if plan.R else None, plan.R,
                              T, call['min_q'], sel, stats, call['owner'], *lib.stream_args(sel)))
    if call['patch']:
        RF.launch(p, call, sel, v['best_w'], _patch_stats(call['raw'], call['tail'], G), run)
    if call['apply']:
        p._trial.stale = not call['patch']                   # unpatched: until the next predict(), exactly as update() leaves it
        run('apply', lambda: abi('mmft_commit_apply', placed.loc_x, placed.loc_y, placed.loc_x.numel(), sel, v['best_w'], call['radius'],
                                 d_mptr, d_node if plan.M else None, G, plan.M, *lib.stream_args(sel)))
    return call


def fetch(call):
    """Stage 3: search.fetch's ONE device -> host copy, which holds the selection too.  The result of commit_moves."""
    res = SE.fetch(call)
    stats, sel = _tail(call['host'], call['tail'], call['plan'].G)
    sum_dq = int(stats[1])
    res.update(selected=sel != 0, n_selected=int(stats[0]), n_candidates=int(stats[2]), rounds=int(stats[3]), sum_dq=sum_dq,
               gain=float(-sum_dq) * 2.0 ** -call['scale_log2'], predicted_nsum=res['base']['nsum'] + sum_dq)
    if call['patch']:
        res['n_patched'] = int(_patch_stats(call['host'], call['tail'], call['plan'].G)[0])
    return res


def commit_moves(p, plan, radius=1, scale_log2=20, max_rows=65536, min_gain=0.0, apply=True, patch=False):
    """Predictor.commit_moves: see there."""
    return fetch(launch(p, prepare(p, plan, radius, scale_log2, max_rows, min_gain, apply, patch)))


def _refine_resident(p, plan, radius, passes, **kw):
    """refine_moves(resident=True): host validation once, `passes` patched commits enqueued back to back - each with a result
    buffer of its own, a row of ONE tensor -, one copy back, the list cut after the first pass that selected nothing, and
    the predict() the call leaves behind."""
    first = prepare(p, plan, radius, patch=True, **kw)
    raws = torch.empty((passes, first.pop('raw').numel()), dtype=torch.int64, device=p.device)       # (its own buffer: only its size)
    calls = [launch(p, dict(first, raw=raws[k])) for k in range(passes)]
    host = raws.cpu()                                        # the one synchronisation
    out = []
    for k, call in enumerate(calls):
        call['raw'] = host[k]                                # (search.fetch's copy is none: the row is on the host already)
        out.append(fetch(call))
        if out[-1]['n_selected'] == 0:                       # the later passes found the same state and did the same: nothing
            break
    p.predict()
    return out


def refine_moves(p, plan, radius=1, passes=4, resident=False, **kw):
    """Predictor.refine_moves: see there."""
    if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or passes < 1:
        raise ValueError(f'refine_moves: passes must be an integer of at least 1, got {passes!r}')
    if not kw.get('apply', True):
        raise ValueError('refine_moves: every pass applies its moves (apply=False is commit_moves\' alone)')
    if resident:
        if 'patch' in kw:
            raise ValueError('refine_moves: resident=True patches every pass; patch= is not its caller\'s to set')
        return _refine_resident(p, plan, radius, int(passes), **kw)
    out = []
    for _ in range(int(passes)):
        out.append(commit_moves(p, plan, radius, **kw))
        p.predict()                                          # the truth of the pass, and what the next one reads
        if out[-1]['n_selected'] == 0:
            break
    return out
