"""Exact search and commit of cell swaps on the device (include/mmft_swap.h).

A detailed placer that works on a legal placement can rarely use a displacement as it stands - the target site is occupied -;
its basic legal move is the swap: two cells exchange positions.  Predictor.swap_plan pairs the groups of a search plan, once;
swap_moves scores every swap, each taken alone, on its affected rows only, with the anchors read on the device at call
time; commit_swaps selects a conflict-free set - mmft_commit_select as it stands, over a table in which a pair's groups
count as rows - and writes its pins in place.

    check_pairs                       host validation of (pair_a, pair_b) against a plan's groups
    swapped_coords                    the rule: where the pins of both groups of each pair sit under its swap
    pair_tables                       prow_ptr, prow_row, prow_pair and the select table, from the plan's grow_*
    score_host / best_pair_host       mmft_swap_score restated in numpy (search.tables_host), the best pair per group
    select_host / apply_host          the selection (commit.select_host on the select table), mmft_swap_apply in numpy
    prepare / launch / fetch          the three stages of a call, staged like mmft.search: ONE result buffer, ONE copy back
    swap_plan / swap_moves / commit_swaps   what the Predictor's methods of those names delegate to

The entry points are bound by `abi`, an accessor of this module: the table of mmft.lib's accessors is pinned by its own ledger
and is not touched here.
"""
import numpy as np
import torch

from . import commit as CM
from . import lib
from . import refine as RF
from . import search as SE
from . import trial as TR

abi = lib.Header('mmft_swap.h')          # cell swaps: rows under a pair's swap, per-pair scores, the write of a selected set
abi_decls = abi.decls

MAX_PINS = TR.MAX_MOVES                  # pins of both groups of a pair together (the kernel stages them in LDS)
MAX_T = CM.MAX_T
TABLES = SE.TABLES


# ------------------------------------------------------------------------------------------------ host validation
def check_pairs(mv_ptr, pair_a, pair_b, who='swap_plan'):
    """(pair_a int64 [K], pair_b int64 [K]) or an exception; host only.  ValueError unless both are numpy arrays or tensors of
    int64, 1-D, of one length K >= 1; IndexError for a group id outside [0, G); ValueError for a pair of one group with
    itself, a pair with an empty group and a pair whose groups hold more than MAX_PINS pins together.  The same pair twice,
    or (a, b) beside (b, a), is allowed: they conflict."""
    mv_ptr = np.asarray(mv_ptr, dtype=np.int64)
    G = mv_ptr.shape[0] - 1
    out = []
    for name, v in (('pair_a', pair_a), ('pair_b', pair_b)):
        h = v.detach().cpu().numpy() if torch.is_tensor(v) else v
        if not isinstance(h, np.ndarray) or h.dtype != np.int64:
            raise ValueError(f'{who}: {name} must be a numpy array or tensor of int64, got {getattr(h, "dtype", type(v).__name__)}')
        if h.ndim != 1:
            raise ValueError(f'{who}: {name} must be 1-D, got shape {h.shape}')
        out.append(np.ascontiguousarray(h))
    a, b = out
    if a.shape != b.shape or a.shape[0] < 1:
        raise ValueError(f'{who}: pair_a and pair_b must hold the same number of pairs, at least one (got {a.shape[0]} and {b.shape[0]})')
    for name, v in (('pair_a', a), ('pair_b', b)):
        if int(v.min()) < 0 or int(v.max()) >= G:
            raise IndexError(f'{who}: {name} names a group outside the plan\'s {G}')
    if (a == b).any():
        k = int(np.flatnonzero(a == b)[0])
        raise ValueError(f'{who}: pair {k} swaps group {int(a[k])} with itself')
    size = np.diff(mv_ptr)
    empty = (size[a] == 0) | (size[b] == 0)
    if empty.any():
        k = int(np.flatnonzero(empty)[0])
        raise ValueError(f'{who}: pair {k} holds an empty group (a group\'s first pin is its anchor)')
    both = size[a] + size[b]
    if int(both.max()) > MAX_PINS:
        k = int(np.argmax(both))
        raise ValueError(f'{who}: the groups of pair {k} hold {int(size[a[k]])} + {int(size[b[k]])} pins, at most {MAX_PINS} together '
                         'are supported')
    return a, b


# ------------------------------------------------------------------------------------------------ the rule and the tables
def _ranges(ptr, idx):
    """The ranges ptr[i] .. ptr[i + 1] for i in idx, one after another: (flat positions, the position in idx of each)."""
    start, count = ptr[idx], ptr[idx + 1] - ptr[idx]
    first = np.cumsum(count) - count
    flat = np.arange(int(count.sum()), dtype=np.int64) - np.repeat(first - start, count)
    return flat, np.repeat(np.arange(idx.shape[0], dtype=np.int64), count)


def swapped_coords(loc_x, loc_y, mv_ptr, mv_node, pair_a, pair_b):
    """(cand_ptr int64 [K + 1], node int64, x int32, y int32): per pair the pins of group a, then those of group b, and where
    they sit under the swap.  With A and B the groups' anchors (their first pins), a pin n of a sits at
    sat32(loc[n] + (loc[B] - loc[A])) and a pin of b at sat32(loc[n] + (loc[A] - loc[B])), per axis; difference and sum in 64
    bits, saturated once (search.moved_coords).  Node ids as mv_node has them."""
    mv_ptr, mv_node = np.asarray(mv_ptr, dtype=np.int64), np.asarray(mv_node, dtype=np.int64)
    a, b = np.asarray(pair_a, dtype=np.int64), np.asarray(pair_b, dtype=np.int64)
    K = a.shape[0]
    both = np.stack([a, b], axis=1).reshape(-1)                            # a0, b0, a1, b1, ...
    flat, half = _ranges(mv_ptr, both)
    node = mv_node[flat]
    A, B = mv_node[mv_ptr[a]], mv_node[mv_ptr[b]]
    out = []
    for loc in (loc_x, loc_y):
        loc = np.asarray(loc).astype(np.int64)
        d = loc[B] - loc[A]                                                # [K], exact in 64 bits
        out.append(SE.moved_coords(loc[node], np.where(half % 2 == 0, d[half // 2], -d[half // 2])))
    size = np.diff(mv_ptr)
    cand_ptr = np.concatenate([[0], np.cumsum(size[a] + size[b])]).astype(np.int64)
    assert cand_ptr.shape[0] == K + 1
    return cand_ptr, node, out[0], out[1]


def pair_tables(grow_ptr, grow_row, pair_a, pair_b, T, G=None):
    """(prow_ptr int64 [K + 1], prow_row int64 [RP], prow_pair int64 [RP], sel_ptr int64 [K + 1], sel_row int64 [RP + 2 K]): per
    pair the ascending union, each row once, of the plan's rows of its two groups, the pair of each entry - and THE SELECT
    TABLE, per pair its entries' rows followed by the two pseudo-rows T + pair_a[k] and T + pair_b[k]: over T + G rows, two
    pairs share a row of it iff they share a row or a group."""
    grow_ptr, grow_row = np.asarray(grow_ptr, dtype=np.int64), np.asarray(grow_row, dtype=np.int64)
    a, b = np.asarray(pair_a, dtype=np.int64), np.asarray(pair_b, dtype=np.int64)
    K = a.shape[0]
    fa, ka = _ranges(grow_ptr, a)
    fb, kb = _ranges(grow_ptr, b)
    span = max(int(T), int(grow_row.max()) + 1 if grow_row.size else 1)
    key = np.unique(np.concatenate([ka, kb]) * span + grow_row[np.concatenate([fa, fb])])      # by pair, then by row; a shared row once
    prow_pair, prow_row = key // span, key % span
    prow_ptr = np.zeros(K + 1, dtype=np.int64)
    np.cumsum(np.bincount(prow_pair, minlength=K), out=prow_ptr[1:])
    sel_ptr = prow_ptr + 2 * np.arange(K + 1, dtype=np.int64)
    sel_row = np.empty(key.shape[0] + 2 * K, dtype=np.int64)
    sel_row[np.arange(key.shape[0], dtype=np.int64) + 2 * prow_pair] = prow_row
    sel_row[sel_ptr[1:] - 2], sel_row[sel_ptr[1:] - 1] = int(T) + a, int(T) + b
    return prow_ptr, prow_row, prow_pair, sel_ptr, sel_row


# ------------------------------------------------------------------------------------------------ the kernels on the host
def score_host(pred_base, required, prow_ptr, prow_row, pred_trial, scale_log2=20):
    """mmft_swap_score from host arrays: the six tables [K] of search.tables_host with a pair's entries in the place of a
    group's (pred_trial fp32 [RP], entry e's row under its pair's swap), pick int32 [K] (0 eligible, -1 not), eligible bool
    [K] and gain float64 [K] = -dq * 2^-scale_log2."""
    out = {k: v[:, 0].copy() for k, v in SE.tables_host(pred_base, required, prow_ptr, prow_row,
                                                        np.asarray(pred_trial, dtype=np.float32).reshape(1, -1), scale_log2).items()}
    out['eligible'] = out['new_nan'] == 0
    out['pick'] = np.where(out['eligible'], 0, -1).astype(np.int32)
    out['gain'] = (-out['dq']).astype(np.float64) * 2.0 ** -int(scale_log2)
    return out


def best_pair_host(dq, eligible, pair_a, pair_b, G):
    """(best_pair int64 [G], best_pair_dq int64 [G]): per group the eligible pair that holds it with the smallest key (dq, k),
    and its dq; no such pair: -1 and 0."""
    dq, a, b = np.asarray(dq, dtype=np.int64), np.asarray(pair_a, dtype=np.int64), np.asarray(pair_b, dtype=np.int64)
    ks = np.flatnonzero(np.asarray(eligible, dtype=bool))
    K = dq.shape[0]
    if ks.size and int(np.abs(dq[ks]).max()) < 2 ** 62 // K:                 # the key (dq, k) as one int64: a plain sort
        ks = np.sort(dq[ks] * K + ks)[::-1] % K
    else:
        ks = ks[np.argsort(dq[ks], kind='stable')][::-1]
    best = np.full(int(G), -1, dtype=np.int64)               # descending keys: of the writes to one group the last one stays
    best[np.stack([a[ks], b[ks]], axis=1).reshape(-1)] = np.repeat(ks, 2)
    return best, np.where(best >= 0, dq[np.maximum(best, 0)], 0).astype(np.int64)


def select_host(pick, dq, sel_ptr, sel_row, T, G, min_q=1):
    """commit.select_host with the pairs as its groups, as mmft_swap.h maps it: best_w = pick at radius 1, best_dq = dq, the
    select table over T + G rows."""
    return CM.select_host(pick, dq, 1, sel_ptr, sel_row, int(T) + int(G), min_q)


def apply_host(loc_x, loc_y, sel, pick, pair_a, pair_b, mv_ptr, mv_node):
    """(loc_x, loc_y) int32 copies with the pins of both groups of every pair k, sel[k] != 0 and pick[k] == 0, at their swapped
    coordinates.  The selected pairs share no group, so each is written from the coordinates the call found.  As the
    kernel: a pair of a group with itself, with an empty group or with an anchor outside the arrays is skipped whole, a node
    id outside them is skipped."""
    x, y = np.array(loc_x, dtype=np.int32), np.array(loc_y, dtype=np.int32)
    mv_ptr, mv_node = np.asarray(mv_ptr, dtype=np.int64), np.asarray(mv_node, dtype=np.int64)
    a, b = np.asarray(pair_a, dtype=np.int64), np.asarray(pair_b, dtype=np.int64)
    n = x.shape[0]
    for k in np.flatnonzero((np.asarray(sel) != 0) & (np.asarray(pick) == 0)):
        na, nb = mv_node[mv_ptr[a[k]]:mv_ptr[a[k] + 1]], mv_node[mv_ptr[b[k]]:mv_ptr[b[k] + 1]]
        if a[k] == b[k] or not na.size or not nb.size or not (0 <= na[0] < n and 0 <= nb[0] < n):
            continue
        for was, now in ((np.asarray(loc_x), x), (np.asarray(loc_y), y)):
            d = int(was[nb[0]]) - int(was[na[0]])
            for nodes, by in ((na, d), (nb, -d)):
                nodes = nodes[(nodes >= 0) & (nodes < n)]
                now[nodes] = SE.moved_coords(was[nodes], by)
    return x, y


# ------------------------------------------------------------------------------------------------ the plan
class SwapPlan:
    """What swap_plan returns: K pairs of the groups of a search plan as host tables (pair_a, pair_b, prow_ptr, prow_row,
    prow_pair, sel_ptr, sel_row) and, in ONE int32 buffer on the device, all seven.  Valid for the life of its Predictor: the
    incidence is static and the anchors are read at call time."""

    def __init__(self, owner, plan, pair_a, pair_b, tables, T, device):
        self.owner, self.plan, self.i, self.T = owner, plan, plan.i, int(T)
        self.pair_a, self.pair_b = pair_a, pair_b
        self.prow_ptr, self.prow_row, self.prow_pair, self.sel_ptr, self.sel_row = tables
        self.K, self.RP, self.G = pair_a.shape[0], self.prow_row.shape[0], plan.G
        parts = [pair_a, pair_b, *tables]
        self.ints = torch.from_numpy(np.concatenate([v.astype(np.int32) for v in parts])).to(device)
        cuts = np.concatenate([[0], np.cumsum([v.shape[0] for v in parts])])
        self.dev = [self.ints[cuts[j]:cuts[j + 1]] for j in range(len(parts))]

    @classmethod
    def from_device(cls, owner, plan, ints, K, RP, T):
        """The plan of tables that were built on the device (mmft.pairs): `ints` is the int32 buffer in the layout above, and
        the host tables are decoded from ONE copy of it."""
        self = cls.__new__(cls)
        self.owner, self.plan, self.i, self.T = owner, plan, plan.i, int(T)
        self.K, self.RP, self.G, self.ints = int(K), int(RP), plan.G, ints
        cuts = np.concatenate([[0], np.cumsum([K, K, K + 1, RP, RP, K + 1, RP + 2 * K])])
        assert ints.dtype == torch.int32 and ints.numel() == cuts[-1]
        self.dev = [ints[cuts[j]:cuts[j + 1]] for j in range(7)]
        host = ints.cpu().numpy().astype(np.int64)
        self.pair_a, self.pair_b, self.prow_ptr, self.prow_row, self.prow_pair, self.sel_ptr, self.sel_row = \
            [host[cuts[j]:cuts[j + 1]] for j in range(7)]
        return self


def swap_plan(p, plan, pair_a, pair_b):
    """Predictor.swap_plan: see there."""
    if getattr(p, '_trial', None) is None:
        raise RuntimeError('Predictor.swap_plan(): built without trials=True')
    if not isinstance(plan, SE.SearchPlan):
        raise TypeError(f'swap_plan: plan must come from search_plan(), got {type(plan).__name__}')
    if plan.owner is not p:
        raise ValueError('swap_plan: the plan belongs to another Predictor')
    a, b = check_pairs(plan.mv_ptr, pair_a, pair_b)
    CM.check_plan(plan)
    T = int(p._sel.paths.numel())
    if T + plan.G > MAX_T:
        raise ValueError(f'swap_plan: {T} rows and {plan.G} groups do not fit the {MAX_T} rows of the selection')
    return SwapPlan(p, plan, a, b, pair_tables(plan.grow_ptr, plan.grow_row, a, b, T), T, p.device)


# ------------------------------------------------------------------------------------------------ the Predictor's side
def chunks(prow_ptr, max_rows):
    """[(k0, k1)]: the pairs cut at pair boundaries so that a chunk's entries stay within max_rows; a single larger pair goes
    alone."""
    prow_ptr = np.asarray(prow_ptr, dtype=np.int64)
    K, out, k0 = prow_ptr.shape[0] - 1, [], 0
    while k0 < K:
        k1 = int(np.searchsorted(prow_ptr, prow_ptr[k0] + int(max_rows), side='right')) - 1
        k1 = min(max(k1, k0 + 1), K)
        out.append((k0, k1))
        k0 = k1
    return out


def prepare(p, splan, scale_log2=20, max_rows=65536, min_gain=None, apply=False, who='swap_moves', patch=False):
    """Stage 1, host: trial.check_state's state and mode refusals, validation, the chunks, the call's ONE output buffer - int64
    [dq K | base 3 | stats 4], then int32 [dviol | new_nan | capped | worst | worst_row | pick | sel, K each] and - patch=True -
    behind those the two counts of mmft_refine_patch, int64, per chunk.  min_gain not None: the call selects (commit.min_quanta
    is its threshold) and, with `apply`, writes.  No host table is built and nothing is uploaded: the plan holds the tables.
    Returns the call `launch` takes."""
    if patch and not apply:
        raise ValueError(f'{who}: patch=True writes the rows of the moved pins into the kept state; it needs apply=True')
    TR.check_state(p, who, 'the chunks of the pairs are launched from the host per call')
    if not isinstance(splan, SwapPlan):
        raise TypeError(f'{who}: the plan must come from swap_plan(), got {type(splan).__name__}')
    if splan.owner is not p:
        raise ValueError(f'{who}: the plan belongs to another Predictor')
    SE.check_call(0, 1, scale_log2, max_rows, who)
    K = splan.K
    if patch and not p._trial.kept['pred'].is_contiguous():
        raise ValueError(f'{who}: patch=True writes the kept predictions in place; they are not contiguous')
    cuts = chunks(splan.prow_ptr, max_rows)
    tail = K + 7 + (7 * K + 1) // 2
    call = dict(splan=splan, scale_log2=int(scale_log2), chunks=cuts, n64=K + 7, tail=tail, patch=bool(patch),
                raw=torch.empty(tail + (2 * len(cuts) if patch else 0), dtype=torch.int64, device=p.device),
                min_q=None if min_gain is None else CM.min_quanta(min_gain, scale_log2), apply=bool(apply))
    if call['min_q'] is not None:
        owner = getattr(splan, 'commit_owner', None)         # scratch over the rows and the groups, kept with the plan
        if owner is None:
            owner = splan.commit_owner = torch.empty((CM.owner_bytes(splan.T + splan.G) + 7) // 8, dtype=torch.int64, device=p.device)
        call['owner'] = owner
    return call


def _views(raw, K, n64):
    """The tables inside the call's buffer (torch tensor or numpy array alike)."""
    i64, i32 = raw[:n64], raw[n64:n64 + (7 * K + 1) // 2].view(torch.int32 if torch.is_tensor(raw) else np.int32)
    f32 = torch.float32 if torch.is_tensor(raw) else np.float32
    return dict(dq=i64[:K], base=i64[K:K + 3], stats=i64[K + 3:K + 7], dviol=i32[:K], new_nan=i32[K:2 * K], capped=i32[2 * K:3 * K],
                worst=i32[3 * K:4 * K].view(f32), worst_row=i32[4 * K:5 * K], pick=i32[5 * K:6 * K], sel=i32[6 * K:7 * K])


def launch(p, call, timed=None):
    """Stage 2, device, on the current stream: per chunk of pairs mmft_swap_rows over its entries, mmft_head_mlp_fwd over
    their rows and mmft_swap_score (the first one with the base figures); then, for a call that selects, mmft_commit_select
    over the select table and - apply - mmft_swap_apply on the resident pins, after which the trial state is stale as after
    update().  patch=True: between the two, mmft_refine_patch (mmft_refine.h, as it stands) with the pairs as its groups -
    best_w = pick at radius 1, grow_row = prow_row, grow_grp = prow_pair, G = K - writes the selected pairs' entries into the
    kept x and pred, and the trial state stays fresh.  A call of one chunk patches from the rows and predictions of its
    scoring pass, in one launch; a call of several runs mmft_swap_rows and the head again per chunk - the pins have not
    moved yet - and patches that chunk's slice, each chunk with two counts of its own.  Returns the call.  `timed`: a callable
    that is handed each part as a function."""
    run = timed if timed is not None else (lambda name, fn: fn())
    splan, placed, b, kept = call['splan'], p._placed, p.batch, p._trial.kept
    plan = splan.plan
    x, GP, pred = kept['x'], kept['GP'], kept['pred']
    d_pa, d_pb, d_pptr, d_prow, d_ppair, d_sptr, d_srow = splan.dev
    d_mptr, d_node = plan.dev[3], plan.dev[4]
    fcn, mods = p.pmodel.fcn, list(p.pmodel.mlp_fuse.layers)
    width, Dout, T = x.shape[1], fcn.weight.shape[0], pred.numel()
    K, RP, G, scale = splan.K, splan.RP, splan.G, call['scale_log2']
    if T != splan.T:
        raise ValueError(f'swap plan made for {splan.T} rows, the kept predictions hold {T}')
    v = _views(call['raw'], K, call['n64'])
    most = max(int(splan.prow_ptr[k1] - splan.prow_ptr[k0]) for k0, k1 in call['chunks'])
    xt = torch.empty((most, width), dtype=torch.float32, device=p.device) if RP else None
    pred_t = torch.empty(most, dtype=torch.float32, device=p.device) if RP else None
    rows = p.slack.rows_of(splan.i)

    def entry_rows(e0, e1):
        abi('mmft_swap_rows', placed.nodes, placed.lens, placed.maxlen, placed.loc_x, placed.loc_y, placed.map_x, placed.map_y,
            p._sel.paths, p._sel.feat_off if b.B > 1 else None, T, d_prow, d_ppair, RP, d_pa, d_pb, K, d_mptr, d_node, G, e0, e1,
            GP, fcn.bias, x, x.stride(0), xt, width, width, kept['cnn_col'], Dout, b.masks.run_block, *lib.stream_args(x))
        lib.head('mmft_head_mlp_fwd', xt, width, mods[0].weight, mods[0].bias, mods[2].weight, mods[2].bias, None, pred_t,
                 e1 - e0, mods[0].weight.shape[1], mods[0].weight.shape[0], 1, *lib.stream_args(x))

    def score():
        for k0, k1 in call['chunks']:
            e0, e1 = int(splan.prow_ptr[k0]), int(splan.prow_ptr[k1])
            if e1 > e0:
                entry_rows(e0, e1)
            abi('mmft_swap_score', pred_t, pred.reshape(-1), p.slack.required, T, d_pptr, d_prow if RP else None, K, RP, k0, k1, scale,
                v['dq'], v['dviol'], v['new_nan'], v['capped'], v['worst'], v['worst_row'], v['pick'],
                v['base'] if k0 == 0 else None, rows, rows.numel(), *lib.stream_args(x))
    run('score', score)
    call['xt'] = xt
    if call['min_q'] is not None:
        run('select', lambda: CM.abi('mmft_commit_select', v['pick'], v['dq'], K, 1, d_sptr, d_srow, RP + 2 * K, T + G, call['min_q'],
                                     v['sel'], v['stats'], call['owner'], *lib.stream_args(x)))
        if call['patch']:
            counts, one = call['raw'][call['tail']:], len(call['chunks']) == 1

            def patch():
                for c, (k0, k1) in enumerate(call['chunks']):
                    e0, e1 = int(splan.prow_ptr[k0]), int(splan.prow_ptr[k1])
                    if e1 > e0 and not one:                  # (one chunk: xt and pred_t of the scoring pass hold these rows)
                        entry_rows(e0, e1)
                    some = e1 > e0
                    RF.abi('mmft_refine_patch', x, x.stride(0), pred.reshape(-1), T, xt if some else None, width, pred_t if some else None,
                           v['sel'], v['pick'], 1, d_prow[e0:] if some else None, d_ppair[e0:] if some else None, e1 - e0, K,
                           kept['cnn_col'], Dout, counts[2 * c:2 * c + 2], *lib.stream_args(x))
            run('patch', patch)
        if call['apply']:
            p._trial.stale = not call['patch']               # unpatched: until the next predict(), exactly as update() leaves it
            run('apply', lambda: abi('mmft_swap_apply', placed.loc_x, placed.loc_y, placed.loc_x.numel(), v['sel'], v['pick'], d_pa, d_pb, K,
                                     d_mptr, d_node if plan.M else None, G, plan.M, *lib.stream_args(x)))
    return call


def fetch(call):
    """Stage 3: ONE device -> host copy (kept as call['host']), decoded; best_pair / best_pair_dq are made here, on the host,
    from that copy.  The result of swap_moves or commit_swaps."""
    splan, scale = call['splan'], call['scale_log2']
    K = splan.K
    host = call['host'] = call['raw'].cpu().numpy()
    v = _views(host, K, call['n64'])
    res = {k: v[k].copy() for k in TABLES}
    res['eligible'] = v['pick'] == 0
    res['gain'] = (-res['dq']).astype(np.float64) * 2.0 ** -scale
    res['base'] = dict(nsum=int(v['base'][0]), violations=int(v['base'][1]), n_nan=int(v['base'][2]))
    res['prow_ptr'], res['rows'] = splan.prow_ptr, splan.prow_row
    res['best_pair'], res['best_pair_dq'] = best_pair_host(res['dq'], res['eligible'], splan.pair_a, splan.pair_b, splan.G)
    if call['min_q'] is not None:
        stats, sum_dq = v['stats'], int(v['stats'][1])
        res['pair_gain'] = res['gain']
        res.update(selected=v['sel'] != 0, n_selected=int(stats[0]), n_candidates=int(stats[2]), rounds=int(stats[3]), sum_dq=sum_dq,
                   gain=float(-sum_dq) * 2.0 ** -scale, predicted_nsum=res['base']['nsum'] + sum_dq)
        if call['patch']:                                    # the chunks' counts, summed here
            res['n_patched'] = int(host[call['tail']:].reshape(-1, 2)[:, 0].sum())
    return res


def swap_moves(p, splan, scale_log2=20, max_rows=65536):
    """Predictor.swap_moves: see there."""
    return fetch(launch(p, prepare(p, splan, scale_log2, max_rows)))


def commit_swaps(p, splan, scale_log2=20, max_rows=65536, min_gain=0.0, apply=True, patch=False):
    """Predictor.commit_swaps: see there."""
    return fetch(launch(p, prepare(p, splan, scale_log2, max_rows, min_gain, apply, who='commit_swaps', patch=patch)))
