"""Shared inputs of test_swap_cpu.py / test_swap_gpu.py: literal Python-loop restatements of the swap rule, of the pair tables,
of the score, of the best pair per group and of the write of include/mmft_swap.h; pin groups and pairs on the kernel cases of
search_cases.py; the hand-built predictions of search_cases.py turned into pairs; and a hand-built selection.  A plain module:
it holds no test."""
import math

import numpy as np

import search_cases as SC
import trial_cases as TC

I32_MIN, I32_MAX = SC.I32_MIN, SC.I32_MAX
F = np.float32
I64 = lambda a: np.array(a, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ literal restatements
def sat32(v):
    return max(I32_MIN, min(I32_MAX, int(v)))


def swapped_literal(px, py, mv_ptr, mv_node, pair_a, pair_b):
    """(cand_ptr, node, x, y): per pair the pins of a, then those of b, at sat32(loc[n] + (loc[B] - loc[A])) and
    sat32(loc[n] + (loc[A] - loc[B])), A and B the groups' first pins; Python integers, so no sum wraps."""
    ptr, node, xs, ys = [0], [], [], []
    for a, b in zip(pair_a, pair_b):
        na = [int(n) for n in mv_node[mv_ptr[a]:mv_ptr[a + 1]]]
        nb = [int(n) for n in mv_node[mv_ptr[b]:mv_ptr[b + 1]]]
        A, B = na[0], nb[0]
        for pins, (src, dst) in ((na, (A, B)), (nb, (B, A))):
            for n in pins:
                node.append(n)
                xs.append(sat32(int(px[n]) + (int(px[dst]) - int(px[src]))))
                ys.append(sat32(int(py[n]) + (int(py[dst]) - int(py[src]))))
        ptr.append(len(node))
    return I64(ptr), I64(node), I64(xs), I64(ys)


def pair_tables_literal(grow_ptr, grow_row, pair_a, pair_b, T):
    """(prow_ptr, prow_row, prow_pair, sel_ptr, sel_row) as plain loops: per pair the sorted set of both groups' rows, and in the
    select table those rows followed by T + a and T + b."""
    prow_ptr, prow_row, prow_pair, sel_ptr, sel_row = [0], [], [], [0], []
    for k, (a, b) in enumerate(zip(pair_a, pair_b)):
        rows = sorted({int(r) for g in (a, b) for r in grow_row[grow_ptr[g]:grow_ptr[g + 1]]})
        prow_row += rows
        prow_pair += [k] * len(rows)
        prow_ptr.append(len(prow_row))
        sel_row += rows + [T + int(a), T + int(b)]
        sel_ptr.append(len(sel_row))
    return I64(prow_ptr), I64(prow_row), I64(prow_pair), I64(sel_ptr), I64(sel_row)


def score_literal(pred_base, required, prow_ptr, prow_row, pred_trial, scale_log2):
    """The six tables, pick and eligible of mmft_swap_score word by word: a loop over pairs and their entries."""
    K = len(prow_ptr) - 1
    out = dict(dq=np.zeros(K, dtype=np.int64), dviol=np.zeros(K, dtype=np.int32), new_nan=np.zeros(K, dtype=np.int32),
               capped=np.zeros(K, dtype=np.int32), worst=np.full(K, np.nan, dtype=F), worst_row=np.full(K, -1, dtype=np.int32),
               pick=np.zeros(K, dtype=np.int32), eligible=np.zeros(K, dtype=bool))
    for k in range(K):
        worst = None
        for e in range(int(prow_ptr[k]), int(prow_ptr[k + 1])):
            r = int(prow_row[e])
            if not 0 <= r < len(pred_base):
                continue
            sb, st = SC.slack_literal(required[r], pred_base[r]), SC.slack_literal(required[r], pred_trial[e])
            (qb, cb), (qt, ct) = SC.quantum_literal(sb, scale_log2), SC.quantum_literal(st, scale_log2)
            out['dq'][k] += qt - qb
            out['dviol'][k] += int(st < 0) - int(sb < 0)
            out['new_nan'][k] += int(math.isnan(st) and not math.isnan(sb))
            out['capped'][k] += int(cb or ct)
            if not math.isnan(st) and (worst is None or (st, r) < worst):
                worst = (st, r)
        if worst is not None:
            out['worst'][k], out['worst_row'][k] = worst
        out['eligible'][k] = out['new_nan'][k] == 0
        out['pick'][k] = 0 if out['eligible'][k] else -1
    return out


def best_pair_literal(dq, eligible, pair_a, pair_b, G):
    best, best_dq = [-1] * G, [0] * G
    for g in range(G):
        keys = [(int(dq[k]), k) for k in range(len(dq)) if eligible[k] and g in (int(pair_a[k]), int(pair_b[k]))]
        if keys:
            best_dq[g], best[g] = min(keys)
    return I64(best), I64(best_dq)


def apply_literal(loc_x, loc_y, sel, pick, pair_a, pair_b, mv_ptr, mv_node):
    """The write of mmft_swap_apply in plain Python: every selected pair from the coordinates as they were."""
    x, y, n = [int(v) for v in loc_x], [int(v) for v in loc_y], len(loc_x)
    for k in range(len(sel)):
        if not sel[k] or pick[k] != 0:
            continue
        a, b = int(pair_a[k]), int(pair_b[k])
        na, nb = [int(v) for v in mv_node[mv_ptr[a]:mv_ptr[a + 1]]], [int(v) for v in mv_node[mv_ptr[b]:mv_ptr[b + 1]]]
        if a == b or not na or not nb or not (0 <= na[0] < n and 0 <= nb[0] < n):
            continue
        dx, dy = int(loc_x[nb[0]]) - int(loc_x[na[0]]), int(loc_y[nb[0]]) - int(loc_y[na[0]])
        for pins, s in ((na, 1), (nb, -1)):
            for v in pins:
                if 0 <= v < n:
                    x[v], y[v] = sat32(int(loc_x[v]) + s * dx), sat32(int(loc_y[v]) + s * dy)
    return x, y


def same_tables(got, want, where=''):
    """Two results of the score agree: the integer tables equal, `worst` bitwise (a NaN equals itself)."""
    for k in ('dq', 'dviol', 'new_nan', 'capped', 'worst_row'):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (where, k, got[k], want[k])
    assert got['worst'].dtype == np.float32 and np.array_equal(got['worst'].view(np.uint32), np.asarray(want['worst'], dtype=F).view(np.uint32)), \
        (where, 'worst', got['worst'], want['worst'])
    assert np.array_equal(got['eligible'], want['eligible']), (where, 'eligible')


# ------------------------------------------------------------------------------------------------ kernel cases
def tables(case):
    """search_cases.tables(case) - the pin at (I32_MAX, I32_MIN) included - with one padding pin, the TWIN, put at the
    coordinates of an on-path pin: two groups whose anchors coincide swap by the zero move.  Returns (path_nodes, path_lens,
    pin_x, pin_y, the saturating pin, the on-path pin, its twin)."""
    nodes, lens, px, py, rep, far = SC.tables(case)
    rows = [TC.live(nodes, lens, q) for q in range(nodes.shape[0])]
    multi = [q for q in range(len(rows) - 1) if len(set(rows[q])) >= 2]
    mate = next(v for q in multi for v in rows[q] if v != far)
    twin = px.shape[0] - 2                                               # a padding pin: no path holds it
    assert all(twin not in r for r in rows)
    px, py = px.copy(), py.copy()
    px[twin], py[twin] = px[mate], py[mate]
    return nodes, lens, px, py, far, mate, twin


def groups(case):
    """[(tag, nodes)]: the pin groups of the kernel tests on `tables(case)`; node ids in the tables' numbering, distinct inside a
    group.  Groups that a pair of `pairs` joins hold distinct pins."""
    nodes, lens, px, py, far, mate, twin = tables(case)
    N = px.shape[0]
    rows = [TC.live(nodes, lens, q) for q in range(nodes.shape[0])]
    longest = max(range(len(rows)), key=lambda q: len(set(rows[q])))
    multi = [q for q in range(len(rows) - 1) if len(set(rows[q])) >= 2]
    u, v = next(ns[:2] for q in multi for ns in [[n for n in dict.fromkeys(rows[q]) if n != far]] if len(ns) >= 2)      # two pins of ONE row
    out = [('single', [mate]),
           ('three_of_one_row', [n for n in sorted(set(rows[longest])) if n != far][:3]),
           ('on_no_row', [N - 1]),
           ('saturating', [far])]
    lone = next(n for q in multi for n in rows[q] if n not in (far, mate))
    first = [n for n in sorted(set(rows[longest])) if n != lone][:63]
    many = first + [n for n in range(N) if n not in set(first) and n != lone][:63 - len(first)]
    assert len(many) == 63 == len(set(many)) and lone not in many
    out += [('sixty_three', many), ('lone', [lone])]
    out += [('thirty_two_a', list(range(0, 64, 2))), ('thirty_two_b', list(range(1, 64, 2)))]
    out += [('same_row_a', [u]), ('same_row_b', [v]), ('twin', [twin])]
    if case.name == 'long_walk_16x16':
        out.append(('shared_by_two_stages', [rows[0][255]]))            # staged as nodes 0 .. 255, then 255 .. 299
    assert all(g and len(set(g)) == len(g) for _, g in out)
    return out


def pairs(case):
    """(pair_a, pair_b, tags): the pairs of the kernel tests, as indices into `groups(case)`."""
    tags = [g[0] for g in groups(case)]
    named = [('same_row_a', 'same_row_b'), ('same_row_b', 'same_row_a'), ('single', 'on_no_row'), ('saturating', 'single'),
             ('three_of_one_row', 'saturating'), ('sixty_three', 'lone'), ('lone', 'sixty_three'), ('thirty_two_a', 'thirty_two_b'),
             ('single', 'twin'), ('on_no_row', 'twin')]
    if 'shared_by_two_stages' in tags:
        named.append(('shared_by_two_stages', 'on_no_row'))
    return I64([tags.index(a) for a, _ in named]), I64([tags.index(b) for _, b in named]), named


def plan(case, paths):
    """(grow_ptr, grow_row, grow_grp, mv_ptr, mv_node) of groups(case) over the selection `paths`, by search_cases' literal loop."""
    nodes, lens = tables(case)[:2]
    gs = groups(case)
    pins = I64([n for _, g in gs for n in g])
    ptr = I64(np.concatenate([[0], np.cumsum([len(g) for _, g in gs])]))
    return SC.plan_literal(nodes, lens, paths, 0, pins, ptr)


# ------------------------------------------------------------------------------------------------ hand-built scores
def from_window(pred_base, required, grow_ptr, grow_row, trial, scale_log2):
    """A window case of search_cases.py as pairs: pair g * W + w holds group g's entries with the predictions of offset w.
    Returns (pred_base, required, prow_ptr, prow_row, pred_trial [RP], scale_log2)."""
    W = trial.shape[0]
    ptr, rows, pred = [0], [], []
    for g in range(len(grow_ptr) - 1):
        a, b = int(grow_ptr[g]), int(grow_ptr[g + 1])
        for w in range(W):
            rows += [int(r) for r in grow_row[a:b]]
            pred += [trial[w, e] for e in range(a, b)]
            ptr.append(len(rows))
    return pred_base, required, I64(ptr), I64(rows), np.array(pred, dtype=F), scale_log2


SCORE_CASES = dict(special_rows=lambda: from_window(*SC.special_rows()), special_cap=lambda: from_window(*SC.special_cap()),
                   special_ineligible=lambda: from_window(*SC.special_ineligible()[:6]), seeded=lambda: from_window(*SC.seeded_scores()))


# ------------------------------------------------------------------------------------------------ a hand-built selection
def select_case():
    """Thirteen groups, seven pairs, min_q = 3.  Rows per group: 0 none, 1 [0], 2 [1], 3 [2, 3], 4 [4], 5 [3, 5], 6 .. 12 one row
    of their own each.
        pair 0 (0, 1) dq -5     shares group 0 - which lies on no row - with pair 1 and nothing else: loses to it
        pair 1 (0, 2) dq -7     taken
        pair 2 (3, 4) dq -9     taken
        pair 3 (5, 6) dq -4     shares row 3, and no group, with pair 2: loses to it
        pair 4 (7, 8) dq -3     disjoint from everything: taken
        pair 5 (9, 10) dq -100  ineligible (pick -1): never selected
        pair 6 (11, 12) dq -2   > -min_q: no candidate
    Returns (grow_ptr, grow_row, pair_a, pair_b, pick, dq, T, min_q, the expected sel, the expected number of candidates)."""
    rows = [[], [0], [1], [2, 3], [4], [3, 5], [6], [7], [8], [9], [10], [11], [12]]
    grow_ptr = I64(np.concatenate([[0], np.cumsum([len(r) for r in rows])]))
    grow_row = I64([r for g in rows for r in g])
    pair_a, pair_b = I64([0, 0, 3, 5, 7, 9, 11]), I64([1, 2, 4, 6, 8, 10, 12])
    pick, dq = np.array([0, 0, 0, 0, 0, -1, 0], dtype=np.int32), I64([-5, -7, -9, -4, -3, -100, -2])
    return grow_ptr, grow_row, pair_a, pair_b, pick, dq, 13, 3, [0, 1, 1, 0, 1, 0, 0], 5


def lost_how(selected, candidates, prow_ptr, prow_row, pair_a, pair_b):
    """(by a shared row, by a shared group alone): the candidates that were not selected, split by what they share with the
    selected pairs - a row (whatever else), or no row but a group."""
    taken = [k for k in range(len(selected)) if selected[k]]
    rows_of = lambda k: set(prow_row[prow_ptr[k]:prow_ptr[k + 1]].tolist())
    by_row, by_group = [], []
    for k in range(len(selected)):
        if not candidates[k] or selected[k]:
            continue
        if any(rows_of(k) & rows_of(j) for j in taken):
            by_row.append(k)
        elif any({int(pair_a[k]), int(pair_b[k])} & {int(pair_a[j]), int(pair_b[j])} for j in taken):
            by_group.append(k)
    return by_row, by_group


def apply_case():
    """24 pins, some at the ends of int32; groups 0 [0, 4] (anchor at (I32_MAX, I32_MIN)), 1 [1, 5, 6], 2 [7], 3 [8, 9], 4 [10],
    5 [11, 12], 6 [13, -1, 99, 14] (node ids outside the arrays), 7 [15], 8 [] , 9 [16], 10 [40] (its anchor outside), 11 [17].
    Pairs: selected (0, 1) - the saturating one -, unselected (2, 3), selected with pick -1 (4, 5), selected (6, 7), selected with
    an empty group (8, 9), with an anchor outside (10, 11), and (9, 9).
    Returns dict(loc_x, loc_y, sel, pick, pair_a, pair_b, mv_ptr, mv_node)."""
    n = 24
    rng = np.random.default_rng(5)
    x, y = rng.integers(-5, 20, n), rng.integers(-5, 20, n)
    x[[0, 1]], y[[0, 1]] = [I32_MAX, -3], [I32_MIN, 7]
    x[4], y[4] = -4, 30                                                  # beside the saturating anchor: both sums leave int32
    x[5], y[6] = I32_MIN + 2, I32_MAX - 1
    gs = [[0, 4], [1, 5, 6], [7], [8, 9], [10], [11, 12], [13, -1, 99, 14], [15], [], [16], [40], [17]]
    ptr = I64(np.concatenate([[0], np.cumsum([len(g) for g in gs])]))
    return dict(loc_x=x.astype(np.int32), loc_y=y.astype(np.int32), sel=np.array([1, 0, 1, 2, 1, 1, 1], dtype=np.int32),
                pick=np.array([0, 0, -1, 0, 0, 0, 0], dtype=np.int32), pair_a=I64([0, 2, 4, 6, 8, 10, 9]), pair_b=I64([1, 3, 5, 7, 9, 11, 9]),
                mv_ptr=ptr, mv_node=I64([v for g in gs for v in g]))
