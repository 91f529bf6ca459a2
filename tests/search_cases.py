"""Shared inputs of test_search_cpu.py / test_search_gpu.py: literal Python-loop restatements of the plan and of the scores of
include/mmft_search.h, seeded pin groups on the kernel cases of trial_cases.py, the explicit expansion of a window into
trial-move candidates, and hand-built predictions that hold every edge of the score.  A plain module: it holds no test."""
import math

import numpy as np

import trial_cases as TC

I32_MIN, I32_MAX = TC.I32_MIN, TC.I32_MAX
F = np.float32
NAN, INF = float('nan'), float('inf')


# ------------------------------------------------------------------------------------------------ literal restatements
def window(radius):
    """[(dx, dy)] of the offsets 0 .. W - 1, from the words of the header."""
    side = 2 * radius + 1
    return [(w // side - radius, w % side - radius) for w in range(side * side)]


def sat32(v):
    return max(I32_MIN, min(I32_MAX, int(v)))


def plan_literal(path_nodes, path_lens, paths, node_off, pins, group_ptr):
    """(grow_ptr, grow_row, grow_grp, mv_ptr, mv_node) as plain loops over groups, rows and pins."""
    maxlen = path_nodes.shape[1]
    grow_ptr, grow_row, grow_grp, mv_node = [0], [], [], []
    for g in range(len(group_ptr) - 1):
        mine = {int(p) + int(node_off) for p in pins[group_ptr[g]:group_ptr[g + 1]]}
        mv_node += [int(p) + int(node_off) for p in pins[group_ptr[g]:group_ptr[g + 1]]]
        for t, q in enumerate(paths):
            if mine & {int(v) for v in path_nodes[q, :min(int(path_lens[q]), maxlen)]}:
                grow_row.append(t)
                grow_grp.append(g)
        grow_ptr.append(len(grow_row))
    i64 = lambda a: np.array(a, dtype=np.int64)
    return i64(grow_ptr), i64(grow_row), i64(grow_grp), i64([int(v) for v in group_ptr]), i64(mv_node)


def slack_literal(required, pred):
    """The rule of mmft_report.h on two fp32 values: one fp32 subtraction, -0.0 -> +0.0; NaN stays NaN."""
    with np.errstate(invalid='ignore', over='ignore'):
        s = float(F(F(required) - F(pred)))
    return s if math.isnan(s) else s + 0.0


def quantum_literal(s, scale_log2):
    """(q, capped) of THE QUANTUM of mmft_crit_sums.h for one slack, in exact integer / fraction arithmetic."""
    from fractions import Fraction
    if math.isnan(s) or not s < 0:
        return 0, False
    if s == -INF or Fraction(-s) >= Fraction(2) ** (32 - scale_log2):
        return 2 ** 32, True
    v = Fraction(-s) * 2 ** scale_log2
    lo = v.numerator // v.denominator
    rest = v - lo
    q = lo + (1 if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2) else 0)     # to nearest, ties to even
    return q, False


def score_literal(pred_base, required, grow_ptr, grow_row, pred_trial, radius, scale_log2):
    """Every table and the best of include/mmft_search.h word by word: loops over groups, offsets and entries."""
    win = window(radius)
    G, W, R = len(grow_ptr) - 1, len(win), len(grow_row)
    pred_trial = np.asarray(pred_trial, dtype=F).reshape(W, R)
    out = dict(dq=np.zeros((G, W), dtype=np.int64), dviol=np.zeros((G, W), dtype=np.int32), new_nan=np.zeros((G, W), dtype=np.int32),
               capped=np.zeros((G, W), dtype=np.int32), worst=np.full((G, W), np.nan, dtype=F), worst_row=np.full((G, W), -1, dtype=np.int32),
               best_w=np.full(G, -1, dtype=np.int32), best_dx=np.zeros(G, dtype=np.int32), best_dy=np.zeros(G, dtype=np.int32),
               best_dq=np.zeros(G, dtype=np.int64), best_gain=np.zeros(G, dtype=np.float64))
    for g in range(G):
        best = None
        for w in range(W):
            worst = None
            for e in range(int(grow_ptr[g]), int(grow_ptr[g + 1])):
                r = int(grow_row[e])
                if not 0 <= r < len(pred_base):
                    continue
                sb, st = slack_literal(required[r], pred_base[r]), slack_literal(required[r], pred_trial[w, e])
                (qb, cb), (qt, ct) = quantum_literal(sb, scale_log2), quantum_literal(st, scale_log2)
                out['dq'][g, w] += qt - qb
                out['dviol'][g, w] += int(st < 0) - int(sb < 0)
                out['new_nan'][g, w] += int(math.isnan(st) and not math.isnan(sb))
                out['capped'][g, w] += int(cb or ct)
                if not math.isnan(st) and (worst is None or (st, r) < worst):
                    worst = (st, r)
            if worst is not None:
                out['worst'][g, w], out['worst_row'][g, w] = worst
            if out['new_nan'][g, w] == 0:
                key = (int(out['dq'][g, w]), abs(win[w][0]) + abs(win[w][1]), w)
                if best is None or key < best:
                    best = key
        if best is not None:
            w = best[2]
            out['best_w'][g], out['best_dx'][g], out['best_dy'][g], out['best_dq'][g] = w, win[w][0], win[w][1], best[0]
            out['best_gain'][g] = -best[0] * 2.0 ** -scale_log2
    return out


def same_tables(got, want, where=''):
    """Two results of the score agree: the integer tables equal, `worst` and best_gain bitwise (a NaN equals itself)."""
    for k in ('dq', 'dviol', 'new_nan', 'capped', 'worst_row', 'best_w', 'best_dx', 'best_dy', 'best_dq'):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (where, k, got[k], want[k])
    assert got['worst'].dtype == np.float32 and np.array_equal(got['worst'].view(np.uint32), np.asarray(want['worst'], dtype=F).view(np.uint32)), \
        (where, 'worst', got['worst'], want['worst'])
    assert np.array_equal(got['best_gain'].view(np.uint64), want['best_gain'].view(np.uint64)), (where, 'best_gain')


# ------------------------------------------------------------------------------------------------ hand-built scores
def special_rows():
    """(pred_base, required, grow_ptr, grow_row, pred_trial [9, R], scale_log2) at radius 1 (centre w = 4): every edge of the
    score in one input.  Row by row (required, base prediction -> base slack):
        0   1.0   2.0   -1        violates
        1   1.0   NaN   NaN       a NaN base row: a NaN trial is not NEW, a number makes the row valid again
        2   2.0   2.0   +0
        3  -0.0   0.0   -0.0 -> +0.0: does not violate, ties with row 2 on the worst slack
        4   0.5   1.5   -1
        5   3.0   1.0   +2
    Groups: 0 = rows 0, 2, 3 (NaN, +-inf and -0.0 predictions); 1 = row 1; 2 = no rows; 3 = rows 0, 4, 5.  (Ties of the
    best key, an ineligible minimum and the cap have inputs of their own below.)"""
    required = np.array([1.0, 1.0, 2.0, -0.0, 0.5, 3.0], dtype=F)
    pred_base = np.array([2.0, NAN, 2.0, 0.0, 1.5, 1.0], dtype=F)
    grow_ptr = np.array([0, 3, 4, 4, 7], dtype=np.int64)
    grow_row = np.array([0, 2, 3, 1, 0, 4, 5], dtype=np.int64)
    W, R = 9, grow_row.shape[0]
    trial = np.tile(pred_base[grow_row], (W, 1)).astype(F)               # every offset starts as the zero move
    # group 0 (entries 0, 1, 2 = rows 0, 2, 3)
    trial[0, 0] = NAN                                                     # a new NaN: ineligible
    trial[1, 0] = INF                                                     # slack -inf: capped, the worst of all
    trial[2, 0] = -INF                                                    # slack +inf: valid, does not violate
    trial[3, 2] = -0.0                                                    # -0.0 - (-0.0): slack +0.0 either way
    trial[5, 1] = 2.5                                                     # row 2 starts to violate
    trial[6, 0], trial[6, 1] = 0.0, 3.0                                   # row 0 cured (+1), row 2 at -1: dq 0, dviol 0
    # group 1 (entry 3 = row 1, a NaN base row)
    trial[0, 3] = 5.0                                                     # valid again and violating: dq > 0, not a new NaN
    trial[8, 3] = 0.0
    # group 3 (entries 4, 5, 6 = rows 0, 4, 5): equal slack on rows 0 and 4 - the smallest row is the worst row
    trial[7, 4], trial[7, 5] = 1.5, 1.0                                   # both at -0.5
    return pred_base, required, grow_ptr, grow_row, trial, 20


def special_ties():
    """Radius 1, one group of one violating row (slack -1): offsets 0 (distance 2), 1, 3 and 7 (distance 1) all cure it by
    the same amount, every other offset but the centre makes it worse.  The key (dq, |dx| + |dy|, w) picks w = 1.  A second
    group: offsets 0 and 8 (both distance 2) tie - w = 0 wins."""
    required, pred_base = np.array([0.0, 0.0], dtype=F), np.array([1.0, 1.0], dtype=F)
    grow_ptr, grow_row = np.array([0, 1, 2], dtype=np.int64), np.array([0, 1], dtype=np.int64)
    trial = np.full((9, 2), 2.0, dtype=F)
    trial[4] = 1.0
    trial[[0, 1, 3, 7], 0] = 0.5
    trial[[0, 8], 1] = 0.25
    return pred_base, required, grow_ptr, grow_row, trial, 20, [1, 0]


def special_ineligible():
    """Radius 1, one group of two rows: offset 2 has by far the smallest dq but turns row 1 into a NaN - ineligible; offset 6
    is the best eligible one."""
    required, pred_base = np.array([0.0, 0.0], dtype=F), np.array([4.0, 1.0], dtype=F)
    grow_ptr, grow_row = np.array([0, 2], dtype=np.int64), np.array([0, 1], dtype=np.int64)
    trial = np.tile(pred_base, (9, 1)).astype(F)
    trial[2] = (-5.0, NAN)
    trial[6] = (3.0, 1.0)
    return pred_base, required, grow_ptr, grow_row, trial, 20, [6]


def special_cap():
    """scale_log2 = 30: the cap is at -slack >= 4.  One group of three rows: the base of row 0 is capped already, row 1 reaches
    the cap under offset 0, row 2 is just below it (4 - 2^-22: q = 2^32 - 256)."""
    required = np.zeros(3, dtype=F)
    pred_base = np.array([5.0, 1.0, 1.0], dtype=F)
    grow_ptr, grow_row = np.array([0, 3], dtype=np.int64), np.arange(3, dtype=np.int64)
    trial = np.tile(pred_base, (9, 1)).astype(F)
    trial[0, 1] = 4.0
    trial[1, 2] = np.nextafter(F(4.0), F(0.0))
    trial[2, 0] = 0.5                                                    # row 0 leaves the cap: still counted, its base is capped
    return pred_base, required, grow_ptr, grow_row, trial, 30


def seeded_scores(seed=31, T=600, radius=1):
    """(pred_base, required, grow_ptr, grow_row, pred_trial [W, R], scale_log2): T = 600 rows and groups of 0, 1, 257 and 600
    rows - none, one lane, more than four trips of a wave's 64 lanes with a remainder, every row -, predictions around the
    required times over nine decades, with NaN and infinite ones sprinkled into the odd offsets."""
    rng = np.random.default_rng(seed)
    required = rng.normal(0, 1, T).astype(F)
    pred_base = (required + rng.normal(0, 10.0 ** rng.uniform(-6, 3, T))).astype(F)
    pred_base[[5, 300]] = NAN
    sizes = [0, 1, 257, 600]
    grow_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    grow_row = np.concatenate([np.sort(rng.permutation(T)[:s]) for s in sizes]).astype(np.int64)
    W, R = (2 * radius + 1) ** 2, grow_row.shape[0]
    trial = (required[grow_row][None, :] + rng.normal(0, 10.0 ** rng.uniform(-6, 3, (W, R)))).astype(F)
    odd = (np.arange(W) % 2 == 1)[:, None]                                # the even offsets stay finite: some of them can win
    trial[odd & (rng.random((W, R)) < 0.01)] = NAN
    trial[odd & (rng.random((W, R)) < 0.01)] = INF
    trial[2 * radius * (radius + 1)] = pred_base[grow_row]                # the centre is the zero move
    return pred_base, required, grow_ptr, grow_row, trial, 20


# ------------------------------------------------------------------------------------------------ kernel cases
def tables(case):
    """trial_cases.tables(case) with ONE on-path pin's resident coordinates put at the ends of int32 - (I32_MAX, I32_MIN) -:
    a window offset added to it must saturate, not wrap.  Returns (path_nodes, path_lens, pin_x, pin_y, repeat_row, the pin)."""
    nodes, lens, px, py, rep = TC.tables(case)
    rows = [TC.live(nodes, lens, q) for q in range(nodes.shape[0])]
    multi = [q for q in range(len(rows) - 1) if len(set(rows[q])) >= 2]
    far = rows[multi[-1]][-1]
    px, py = px.copy(), py.copy()
    px[far], py[far] = I32_MAX, I32_MIN
    return nodes, lens, px, py, rep, far


def groups(case):
    """[(tag, nodes)]: the pin groups the kernel test runs on `tables(case)`, seeded per case; node ids in the tables' numbering,
    distinct inside a group."""
    nodes, lens, px, py, rep, far = tables(case)
    rng = np.random.default_rng(2000 + len(case.name) + case.map_x)
    N = px.shape[0]
    rows = [TC.live(nodes, lens, q) for q in range(nodes.shape[0])]
    longest = max(range(len(rows)), key=lambda q: len(set(rows[q])))
    multi = [q for q in range(len(rows) - 1) if len(set(rows[q])) >= 2]
    q = multi[int(rng.integers(len(multi)))]
    out = [('single', [rows[q][int(rng.integers(len(rows[q])))]]),
           ('repeated_in_its_row', [rows[rep][0]]),
           ('three_of_one_row', sorted(set(rows[longest]))[:3])]
    first = sorted(set(rows[longest]))[:64]
    many = first + [v for v in range(N) if v not in set(first)][:64 - len(first)]
    assert len(many) == 64 == len(set(many))
    out.append(('sixty_four', many))
    out.append(('on_no_row', [N - 1, N - 2]))                            # padding pins: no path holds them
    out.append(('saturating', [far]))
    if case.name == 'long_walk_16x16':
        out.append(('shared_by_two_stages', [rows[0][255]]))            # staged as nodes 0 .. 255, then 255 .. 299
    return out


def explicit(px, py, group_nodes, radius):
    """The window written out as trial-move candidates: candidate g * W + w holds group g's pins at sat32(resident + offset).
    Returns (mv_ptr [G W + 1], mv_node, mv_x, mv_y) as int64 arrays."""
    win = window(radius)
    ptr, node, xs, ys = [0], [], [], []
    for pins in group_nodes:
        for dx, dy in win:
            node += [int(n) for n in pins]
            xs += [sat32(int(px[n]) + dx) for n in pins]
            ys += [sat32(int(py[n]) + dy) for n in pins]
            ptr.append(len(node))
    i64 = lambda a: np.array(a, dtype=np.int64)
    return i64(ptr), i64(node), i64(xs), i64(ys)
