"""Hand-built inputs of the commit kernels (include/mmft_commit.h) and their literal definitions, shared by test_commit_cpu.py and
test_commit_gpu.py.  A plain module: it holds no test.

A SELECT CASE is dict(best_w, best_dq, radius, grow_ptr, grow_row, T, min_q); an APPLY CASE dict(loc_x, loc_y, sel, best_w,
radius, mv_ptr, mv_node)."""
import functools

import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
I64 = lambda a: np.asarray(a, dtype=np.int64)


def centre(radius):
    return 2 * radius * (radius + 1)


def _case(best_w, best_dq, rows, T, radius=1, min_q=1):
    """rows: per group the list of its rows."""
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    flat = I64([v for r in rows for v in r])
    return dict(best_w=I64(best_w), best_dq=I64(best_dq), radius=radius, grow_ptr=ptr, grow_row=flat, T=T, min_q=min_q)


# ------------------------------------------------------------------------------------------------ the literal definitions
def select_literal(best_w, best_dq, radius, grow_ptr, grow_row, T, min_q):
    """The sequential loop of the header, in plain Python: (sel list, selected, sum, candidates)."""
    G = len(best_w)
    cands = [g for g in range(G) if best_w[g] >= 0 and best_w[g] != centre(radius) and int(best_dq[g]) <= -min_q]
    taken_rows, sel = set(), [0] * G
    for g in sorted(cands, key=lambda g: (int(best_dq[g]), g)):
        rows = {int(r) for r in grow_row[grow_ptr[g]:grow_ptr[g + 1]] if 0 <= r < T}
        if not rows & taken_rows:
            taken_rows |= rows
            sel[g] = 1
    return sel, sum(sel), sum(int(best_dq[g]) for g in range(G) if sel[g]), len(cands)


def sat32(v):
    return max(I32_MIN, min(I32_MAX, v))


def apply_literal(loc_x, loc_y, sel, best_w, radius, mv_ptr, mv_node):
    x, y = [int(v) for v in loc_x], [int(v) for v in loc_y]
    side = 2 * radius + 1
    for g in range(len(sel)):
        w = int(best_w[g])
        if not sel[g] or not 0 <= w < side * side:
            continue
        for n in mv_node[mv_ptr[g]:mv_ptr[g + 1]]:
            if 0 <= n < len(x):
                x[n], y[n] = sat32(x[n] + w // side - radius), sat32(y[n] + w % side - radius)
    return x, y


# ------------------------------------------------------------------------------------------------ the select cases
def chain(up):
    """64 groups, g and g + 1 share row g; the keys increase (up) or decrease along the chain.  Every candidate but the ends
    is beaten by exactly one neighbour until that one is settled: 32 rounds either way."""
    G = 64
    rows = [[r for r in (g - 1, g) if 0 <= r < G - 1] for g in range(G)]
    dq = [-1000 + g if up else -1000 - g for g in range(G)]
    return _case([0] * G, dq, rows, T=G - 1)


def clique():
    """40 groups on one row (and a row of their own each): the smallest key takes it, the 39 others die at once."""
    G = 40
    dq = [-(7 + (g * 17) % 40) for g in range(G)]             # distinct (17 and 40 are coprime)
    return _case([1] * G, dq, [[5, 10 + g] for g in range(G)], T=64)


def ties():
    """Equal best_dq everywhere: g alone decides.  A clique of 6 on row 0, a chain of 7 behind it, two groups on one row."""
    rows = [[0]] * 6 + [[r for r in (k, k + 1)] for k in range(1, 8)] + [[20], [20]]
    return _case([0] * len(rows), [-9] * len(rows), rows, T=21)


def thresholds():
    """No best offset, the centre, best_dq == 0, and best_dq just above, at and just below -min_q; all on rows of their own
    but for the last two, which share one (the one below -min_q has the smaller key)."""
    c, min_q = centre(1), 5
    best_w = [-1, c, 0, 0, 0, 0, 0, 8]
    best_dq = [-50, -50, 0, -4, -5, -6, -5, -6]
    rows = [[0], [1], [2], [3], [4], [5], [6, 7], [7]]
    return _case(best_w, best_dq, rows, T=8, min_q=min_q)


def edges():
    """A candidate without entries; entries outside [0, T) - shared by two candidates, which conflict on nothing -; a group
    whose rows are all outside; a non-candidate on a contested row, which blocks nobody."""
    T = 6
    best_w = [0, 0, 0, 0, 4, 0]
    best_dq = [-3, -8, -8, -2, -99, -1]
    rows = [[], [-1, 2, T], [-1, 3, T + 5], [T, 2 ** 24], [2, 3], [3]]
    return _case(best_w, best_dq, rows, T=T)


def big():
    """best_dq near -2^56 and +2^56: the keys are compared as int64 and the sum is exact."""
    b = 2 ** 56
    best_dq = [-b, -b - 1, -b + 1, b, -b - 1, b - 1, -1]
    rows = [[0, 1], [1, 2], [2, 3], [0], [3, 4], [4], [4, 0]]
    return _case([0] * 7, best_dq, rows, T=5)


def seeded(G=300, T=600, per=(8, 25), seed=11, radius=2):
    """Random rows per group, dense enough that most candidates conflict; some groups are no candidates."""
    rng = np.random.default_rng(seed)
    rows = [sorted(rng.choice(T, int(rng.integers(*per)), replace=False).tolist()) for _ in range(G)]
    W = (2 * radius + 1) ** 2
    best_w = rng.integers(-1, W, G)
    best_dq = np.where(rng.random(G) < 0.1, 0, -rng.integers(1, 50, G))            # few values: many ties
    return _case(best_w, best_dq, rows, T=T, radius=radius, min_q=3)


def wide():
    """More groups than the workgroup has threads: 2500 groups of a few rows."""
    return seeded(G=2500, T=4000, per=(0, 5), seed=12, radius=1)


SELECT_CASES = dict(chain_up=functools.partial(chain, True), chain_down=functools.partial(chain, False), clique=clique, ties=ties,
                    thresholds=thresholds, edges=edges, big=big, seeded=seeded, wide=wide)


@functools.lru_cache(maxsize=None)
def select_case(name):
    """(case, its literal result): built and solved once per name."""
    c = SELECT_CASES[name]()
    return c, select_literal(**c)


# ------------------------------------------------------------------------------------------------ the apply case
def apply_case(radius=1):
    """40 pins, some at the ends of int32; groups that are selected, not selected, selected with a best_w outside [0, W), empty,
    and one with node ids outside the arrays."""
    n, W = 40, (2 * radius + 1) ** 2
    rng = np.random.default_rng(3)
    x, y = rng.integers(-5, 20, n), rng.integers(-5, 20, n)
    x[[0, 1, 2, 3]] = [I32_MAX, I32_MAX - 1, I32_MIN, I32_MIN + 1]
    y[[0, 1, 2, 3]] = [I32_MIN, I32_MIN + 1, I32_MAX, I32_MAX - 1]
    groups = [[0, 2], [1, 3], [4, 5, 6], [7], [8, 9], [], [10, -1, n, 11, 2 ** 30], [12], [13, 14]]
    sel = [1, 1, 0, 1, 1, 1, 1, 1, 2]
    best_w = [W - 1, 0, 0, W, -1, 1, 1, centre(radius), 2]
    ptr = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    return dict(loc_x=x.astype(np.int32), loc_y=y.astype(np.int32), sel=np.asarray(sel, dtype=np.int32), best_w=I64(best_w),
                radius=radius, mv_ptr=ptr, mv_node=I64([v for g in groups for v in g]))
