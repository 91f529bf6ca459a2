"""Shared inputs of test_pairs_cpu.py / test_pairs_gpu.py: THE RULE of include/mmft_pairs.h as a literal double loop that also
says why a pair is not one, a seeded set of groups on a small grid with rows of their own, the kernel cases of swap_cases.py
as inputs of the rule, and the tables a device build must equal.  A plain module: it holds no test."""
import numpy as np

import place_cases as C
import swap_cases as WC
from mmft import swap as SW

I64 = WC.I64
I32_MIN, I32_MAX = WC.I32_MIN, WC.I32_MAX
MAX_REACH = 2 ** 31 - 1
KERNEL_CASES = ['single_block_8x8', 'edges_16x16', 'clamped_16x16', 'wide_32x64', 'long_walk_16x16']
SIZES, CLASSES, GRID = (0, 1, 8, 40), (0, 1, 2), 12


def why_not(mv_ptr, mv_node, px, py, reach, klass, a, b):
    """The set of reasons for which (a, b) is no near pair: 'empty', 'anchor', 'size', 'class', 'coincide', 'far'.  Python
    integers: no difference wraps.  An empty set: a near pair."""
    na, nb = [[int(v) for v in mv_node[mv_ptr[g]:mv_ptr[g + 1]]] for g in (a, b)]
    if not na or not nb:
        return {'empty'}
    if not (0 <= na[0] < len(px) and 0 <= nb[0] < len(px)):
        return {'anchor'}
    out = set()
    if len(na) + len(nb) > 64:
        out.add('size')
    if klass is not None and int(klass[a]) != int(klass[b]):
        out.add('class')
    d = max(abs(int(px[na[0]]) - int(px[nb[0]])), abs(int(py[na[0]]) - int(py[nb[0]])))
    if d == 0:
        out.add('coincide')
    if d > int(reach):
        out.add('far')
    return out


def near_literal(mv_ptr, mv_node, px, py, reach, klass=None):
    """(pair_a, pair_b, {(a, b): reasons} of every pair a < b that is none) by a literal double loop."""
    G = len(mv_ptr) - 1
    pa, pb, no = [], [], {}
    for a in range(G):
        for b in range(a + 1, G):
            why = why_not(mv_ptr, mv_node, px, py, reach, klass, a, b)
            if why:
                no[(a, b)] = why
            else:
                pa.append(a)
                pb.append(b)
    return I64(pa), I64(pb), no


def seeded(seed, G=257, rows=40):
    """G groups whose anchors lie on a GRID x GRID grid, sizes from SIZES, classes from CLASSES; a group's other pins lie
    anywhere; every pin belongs to one group.  Each non-empty group lies on up to six of `rows` rows (some on none), ascending,
    each once.  Returns dict(mv_ptr, mv_node, px, py, klass, grow_ptr, grow_row, T)."""
    rng = np.random.default_rng(seed)
    size = rng.choice(SIZES, G)
    mv_ptr = I64(np.concatenate([[0], np.cumsum(size)]))
    M = int(mv_ptr[-1])
    mv_node = I64(rng.permutation(M + 3)[:M])                  # three pins of no group
    px, py = rng.integers(-3, 40, M + 3).astype(np.int32), rng.integers(-3, 40, M + 3).astype(np.int32)
    has = size > 0
    anchors = mv_node[mv_ptr[:-1][has]]
    px[anchors], py[anchors] = rng.integers(0, GRID, anchors.shape[0]), rng.integers(0, GRID, anchors.shape[0])
    klass = rng.choice(CLASSES, G).astype(np.int64)
    lists = [np.sort(rng.choice(rows, int(rng.integers(0, 7)), replace=False)) if s else np.zeros(0, dtype=np.int64) for s in size]
    grow_ptr = I64(np.concatenate([[0], np.cumsum([len(v) for v in lists])]))
    grow_row = I64(np.concatenate(lists)) if lists else I64([])
    return dict(mv_ptr=mv_ptr, mv_node=mv_node, px=px, py=py, klass=klass, grow_ptr=grow_ptr, grow_row=grow_row, T=rows)


def kernel_case(name):
    """The groups of swap_cases on a kernel case as inputs of the rule: every path selected, some twice, as test_swap_cpu.py
    selects them."""
    c = C.CASES[name]
    nodes, lens, px, py, far, mate, twin = WC.tables(c)
    rng = np.random.default_rng(5)
    paths = np.concatenate([rng.permutation(nodes.shape[0]), rng.integers(0, nodes.shape[0], 3)])
    grow_ptr, grow_row, _, mv_ptr, mv_node = WC.plan(c, paths)
    tags = [g[0] for g in WC.groups(c)]
    return dict(mv_ptr=mv_ptr, mv_node=mv_node, px=px, py=py, klass=None, grow_ptr=grow_ptr, grow_row=grow_row, T=paths.shape[0],
                tags=tags, far=far, mate=mate, twin=twin)


def layout(pair_a, pair_b, tables):
    """The int32 words of a swap plan: pair_a | pair_b | prow_ptr | prow_row | prow_pair | sel_ptr | sel_row."""
    return np.concatenate([np.asarray(v).astype(np.int32) for v in (pair_a, pair_b, *tables)])


def expected(case, pair_a, pair_b):
    """(the seven tables int64, the words of the plan) of a case on the given pairs, through swap.pair_tables."""
    tabs = SW.pair_tables(case['grow_ptr'], case['grow_row'], pair_a, pair_b, case['T'])
    return (pair_a, pair_b, *tabs), layout(pair_a, pair_b, tabs)
