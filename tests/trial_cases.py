"""Shared inputs of test_trial_cpu.py / test_trial_gpu.py: the kernel cases of place_cases.py extended for trial moves, seeded
candidates per case, hand-built incidence tables for expand_candidates and literal restatements of the expansion and of the
reduction.  A plain module: it holds no test."""
import numpy as np

import place_cases as PC

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
MIN_PINS = 80           # every case's pin table is padded to this many pins: a candidate of 64 moves needs distinct nodes


# ------------------------------------------------------------------------------------------------ kernel cases
def tables(case):
    """(path_nodes, path_lens, pin_x, pin_y, repeat_row) of a place_cases.Case, extended by
      - one path [a, b, a] on two existing pins: place_cases gives every path point a pin of its own, so no pin repeats in a
        row there; `repeat_row` is that path's index and its first node the pin that repeats,
      - pins no path holds, up to MIN_PINS and at least two, scattered over and around the map."""
    nodes, lens, px, py = case.arrays()
    rng = np.random.default_rng(len(case.name))
    q = int(np.flatnonzero(np.minimum(lens, case.maxlen) >= 2)[0])
    a, b = int(nodes[q, 0]), int(nodes[q, 1])
    extra = np.full((1, case.maxlen), -1, dtype=np.int64)
    extra[0, :3] = (a, b, a)
    nodes, lens = np.concatenate([nodes, extra]), np.concatenate([lens, [3]])
    pad = max(MIN_PINS - px.shape[0], 2)                                # at least two: candidates() moves the last two
    px = np.concatenate([px, rng.integers(-2, case.map_x + 2, pad)])
    py = np.concatenate([py, rng.integers(-2, case.map_y + 2, pad)])
    return nodes, lens, px.astype(np.int64), py.astype(np.int64), nodes.shape[0] - 1


def live(nodes, lens, q):
    return [int(v) for v in nodes[q, :min(int(lens[q]), nodes.shape[1])]]


def candidates(case):
    """[(tag, nodes, xs, ys)]: the candidates the kernel test runs on `tables(case)`, seeded per case; node ids in the tables'
    numbering, distinct inside a candidate."""
    nodes, lens, px, py, rep = tables(case)
    rng = np.random.default_rng(1000 + len(case.name) + case.map_x)
    mx, my, N = case.map_x, case.map_y, px.shape[0]
    rows = [live(nodes, lens, q) for q in range(nodes.shape[0])]
    longest = max(range(len(rows)), key=lambda q: len(set(rows[q])))
    multi = [q for q in range(len(rows) - 1) if len(set(rows[q])) >= 2]
    out = []
    q = multi[int(rng.integers(len(multi)))]
    n = rows[q][int(rng.integers(len(rows[q])))]
    out.append(('one_cell_x', [n], [int(px[n]) + 1], [int(py[n])]))
    n = rows[q][0]
    out.append(('one_cell_y', [n], [int(px[n])], [int(py[n]) - 1]))
    for j in range(2):
        q = multi[int(rng.integers(len(multi)))]
        n = rows[q][int(rng.integers(len(rows[q])))]
        out.append((f'jump{j}', [n], [int(rng.integers(0, mx))], [int(rng.integers(0, my))]))
    n = rows[multi[0]][0]
    out.append(('off_the_map', [n], [mx + 7], [-5]))
    out.append(('int32_extremes', [n], [I32_MIN], [I32_MAX]))
    out.append(('int32_extremes_other_way', [rows[multi[-1]][-1]], [I32_MAX], [I32_MIN]))
    several = sorted(set(rows[longest]))[:3]
    out.append(('several_of_one_row', several, [int(rng.integers(-1, mx + 1)) for _ in several], [int(rng.integers(-1, my + 1)) for _ in several]))
    out.append(('repeated_in_its_row', [rows[rep][0]], [int(rng.integers(0, mx))], [int(rng.integers(0, my))]))
    first = sorted(set(rows[longest]))[:64]
    fill = [v for v in range(N) if v not in set(first)][:64 - len(first)]
    many = first + fill
    assert len(many) == 64 == len(set(many))
    out.append(('sixty_four', many, [int(v) for v in rng.integers(0, mx, 64)], [int(v) for v in rng.integers(0, my, 64)]))
    out.append(('on_no_row', [N - 1, N - 2], [0, mx - 1], [my - 1, 0]))          # padding pins: no path holds them
    if case.name == 'long_walk_16x16':
        # walk_300 is staged as nodes 0 .. 255, then 255 .. 299: node 255 is read by both stages
        shared = rows[0][255]
        out.append(('shared_by_two_stages', [shared], [(int(px[shared]) + 9) % mx], [(int(py[shared]) + 5) % my]))
        out.append(('both_sides_of_the_stage', [rows[0][254], rows[0][255], rows[0][256]], [0, mx - 1, 3], [my - 1, 0, 2]))
    return out


def moved(px, py, cand):
    """Copies of the pin table with the candidate written in: what update() would leave."""
    x, y = px.copy(), py.copy()
    _, n, xs, ys = cand
    x[n], y[n] = xs, ys
    return x, y


# ------------------------------------------------------------------------------------------------ expansion
def hand_incidence():
    """(path_nodes, path_lens, paths, maxlen, node_off, n_nodes): two designs (5 and 4 nodes, offsets 0 and 5) and a selection
    of six rows that holds every case of the expansion:
      row 0  path 0  [0, 1, 0, 2]   pin 0 twice in one row
      row 1  path 1  [1, 2]         pins 1 and 2 share rows 0 and 1
      row 2  path 2  [3, 1, 2]
      row 3  path 4  [5, 6]         design 1 (table ids 5 .. 8)
      row 4  path 5  [6, 7, 5]
      row 5  path 1  [1, 2]         the same path selected twice
    path 3 ([4, 4]) is not selected: pin 4 is on no selected row.  Pin 8 is on no path at all."""
    maxlen = 4
    rows = [[0, 1, 0, 2], [1, 2, -1, -1], [3, 1, 2, -1], [4, 4, -1, -1], [5, 6, -1, -1], [6, 7, 5, -1]]
    nodes, lens = np.array(rows, dtype=np.int64), np.array([4, 2, 3, 2, 2, 3], dtype=np.int64)
    return nodes, lens, np.array([0, 1, 2, 4, 5, 1], dtype=np.int64), maxlen, np.array([0, 5, 9], dtype=np.int64), 9


def truncated_incidence():
    """A table of maxlen 3 whose path 0 has stored length 7 ([0, 1, 2] and four nodes cut off) next to a full row: the expansion
    must take the row's first maxlen nodes and nothing else."""
    nodes = np.array([[0, 1, 2], [3, 4, 0]], dtype=np.int64)
    return nodes, np.array([7, 3], dtype=np.int64), np.array([0, 1], dtype=np.int64), 3, np.array([0, 5], dtype=np.int64), 5


def expand_literal(path_nodes, path_lens, paths, node_off, pins, cand_ptr):
    """expand_candidates as a plain loop over candidates, rows and pins."""
    maxlen = path_nodes.shape[1]
    pair_ptr, pair_row, pair_cand = [0], [], []
    for k in range(len(cand_ptr) - 1):
        mine = {int(p) + int(node_off) for p in pins[cand_ptr[k]:cand_ptr[k + 1]]}
        for t, q in enumerate(paths):
            row = [int(v) for v in path_nodes[q, :min(int(path_lens[q]), maxlen)]]
            if mine & set(row):
                pair_row.append(t)
                pair_cand.append(k)
        pair_ptr.append(len(pair_row))
    return np.array(pair_ptr, dtype=np.int64), np.array(pair_row, dtype=np.int64), np.array(pair_cand, dtype=np.int64)


# ------------------------------------------------------------------------------------------------ reduction
def reduce_literal(pred_base, required, design_rows, pair_ptr, pair_row, pred_trial):
    """[K + 1][6] of include/mmft_trial.h word by word, except the ORDER of the tns sum (math.fsum: the exact sum, rounded
    once) - the caller compares tns under the bound two fp64 orders can differ by."""
    import math
    F = np.float32
    out = []
    for k in range(len(pair_ptr)):                                     # the last one, k == K: the base
        trial = {} if k == len(pair_ptr) - 1 else {int(pair_row[p]): F(pred_trial[p]) for p in range(pair_ptr[k], pair_ptr[k + 1])}
        n_valid = n_nan = n_viol = 0
        best, terms = None, []
        for r in design_rows:
            r = int(r)
            with np.errstate(invalid='ignore', over='ignore'):
                s = F(F(required[r]) - trial.get(r, F(pred_base[r]))) if 0 <= r < len(pred_base) else F(np.nan)
            if math.isnan(s):
                n_nan += 1
                continue
            s = float(s) + 0.0                                          # -0.0 -> +0.0
            n_valid += 1
            if best is None or (s, r) < best:
                best = (s, r)
            if s < 0:
                n_viol += 1
                terms.append(s)
        out.append((n_valid, n_nan, n_viol, best[0] if best else math.nan, best[1] if best else -1, math.fsum(terms)))
    return np.array(out, dtype=np.float64)
