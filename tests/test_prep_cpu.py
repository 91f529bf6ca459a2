"""The preprocessing restatement (oracle/prep_restatement.py) is pinned to the reference's own functions by the fixtures
of tests/test_prep_golden_cpu.py; these checks tie it to the definitions as well: longest-path levels by brute force, path
validity, mask rows as explicit unions of rectangles."""
import numpy as np
import torch

from oracle import prep_restatement as PR


def random_dag(n, e, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, size=e)
    b = rng.integers(0, n, size=e)
    keep = a != b
    src, dst = np.minimum(a, b)[keep], np.maximum(a, b)[keep]           # edges go from the smaller to the larger id
    pairs = sorted(set(zip(src.tolist(), dst.tolist())), key=lambda p: rng.random())
    src = np.array([p[0] for p in pairs], dtype=np.int64)
    dst = np.array([p[1] for p in pairs], dtype=np.int64)
    return src, dst


def test_levels_are_longest_paths_and_paths_descend_one_level():
    n = 300
    src, dst = random_dag(n, 900, 1)
    suc, pre = PR.adjacency(n, src, dst)
    indeg = np.bincount(dst, minlength=n)
    pis = [v for v in range(n) if indeg[v] == 0 and suc[v]][:20]
    levels, remaining = PR.cal_topo_level(suc, pis)
    # brute force: longest path from any PI (ids are a topological order by construction)
    best = np.full(n, -1)
    best[pis] = 0
    for v in range(n):
        if best[v] >= 0:
            for w in suc[v]:
                best[w] = max(best[w], best[v] + 1)
    node2level = {}
    for l, s in enumerate(levels):
        for v in s:
            assert v not in node2level
            node2level[v] = l
    assert set(node2level) == remaining == {v for v in range(n) if best[v] >= 0}
    assert all(node2level[v] == best[v] for v in node2level)
    ends = [v for v in node2level if node2level[v] >= 3][:25]
    for e in ends:
        p = PR.find_critical_path(e, pre, node2level)
        assert p[0] == e and len(p) == node2level[e]                    # stops at level 1 (while cur_level >= 2)
        assert all(node2level[p[i + 1]] == node2level[p[i]] - 1 and p[i + 1] in pre[p[i]] for i in range(len(p) - 1))


def test_mask_rows_and_norm():
    rng = np.random.default_rng(3)
    loc = {v: (int(rng.integers(0, 12)), int(rng.integers(0, 9))) for v in range(40)}
    paths = [[3, 7, 9], [5], [1, 2, 3, 4, 5, 6]]
    rows = PR.path_mask_rows(paths, loc, 12, 9)
    for p, r in zip(paths, rows):
        cells = set()
        for a, b in zip(p[:-1], p[1:]):
            for x in range(min(loc[a][0], loc[b][0]), max(loc[a][0], loc[b][0]) + 1):
                for y in range(min(loc[a][1], loc[b][1]), max(loc[a][1], loc[b][1]) + 1):
                    cells.add(x * 9 + y)
        assert r == sorted(cells)
    assert rows[1] == []
    f = torch.randn(50, 5)
    g = PR.norm(f, 2)
    assert torch.equal(g[:, :2], f[:, :2])
    assert float(g[:, 2:].min()) == 0.0 and float(g[:, 2:].max()) == 1.0
