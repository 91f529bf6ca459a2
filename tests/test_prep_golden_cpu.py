"""The preprocessing fixtures tests/golden/prep_*.npz hold what the reference's own cal_topo_level, find_critical_path,
mask loop (the inline slice of parse_netlist) and norm computed (tests/golden/make_golden_prep.py).  Here, without the
reference tree: oracle/prep_restatement.py, mmft.placement.rasterize_host and PathMasks.from_sparse_coo reproduce them
exactly, and every edge the fixtures were built for is still in them.  tests/test_prep_gpu.py holds the kernels to the same
files."""
import os

import numpy as np
import pytest
import torch

from oracle import prep_restatement as PR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GRAPHS = ('prep_edges', 'prep_random_600')
MAP_SIZES = ((5, 7), (37, 45), (96, 96), (256, 256))
_cache = {}


class Fixture:
    """One graph fixture as plain numpy arrays, with the recorded outputs in the forms the tests compare."""

    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN, name + '.npz'))
        self.names = z['names'].tolist()
        self.n = len(self.names)
        self.src, self.dst, self.kind = z['src'].astype(np.int64), z['dst'].astype(np.int64), z['edge_kind']
        self.pis, self.ends = z['pis'].astype(np.int64), z['endpoints'].astype(np.int64)
        self.level, self.nl = z['level'].astype(np.int64), int(z['num_levels'])
        ptr, flat = z['path_ptr'], z['path_flat']
        self.paths = [flat[ptr[i]:ptr[i + 1]].tolist() for i in range(ptr.shape[0] - 1)]
        self.stop = np.array(['clk' in nm.lower() for nm in self.names])
        self.mask_paths = int(z['mask_paths'])
        assert [tuple(s) for s in z['map_sizes'].tolist()] == list(MAP_SIZES)
        self.pins, self.rows = {}, {}
        for mx, my in MAP_SIZES:
            tag = f'{mx}x{my}'
            self.pins[mx, my] = (z['pin_x_' + tag].astype(np.int64), z['pin_y_' + tag].astype(np.int64))
            bm = np.unpackbits(z['mask_' + tag], axis=1)
            assert bm.shape[0] == self.mask_paths and not bm[:, mx * my:].any()
            self.rows[mx, my] = [np.flatnonzero(r[:mx * my]) for r in bm]

    def level_sets(self):
        return [np.flatnonzero(self.level == l).tolist() for l in range(self.nl)]

    def path_table(self, count=None):
        """(paths [count, maxlen] -1 padded, lens) in the layout prep.trace_critical_paths emits."""
        paths = self.paths[:count]
        maxlen = max(int(self.level.max()) + 1, 1)
        tab = np.full((len(paths), maxlen), -1, dtype=np.int32)
        for i, p in enumerate(paths):
            tab[i, :len(p)] = p
        return tab, np.array([len(p) for p in paths], dtype=np.int32)

    def row_csr(self, size):
        rows = self.rows[size]
        return np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), np.concatenate(rows).astype(np.int64)


def fixture(name):
    if name not in _cache:
        _cache[name] = Fixture(name)
    return _cache[name]


def norm_fixture():
    z = np.load(os.path.join(GOLDEN, 'prep_norm.npz'))
    return torch.from_numpy(z['feat']), torch.from_numpy(z['out']), int(z['start_idx'])


def same_bits(a, b):
    """fp32 tensors equal bit for bit, NaNs only required to sit in the same places."""
    a, b = a.contiguous(), b.contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a.view(torch.int32)[~na], b.view(torch.int32)[~nb])


@pytest.mark.parametrize('name', GRAPHS)
def test_restatement_reproduces_reference_levels_and_paths(name):
    fx = fixture(name)
    suc, pre = PR.adjacency(fx.n, fx.src, fx.dst)
    levels, remaining = PR.cal_topo_level(suc, fx.pis.tolist())
    assert len(levels) == fx.nl and [sorted(s) for s in levels] == fx.level_sets()
    assert sorted(remaining) == np.flatnonzero(fx.level >= 0).tolist()
    node2level = {v: int(fx.level[v]) for v in range(fx.n) if fx.level[v] >= 0}
    assert [PR.find_critical_path(int(e), pre, node2level, fx.stop) for e in fx.ends] == fx.paths


@pytest.mark.parametrize('size', MAP_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('name', GRAPHS)
def test_restatement_and_host_rasteriser_reproduce_reference_mask_rows(name, size):
    from mmft.placement import rasterize_host
    fx = fixture(name)
    (px, py), want = fx.pins[size], [r.tolist() for r in fx.rows[size]]
    loc = {v: (int(px[v]), int(py[v])) for v in range(fx.n)}
    assert PR.path_mask_rows(fx.paths[:fx.mask_paths], loc, *size) == want
    tab, lens = fx.path_table(fx.mask_paths)
    ip, cols = rasterize_host(tab, lens, px, py, *size)
    wip, wcols = fx.row_csr(size)
    assert np.array_equal(ip, wip) and np.array_equal(cols, wcols)


@pytest.mark.parametrize('size', MAP_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('name', GRAPHS)
def test_path_masks_from_the_reference_coo_rows(name, size):
    """The reference hands the rows over as a sparse COO tensor of int64 ones in no particular order."""
    from mmft.fusion import PathMasks
    fx = fixture(name)
    wip, wcols = fx.row_csr(size)
    r = np.repeat(np.arange(fx.mask_paths), np.diff(wip))
    perm = np.random.default_rng(5).permutation(r.shape[0])
    sp = torch.sparse_coo_tensor(torch.from_numpy(np.stack([r[perm], wcols[perm]])),
                                 torch.ones(r.shape[0], dtype=torch.int64), (fx.mask_paths, size[0] * size[1]))
    m = PathMasks.from_sparse_coo(sp, 'cpu')
    assert m.num_paths == fx.mask_paths and m.P == size[0] * size[1]
    assert np.array_equal(m.host_indptr, wip) and np.array_equal(m.host_cols, wcols)


def test_restatement_reproduces_reference_norm():
    feat, out, start = norm_fixture()
    assert same_bits(PR.norm(feat, start), out)


def test_edge_fixture_still_holds_every_case():
    """A regenerated prep_edges must not silently lose a case it was built for."""
    fx = fixture('prep_edges')
    id_ = {nm: i for i, nm in enumerate(fx.names)}
    lv = lambda nm: int(fx.level[id_[nm]])
    path = {fx.names[e]: [fx.names[v] for v in p] for e, p in zip(fx.ends.tolist(), fx.paths)}
    pre = {nm: [fx.names[s] for s, d in zip(fx.src, fx.dst) if fx.names[d] == nm] for nm in fx.names}
    is_clk = lambda nm: 'clk' in nm.lower()
    # frontiers: d is reached over paths of 1, 2 and 3 edges and keeps the last
    assert pre['d'][-3:] == ['a0', 'b', 'c'] and [lv(x) for x in ('a0', 'b', 'c', 'd')] == [0, 1, 2, 3]
    # a primary input reachable from another one keeps its later level; one without successors stays at 0
    pis = [fx.names[p] for p in fx.pis]
    assert 'p2' in pis and lv('p2') == 2 and 'lonely' in pis and lv('lonely') == 0
    assert id_['lonely'] not in fx.src.tolist()
    # removed nodes: unreachable ones that feed a reachable node, ahead of its other predecessors, one of them clk-named
    assert pre['d'][:2] == ['u0', 'u_clk'] and lv('u0') == lv('u_clk') == lv('u1') == lv('iso') == -1
    # a duplicated edge
    pairs = list(zip(fx.src.tolist(), fx.dst.tolist()))
    assert pairs.count((id_['b'], id_['c'])) == 2
    # clk-named predecessor before the matching one: halts (path shorter than the level); after it: goes on
    assert is_clk(pre['f'][0]) and lv(pre['f'][1]) == lv('f') - 1 and path['f'] == ['f'] and len(path['z']) == 2 < lv('z')
    assert is_clk(pre['g'][1]) and lv(pre['g'][0]) == lv('g') - 1 and len(path['g']) == lv('g')
    # clk-named and the only predecessor one level below
    assert [lv(p) == lv('h') - 1 for p in pre['h']] == [False, True] and is_clk(pre['h'][1]) and path['h'] == ['h']
    # upper case
    assert pre['w'][0] == 'reg/CLK' and 'clk' not in pre['w'][0] and lv(pre['w'][1]) == lv('w') - 1 and path['w'] == ['w']
    # endpoints at levels 0, 1, 2 and the deepest; one listed twice; one-pin paths give empty mask rows
    ends = [fx.names[e] for e in fx.ends]
    assert {0, 1, 2, fx.nl - 1} <= {lv(e) for e in ends} and ends.count('g4') == 2 and len(path['g4']) == fx.nl - 1
    for i, e in enumerate(ends):
        if lv(e) <= 1:
            assert len(fx.paths[i]) == 1 and all(len(fx.rows[s][i]) == 0 for s in MAP_SIZES)
    # all in-edges of a node are of one kind, and both kinds occur
    assert all(len({int(k) for k, d in zip(fx.kind, fx.dst) if d == v}) <= 1 for v in range(fx.n)) and set(fx.kind.tolist()) == {0, 1}


def test_random_fixture_reaches_the_second_block():
    fx = fixture('prep_random_600')
    assert fx.n > 256 and len(fx.ends) > 256 and len(set(zip(fx.src.tolist(), fx.dst.tolist()))) < len(fx.src)
    indeg = np.bincount(fx.dst, minlength=fx.n)
    assert (indeg[fx.pis] > 0).any() and (fx.level[fx.pis] > 0).any()          # primary inputs below other primary inputs
    assert sorted(fx.ends.tolist()) == np.flatnonzero(fx.level >= 1).tolist()
    lens = np.array([len(p) for p in fx.paths])
    assert (lens < np.maximum(fx.level[fx.ends], 1)).any() and (lens == np.maximum(fx.level[fx.ends], 1)).any()
    assert 0.05 < fx.stop.mean() < 0.2 and any('CLK' in nm for nm in fx.names) and any('clk' in nm for nm in fx.names)
    assert all(len({int(k) for k in fx.kind[fx.dst == v]}) <= 1 for v in range(fx.n))


@pytest.mark.parametrize('size', MAP_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_mask_fixture_still_holds_every_box_case(size):
    """Every box shape the mask kernel treats differently occurs among the drive-sink pairs of prep_edges at this map size."""
    fx = fixture('prep_edges')
    mx, my = size
    px, py = fx.pins[size]
    seen = set()
    for p in fx.paths:
        for a, b in zip(p[:-1], p[1:]):
            x1, x2, y1, y2 = min(px[a], px[b]), max(px[a], px[b]), min(py[a], py[b]), max(py[a], py[b])
            assert 0 <= x1 and x2 < mx and 0 <= y1 and y2 < my
            full_rows = y1 == 0 and y2 == my - 1
            if (x1, y1) == (x2, y2):
                seen.add('one cell')
            if full_rows and x1 == 0 and x2 == mx - 1:
                seen.add('full map')
            elif full_rows and x2 > x1:
                seen.add('full rows')
            if x2 * my + y2 == mx * my - 1 and not (x1 == 0 and y1 == 0):
                seen.add('ends on the last cell')
            if (x1 * my + y1) % 32 == 31 and y2 > y1:
                seen.add('starts on bit 31')
            if (x1 * my + y1) % 32 == 0 and y2 > y1:
                seen.add('starts on bit 0')
            if ((x1 * my + y2) >> 5) - ((x1 * my + y1) >> 5) >= 2:
                seen.add('whole word inside a row range')
    want = {'one cell', 'full map', 'full rows', 'ends on the last cell', 'starts on bit 31', 'starts on bit 0'}
    if my >= 96:
        want.add('whole word inside a row range')
    assert seen >= want, want - seen
    words = (mx * my + 31) // 32
    assert (mx * my % 32 != 0) == (size in ((5, 7), (37, 45))) and (words > 256) == (mx >= 96)
    if size == (96, 96):                                                        # a row with >= 33 consecutive columns
        def longest_run(r):
            cuts = np.concatenate([[-1], np.flatnonzero(np.diff(r) != 1), [len(r) - 1]])
            return int(np.diff(cuts).max())
        assert any(longest_run(r) >= 33 for r in fx.rows[size] if len(r))


def test_norm_fixture_still_holds_every_column_case():
    feat, out, start = norm_fixture()
    assert feat.shape == (2049, 7) and start == 2 and torch.equal(out[:, :2], feat[:, :2])
    const = [c for c in range(2, 7) if float(feat[:, c].min()) == float(feat[:, c].max())]
    assert len(const) == 1 and torch.isnan(out[:, const[0]]).all()
    nan_col = [c for c in range(7) if torch.isnan(feat[:, c]).any()]
    inf_col = [c for c in range(7) if torch.isinf(feat[:, c]).any()]
    assert len(nan_col) == 1 and torch.isnan(out[:, nan_col[0]]).all() and int(torch.isnan(feat[:, nan_col[0]]).sum()) == 1
    assert len(inf_col) == 1 and int(torch.isnan(out[:, inf_col[0]]).sum()) == 1 and float(out[:, inf_col[0]].nan_to_num().abs().max()) == 0
    tiny = torch.finfo(torch.float32).tiny
    t = [c for c in range(2, 7) if 0 < float(feat[:, c].abs().max()) < 2e-38]
    assert len(t) == 1 and bool(((feat[:, t[0]] == 0) & torch.signbit(feat[:, t[0]])).any())
    d = feat[:, t[0]] - feat[:, t[0]].min()
    assert bool(((d > 0) & (d < tiny)).any())                                  # subnormal numerators: a flush to zero would show
    assert float(out[:, t[0]].min()) == 0.0 and float(out[:, t[0]].max()) == 1.0
    ordinary = [c for c in range(2, 7) if c not in const + nan_col + inf_col + t]
    assert len(ordinary) == 1 and float(out[:, ordinary[0]].min()) == 0.0 and float(out[:, ordinary[0]].max()) == 1.0
