"""Generate tests/golden/prep_*.npz by running the REFERENCE's own preprocessing code (run only where the reference
tree exists, as tests/golden/make_golden.py, whose location of it this script shares):

    python tests/golden/make_golden_prep.py

The reference's parser module does not import here (pyverilog and dgl are absent), and nothing of it is copied: its
syntax tree is read at run time and only these pieces are compiled and executed, unmodified:

* the methods Parser.cal_topo_level and Parser.find_critical_path, against a SimpleNamespace(graph=<networkx DiGraph of
  pin names>, node2level=...): they touch nothing else;
* the seven statements of Parser.parse_netlist from `self.path_masks = th.zeros(...)` through
  `self.path_masks = mask_2` (the mask loop is inline there, it has no function of its own), with self, th, ept2path,
  map_size_x and map_size_y supplied as names; masking == 'critical'.  The result is the reference's sparse COO tensor;
* minMax_scalar and norm of src/train.py.

Before a fixture is written, oracle/prep_restatement.py must give the same result on it: levels and paths equal, mask
rows equal as sorted sets, norm bitwise equal with NaNs in the same places.  That assertion is what pins the restatement;
tests/test_prep_golden_cpu.py and tests/test_prep_gpu.py then read the fixtures only.

Every fixture holds plain arrays.  A graph fixture: names, src / dst in edge insertion order, edge_kind (0 net, 1 cell, one
kind per destination node, as for a real pin), pis, endpoints in timing-path order; level (-1: removed by the reference),
num_levels, path_flat / path_ptr; per map size pin_x / pin_y and the mask rows as np.packbits bitmaps.  The files are
written with fixed zip timestamps, so a second run gives the same bytes.

No listed input was left out: the reference terminated and raised nothing on every one of them.
"""
import ast
import io
import os
import signal
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G                                           # noqa: E402  (sets sys.path; REF = the reference's src/)

from mmft.detrand import det_uniform, det_ints                   # noqa: E402
from oracle import prep_restatement as PR                         # noqa: E402

MAP_SIZES = ((5, 7), (37, 45), (96, 96), (256, 256))
RANDOM_MASK_PATHS = 24


# ----------------------------------------------------------------------------- the reference's code, from its syntax tree
def _tree(fname):
    with open(os.path.join(G.REF, fname)) as f:
        return ast.parse(f.read())


def _compile(nodes, names):
    mod = ast.fix_missing_locations(ast.Module(body=list(nodes), type_ignores=[]))
    ns = dict(names)
    exec(compile(mod, '<reference>', 'exec'), ns)
    return ns


def reference_functions():
    import networkx                                               # noqa: F401  (the graph type the methods expect)
    parser = [n for n in _tree('verilog_parser_asap7.py').body if isinstance(n, ast.ClassDef) and n.name == 'Parser']
    assert len(parser) == 1
    methods = {n.name: n for n in parser[0].body if isinstance(n, ast.FunctionDef)}
    quiet = {'th': torch, 'print': lambda *a, **k: None}
    ns = _compile([methods['cal_topo_level'], methods['find_critical_path']], quiet)
    body = methods['parse_netlist'].body
    text = [ast.unparse(s) for s in body]
    first = [i for i, t in enumerate(text) if t.startswith('self.path_masks = th.zeros(')]
    last = [i for i, t in enumerate(text) if t == 'self.path_masks = mask_2']
    assert len(first) == 1 and len(last) == 1 and last[0] - first[0] + 1 == 7, 'the mask slice of parse_netlist has moved'
    mask_code = compile(ast.fix_missing_locations(ast.Module(body=body[first[0]:last[0] + 1], type_ignores=[])),
                        '<reference mask slice>', 'exec')
    train = {n.name: n for n in _tree('train.py').body if isinstance(n, ast.FunctionDef)}
    tn = _compile([train['minMax_scalar'], train['norm']], {'th': torch})

    def mask_rows(names, paths, end_names, pin_x, pin_y, map_x, map_y):
        """Runs the slice; returns the COO tensor's rows as sorted column arrays."""
        self = types.SimpleNamespace(
            num_paths=len(end_names), masking='critical',
            timing_paths=[types.SimpleNamespace(end=e) for e in end_names],
            pin_loc_map={nm: (0, 0, int(pin_x[i]), int(pin_y[i])) for i, nm in enumerate(names)})
        env = dict(quiet, self=self, ept2path=paths, map_size_x=map_x, map_size_y=map_y)
        exec(mask_code, env)
        sp = self.path_masks
        assert sp.is_sparse and tuple(sp.shape) == (len(end_names), map_x * map_y)
        idx, val = sp._indices().numpy(), sp._values().numpy()
        assert val.dtype == np.int64 and (val == 1).all()
        rows = [np.sort(idx[1][idx[0] == r]) for r in range(len(end_names))]
        assert all((np.diff(r) > 0).all() for r in rows)         # the reference de-duplicates each row itself
        return rows

    return ns['cal_topo_level'], ns['find_critical_path'], mask_rows, tn['norm']


# ----------------------------------------------------------------------------- helpers
def save(name, **arrs):
    """np.load-able .npz with fixed timestamps: the same arrays give the same bytes."""
    path = os.path.join(HERE, name + '.npz')
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrs[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue(), compresslevel=9)
    kb = os.path.getsize(path) / 1024
    assert kb < 100, f'{name}.npz is {kb:.1f} KB'
    print(f'  wrote {name}.npz  ({kb:.1f} KB)')
    return kb


def pack_rows(rows, P):
    bm = np.zeros((len(rows), P), dtype=np.uint8)
    for i, r in enumerate(rows):
        bm[i, r] = 1
    return np.packbits(bm, axis=1)


class Graph:
    def __init__(self, names, edges, pis, ends):
        self.names = list(names)
        assert len(set(self.names)) == len(self.names)
        self.id = {nm: i for i, nm in enumerate(self.names)}
        self.src = np.array([self.id[a] if isinstance(a, str) else a for a, _ in edges], dtype=np.int32)
        self.dst = np.array([self.id[b] if isinstance(b, str) else b for _, b in edges], dtype=np.int32)
        self.pis = np.array([self.id[p] if isinstance(p, str) else p for p in pis], dtype=np.int32)
        self.ends = np.array([self.id[e] if isinstance(e, str) else e for e in ends], dtype=np.int32)
        self.n = len(self.names)
        self.kind = (self.dst % 2).astype(np.uint8)              # one kind per destination node

    def networkx(self):
        import networkx as nx
        g = nx.DiGraph()
        g.add_nodes_from(self.names)
        for s, d in zip(self.src.tolist(), self.dst.tolist()):    # insertion order = predecessors() order
            g.add_edge(self.names[s], self.names[d])
        return g


def run_graph(gr, ref_levels, ref_path):
    """Levels and paths from the reference's methods; the restatement must agree."""
    names = gr.names
    g = gr.networkx()
    self = types.SimpleNamespace(graph=g, node2level={})
    end_names = [names[e] for e in gr.ends.tolist()]
    signal.alarm(120)                                             # a walk that finds no predecessor would spin
    topo = ref_levels(self, {names[p] for p in gr.pis.tolist()}, set(end_names), {e: i for i, e in enumerate(end_names)})
    for i, (nodes, _, _) in enumerate(topo):
        for nd in nodes:
            assert nd not in self.node2level
            self.node2level[nd] = i
    assert set(self.node2level) == set(g.nodes())                # the method removed every other node from the graph
    paths = {e: ref_path(self, e) for e in end_names}
    signal.alarm(0)
    level = np.full(gr.n, -1, dtype=np.int32)
    for nm, l in self.node2level.items():
        level[gr.id[nm]] = l
    id_paths = [[gr.id[nm] for nm in paths[e]] for e in end_names]
    # ---- restatement == reference
    suc, pre = PR.adjacency(gr.n, gr.src, gr.dst)
    levels_r, remaining = PR.cal_topo_level(suc, gr.pis.tolist())
    assert len(levels_r) == len(topo), 'restatement: number of levels'
    lv_r = np.full(gr.n, -1, dtype=np.int32)
    for l, s in enumerate(levels_r):
        lv_r[list(s)] = l
    assert np.array_equal(lv_r, level) and remaining == {gr.id[nm] for nm in self.node2level}, 'restatement: levels'
    node2level = {v: int(level[v]) for v in range(gr.n) if level[v] >= 0}
    is_clk = np.array(['clk' in nm.lower() for nm in names])
    got = [PR.find_critical_path(int(e), pre, node2level, is_clk) for e in gr.ends]
    assert got == id_paths, 'restatement: critical paths'
    return level, len(topo), paths, id_paths


def run_masks(gr, paths, id_paths, rows_n, pins, ref_masks):
    """Per map size the reference's mask rows of the first rows_n timing paths; the restatement must agree."""
    out = {}
    end_names = [gr.names[e] for e in gr.ends.tolist()][:rows_n]
    for (mx, my) in MAP_SIZES:
        px, py = pins(mx, my)
        rows = ref_masks(gr.names, paths, end_names, px, py, mx, my)
        loc = {v: (int(px[v]), int(py[v])) for v in range(gr.n)}
        want = PR.path_mask_rows(id_paths[:rows_n], loc, mx, my)
        assert [r.tolist() for r in rows] == want, f'restatement: mask rows at {mx} x {my}'
        tag = f'{mx}x{my}'
        out['pin_x_' + tag], out['pin_y_' + tag] = px.astype(np.int32), py.astype(np.int32)
        out['mask_' + tag] = pack_rows(rows, mx * my)
    return out


def graph_arrays(gr, level, nl, id_paths):
    ptr = np.zeros(len(id_paths) + 1, dtype=np.int32)
    np.cumsum([len(p) for p in id_paths], out=ptr[1:])
    return dict(names=np.array(gr.names), src=gr.src, dst=gr.dst, edge_kind=gr.kind, pis=gr.pis, endpoints=gr.ends,
                level=level, num_levels=np.int32(nl), path_flat=np.array([v for p in id_paths for v in p], dtype=np.int32),
                path_ptr=ptr, map_sizes=np.array(MAP_SIZES, dtype=np.int32))


# ----------------------------------------------------------------------------- prep_edges
EDGE_NAMES = ('a0', 'a1', 'b', 'c', 'd', 'p2', 'm', 'lonely', 'u0', 'u1', 'u_clk', 'iso', 'e', 'x_clk_buf', 'f', 'g',
              'clkdiv', 'h', 'reg/CLK', 'w', 'z', 'g2', 'g3', 'g4', 's1', 's2', 't', 'q/A', 'q/Y')
EDGE_EDGES = (
    ('u1', 'u0'), ('u0', 'd'), ('u_clk', 'd'),                   # unreachable (one clk-named) into a reachable node, first in d's fan-in
    ('a0', 'b'), ('b', 'c'), ('b', 'c'),                         # a duplicated edge
    ('a0', 'd'), ('b', 'd'), ('c', 'd'),                         # d sits in frontiers 1, 2 and 3
    ('a1', 'm'), ('m', 'p2'),                                    # p2: a primary input reachable from the primary input a1
    ('p2', 'q/A'), ('q/A', 'q/Y'),
    ('d', 'e'), ('a0', 'x_clk_buf'), ('a1', 'reg/CLK'),
    ('x_clk_buf', 'f'), ('e', 'f'),                              # clk-named before the matching predecessor: the walk halts at f
    ('e', 'g'), ('x_clk_buf', 'g'),                              # clk-named after it: the walk goes on through e
    ('e', 'clkdiv'), ('b', 'h'), ('clkdiv', 'h'),                # clk-named and the only predecessor one level below h: halts
    ('reg/CLK', 'w'), ('g', 'w'),                                # upper case counts
    ('f', 'z'),
    ('g', 'g2'), ('g2', 'g3'), ('g3', 'g4'),                     # the deepest level
    ('a1', 's1'), ('s1', 's2'), ('m', 's2'), ('s2', 't'),
)
EDGE_PIS = ('a0', 'a1', 'p2', 'lonely')                          # lonely: a primary input without successors
EDGE_ENDS = ('g4', 'a0', 'b', 'c', 'p2', 'f', 'g', 'h', 'w', 'clkdiv', 'z', 'g4', 'd', 's2', 'lonely', 't', 'q/Y')


def _word_start(mx, my, bit):
    """A cell (x, y) with (x * my + y) % 32 == bit and room for a longer row range to its right: the largest room."""
    best = None
    for x in range(mx):
        for y in range(my - 1):
            if (x * my + y) % 32 == bit and (best is None or my - 1 - y > best[2]):
                best = (x, y, my - 1 - y)
    return best[0], best[1]


def edge_pins(gr):
    def pins(mx, my):
        seed = 9000 + 7 * mx + my
        px, py = det_ints((gr.n,), seed, 0, mx), det_ints((gr.n,), seed + 1, 0, my)

        def put(nm, x, y):
            px[gr.id[nm]], py[gr.id[nm]] = x, y
        put('z', mx // 2, my // 3); put('f', mx // 2, my // 3)                  # a one-cell box (path z, f)
        put('p2', 0, 0); put('m', mx - 1, my - 1)                               # the full map (path p2, m)
        put('s2', 1, 0); put('s1', min(3, mx - 2), my - 1)                      # full rows over several x (path s2, s1)
        put('c', mx - 1, my - 1); put('b', mx - 2, my - 3)                      # a box that ends on the last cell
        x31, y31 = _word_start(mx, my, 31)                                      # a row range that starts on bit 31 of a word
        put('g3', x31, y31); put('g2', x31, min(my - 1, y31 + 40))
        x0, y0 = _word_start(mx, my, 0)                                         # ... and one that starts on bit 0
        put('clkdiv', x0, y0); put('e', x0, min(my - 1, y0 + 70))
        return px, py
    return pins


def golden_edges(ref):
    ref_levels, ref_path, ref_masks, _ = ref
    gr = Graph(EDGE_NAMES, EDGE_EDGES, EDGE_PIS, EDGE_ENDS)
    level, nl, paths, id_paths = run_graph(gr, ref_levels, ref_path)
    arrs = graph_arrays(gr, level, nl, id_paths)
    arrs.update(run_masks(gr, paths, id_paths, len(id_paths), edge_pins(gr), ref_masks))
    return save('prep_edges', mask_paths=np.int32(len(id_paths)), **arrs)


# ----------------------------------------------------------------------------- prep_random_600
def golden_random(ref):
    ref_levels, ref_path, ref_masks, _ = ref
    n, e = 600, 1800
    a, b = det_ints((e,), 601, 0, n), det_ints((e,), 602, 0, n)
    keep = a != b
    src, dst = np.minimum(a, b)[keep], np.maximum(a, b)[keep]   # smaller -> larger id, duplicates kept
    assert len(set(zip(src.tolist(), dst.tolist()))) < src.shape[0]
    clk = det_uniform((n,), 603, 0.0, 1.0) < 0.10
    names = [(f'r{i}/CLK' if i % 2 else f'clk_r{i}') if clk[i] else f'r{i}/Y' for i in range(n)]
    order = np.argsort(det_uniform((n,), 604), kind='stable')
    pis = np.sort(order[:40])                                    # drawn from all nodes, with or without predecessors
    probe = Graph(names, list(zip(src.tolist(), dst.tolist())), pis.tolist(), [])
    suc, _ = PR.adjacency(n, probe.src, probe.dst)
    # which nodes the reference will keep at level >= 1 is a property of the graph alone (reachable from a primary input
    # through at least one edge as the LAST frontier): take them from the reference's own levels, run without endpoints
    level0, _, _, _ = run_graph(probe, ref_levels, ref_path)
    ends = [v for v in range(n) if level0[v] >= 1]
    assert len(ends) > 256 and (np.bincount(dst, minlength=n)[pis] > 0).any()
    gr = Graph(names, list(zip(src.tolist(), dst.tolist())), pis.tolist(), ends)
    level, nl, paths, id_paths = run_graph(gr, ref_levels, ref_path)
    assert np.array_equal(level, level0)
    arrs = graph_arrays(gr, level, nl, id_paths)

    def pins(mx, my):
        seed = 9500 + 7 * mx + my
        return det_ints((n,), seed, 0, mx), det_ints((n,), seed + 1, 0, my)
    arrs.update(run_masks(gr, paths, id_paths, RANDOM_MASK_PATHS, pins, ref_masks))
    return save('prep_random_600', mask_paths=np.int32(RANDOM_MASK_PATHS), **arrs)


# ----------------------------------------------------------------------------- prep_norm
def golden_norm(ref):
    ref_norm = ref[3]
    n, start = 2049, 2                                           # one row into the kernel's second strip of 2048 rows
    f = np.zeros((n, 7), dtype=np.float32)
    f[:, 0] = np.round(det_uniform((n,), 701, -4.0, 4.0) * 8) / 8          # left of start_idx: untouched
    f[:, 1] = det_uniform((n,), 702, 0.0, 50.0)
    f[:, 2] = det_uniform((n,), 703, -3.0, 5.0)                            # ordinary
    f[:, 3] = 2.5                                                          # constant: 0 / 0
    f[:, 4] = det_uniform((n,), 704, -1.0, 1.0); f[1234, 4] = np.nan       # holding a NaN
    f[:, 5] = det_uniform((n,), 705, 0.0, 9.0); f[2048, 5] = np.inf        # holding +inf, in the second strip
    f[:, 6] = (det_uniform((n,), 706, -1.5, 1.5).astype(np.float64) * 1e-38).astype(np.float32)   # subnormal differences
    f[77, 6] = -0.0
    assert np.signbit(f[77, 6]) and (np.abs(f[:, 6]) < np.finfo(np.float32).tiny).any()
    x = torch.from_numpy(f.copy())
    out = ref_norm(x.clone(), start)
    mine = PR.norm(x.clone(), start)
    a, b = out.numpy(), mine.numpy()
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.int32)[~np.isnan(a)], b.view(np.int32)[~np.isnan(b)]), \
        'restatement: norm'
    assert np.isnan(a[:, 3]).all() and np.isnan(a[:, 4]).all() and np.isnan(a[2048, 5]) and (np.delete(a[:, 5], 2048) == 0).all()
    return save('prep_norm', feat=f, out=a, start_idx=np.int32(start))


def main():
    torch.set_num_threads(1)
    ref = reference_functions()
    print('reference: cal_topo_level, find_critical_path, the mask slice of parse_netlist, minMax_scalar / norm extracted')
    total = golden_edges(ref) + golden_random(ref) + golden_norm(ref)
    assert total < 300, total
    print(f'all fixtures written ({total:.1f} KB); oracle/prep_restatement.py agrees with the reference on every one of them')


if __name__ == '__main__':
    main()
