"""Criticality per pin and per map cell, on the GPU: mmft_criticality (include/mmft_crit.h) bitwise against
mmft.criticality.reference_criticality on every case x slack pattern x batch layout of crit_cases, its independence of the
rows' order, and Predictor(criticality=...) next to report=, placement=True and incremental=True.  Every comparison is bitwise:
the result is made of minima, integer counts and one correctly rounded fp32 division."""
import functools

import numpy as np
import pytest
import torch

import crit_cases as C
import place_cases as PC
from mmft import criticality as K
from mmft import lib
from mmft import placement as PL
from test_head_kernels_gpu import I32
from test_infer_gpu import _models

pytestmark = pytest.mark.gpu
PINS = ('node_slack', 'node_row', 'node_viol', 'node_crit', 'counts')
GUARD = 64


# ------------------------------------------------------------------------------------------------ 1. the kernel
@functools.lru_cache(maxsize=None)
def _reference(name, pattern, layout):
    return C.reference(C.batch(name, pattern, layout))


class _Device:
    """The tables of a case on the device, output buffers and a workspace with a guard behind it."""

    def __init__(self, name, B, dev):
        nodes, lens, px, py = C.tables(name)
        c = PC.CASES[name]
        self.c, self.N, self.B, self.dev = c, int(px.shape[0]), B, dev
        self.tabs = [I32(a, dev) for a in (nodes, lens, px, py)]
        self.bufs = K.CritBuffers(self.N, B, c.P, dev)
        self.pins = K.CritBuffers(self.N, B, c.P, dev, cells=False)
        self.need = lib.crit('mmft_criticality_workspace_bytes', self.N, B, c.P)
        self.ws = torch.empty(self.need + GUARD, dtype=torch.uint8, device=dev)
        assert self.ws.data_ptr() % 8 == 0

    def dirty(self):
        for t in (self.bufs.raw, self.pins.raw, self.ws):
            t.view(torch.uint8).fill_(0xA5)

    def run(self, b, cells=True):
        pred, required = torch.from_numpy(b.pred).to(self.dev), torch.from_numpy(b.required).to(self.dev)
        paths = I32(b.paths, self.dev)
        rd = None if b.row_design is None else I32(b.row_design, self.dev)
        bufs = self.bufs if cells else self.pins
        ns, nr, nv, nc, cs, cv, counts = bufs.tensors()
        d, st = lib.stream_args(pred)
        c = self.c
        if cells:
            lib.crit('mmft_criticality', pred, required, self.tabs[0], self.tabs[1], c.maxlen, self.tabs[2], self.tabs[3], c.map_x, c.map_y,
                     paths, rd, b.T, self.N, self.B, ns, nr, nv, nc, cs, cv, counts, self.ws, self.need, d, st)
        else:
            lib.crit('mmft_criticality', pred, required, self.tabs[0], self.tabs[1], c.maxlen, None, None, 0, 0,
                     paths, rd, b.T, self.N, self.B, ns, nr, nv, nc, None, None, counts, self.ws,
                     lib.crit('mmft_criticality_workspace_bytes', self.N, self.B, 0), d, st)
        got = bufs.host()
        assert bool((self.ws[self.need:] == 0xA5).all()), 'written behind the workspace'
        return got


@pytest.mark.parametrize('name', C.NAMES)
def test_criticality_equals_the_reference_bitwise(dev, name):
    for layout in C.LAYOUTS:
        D = _Device(name, C.designs(name, layout)[1], dev)
        for pattern in C.PATTERNS:
            b = C.batch(name, pattern, layout)
            ref = _reference(name, pattern, layout)
            D.dirty()                                                   # outputs and workspace hold 0xA5 bytes
            got = D.run(b)
            assert not C.differences(got, ref), (name, pattern, layout, C.differences(got, ref))
            again = D.run(b)                                            # on the buffers the first call left: stale keyed words would show
            assert not C.differences(again, ref), (name, pattern, layout, 'second call', C.differences(again, ref))
            D.dirty()
            pins = D.run(b, cells=False)                                # no cell outputs, no map, no coordinates
            assert pins[4] is None and pins[5] is None
            assert not C.differences(pins, ref, fields=PINS), (name, pattern, layout, 'pins only', C.differences(pins, ref, fields=PINS))


@pytest.mark.parametrize('name', C.NAMES)
def test_the_result_does_not_depend_on_the_order_of_the_rows(dev, name):
    D = _Device(name, 3, dev)
    for pattern in ('ties', 'specials', 'random'):
        b = C.batch(name, pattern, 'three')
        ref = _reference(name, pattern, 'three')
        for seed in (1, 2):
            q = C.permuted(b, seed)
            assert not np.array_equal(q.paths, b.paths)
            D.dirty()
            got = D.run(q)
            same = ('node_slack', 'node_viol', 'node_crit', 'cell_slack', 'cell_viol', 'counts')
            assert not C.differences(got, ref, fields=same), (name, pattern, seed, C.differences(got, ref, fields=same))
            assert np.array_equal(got[1], C.reference(q)[1])            # node_row: rows of the permuted batch


def test_more_rows_than_one_workgroup_combines_and_more_designs_than_it_keeps_in_lds(dev):
    """The designs' minima and counts are combined per 1024 rows, in LDS for the designs below 256: 2 500 rows (three such
    slices, the last one partial) on designs 0, 5, 255, 256 and 299 of 300."""
    name = 'seeded_16x16'
    parts = [C.batch(name, pattern, 'one') for pattern in ('random', 'specials', 'ties')] * 10
    rng = np.random.default_rng(8)
    b = C.permuted(C.batch(name, 'random', 'one'), 0)
    b.paths = np.concatenate([p.paths for p in parts])
    b.T = b.paths.shape[0]
    b.pred = np.concatenate([p.pred for p in parts]) + rng.integers(-2, 3, b.T).astype(np.float32) * np.float32(0.25)
    b.required = np.concatenate([p.required for p in parts])
    b.row_design, b.B = np.array([0, 5, 255, 256, 299])[rng.integers(0, 5, b.T)], 300
    assert b.T > 2 * 1024 and b.T % 1024
    ref = C.reference(b)
    assert (ref[6][[0, 5, 255, 256, 299], 0] > 0).all() and ref[6][:, 1].sum() > 0 and ref[6].sum() == b.T
    D = _Device(name, b.B, dev)
    for _ in range(2):
        D.dirty()
        got = D.run(b)
        assert not C.differences(got, ref), C.differences(got, ref)


def test_bad_arguments_launch_nothing(dev):
    name = 'edges_16x16'
    D = _Device(name, 1, dev)
    b = C.batch(name, 'random', 'one')
    D.dirty()
    D.run(b)
    torch.cuda.synchronize()
    D.dirty()
    pred, required, paths = torch.from_numpy(b.pred).to(dev), torch.from_numpy(b.required).to(dev), I32(b.paths, dev)
    ns, nr, nv, nc, cs, cv, counts = D.bufs.tensors()
    d, st = lib.stream_args(pred)
    good = [pred, required, D.tabs[0], D.tabs[1], D.c.maxlen, D.tabs[2], D.tabs[3], 16, 16, paths, None, b.T, D.N, 1, ns, nr, nv, nc, cs, cv,
            counts, D.ws, D.need, d, st]
    wrong = {'T = 0': {11: 0}, 'N = 0': {12: 0}, 'B = 0': {13: 0}, 'maxlen = 0': {4: 0}, 'P = 96': {7: 8, 8: 12}, 'P > 65536': {7: 512, 8: 256},
             'null pred': {0: None}, 'null nodes': {2: None}, 'null loc_x': {5: None}, 'null node_crit': {17: None}, 'null counts': {20: None},
             'cell_slack alone': {19: None}, 'cell_viol alone': {18: None}, 'small workspace': {22: D.need - 1},
             'odd workspace': {21: D.ws.data_ptr() + 4}, 'null workspace': {21: None}}
    for what, change in wrong.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        with pytest.raises(RuntimeError, match=r'mmft_criticality failed \(-1\): criticality'):
            lib.crit('mmft_criticality', *args)
        torch.cuda.synchronize()
        assert bool((D.bufs.raw.view(torch.uint8) == 0xA5).all()) and bool((D.ws == 0xA5).all()), what


# ------------------------------------------------------------------------------------------------ 2. Predictor
def _designs():
    from mmft.synth import synth_design
    return [PC.placed(synth_design(N=n, L=12, tile=32, seed=810 + i, end_frac=0.25), seed=70 + i) for i, n in enumerate((2048, 1536))]


def _live_models(designs, dev, **kw):
    """test_infer_gpu's models with the U-Net's last bias raised (a feature map that is not all zero: the masks matter to the
    predictions), and required times at the median prediction: about half of the endpoints violate."""
    from mmft.infer import Predictor
    pmodel, cnn = _models(designs, dev)
    with torch.no_grad():
        cnn.outc.conv[0].bias.fill_(2.0)
    median = float(Predictor(pmodel, cnn, designs, dev, graphed=False).predict()[0].median())
    for d in designs:
        d.required_time[:] = median
    return pmodel, cnn


def _expected(p, designs, pred, pins=None, cells=True):
    """reference_criticality of a predict()'s own output: required times and designs from the endpoint ids, the path of each
    row checked against its endpoint, host tables batched by PlacedPaths on the CPU, the masks from Predictor.masks()."""
    node_off = np.asarray(p.batch.node_off)
    design = np.searchsorted(node_off, p.endpoints, side='right') - 1
    required = np.array([designs[d].required_time.reshape(-1)[e - node_off[d]] for d, e in zip(design, p.endpoints)], dtype=np.float32)
    host = PL.PlacedPaths(designs, node_off, 'cpu')
    nodes, lens = host.nodes.numpy(), host.lens.numpy()
    paths = p._sel[1].cpu().numpy().astype(np.int64)
    has_pins = lens[paths] > 0
    assert has_pins.any() and (nodes[paths[has_pins], 0] == p.endpoints[has_pins]).all()          # a path starts at its endpoint
    pins = pins if pins is not None else [(d.pin_x, d.pin_y) for d in designs]
    px, py = np.concatenate([x for x, _ in pins]), np.concatenate([y for _, y in pins])
    masks = None
    if cells:
        parts = [p.masks(i) for i in range(len(designs))]
        ip = np.concatenate([[0]] + [q[0][1:] + off for q, off in zip(parts, np.cumsum([0] + [int(q[0][-1]) for q in parts[:-1]]))])
        masks = (ip, np.concatenate([q[1] for q in parts]))
    m = int(designs[0].map_size)
    ref = K.reference_criticality(pred.cpu().numpy().reshape(-1), required, nodes, lens, px, py, m, m, paths,
                                  design if len(designs) > 1 else None, int(node_off[-1]), len(designs), cells=cells, masks=masks)
    if cells:                                                           # ... and those masks are the rule's, on these pins
        assert not C.differences(ref, K.reference_criticality(pred.cpu().numpy().reshape(-1), required, nodes, lens, px, py, m, m, paths,
                                                              design if len(designs) > 1 else None, int(node_off[-1]), len(designs)))
    return ref, design, required


def _same_decoded(got, ref, node_off, m):
    want = K.decode(*ref, node_off=node_off, map_x=m, map_y=m)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w)
        for k in g:
            if isinstance(w[k], np.ndarray):
                assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape
                assert np.array_equal(C._bits(g[k]), C._bits(w[k])), k
            else:
                assert g[k] == w[k], k


def test_predictor_criticality_with_a_report_and_moving_pins(dev):
    from mmft.infer import Predictor
    designs = _designs()
    m = int(designs[0].map_size)
    assert m >= 16 and designs[0].N != designs[1].N
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        plain = Predictor(pmodel, cnn, designs, dev, placement=True)
        p = Predictor(pmodel, cnn, designs, dev, criticality=True, placement=True, report=dict(k=8))
        with pytest.raises(RuntimeError, match='predict'):
            p.criticality()
        with pytest.raises(RuntimeError, match='no criticality'):
            plain.criticality()
        node_off = p.batch.node_off
        for call in range(3):                                           # eager, the capturing call, a replay
            y0, (y, ends) = plain.predict(), p.predict()
            assert torch.equal(y, y0[0]) and np.array_equal(ends, y0[1]), call          # what it predicts without the option, bitwise
            ref, design, required = _expected(p, designs, y)
            got = p.criticality()
            _same_decoded(got, ref, node_off, m)
            slack = K.reference_slack(y.cpu().numpy().reshape(-1), required)
            for i, r in enumerate(p.report()):                          # the report's WNS is the w of the design
                assert r['wns'] == float(slack[design == i].min()) and r['n'] == got[i]['n'] and r['n_nan'] == got[i]['n_nan'] == 0
                crit = got[i]['node_crit']
                assert crit.max() <= 1.0 and ((crit > 0) & (crit < 1)).any() and (got[i]['node_slack'][crit == 1.0] == np.float32(r['wns'])).all()
                assert (got[i]['cell_viol'] > 0).any() and got[i]['cell_slack'].min() >= np.float32(r['wns'])
        assert p._replay.graph is not None and p._replay.calls == 3 and p._crit in p._replay.keep and p._crit.placed is p._placed
        one = p.criticality(1)
        assert np.array_equal(one['node_slack'], got[1]['node_slack']) and one['n'] == got[1]['n']
        with pytest.raises(IndexError):
            p.criticality(2)
        # design 1's pins move: the replayed cell maps follow them, design 0's stay
        before = got
        xy = PC.move(designs[1], seed=75, frac=0.3)
        for q in (plain, p):
            q.update(1, pin_x=xy[0], pin_y=xy[1])
        y0, y = plain.predict()[0], p.predict()[0]
        assert torch.equal(y, y0) and p._replay.calls == 4
        ref, _, _ = _expected(p, designs, y, pins=[(designs[0].pin_x, designs[0].pin_y), xy])
        after = p.criticality()
        _same_decoded(after, ref, node_off, m)
        assert not np.array_equal(after[1]['cell_viol'], before[1]['cell_viol'])
        # design 0: the same masks; its predictions did not move either (its own image, its own netlist), so the maps are equal
        assert np.array_equal(after[0]['cell_viol'], before[0]['cell_viol']) and \
            np.array_equal(C._bits(after[0]['cell_slack']), C._bits(before[0]['cell_slack']))


def test_predictor_criticality_without_placement_mode_and_next_to_incremental_sweeps(dev):
    from mmft.infer import Predictor
    designs = _designs()
    m = int(designs[0].map_size)
    rng = np.random.default_rng(5)
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        plain = Predictor(pmodel, cnn, designs, dev)
        p = Predictor(pmodel, cnn, designs, dev, criticality=dict(cells=False))
        assert p._placed is None and p._crit.placed is not None
        for call in range(3):
            y0, y = plain.predict()[0], p.predict()[0]
            assert torch.equal(y, y0), call
            ref, _, _ = _expected(p, designs, y, cells=False)
            got = p.criticality()
            _same_decoded(got, ref, p.batch.node_off, m)
            assert all(g['cell_slack'] is None and g['cell_viol'] is None for g in got) and sum(g['n'] for g in got) == y.numel()
        xy = PC.move(designs[0], seed=76, frac=0.3)
        with pytest.raises(ValueError, match='placement=True'):
            p.update(0, pin_x=xy[0], pin_y=xy[1])
        # incremental sweeps and the fan-in cone next to it: after a sparse edit, the criticality of the new predictions
        q = Predictor(pmodel, cnn, designs, dev, criticality=True, incremental=True, cone=True)
        for call in range(3):
            y = q.predict()[0]
            assert torch.equal(y, y0), call
        before = y.clone()
        rows = np.sort(rng.permutation(designs[0].N)[:40]).astype(np.int64)
        new = (designs[0].cell_feat[rows] + rng.standard_normal((40, designs[0].cell_feat.shape[1]))).astype(np.float32)
        q.update(0, cell_feat=new, rows=rows)
        y = q.predict()[0]
        assert q.incremental_active and q._replay.graph is not None and not torch.equal(y, before)
        ref, _, _ = _expected(q, designs, y)
        _same_decoded(q.criticality(), ref, q.batch.node_off, m)


def test_predictor_criticality_refusals(dev):
    from mmft.infer import Predictor
    from mmft.synth import synth_design
    from mmft.train import build_models
    designs = _designs()
    bare = synth_design(N=1536, L=12, tile=32, seed=811, end_frac=0.25)
    pmodel, cnn = _models(designs, dev)
    with pytest.raises(ValueError, match='design 1 carries no placement data'):
        Predictor(pmodel, cnn, [designs[0], bare], dev, criticality=True)
    with pytest.raises(ValueError, match='criticality='):
        Predictor(pmodel, cnn, designs, dev, criticality=dict(cells=True, k=4))
    two, cnn2 = build_models(map_size=designs[0].map_size, device=dev, seed=19, nlabels=2)
    with pytest.raises(ValueError, match='regression'):
        Predictor(two, cnn2, designs, dev, criticality=True)
    p = Predictor(pmodel, cnn, designs, dev)
    with pytest.raises(RuntimeError, match='no criticality'):
        p.criticality()
    p = Predictor(pmodel, cnn, designs, dev, criticality=True)
    with pytest.raises(RuntimeError, match='predict'):
        p.criticality()
