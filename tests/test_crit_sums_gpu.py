"""Negative-slack sums and TNS shares per pin and per cell, on the GPU: mmft_criticality_sums (include/mmft_crit_sums.h) bitwise
against mmft.criticality.reference_criticality_sums on every case x slack pattern x batch layout of crit_cases and on the
hand-built batch of crit_sums_cases, at three scales, with cells and with pins only; its seven old outputs bitwise against
mmft_criticality on the same inputs; its independence of the rows' order; and Predictor(criticality=dict(sums=True, ...)) eager
and replayed, after update(pin_x, pin_y) and next to report=.  Every comparison is bitwise: the result is made of minima,
integer counts, integer sums, one correctly rounded fp32 division and one correctly rounded fp64 division."""
import functools

import numpy as np
import pytest
import torch

import crit_cases as C
import crit_sums_cases as S
import place_cases as PC
from mmft import criticality as K
from mmft import lib
from mmft import placement as PL
from test_crit_gpu import _designs, _live_models
from test_head_kernels_gpu import I32

pytestmark = pytest.mark.gpu
PINS = ('node_slack', 'node_row', 'node_viol', 'node_crit', 'counts', 'node_nsum', 'design_nsum', 'saturated', 'node_share')
GUARD = 64


# ------------------------------------------------------------------------------------------------ 1. the kernels
@functools.lru_cache(maxsize=None)
def _reference(name, pattern, layout, scale_log2):
    return S.reference(S.hand() if name == 'repeat_8x8' else C.batch(name, pattern, layout), scale_log2)


class _Device:
    """The tables of a batch on the device, output buffers (of the sums and of mmft_criticality) and a workspace with a guard
    behind it."""

    def __init__(self, b, dev, B=None):
        self.N, self.B, self.dev, self.b = b.N, b.B if B is None else B, dev, b
        self.tabs = [I32(a, dev) for a in (b.nodes, b.lens, b.px, b.py)]
        self.bufs = K.CritSumsBuffers(self.N, self.B, b.P, dev)
        self.pins = K.CritSumsBuffers(self.N, self.B, b.P, dev, cells=False)
        self.old = K.CritBuffers(self.N, self.B, b.P, dev)
        self.need = lib.csum('mmft_criticality_sums_workspace_bytes', self.N, self.B, b.P)
        self.ws = torch.empty(self.need + GUARD, dtype=torch.uint8, device=dev)
        assert self.ws.data_ptr() % 8 == 0

    def dirty(self):
        for t in (self.bufs.raw, self.pins.raw, self.old.raw, self.ws):
            t.view(torch.uint8).fill_(0xA5)

    def rows(self, b):
        return (torch.from_numpy(b.pred).to(self.dev), torch.from_numpy(b.required).to(self.dev), I32(b.paths, self.dev),
                None if b.row_design is None else I32(b.row_design, self.dev))

    def run(self, b, scale_log2, cells=True):
        pred, required, paths, rd = self.rows(b)
        bufs = self.bufs if cells else self.pins
        ns, nr, nv, nc, cs, cv, counts, nsum, csum, dsum, sat, nsh, csh = bufs.tensors()
        d, st = lib.stream_args(pred)
        c = self.b
        if cells:
            lib.csum('mmft_criticality_sums', pred, required, self.tabs[0], self.tabs[1], c.maxlen, self.tabs[2], self.tabs[3], c.map_x, c.map_y,
                     paths, rd, b.T, self.N, self.B, ns, nr, nv, nc, cs, cv, counts, scale_log2, nsum, csum, dsum, sat, nsh, csh,
                     self.ws, self.need, d, st)
        else:
            lib.csum('mmft_criticality_sums', pred, required, self.tabs[0], self.tabs[1], c.maxlen, None, None, 0, 0,
                     paths, rd, b.T, self.N, self.B, ns, nr, nv, nc, None, None, counts, scale_log2, nsum, None, dsum, sat, nsh, None,
                     self.ws, lib.csum('mmft_criticality_sums_workspace_bytes', self.N, self.B, 0), d, st)
        got = bufs.host()
        assert bool((self.ws[self.need:] == 0xA5).all()), 'written behind the workspace'
        return got

    def run_old(self, b):
        pred, required, paths, rd = self.rows(b)
        ns, nr, nv, nc, cs, cv, counts = self.old.tensors()
        d, st = lib.stream_args(pred)
        c = self.b
        lib.crit('mmft_criticality', pred, required, self.tabs[0], self.tabs[1], c.maxlen, self.tabs[2], self.tabs[3], c.map_x, c.map_y,
                 paths, rd, b.T, self.N, self.B, ns, nr, nv, nc, cs, cv, counts, self.ws, self.need, d, st)
        return self.old.host()


@pytest.mark.parametrize('name', C.NAMES + ('repeat_8x8',))
def test_sums_equal_the_reference_bitwise(dev, name):
    hand = name == 'repeat_8x8'
    for layout in ('two',) if hand else C.LAYOUTS:
        D = None
        for pattern in ('hand',) if hand else C.PATTERNS:
            b = S.hand() if hand else C.batch(name, pattern, layout)
            D = D or _Device(b, dev)
            for L in S.SCALES:
                ref = _reference(name, pattern, layout, L)
                D.dirty()                                               # outputs and workspace hold 0xA5 bytes
                got = D.run(b, L)
                assert not S.differences(got, ref), (name, pattern, layout, L, S.differences(got, ref))
                again = D.run(b, L)                                     # on the buffers the first call left: stale sums would show
                assert not S.differences(again, ref), (name, pattern, layout, L, 'second call', S.differences(again, ref))
                D.dirty()
                pins = D.run(b, L, cells=False)                         # no cell outputs, no map, no coordinates
                assert all(pins[i] is None for i in (4, 5, 8, 12))
                assert not S.differences(pins, ref, fields=PINS), (name, pattern, layout, L, 'pins only', S.differences(pins, ref, fields=PINS))


@pytest.mark.parametrize('name', C.NAMES)
def test_the_seven_old_outputs_are_those_of_mmft_criticality(dev, name):
    D = _Device(C.batch(name, 'random', 'three'), dev)
    for pattern in C.PATTERNS:
        b = C.batch(name, pattern, 'three')
        D.dirty()
        old = D.run_old(b)
        for L in (0, 30):
            D.dirty()
            new = D.run(b, L)
            assert not C.differences(new[:7], old), (name, pattern, L, C.differences(new[:7], old))


@pytest.mark.parametrize('name', C.NAMES)
def test_the_sums_do_not_depend_on_the_order_of_the_rows(dev, name):
    D = _Device(C.batch(name, 'random', 'three'), dev)
    order_free = ('node_nsum', 'cell_nsum', 'design_nsum', 'saturated', 'cell_share')
    for pattern in ('ties', 'specials', 'random'):
        b = C.batch(name, pattern, 'three')
        ref = _reference(name, pattern, 'three', 20)
        for seed in (1, 2):
            q = C.permuted(b, seed)
            assert not np.array_equal(q.paths, b.paths)
            D.dirty()
            got = D.run(q, 20)
            assert not S.differences(got, ref, fields=order_free), (name, pattern, seed, S.differences(got, ref, fields=order_free))
            # node_share divides by the sum of the design of node_row, a row of the permuted batch: two rows of different designs
            # may tie on a pin's worst slack in these batches (in a real batch a pin belongs to one design)
            assert np.array_equal(S._bits(got[11]), S._bits(S.reference(q, 20)[11])), (name, pattern, seed)


def test_more_rows_than_one_workgroup_combines_and_more_designs_than_it_keeps_in_lds(dev):
    """The designs' sums and saturated rows are combined per 1024 rows, in LDS for the designs below 256: 2 500 rows (three such
    slices, the last one partial) on designs 0, 5, 255, 256 and 299 of 300 (the batch of test_crit_gpu.py)."""
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
    ref = S.reference(b, 20)
    used = [0, 5, 255, 256, 299]
    assert (ref[9][used] > 0).all() and (ref[10][used] > 0).all() and ref[9].sum() == ref[9][used].sum()
    D = _Device(b, dev)
    for _ in range(2):
        D.dirty()
        got = D.run(b, 20)
        assert not S.differences(got, ref), S.differences(got, ref)


def test_many_saturated_rows_and_single_quanta_sum_exactly(dev):
    """5000 saturated rows and 7 rows of one quantum through one pin: 5000 * 2^32 + 7 in the pin's word and in the design's."""
    T = 5007
    slack = np.full(T, -np.inf, dtype=np.float32)
    slack[::716] = np.float32(-(2.0 ** -20))
    b = S.hand()
    q = C.permuted(b, 0)
    q.paths, q.row_design, q.T = np.full(T, 2, dtype=np.int64), np.zeros(T, dtype=np.int64), T       # path 2: pin 4 alone
    q.pred, q.required = -slack, np.zeros(T, dtype=np.float32)
    D = _Device(b, dev)
    D.dirty()
    got = D.run(q, 20)
    assert int(got[7][4]) == 5000 * (1 << 32) + 7 == int(got[9][0]) and got[10].tolist() == [5000, 0] and got[11][4] == 1.0
    assert not S.differences(got, S.reference(q, 20))


def test_bad_arguments_launch_nothing(dev):
    b = C.batch('edges_16x16', 'random', 'one')
    D = _Device(b, dev)
    D.dirty()
    D.run(b, 20)
    torch.cuda.synchronize()
    D.dirty()
    pred, required, paths, _ = D.rows(b)
    ns, nr, nv, nc, cs, cv, counts, nsum, csum, dsum, sat, nsh, csh = D.bufs.tensors()
    d, st = lib.stream_args(pred)
    good = [pred, required, D.tabs[0], D.tabs[1], b.maxlen, D.tabs[2], D.tabs[3], 16, 16, paths, None, b.T, D.N, 1, ns, nr, nv, nc, cs, cv,
            counts, 20, nsum, csum, dsum, sat, nsh, csh, D.ws, D.need, d, st]
    wrong = {'T = 0': {11: 0}, 'N = 0': {12: 0}, 'maxlen = 0': {4: 0}, 'P = 96': {7: 8, 8: 12}, 'null pred': {0: None}, 'null counts': {20: None},
             'scale -1': {21: -1}, 'scale 31': {21: 31}, 'null node_nsum': {22: None}, 'null cell_nsum': {23: None}, 'null design_nsum': {24: None},
             'null saturated': {25: None}, 'null node_share': {26: None}, 'null cell_share': {27: None},
             'cell sums without cells': {18: None, 19: None}, 'cells without cell sums': {23: None, 27: None},
             'odd node_nsum': {22: nsum.data_ptr() + 4}, 'small workspace': {29: D.need - 1}, 'odd workspace': {28: D.ws.data_ptr() + 4},
             'null workspace': {28: None}}
    for what, change in wrong.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        with pytest.raises(RuntimeError, match=r'mmft_criticality_sums failed \(-1\): criticality_sums'):
            lib.csum('mmft_criticality_sums', *args)
        torch.cuda.synchronize()
        assert bool((D.bufs.raw.view(torch.uint8) == 0xA5).all()) and bool((D.ws == 0xA5).all()), what


def test_the_wrapper_launches_what_the_raw_call_launches(dev):
    """mmft.criticality.criticality_sums on PlacedPaths of its own, buffers and workspace from the wrapper."""
    from mmft.synth import synth_design
    d = PC.placed(synth_design(N=512, L=8, tile=32, seed=3, end_frac=0.25), seed=4)
    pp = PL.PlacedPaths([d], np.array([0, d.N]), dev)
    T = min(int(d.path_nodes.shape[0]), 48)
    rng = np.random.default_rng(2)
    pred, required = rng.standard_normal(T).astype(np.float32), np.zeros(T, dtype=np.float32)
    paths = np.arange(T, dtype=np.int64)
    for cells in (True, False):
        out = K.criticality_sums(torch.from_numpy(pred).to(dev), torch.from_numpy(required).to(dev), pp, I32(paths, dev), None, 1,
                                 scale_log2=12, cells=cells)
        got = tuple(None if t is None else t.cpu().numpy() for t in out)
        ref = K.reference_criticality_sums(pred, required, d.path_nodes, d.path_lens, d.pin_x, d.pin_y, pp.map_x, pp.map_y, paths, None, d.N, 1,
                                           scale_log2=12, cells=cells)
        assert not S.differences(got, ref), (cells, S.differences(got, ref))


# ------------------------------------------------------------------------------------------------ 2. Predictor
def _expected(p, designs, pred, scale_log2, pins=None, cells=True):
    """reference_criticality_sums of a predict()'s own output (the construction of test_crit_gpu._expected: required times and
    designs from the endpoint ids, host tables batched by PlacedPaths on the CPU, the masks from Predictor.masks())."""
    node_off = np.asarray(p.batch.node_off)
    design = np.searchsorted(node_off, p.endpoints, side='right') - 1
    required = np.array([designs[d].required_time.reshape(-1)[e - node_off[d]] for d, e in zip(design, p.endpoints)], dtype=np.float32)
    host = PL.PlacedPaths(designs, node_off, 'cpu')
    nodes, lens = host.nodes.numpy(), host.lens.numpy()
    paths = p._sel[1].cpu().numpy().astype(np.int64)
    pins = pins if pins is not None else [(d.pin_x, d.pin_y) for d in designs]
    px, py = np.concatenate([x for x, _ in pins]), np.concatenate([y for _, y in pins])
    masks = None
    if cells:
        parts = [p.masks(i) for i in range(len(designs))]
        ip = np.concatenate([[0]] + [q[0][1:] + off for q, off in zip(parts, np.cumsum([0] + [int(q[0][-1]) for q in parts[:-1]]))])
        masks = (ip, np.concatenate([q[1] for q in parts]))
    m = int(designs[0].map_size)
    ref = K.reference_criticality_sums(pred.cpu().numpy().reshape(-1), required, nodes, lens, px, py, m, m, paths,
                                       design if len(designs) > 1 else None, int(node_off[-1]), len(designs), scale_log2=scale_log2,
                                       cells=cells, masks=masks)
    return ref, design, required


def _same_decoded(got, ref, node_off, m, scale_log2):
    want = K.decode_sums(*ref, node_off=node_off, scale_log2=scale_log2, map_x=m, map_y=m)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w)
        for k in g:
            if isinstance(w[k], np.ndarray):
                assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape
                assert np.array_equal(g[k].view(np.int64 if g[k].dtype == np.float64 else np.int32), w[k].view(np.int64 if w[k].dtype == np.float64 else np.int32)), k
            else:
                assert g[k] == w[k], k


SUM_KEYS = ('node_tns', 'cell_tns', 'tns', 'node_share', 'cell_share', 'saturated')


def test_predictor_sums_eager_replayed_with_a_report_and_moving_pins(dev):
    from mmft.infer import Predictor
    designs = _designs()
    m, L = int(designs[0].map_size), 20
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        plain = Predictor(pmodel, cnn, designs, dev, placement=True, criticality=True)
        p = Predictor(pmodel, cnn, designs, dev, criticality=dict(sums=True, scale_log2=L), placement=True, report=dict(k=8))
        assert isinstance(p._crit.bufs, K.CritSumsBuffers) and isinstance(plain._crit.bufs, K.CritBuffers)
        with pytest.raises(RuntimeError, match='predict'):
            p.criticality()
        node_off = p.batch.node_off
        for call in range(3):                                           # eager, the capturing call, a replay
            y0, (y, ends) = plain.predict(), p.predict()
            assert torch.equal(y, y0[0]) and np.array_equal(ends, y0[1]), call
            ref, design, required = _expected(p, designs, y, L)
            got, old = p.criticality(), plain.criticality()
            _same_decoded(got, ref, node_off, m, L)
            slack = K.reference_slack(y.cpu().numpy().reshape(-1), required)
            for i, r in enumerate(p.report()):
                # without the option: the same keys as ever, and the same values under them
                assert sorted(old[i]) == sorted(set(got[i]) - set(SUM_KEYS)) == sorted(K.FIELDS[:6] + ('n', 'n_nan'))
                assert all(np.array_equal(C._bits(old[i][k]), C._bits(got[i][k])) if isinstance(old[i][k], np.ndarray) else old[i][k] == got[i][k]
                           for k in old[i])
                # the design's TNS next to the report's: every violating row is off by at most half a quantum, the report's
                # fp64 sum by a few ulps - as long as no row hit the cap
                n_viol = int((slack[design == i] < 0).sum())
                assert got[i]['saturated'] == 0 and n_viol == r['violations'] and n_viol > 0
                print(f'call {call} design {i}: tns {got[i]["tns"]!r} report {r["tns"]!r} violating {n_viol}')
                assert abs(got[i]['tns'] - r['tns']) <= n_viol * 2.0 ** -(L + 1) + 1e-12 * abs(r['tns'])
                assert got[i]['tns'] < 0 and got[i]['node_tns'].min() >= got[i]['tns'] and got[i]['cell_tns'].min() >= got[i]['tns']
                share = got[i]['node_share']
                assert share.max() <= 1.0 and ((share > 0) & (share < 1)).any() and (got[i]['cell_share'] > 0).any()
        assert p._replay.graph is not None and p._replay.calls == 3 and p._crit in p._replay.keep and p._crit.placed is p._placed
        one = p.criticality(1)
        assert np.array_equal(one['node_tns'], got[1]['node_tns']) and one['tns'] == got[1]['tns']
        # design 1's pins move: the replayed cell sums follow them, design 0's stay
        before = got
        xy = PC.move(designs[1], seed=75, frac=0.3)
        for q in (plain, p):
            q.update(1, pin_x=xy[0], pin_y=xy[1])
        y0, y = plain.predict()[0], p.predict()[0]
        assert torch.equal(y, y0) and p._replay.calls == 4
        ref, _, _ = _expected(p, designs, y, L, pins=[(designs[0].pin_x, designs[0].pin_y), xy])
        after = p.criticality()
        _same_decoded(after, ref, node_off, m, L)
        assert not np.array_equal(after[1]['cell_tns'], before[1]['cell_tns'])
        assert np.array_equal(after[0]['cell_tns'], before[0]['cell_tns']) and np.array_equal(C._bits(after[0]['cell_share']), C._bits(before[0]['cell_share']))


def test_predictor_sums_pins_only_without_placement_mode_and_eager(dev):
    from mmft.infer import Predictor
    designs = _designs()
    m = int(designs[0].map_size)
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        plain = Predictor(pmodel, cnn, designs, dev)
        p = Predictor(pmodel, cnn, designs, dev, criticality=dict(cells=False, sums=True, scale_log2=30))
        e = Predictor(pmodel, cnn, designs, dev, criticality=dict(sums=True), graphed=False)
        assert p._placed is None and p._crit.placed is not None and e._crit.scale_log2 == 20
        for call in range(3):
            y0, y, ye = plain.predict()[0], p.predict()[0], e.predict()[0]
            assert torch.equal(y, y0) and torch.equal(ye, y0), call
            ref, _, _ = _expected(p, designs, y, 30, cells=False)
            got = p.criticality()
            _same_decoded(got, ref, p.batch.node_off, m, 30)
            assert all(g['cell_tns'] is None and g['cell_share'] is None and g['cell_slack'] is None for g in got)
            ref, _, _ = _expected(e, designs, ye, 20)
            _same_decoded(e.criticality(), ref, e.batch.node_off, m, 20)
        assert p._replay.graph is not None and e._replay is None
