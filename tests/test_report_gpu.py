"""The timing report on the GPU: mmft_timing_report (include/mmft_report.h, csrc/report.hip) against mmft.report.reference_report
on the inputs of report_cases.py - exactly, TNS within the fp64 summation bound - and its users, Predictor(report=) and
evaluate.timing_report."""
import functools

import numpy as np
import pytest
import torch

import report_cases as C
from mmft import lib
from mmft import report as R

pytestmark = pytest.mark.gpu

INT_FILL = 0x7fffffff
NAN_FILL = 0x7ff8dead00000000             # a NaN the kernel does not write: a stale wns is told from a written one


def _hist(nbins):
    return (C.HIST_LO, C.HIST_HI, nbins) if nbins else None


@functools.lru_cache(maxsize=None)
def _layout():
    return C.layout()


@functools.lru_cache(maxsize=None)
def _host(name):
    return C.regime(name)


@functools.lru_cache(maxsize=None)
def _reference(name, k, nbins):
    """Computed once per case and shared; nothing writes to it."""
    pred, required = _host(name)
    _, ptr, rows = _layout()
    ref = R.reference_report(pred, required, ptr, rows, k, _hist(nbins))
    return ref, C.tns_bound(ref[0], pred, required, ptr, rows)


@functools.lru_cache(maxsize=None)
def _device(name, dev):
    pred, required = _host(name)
    _, ptr, rows = _layout()
    return tuple(torch.from_numpy(a).to(dev) for a in (pred, required, ptr, rows))


def _filled(k, nbins, dev, B=C.B):
    """Output buffers pre-filled with NaN / 0x7fffffff."""
    bufs = R.ReportBuffers(B, k, _hist(nbins), dev)
    s, wr, ws, h = bufs.tensors()
    s.view(torch.int64).fill_(NAN_FILL)
    wr.fill_(INT_FILL)
    ws.fill_(float('nan'))
    if h is not None:
        h.fill_(INT_FILL)
    return bufs


def _workspace(k, nbins, dev, byte=0xAB, T=C.T, B=C.B):
    need = R.workspace_bytes(T, B, k, _hist(nbins))
    return torch.full(((need + 7) // 8 * 8,), byte, dtype=torch.uint8, device=dev)


def _check(got, name, k, nbins):
    ref, bound = _reference(name, k, nbins)
    s = got[0]
    print(f'{name} k={k} nbins={nbins}: tns got {s[:, 5].tolist()} ref {ref[0][:, 5].tolist()} bound {bound.tolist()}')
    assert C.same_report(got, ref, tns_exact=False)
    for b in range(C.B):
        if np.isfinite(ref[0][b, 5]):
            assert abs(s[b, 5] - ref[0][b, 5]) <= bound[b], (b, s[b, 5], ref[0][b, 5], bound[b])
        else:
            assert s[b, 5] == ref[0][b, 5], b
    assert not (s.view(np.int64) == NAN_FILL).any() and not np.isnan(got[2]).any()            # every element was written


@pytest.mark.parametrize('nbins', C.NBINS)
@pytest.mark.parametrize('k', C.KS)
@pytest.mark.parametrize('name', C.REGIMES)
def test_report_equals_the_reference(dev, name, k, nbins):
    pred, required, ptr, rows = _device(name, dev)
    bufs, ws = _filled(k, nbins, dev), _workspace(k, nbins, dev)
    out = R.timing_report(pred, required, ptr, rows, k, _hist(nbins), out=bufs.tensors(), workspace=ws)
    assert out[0].data_ptr() == bufs.tensors()[0].data_ptr() and (out[3] is None) == (nbins == 0)
    first = bufs.host()[0]
    _check(first, name, k, nbins)
    assert int(ws[:4 * C.B].view(torch.int32).abs().sum()) == 0                                # the designs' counters
    # over the stale scratch and counters: the same bits, the counters zero again
    again = _filled(k, nbins, dev)
    R.timing_report(pred, required, ptr, rows, k, _hist(nbins), out=again.tensors(), workspace=ws)
    assert C.same_report(again.host()[0], first) and int(ws[:4 * C.B].view(torch.int32).abs().sum()) == 0
    # other garbage in the workspace: the part results are not read before they are written
    other = _filled(k, nbins, dev)
    R.timing_report(pred, required, ptr, rows, k, _hist(nbins), out=other.tensors(), workspace=_workspace(k, nbins, dev, byte=0x5C))
    assert C.same_report(other.host()[0], first)


def test_report_allocates_its_own_buffers_and_scratch(dev):
    pred, required, ptr, rows = _device('normal', dev)
    out = R.timing_report(pred, required, ptr, rows, 7, _hist(64))
    _check(tuple(t.cpu().numpy() for t in out), 'normal', 7, 64)
    with pytest.raises(RuntimeError, match='GPU only'):
        R.timing_report(pred.cpu(), required, ptr, rows, 7)
    with pytest.raises(ValueError):
        R.timing_report(pred[:-1], required, ptr, rows, 7)
    with pytest.raises(ValueError):
        R.timing_report(pred, required, ptr, rows, 65)


def test_report_replayed_from_a_captured_graph_follows_the_predictions(dev):
    k, nbins = 7, 64
    pred, required, ptr, rows = _device('normal', dev)
    new = _device('inf', dev)[0]
    static = pred.clone()
    bufs, ws = _filled(k, nbins, dev), _workspace(k, nbins, dev)
    R.timing_report(static, required, ptr, rows, k, _hist(nbins), out=bufs.tensors(), workspace=ws)      # eager first
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                                       # one stream, no branches
        R.timing_report(static, required, ptr, rows, k, _hist(nbins), out=bufs.tensors(), workspace=ws)
    graph.replay()
    _check(bufs.host()[0], 'normal', k, nbins)
    static.copy_(new)
    graph.replay()
    replayed = bufs.host()[0]
    eager = _filled(k, nbins, dev)
    R.timing_report(new, required, ptr, rows, k, _hist(nbins), out=eager.tensors(), workspace=_workspace(k, nbins, dev))
    assert C.same_report(replayed, eager.host()[0])
    assert not C.same_report(replayed, _reference('normal', k, nbins)[0], tns_exact=False)


@pytest.mark.parametrize('what', ['k0', 'k65', 'nbins65', 'short_workspace', 'hist_range'])
def test_bad_arguments_are_refused_and_write_nothing(dev, what):
    pred, required, ptr, rows = _device('normal', dev)
    k, nbins, lo, hi = 7, 4, -1.0, 1.0
    bufs, ws = _filled(64, 64, dev), _workspace(64, 64, dev)
    nbytes = ws.numel()
    if what == 'k0':
        k = 0
    elif what == 'k65':
        k = 65
    elif what == 'nbins65':
        nbins = 65
    elif what == 'short_workspace':
        nbytes = R.workspace_bytes(C.T, C.B, k, (lo, hi, nbins)) - 8
    else:
        lo = hi
    before = bufs.raw.clone()
    s, wr, wsl, h = bufs.tensors()
    with pytest.raises(RuntimeError, match='timing_report'):
        lib.ext('mmft_timing_report', pred, required, ptr, rows, C.T, C.B, k, lo, hi, nbins, s, wr, wsl, h, ws, nbytes, *lib.stream_args(pred))
    torch.cuda.synchronize()
    assert torch.equal(bufs.raw, before) and bool((ws == 0xAB).all())


def test_the_launch_profiler_counts_one_kernel_per_call(dev):
    pred, required, ptr, rows = _device('normal', dev)
    lib.prof_reset()
    lib.prof_enable(True)
    try:
        for _ in range(3):
            R.timing_report(pred, required, ptr, rows, 7, _hist(64))
        torch.cuda.synchronize()
    finally:
        lib.prof_enable(False)
    rows_ = {r['name']: r for r in lib.prof_report()}
    assert rows_['timing_report_kernel']['launches'] == 3 and len(rows_) == 1, rows_
    assert rows_['timing_report_kernel']['bytes'] == 3 * (12 * C.T + C.B * (48 + 8 * 7 + 4 * 66))


# ------------------------------------------------------------------------------------------------ Predictor
def _designs():
    from mmft.synth import synth_design
    return [synth_design(N=6000, L=12, tile=32, seed=120 + i, end_frac=0.2) for i in range(2)]


def _models(designs, dev, seed=19, **kw):
    from mmft.train import build_models
    pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=seed, **kw)
    with torch.no_grad():
        cnn.train()
        cnn(torch.from_numpy(np.stack([d.image for d in designs])).to(dev))
    return pmodel, cnn


def _expected(p, designs, pred, k, hist):
    """reference_report of a predict()'s own output; designs and required times found from the endpoint ids alone."""
    node_off = np.asarray(p.batch.node_off)
    design = np.searchsorted(node_off, p.endpoints, side='right') - 1
    required = np.array([designs[d].required_time.reshape(-1)[e - node_off[d]] for d, e in zip(design, p.endpoints)], dtype=np.float32)
    ptr, rows = R.group_rows(design, len(designs))
    pred = pred.cpu().numpy()
    ref = R.reference_report(pred, required, ptr, rows, k, hist)
    return ref, C.tns_bound(ref[0], pred, required, ptr, rows), required


def _same_decoded(got, ref, bound, endpoints):
    want = R.decode(*ref, endpoints=endpoints)
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        print(f'design {b}: tns got {g["tns"]!r} ref {w["tns"]!r} bound {bound[b]!r}')
        assert abs(g['tns'] - w['tns']) <= bound[b]
        assert {**g, 'tns': 0.0} == {**w, 'tns': 0.0}, b


def test_predictor_with_a_report_predicts_what_it_predicted_and_reports_it(dev):
    from mmft import evaluate
    from mmft.infer import Predictor
    designs = _designs()
    k, hist = 32, (-0.05, 0.05, 16)
    rng = np.random.default_rng(3)
    with lib.math_mode('bf16'):
        pmodel, cnn = _models(designs, dev)
        # required times at the median prediction: about half of the endpoints violate (the batch copies them when it is built)
        median = float(Predictor(pmodel, cnn, designs, dev, graphed=False).predict()[0].median())
        for d in designs:
            d.required_time[:] = median
        plain = Predictor(pmodel, cnn, designs, dev)
        p = Predictor(pmodel, cnn, designs, dev, report=dict(k=k, hist=hist))
        with pytest.raises(RuntimeError, match='predict'):
            p.report()
        with pytest.raises(RuntimeError, match='no report'):
            plain.report()
        for call in range(4):                                         # eager, the capturing call, two replays
            y0, y = plain.predict()[0], p.predict()[0]
            assert torch.equal(y, y0), call
            ref, bound, required = _expected(p, designs, y, k, hist)
            got = p.report()
            _same_decoded(got, ref, bound, p.endpoints)
        assert p._replay.graph is not None and p._replay.calls == 4
        assert sum(d['n'] for d in got) == y.numel() and all(len(d['worst']) == k for d in got)
        # the old and the new kernel agree on what a violation is
        req_d = torch.from_numpy(required).to(dev)
        sums = evaluate.eval_sums(y.contiguous(), req_d, req_d, torch.zeros_like(req_d)).cpu().tolist()
        assert 0 < sum(d['violations'] for d in got) == int(sums[6] + sums[7]) < y.numel()
        # new features: the replayed report follows the new predictions
        before = y.clone()
        moved = (designs[0].cell_feat + rng.standard_normal(designs[0].cell_feat.shape) * 0.5).astype(np.float32)
        for q in (plain, p):
            q.update(0, cell_feat=moved)
        y0, y = plain.predict()[0], p.predict()[0]
        assert torch.equal(y, y0) and not torch.equal(y, before) and p._replay.calls == 5
        ref, bound, _ = _expected(p, designs, y, k, hist)
        _same_decoded(p.report(), ref, bound, p.endpoints)
    # fp32 mode: eager
    pmodel, cnn = _models(designs, dev)
    p = Predictor(pmodel, cnn, designs[:1], dev, report=dict(k=5))
    for _ in range(2):
        y = p.predict()[0]
        ref, bound, _ = _expected(p, designs[:1], y, 5, None)
        _same_decoded(p.report(), ref, bound, p.endpoints)
    assert p._replay is None and p.report()[0]['hist'] is None


def test_predictor_report_needs_the_regression_head(dev):
    from mmft.infer import Predictor
    designs = _designs()[:1]
    pmodel, cnn = _models(designs, dev, nlabels=2)
    with pytest.raises(ValueError, match='regression'):
        Predictor(pmodel, cnn, designs, dev, report=dict(k=4))
    with pytest.raises(ValueError, match='report='):
        Predictor(*_models(designs, dev), designs, dev, report=dict(k=4, bins=3))
    Predictor(pmodel, cnn, designs, dev)


# ------------------------------------------------------------------------------------------------ evaluate.timing_report
def test_evaluate_timing_report_compares_the_model_with_the_truth(dev):
    from mmft import evaluate
    from mmft.train import TrainStep
    designs = _designs()
    k, hist = 16, (-0.5, 0.5, 8)
    pmodel, cnn = _models(designs, dev)
    ts = TrainStep(pmodel, cnn, designs, dev, with_optimizer=False)
    for ids in ([np.arange(0, d.num_paths, 2) for d in designs], [np.arange(designs[0].num_paths), np.zeros(0, dtype=np.int64)]):
        rep = evaluate.timing_report(ts, ids, k=k, hist=hist, frozen_stats=True)
        with torch.no_grad(), evaluate.frozen_statistics(cnn, True):
            hats, ends_d, ends_h = ts.forward(ids)
        idx = ends_d.long().cpu()
        arrival = ts.batch.arrival.cpu()[idx].reshape(-1).numpy()
        required = ts.batch.required.cpu()[idx].reshape(-1).numpy()
        design = np.searchsorted(np.asarray(ts.batch.node_off), np.asarray(ends_h), side='right') - 1
        ptr, rows = R.group_rows(design, 2)
        assert len(rep) == 2
        for side, values in (('predicted', hats.cpu().numpy()), ('actual', arrival)):
            ref = R.reference_report(values, required, ptr, rows, k, hist)
            _same_decoded([r[side] for r in rep], ref, C.tns_bound(ref[0], values, required, ptr, rows), np.asarray(ends_h))
        for b, r in enumerate(rep):
            n = len(ids[b])
            assert r['predicted']['n'] == r['actual']['n'] == n
            if n == 0:
                assert r['topk_overlap'] is None and r['wns_error'] is None and r['tns_error'] is None
                assert r['predicted']['worst'] == [] and r['predicted']['wns'] is None
                continue
            both = {row for row, _ in r['predicted']['worst']} & {row for row, _ in r['actual']['worst']}
            assert r['topk_overlap'] == len(both) / min(k, n) and 0.0 <= r['topk_overlap'] <= 1.0
            assert r['wns_error'] == r['predicted']['wns'] - r['actual']['wns']
            assert r['tns_error'] == r['predicted']['tns'] - r['actual']['tns']
