"""Inference time and memory in bf16 math mode: predictions for all (or --paths) endpoints of resident designs.

    python tools/bench_predict.py [--config B E] [--paths 0] [--reps 30] [--rounds 7] [--report K] [--out FILE]

Rows, per config (B: 8 designs x 65 536 nodes, 64 levels, 256^2 tiles; E: one design, 1 048 576 nodes, 128 levels, 512^2 tile,
Zipf fan-in):
  baseline          TrainStep(with_optimizer=False).forward under no_grad with frozen_statistics - the path validate() takes,
                    with the selection made once outside the timed call - running the training forward of the sweep
                    (FORWARD_ONLY = False: the launches of a checkout without the flag; the row uses API of such checkouts
                    only, so the same script times them)
  trainstep_fwd_only  the same call with the flag on
  predictor_eager   mmft.infer.Predictor(graphed=False).predict()
  predictor_graph   Predictor().predict() replaying its captured graph
  predictor_graph_report   (--report K) Predictor(report=dict(k=K, hist=(-1, 1, 32))): the replayed graph ends in the timing
                    report kernel, and the call ends in report() - one small device->host copy, decoded
  predictor_graph_host_report   (--report K) the plain replayed predict(), then the same numbers on the host: pred.cpu() and
                    mmft.report.reference_report (numpy) - what a caller without the kernel does
  sweep_keep        the netlist sweep alone under no_grad, mmft.sweep.FORWARD_ONLY = False (the training forward)
  sweep_fwd_only    ... FORWARD_ONLY = True
Timing: device events around `reps` back-to-back calls, after a warm-up of every row; the rows alternate inside each round, so
a drift of the machine hits all of them; per row the median over the rounds and their min .. max.  Memory: peak allocated
bytes over one call of the row and the bytes held in the graph's sweep buffers.  Then one profiled pass of its own (the
library's launch profiler): launches per call and the per-launch time / algorithmic bytes of the level kernels.  The
predictions of all rows must be bitwise equal.  One JSON line per row.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'multimodal-fusion-based-pre-routing-timing-prediction-_amd')
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

from mmft import lib, sweep as S                                  # noqa: E402
from mmft.evaluate import frozen_statistics                       # noqa: E402
from mmft.synth import synth_design                               # noqa: E402
from mmft.train import build_models, DesignBatch, TrainStep       # noqa: E402

try:
    from mmft.infer import Predictor
except ImportError:                                               # an older checkout: the baseline row alone
    Predictor = None

CONFIGS = {'B': dict(designs=8, N=65536, L=64, tile=256, fanin='regular'),
           'E': dict(designs=1, N=1048576, L=128, tile=512, fanin='irregular')}
LEVEL_KERNELS = ('level_fwd_slots_kernel', 'level_fwd_slots_infer_kernel', 'level_fwd_bf16_kernel', 'level_fwd_bf16_infer_kernel',
                 'pair_fwd_gather_kernel', 'mlp2_rows_bf16_kernel<fwd>', 'timing_report_kernel')


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def profile(fn, passes=3):
    lib.prof_reset()
    lib.prof_enable(True)
    try:
        for _ in range(passes):
            fn()
        torch.cuda.synchronize()
    finally:
        lib.prof_enable(False)
    return [dict(r, launches=r['launches'] / passes, ms=r['ms'] / passes, bytes=r['bytes'] / passes) for r in lib.prof_report()]


def buf_bytes(g):
    return sum(t.numel() * t.element_size() for v in g._sweep_bufs.values() for t in (v if isinstance(v, tuple) else (v,))
               if torch.is_tensor(t))


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(), torch.cuda.max_memory_allocated() - base


def run_config(name, cfg, a, emit, dev):
    designs = [synth_design(N=cfg['N'], L=cfg['L'], tile=cfg['tile'], seed=9294 + i, fanin=cfg['fanin']) for i in range(cfg['designs'])]
    rng = np.random.default_rng(6)
    ids = [np.sort(rng.permutation(d.num_paths)[:a.paths]) if a.paths else np.arange(d.num_paths) for d in designs]
    pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=9294)
    has_flag = hasattr(S, 'FORWARD_ONLY')
    rows, graphs, outs = {}, {}, {}
    with lib.math_mode('bf16'), torch.no_grad():
        ts = TrainStep(pmodel, cnn, designs, dev, with_optimizer=False)
        sel = ts.batch.select(ids)

        def baseline(flag=False):
            if has_flag:
                S.FORWARD_ONLY = flag
            try:
                with frozen_statistics(cnn, True):
                    return ts.forward(ids, _sel=sel)[0]
            finally:
                if has_flag:
                    S.FORWARD_ONLY = True
        rows['baseline'], graphs['baseline'] = baseline, ts.batch.graph
        if has_flag:
            ts2 = TrainStep(pmodel, cnn, designs, dev, with_optimizer=False)
            sel2 = ts2.batch.select(ids)

            def trainstep_fwd_only():
                with frozen_statistics(cnn, True):
                    return ts2.forward(ids, _sel=sel2)[0]
            rows['trainstep_fwd_only'], graphs['trainstep_fwd_only'] = trainstep_fwd_only, ts2.batch.graph
        if Predictor is not None:
            pe = Predictor(pmodel, cnn, designs, dev, path_ids_per_design=ids, graphed=False)
            pg = Predictor(pmodel, cnn, designs, dev, path_ids_per_design=ids)
            rows['predictor_eager'], graphs['predictor_eager'] = (lambda: pe.predict()[0]), pe.batch.graph
            rows['predictor_graph'], graphs['predictor_graph'] = (lambda: pg.predict()[0]), pg.batch.graph
        if Predictor is not None and a.report:
            from mmft import report as R
            hist = (-1.0, 1.0, 32)
            pr = Predictor(pmodel, cnn, designs, dev, path_ids_per_design=ids, report=dict(k=a.report, hist=hist))
            ph = Predictor(pmodel, cnn, designs, dev, path_ids_per_design=ids)
            host = dict(required=pr.slack.required.cpu().numpy(), ptr=pr.slack.groups[0].cpu().numpy(),
                        rows=pr.slack.groups[1].cpu().numpy())
            last = {}

            def graph_report():
                y = pr.predict()[0]
                last['device'] = pr.report()
                return y

            def graph_host_report():
                y = ph.predict()[0]
                last['host'] = R.decode(*R.reference_report(y.cpu().numpy(), host['required'], host['ptr'], host['rows'], a.report, hist),
                                        endpoints=ph.endpoints)
                return y
            rows['predictor_graph_report'], graphs['predictor_graph_report'] = graph_report, pr.batch.graph
            rows['predictor_graph_host_report'], graphs['predictor_graph_host_report'] = graph_host_report, ph.batch.graph

        def sweep_row(flag):
            sb = DesignBatch(designs, dev)                 # a graph of its own: the buffers a sweep allocated stay with its graph
            sb.graph.ndata['h'] = torch.zeros((sb.N, 128), dtype=torch.float32, device=dev)
            ends = sb.select(ids)[0]

            def fn():
                if has_flag:
                    S.FORWARD_ONLY = flag
                try:
                    return S.sweep_forward_all(pmodel.gnn, sb.graph, sb.level_nodes, ends)
                finally:
                    if has_flag:
                        S.FORWARD_ONLY = True
            return fn, sb.graph
        rows['sweep_keep'], graphs['sweep_keep'] = sweep_row(False)
        if has_flag:
            rows['sweep_fwd_only'], graphs['sweep_fwd_only'] = sweep_row(True)
        names = list(rows)
        mem = {}
        for nm in names:                                   # first calls (eager, capture), outputs, memory
            for _ in range(3):
                y = rows[nm]()
            torch.cuda.synchronize()
            outs[nm] = (y.clone(), graphs[nm].ndata['h'].clone() if nm.startswith('sweep') else None)
            mem[nm] = peak_bytes(rows[nm]) + (buf_bytes(graphs[nm]),)
        for nm in names:                                   # warm-up of every row
            timed(rows[nm], a.reps)
        ms = {nm: [] for nm in names}
        for _ in range(a.rounds):
            for nm in names:
                ms[nm].append(timed(rows[nm], a.reps))
        for nm in names:
            emit(config=name, row=nm, designs=cfg['designs'], nodes=cfg['N'], levels=cfg['L'], tile=cfg['tile'], paths=int(sum(len(i) for i in ids)),
                 reps=a.reps, rounds=a.rounds, ms_median=statistics.median(ms[nm]), ms_min=min(ms[nm]), ms_max=max(ms[nm]),
                 peak_allocated_bytes=mem[nm][0], peak_over_resident_bytes=mem[nm][1], sweep_buf_bytes=mem[nm][2])
        # equality of everything the rows returned
        pred_rows = [nm for nm in names if not nm.startswith('sweep')]
        eq = {nm: bool(torch.equal(outs[nm][0], outs['baseline'][0])) for nm in pred_rows}
        if has_flag:
            eq['sweep_fwd_only'] = bool(torch.equal(outs['sweep_fwd_only'][0], outs['sweep_keep'][0]) and
                                        torch.equal(outs['sweep_fwd_only'][1], outs['sweep_keep'][1]))
        emit(config=name, row='outputs', bitwise_equal=eq, pred_absmax=float(outs['baseline'][0].abs().max()))
        assert all(eq.values()), eq
        if 'predictor_graph_report' in rows:                # the two reports say the same (TNS: another order of fp64 additions)
            same = all({**d, 'tns': 0} == {**h, 'tns': 0} and abs(d['tns'] - h['tns']) <= 1e-9 * max(1.0, abs(h['tns']))
                       for d, h in zip(last['device'], last['host']))
            emit(config=name, row='reports', equal=same, k=a.report, wns=[d['wns'] for d in last['device']],
                 tns=[d['tns'] for d in last['device']], violations=[d['violations'] for d in last['device']])
            assert same
        # launches, in a pass of its own
        for nm in [n for n in names if n != 'predictor_graph']:
            prof = profile(rows[nm])
            emit(config=name, row=nm + '_launches', launches=sum(r['launches'] for r in prof), ms_kernels=sum(r['ms'] for r in prof),
                 unet_launches=sum(r['launches'] for r in prof if r['name'].startswith('u16_')))
            for r in prof:
                if r['name'] in LEVEL_KERNELS:
                    emit(config=name, row=nm + '_kernel', name=r['name'], launches=r['launches'], us_per_launch=1e3 * r['ms'] / r['launches'],
                         alg_bytes_per_launch=r['bytes'] / r['launches'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', nargs='+', default=['B', 'E'], choices=sorted(CONFIGS))
    ap.add_argument('--paths', type=int, default=0, help='paths per design (0: all)')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--report', type=int, default=0, help='k of the timing report rows (0: none)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda:0')
    lines = []

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        if a.out:                                           # written as the rows come: a later config that fails loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    for name in a.config:
        run_config(name, CONFIGS[name], a, emit, dev)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
