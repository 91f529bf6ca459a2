"""What a what-if query costs with and without incremental sweeps, in bf16 math mode at config B shapes (8 designs x 65 536
nodes, 64 levels).

    python tools/bench_incremental.py [--designs 8] [--paths 1350] [--reps 20] [--rounds 7] [--out FILE]

Every row is the HOST clock around  update(...) for every design + predict() + synchronise  - what a sizing loop waits for per
query - of a replayed Predictor; the edited values alternate between two tables, so every edit really changes its rows' bits:
  full              Predictor(incremental=False).predict(): the whole sweep, no update
  full_edit_64      the same Predictor after update(i, cell_feat=, rows=) of 64 cells per design (a plain sparse copy)
  incr_none         Predictor(incremental=True), no update: no seed, nothing swept
  incr_edit_1 / _64 / _4096   that many edited cells per design, drawn from the middle cell level
  incr_edit_level0  one edited level-0 cell per design (the widest cone a single cell has)
  incr_edit_all     the whole cell_feat table of every design pushed, every row changed: a full sweep through the masked
                    launches - what the L - 1 marking launches and the masked instantiation cost over `full`
The rows alternate inside each of `rounds` rounds; per row the median and min .. max over the rounds of the mean over `reps`
calls, and the number of dirty rows of the last call.  After the timing the incremental Predictor's predictions and h must
equal, bitwise, those of the plain Predictor given the same edits.  Then one profiled (eager) pass per row gives the kernel
time of the marking launches, the masked feature MLPs and the level launches.  One JSON line per row.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'multimodal-fusion-based-pre-routing-timing-prediction-_amd')
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

from mmft import lib                                               # noqa: E402
from mmft.infer import Predictor                                   # noqa: E402
from mmft.synth import config_design                               # noqa: E402
from mmft.train import build_models                                # noqa: E402

MARK = ('fanout_step_kernel',)
FEAT = ('mlp2_feat_fwd_masked_kernel', 'mlp2_feat_fwd_kernel')
LEVEL = ('level_fwd_slots_infer_kernel', 'level_fwd_bf16_infer_kernel', 'pair_fwd_gather_kernel', 'mlp2_rows_bf16_kernel')


def host_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--designs', type=int, default=8)
    ap.add_argument('--paths', type=int, default=1350, help='endpoints per design (0: all)')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda:0')
    lines = []

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    designs = [config_design('B', i) for i in range(a.designs)]
    rng = np.random.default_rng(6)
    ids = [np.sort(rng.permutation(d.num_paths)[:a.paths]) if a.paths else np.arange(d.num_paths) for d in designs]
    pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=9294)
    mid = (designs[0].L // 2) & ~1                                  # the middle CELL level

    def pick(level, k):
        """k cells per design from `level`; where the level holds fewer, from the cell levels nearest to it as well."""
        out = []
        for d in designs:
            near = sorted(range(0, d.L, 2), key=lambda l: (abs(l - level), l))
            pool, n = [], 0
            for l in near:
                pool.append(np.asarray(d.levels[l], dtype=np.int64))
                n += pool[-1].size
                if n >= k:
                    break
            out.append(np.sort(rng.permutation(np.concatenate(pool))[:k]))
        return out
    edits = {'edit_1': pick(mid, 1), 'edit_64': pick(mid, 64), 'edit_4096': pick(mid, 4096), 'edit_level0': pick(0, 1),
             'edit_all': [None] * a.designs}
    # two value tables per design, on the device: the caller's new features
    tables = [[torch.from_numpy(d.cell_feat + np.float32(0.25 * (k + 1))).to(dev) for k in (0, 1)] for d in designs]
    values = {nm: [[t[k] if r is None else t[k][torch.from_numpy(r).to(dev)].contiguous() for k in (0, 1)] for t, r in zip(tables, rs)]
              for nm, rs in edits.items()}
    flip = {(nm, k): 0 for nm in edits for k in (False, True)}          # per (edit, Predictor): each alternates on its own

    with lib.math_mode('bf16'), torch.no_grad():
        plain = Predictor(pmodel, cnn, designs, dev, path_ids_per_design=ids)
        incr = Predictor(pmodel, cnn, designs, dev, path_ids_per_design=ids, incremental=True)
        for _ in range(3):
            ya, yb = plain.predict()[0].clone(), incr.predict()[0].clone()
        assert torch.equal(ya, yb) and incr.incremental_active and incr._replay.graph is not None
        emit(row='shapes', designs=a.designs, nodes=int(incr.batch.N), levels=int(incr.batch.L), endpoints=int(ya.shape[0]),
             middle_level=int(mid), middle_level_cells=[int(len(d.levels[mid])) for d in designs][:2])

        def edit(p, nm):
            key = (nm, p is incr)
            flip[key] ^= 1
            for i, r in enumerate(edits[nm]):
                p.update(i, cell_feat=values[nm][i][flip[key]], rows=r)
            return p.predict()[0]

        rows = {'full': lambda: plain.predict()[0], 'full_edit_64': lambda: edit(plain, 'edit_64'), 'incr_none': lambda: incr.predict()[0]}
        for nm in edits:
            rows['incr_' + nm] = (lambda nm=nm: edit(incr, nm))
        for fn in rows.values():                                     # warm-up of every row
            host_ms(fn, 3)
        ms, dirty = {nm: [] for nm in rows}, {}
        for _ in range(a.rounds):
            for nm, fn in rows.items():
                ms[nm].append(host_ms(fn, a.reps))
                if nm.startswith('incr_'):
                    dirty[nm] = int(incr.dirty_mask().sum())
        for nm in rows:
            emit(row=nm, reps=a.reps, rounds=a.rounds, ms_median=statistics.median(ms[nm]), ms_min=min(ms[nm]), ms_max=max(ms[nm]),
                 dirty_rows=dirty.get(nm))
        # the same edits on both Predictors: the same predictions, the same h
        same = {}
        for p in (plain, incr):                                      # (the timed rows left the two with different tables)
            for i in range(a.designs):
                p.update(i, cell_feat=tables[i][0])
            p.predict()
        for nm in edits:
            flip[nm, True] = flip[nm, False] = 0
            yi, yp = edit(incr, nm).clone(), edit(plain, nm).clone()
            same[nm] = bool(torch.equal(yi, yp) and torch.equal(incr.h, plain.h))
        emit(row='outputs', incremental_equals_full=same)
        assert all(same.values()), same
        # kernel times of one eager pass per row (the launch profiler turns the replay off)
        for nm, fn in rows.items():
            fn()
            lib.prof_reset()
            lib.prof_enable(True)
            try:
                fn()
                torch.cuda.synchronize()
            finally:
                lib.prof_enable(False)
            prof = lib.prof_report()
            group = lambda names: dict(launches=sum(r['launches'] for r in prof if r['name'] in names),
                                       ms=sum(r['ms'] for r in prof if r['name'] in names))
            sweep = group(MARK + FEAT + LEVEL + ('update_rows_diff_kernel',))
            emit(row=nm + '_kernels', marking=group(MARK), feature_mlps=group(FEAT), levels=group(LEVEL),
                 update_rows_diff=group(('update_rows_diff_kernel',)), ms_all_kernels=sum(r['ms'] for r in prof),
                 marking_share_of_sweep=(group(MARK)['ms'] / sweep['ms'] if sweep['ms'] else None))


if __name__ == '__main__':
    main()
