"""What "which change would help" costs, in bf16 math mode at config B shapes (8 designs x 65 536 nodes, 64 levels).

    python tools/bench_sensitivity.py [--designs 8] [--paths 1350] [--reps 10] [--rounds 5] [--out FILE] [--image | --pins]

Every row is the HOST clock around the call + synchronise - what a sizing loop waits for:
  run            Sensitivity.run(objective='sum'): forward in the training form, reverse sweep, the last hop on
                 mmft_mlp2_feat_dx_bf16 - the gradient of the summed arrival times with respect to EVERY cell_feat and net_feat
                 row ('sum', not the default 'tns': the freshly initialised model of this tool predicts no violation on the
                 synthetic designs, and all-zero weights would make the comparison of the two routes empty; the launches and
                 their cost do not depend on the weights)
  run_layers     the same run() with the last hop forced onto the generic layers (linear_fwd, linear_dgrad(mask=H),
                 linear_dgrad), which materialises the hidden tensor H and its gradient
  trial_one_row  Predictor.update(i, cell_feat=, rows=[one cell]) + a replayed predict(): the per-row cost of finding the
                 same thing out by trial (the edited values alternate between two tables)
The rows alternate inside each of `rounds` rounds; per row the median and min .. max over the rounds of the mean over `reps`
calls.  Then one profiled pass of run and of run_layers gives the kernel time of the last hop alone (the launch profiler's
device events) and the bytes its kernels need, and the two routes' gradients are compared.  One JSON line per row.  Needs a
GPU.

--image measures the gradient with respect to the layout image instead:
  run / run_image    Sensitivity.run(objective='sum') of an image=False and of an image=True object on the same modules,
                     alternating as above; run is the parent code path (nothing of it changes with image=False)
  eval_input_grad    unet16.unet_eval_input_grad alone on a tape of the batch's images (host clock), then one profiled pass:
                     every kernel of the 32 launches with its device time, and for the two kernels of
                     include/mmft_sens_image.h the bytes they must move and the rate achieved

--pins measures the discrete sensitivity to one-cell moves of a pin (include/mmft_sens_pins.h), on the placement bench's data
(tests/place_cases.placed(config_design('B', i)): paths of up to 12 nodes on a 128 x 128 map):
  run / run_pins     Sensitivity.run(objective='sum') of a pins=False and of a pins=True object on the same modules,
                     alternating as above; run is the parent code path
  pin_move_kernels   one profiled pass of the two launches alone: device time, the bytes they must move, the rate
  estimate_vs_truth  for --sample seeded (pin, direction) pairs among the pins with a non-zero estimate: pin_move against the
                     change of J that Predictor(placement=True).update() + predict() gives under the same weights - sign
                     agreement and the median relative error, estimate and truth both in bf16 mode and both in fp32 mode
                     (the head is a ReLU MLP, and in bf16 mode it rounds its input rows: information, not a test)
--pins --trace-only runs `--reps` calls of run_pins and nothing else, for a kernel trace taken in a run of its own."""
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
from mmft.sensitivity import Sensitivity                           # noqa: E402
from mmft.synth import config_design                               # noqa: E402
from mmft.train import build_models                                # noqa: E402

def host_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def image_rows(a, emit, designs, ids, pmodel, cnn, dev):
    from mmft import unet16
    from mmft.evaluate import frozen_statistics
    with lib.math_mode('bf16'):
        plain = Sensitivity(pmodel, cnn, designs, dev, path_ids_per_design=ids)
        withimg = Sensitivity(pmodel, cnn, designs, dev, path_ids_per_design=ids, image=True)
        rows = {'run': lambda: plain.run(objective='sum'), 'run_image': lambda: withimg.run(objective='sum')}
        for fn in rows.values():
            host_ms(fn, 3)
        N, _, H, W = withimg.batch.images.shape
        emit(row='shapes', designs=a.designs, nodes=int(plain.batch.N), endpoints=int(plain.T), images=[int(N), 3, int(H), int(W)])
        ms = {nm: [] for nm in rows}
        for _ in range(a.rounds):
            for nm, fn in rows.items():
                ms[nm].append(host_ms(fn, a.reps))
        for nm in rows:
            emit(row=nm, reps=a.reps, rounds=a.rounds, ms_median=statistics.median(ms[nm]), ms_min=min(ms[nm]), ms_max=max(ms[nm]))
        emit(row='run_image_over_run', ratio=statistics.median(ms['run_image']) / statistics.median(ms['run']))
        (_, _, g0), (_, _, g1) = rows['run'](), rows['run_image']()
        emit(row='outputs', same_feature_gradients=all(torch.equal(x[k], y[k]) for x, y in zip(g0, g1) for k in ('cell_feat', 'net_feat')),
             image_grad_max=[float(g['image'].abs().max()) for g in g1], feat_grad_max=float(withimg.feat_grad.abs().max()))
        with frozen_statistics(cnn), torch.no_grad():
            _, tape = unet16.unet_forward_eval_taped(cnn, withimg.batch.images)
            gout = withimg.feat_grad.clone()
            grad = lambda: unet16.unet_eval_input_grad(cnn, tape, gout)
            host_ms(grad, 3)
            t = [host_ms(grad, a.reps) for _ in range(a.rounds)]
            emit(row='eval_input_grad', reps=a.reps, rounds=a.rounds, ms_median=statistics.median(t), ms_min=min(t), ms_max=max(t))
            lib.prof_reset()
            lib.prof_enable(True)
            try:
                grad()
                torch.cuda.synchronize()
            finally:
                lib.prof_enable(False)
        prof = lib.prof_report()
        emit(row='eval_input_grad_kernels', launches=sum(r['launches'] for r in prof), ms=sum(r['ms'] for r in prof),
             kernels={r['name']: [r['launches'], round(r['ms'], 4)] for r in prof})
        for r in prof:
            if r['name'].startswith(('u16_frozen_bwd', 'u16_conv3x3_dgrad_image')):
                emit(row='new_kernel', name=r['name'], launches=r['launches'], ms=r['ms'], bytes_needed=r['bytes'],
                     tb_per_s=r['bytes'] / (r['ms'] * 1e-3) / 1e12 if r['ms'] else None,
                     gflop_per_s=r['flops'] / (r['ms'] * 1e-3) / 1e9 if r['ms'] else None)


def pins_rows(a, emit, designs, ids, pmodel, cnn, dev):
    with lib.math_mode('bf16'):
        withpins = Sensitivity(pmodel, cnn, designs, dev, path_ids_per_design=ids, pins=True)
        if a.trace_only:
            for _ in range(a.reps):
                withpins.run(objective='sum')
            torch.cuda.synchronize()
            return
        plain = Sensitivity(pmodel, cnn, designs, dev, path_ids_per_design=ids)
        rows = {'run': lambda: plain.run(objective='sum'), 'run_pins': lambda: withpins.run(objective='sum')}
        for fn in rows.values():
            host_ms(fn, 3)
        placed = withpins.placed
        lens = torch.minimum(placed.lens[withpins._sel[1].long()], torch.tensor(placed.maxlen, device=dev))
        slots = int(withpins._incidence[1].numel())
        emit(row='shapes', designs=a.designs, nodes=int(plain.batch.N), rows=int(plain.T), maxlen=int(placed.maxlen), map=int(placed.map_x),
             live_positions=int(lens.sum()), first_occurrence_slots=slots, pins_on_a_row=int((withpins._incidence[0].diff() > 0).sum()))
        ms = {nm: [] for nm in rows}
        for _ in range(a.rounds):
            for nm, fn in rows.items():
                ms[nm].append(host_ms(fn, a.reps))
        for nm in rows:
            emit(row=nm, reps=a.reps, rounds=a.rounds, ms_median=statistics.median(ms[nm]), ms_min=min(ms[nm]), ms_max=max(ms[nm]))
        emit(row='run_pins_over_run', ratio=statistics.median(ms['run_pins']) / statistics.median(ms['run']))
        (p0, _, g0), (p1, _, g1) = rows['run'](), rows['run_pins']()
        pm = torch.cat([g['pin_move'] for g in g1])
        emit(row='outputs', same_predictions=bool(torch.equal(p0, p1)),
             same_feature_gradients=all(torch.equal(x[k], y[k]) for x, y in zip(g0, g1) for k in ('cell_feat', 'net_feat')),
             pin_move_nonzero=int((pm != 0).sum()), pin_move_abs_max=float(pm.abs().max()))
        # the two launches alone; the bytes they must move: per row its ids, coordinates and g, per changed cell one wT row and one
        # feat element (counted from row_move's non-zero terms as a lower bound: 1 cell each), row_move written, then read once
        # with the CSR for pin_move
        Dout = int(withpins.proj_grad.shape[1])
        changed = int((withpins.row_move != 0).sum())
        need_rows = 4.0 * (int(lens.sum()) * 3 + withpins.T * (Dout + 3) + changed * (Dout + 1) + withpins.row_move.numel())
        need_sum = 4.0 * (slots * 5 + pm.numel() * 2)
        g = withpins.proj_grad
        lib.prof_reset()
        lib.prof_enable(True)
        try:
            withpins._pin_moves(g)
            torch.cuda.synchronize()
        finally:
            lib.prof_enable(False)
        for r in lib.prof_report():
            if r['name'].startswith('pin_move'):
                need = need_rows if 'rows' in r['name'] else need_sum
                emit(row='pin_move_kernels', name=r['name'], launches=r['launches'], ms=r['ms'], bytes_needed_at_least=need,
                     gb_per_s=need / (r['ms'] * 1e-3) / 1e9 if r['ms'] else None)
    # the estimate against truth: J = sum of the predictions (objective='sum') before and after the move, in both math modes -
    # in bf16 mode the head rounds its input rows to bf16, so the truth of a small move is itself quantised
    rng = np.random.default_rng(7)
    cand = torch.nonzero(pm != 0).cpu().numpy()
    sample = cand[rng.permutation(len(cand))[:a.sample]].tolist()
    off = withpins.batch.node_off
    del plain, withpins
    for mode in ('bf16', 'f32'):
        with lib.math_mode(mode):
            pm_m = torch.cat([g['pin_move'] for g in Sensitivity(pmodel, cnn, designs, dev, path_ids_per_design=ids, pins=True).run(objective='sum')[2]])
            pr = Predictor(pmodel, cnn, designs, dev, path_ids_per_design=ids, placement=True, graphed=False)
            with torch.no_grad():
                base = pr.predict()[0].double().clone()
            est, true = [], []
            for n, d in sample:
                i = int(np.searchsorted(off, n, side='right') - 1)
                x, y = np.array(designs[i].pin_x, dtype=np.int64), np.array(designs[i].pin_y, dtype=np.int64)
                k = n - int(off[i])
                x[k] += (1, -1, 0, 0)[d]
                y[k] += (0, 0, 1, -1)[d]
                pr.update(i, pin_x=x, pin_y=y)
                with torch.no_grad():
                    true.append(float((pr.predict()[0].double() - base).sum()))
                pr.update(i, pin_x=np.asarray(designs[i].pin_x, dtype=np.int64), pin_y=np.asarray(designs[i].pin_y, dtype=np.int64))
                est.append(float(pm_m[n, d]))
            del pr
        est, true = np.array(est), np.array(true)
        moved = true != 0
        emit(row='estimate_vs_truth', math_mode=mode, sample=int(est.size), truth_nonzero=int(moved.sum()),
             sign_agreement=float((np.sign(est[moved]) == np.sign(true[moved])).mean()) if moved.any() else None,
             median_rel_err=float(np.median(np.abs(est[moved] - true[moved]) / np.abs(true[moved]))) if moved.any() else None,
             median_abs_truth=float(np.median(np.abs(true[moved]))) if moved.any() else None,
             median_abs_estimate=float(np.median(np.abs(est))), J=float(base.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--designs', type=int, default=8)
    ap.add_argument('--paths', type=int, default=1350, help='endpoints per design (0: all)')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--image', action='store_true', help='the gradient with respect to the layout image (see the module docstring)')
    ap.add_argument('--pins', action='store_true', help='the change per one-cell move of a pin (see the module docstring)')
    ap.add_argument('--sample', type=int, default=64, help='--pins: (pin, direction) pairs of the estimate-against-truth row')
    ap.add_argument('--trace-only', action='store_true', help='--pins: only `reps` calls of run_pins (for a kernel trace)')
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
    if a.pins:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        from place_cases import placed
        designs = [placed(d, seed=100 + i) for i, d in enumerate(designs)]
    rng = np.random.default_rng(6)
    ids = [np.sort(rng.permutation(d.num_paths)[:a.paths]) if a.paths else np.arange(d.num_paths) for d in designs]
    pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=9294)
    if a.image:
        return image_rows(a, emit, designs, ids, pmodel, cnn, dev)
    if a.pins:
        return pins_rows(a, emit, designs, ids, pmodel, cnn, dev)
    mid = (designs[0].L // 2) & ~1                                  # the middle CELL level
    cell = np.asarray(designs[0].levels[mid][:1], dtype=np.int64)
    tables = [torch.from_numpy(designs[0].cell_feat[cell] + np.float32(0.25 * (k + 1))).to(dev) for k in (0, 1)]
    flip = [0]

    with lib.math_mode('bf16'):
        sens = Sensitivity(pmodel, cnn, designs, dev, path_ids_per_design=ids)
        pred_ = Predictor(pmodel, cnn, designs, dev, path_ids_per_design=ids)

        def run(layers):
            sens.force_layers = layers
            out = sens.run(objective='sum')
            assert sens.last_hop == ('layers' if layers else 'fused'), sens.last_hop
            return out

        def trial():
            flip[0] ^= 1
            pred_.update(0, cell_feat=tables[flip[0]], rows=cell)
            with torch.no_grad():
                return pred_.predict()[0]

        rows = {'run': lambda: run(False), 'run_layers': lambda: run(True), 'trial_one_row': trial}
        for fn in rows.values():                                     # warm-up of every row (the third predict() replays)
            host_ms(fn, 3)
        assert pred_._replay is not None and pred_._replay.graph is not None
        b = sens.batch
        n_cell = sum(len(l) for l in b.level_nodes[0::2])
        n_net = sum(len(l) for l in b.level_nodes[1::2])
        emit(row='shapes', designs=a.designs, nodes=int(b.N), levels=int(b.L), endpoints=int(sens.T), cell_rows=n_cell, net_rows=n_net,
             feature_rows=n_cell + n_net)
        ms = {nm: [] for nm in rows}
        for _ in range(a.rounds):
            for nm, fn in rows.items():
                ms[nm].append(host_ms(fn, a.reps))
        for nm in rows:
            emit(row=nm, reps=a.reps, rounds=a.rounds, ms_median=statistics.median(ms[nm]), ms_min=min(ms[nm]), ms_max=max(ms[nm]))
        emit(row='trial_of_every_feature_row_over_run',
             ratio=(n_cell + n_net) * statistics.median(ms['trial_one_row']) / statistics.median(ms['run']))
        # the two routes' results
        _, _, gf = run(False)
        _, _, gl = run(True)
        emit(row='outputs', fused_vs_layers={k: max(rel_err(x[k], y[k]) for x, y in zip(gf, gl)) for k in ('cell_feat', 'net_feat')},
             nonzero_rows={k: int(sum(int((g[k].abs().amax(1) > 0).sum()) for g in gf)) for k in ('cell_feat', 'net_feat')})
        # kernel time of the last hop alone: one profiled (device events) pass per route; the bytes the fused kernel needs
        fc, fn_ = b.graph.ndata['cell_feat'].shape[1], b.graph.ndata['net_feat'].shape[1]
        need = 4.0 * (n_cell * (128 + 2 * fc) + n_net * (128 + 2 * fn_))
        for layers in (False, True):
            run(layers)
            lib.prof_reset()
            lib.prof_enable(True)
            try:
                sens._last_hop(b.graph._sweep)
                torch.cuda.synchronize()
            finally:
                lib.prof_enable(False)
            prof = lib.prof_report()
            t = sum(r['ms'] for r in prof)
            emit(row='last_hop_layers_kernels' if layers else 'last_hop_fused_kernels', launches=sum(r['launches'] for r in prof),
                 ms=t, kernels={r['name']: round(r['ms'], 4) for r in prof},
                 **({} if layers else dict(bytes_needed=need, tb_per_s=need / (t * 1e-3) / 1e12 if t else None)))


if __name__ == '__main__':
    main()
