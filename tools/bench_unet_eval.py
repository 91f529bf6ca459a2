"""U-Net inference time in bf16 math mode: the train-mode forward under torch.no_grad() (the only inference there was before
eval() was honoured; uses existing API only, so the same script times it on an older checkout) against the eval-mode
forward (frozen running statistics, mmft/unet16.py `_run_forward_eval`), eager and as one captured graph.

    python tools/bench_unet_eval.py [--n 8] [--size 256] [--reps 200] [--rounds 7] [--out FILE]

Timing: device events around `reps` back-to-back forwards, after a warm-up of every row; the rows alternate inside each
round, so a drift of the machine hits all of them; per row the median over the rounds and their min .. max are printed.
Then one profiled pass (the library's launch profiler, a run of its own after the timed rounds): launches per forward and
the per-launch time / algorithmic bytes of the 16 -> 16 layer at full resolution - convolution + finalize + apply on the
train path, the one eval kernel on the eval path.  One JSON line per row.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'multimodal-fusion-based-pre-routing-timing-prediction-_amd')
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

from mmft import lib, unet16    # noqa: E402
import Unet                      # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def captured(fn, dev):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        out = fn()
    return g, out


def profile(fn, passes=5):
    lib.prof_reset()
    lib.prof_enable(True)
    try:
        for _ in range(passes):
            fn()
        torch.cuda.synchronize()
    finally:
        lib.prof_enable(False)
    return [dict(r, launches=r['launches'] / passes, ms=r['ms'] / passes, bytes=r['bytes'] / passes) for r in lib.prof_report()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=8)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda:0')
    torch.manual_seed(3)
    net = Unet.UNet('max').to(dev)
    net.set_per_sample_stats(True)
    x = torch.rand(a.n, 3, a.size, a.size, device=dev)
    has_eval = hasattr(unet16, 'unet_forward_eval')
    lines = []

    def emit(**row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    with lib.math_mode('bf16'), torch.no_grad():
        rows = {}
        net.train()
        fwd = lambda: net(x)
        rows['train_nograd_eager'] = fwd
        g_train, _ = captured(fwd, dev)
        rows['train_nograd_graph'] = g_train.replay
        y_train = net(x).clone()
        if has_eval:
            net.eval()
            y_eval = net(x).clone()
            g_eval, y_static = captured(fwd, dev)
            g_eval.replay()
            torch.cuda.synchronize()
            assert torch.equal(y_static, y_eval)
            rows['eval_graph'] = g_eval.replay

        def run(name):
            if name.endswith('eager'):                     # the eager rows differ only in the module's mode
                net.train(name == 'train_nograd_eager')
                return timed(fwd, a.reps)
            return timed(rows[name], a.reps)
        names = list(rows) + (['eval_eager'] if has_eval else [])
        for nm in names:                                   # warm-up of every row
            run(nm)
        ms = {nm: [] for nm in names}
        for _ in range(a.rounds):
            for nm in names:
                ms[nm].append(run(nm))
        for nm in names:
            emit(row=nm, n=a.n, size=a.size, reps=a.reps, rounds=a.rounds, ms_median=statistics.median(ms[nm]), ms_min=min(ms[nm]),
                 ms_max=max(ms[nm]))
        # launches and the full-resolution 16 -> 16 layer, profiled in a pass of its own
        net.train()
        prof_t = profile(fwd)
        emit(row='train_nograd_launches', launches=sum(r['launches'] for r in prof_t), ms_kernels=sum(r['ms'] for r in prof_t))
        want = ('u16_conv3x3_kernel<16,16,', 'u16_bn_finalize_kernel', 'u16_bn_apply_kernel', 'u16_bn_apply_pool_kernel')
        for r in prof_t:
            if r['name'].startswith(want):
                emit(row='train_kernel', name=r['name'], launches=r['launches'], ms_per_launch=r['ms'] / r['launches'],
                     bytes_per_launch=r['bytes'] / r['launches'])
        if has_eval:
            net.eval()
            prof_e = profile(fwd)
            emit(row='eval_launches', launches=sum(r['launches'] for r in prof_e), ms_kernels=sum(r['ms'] for r in prof_e))
            for r in prof_e:
                if r['name'].startswith('u16_conv3x3_eval_kernel<16,16,'):
                    emit(row='eval_kernel', name=r['name'], launches=r['launches'], ms_per_launch=r['ms'] / r['launches'],
                         bytes_per_launch=r['bytes'] / r['launches'])
            emit(row='outputs', eval_vs_train_max_abs=float((y_eval - y_train).abs().max()), train_max=float(y_train.abs().max()))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
