"""bench.py prints ONE JSON line with the contract fields (task statement); with --full also `roofline`, `cpu_baseline`,
the held-out evaluation and its fp32 drift."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SMALL = ['--gpus', '1', '--steps', '3', '--warmup', '1', '--designs', '2', '--nodes', '4096', '--levels', '16', '--tile', '64',
         '--batch-paths', '64']


def test_bench_line_contract(dev, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--designs', '2',
           '--nodes', '4096', '--levels', '16', '--tile', '64', '--batch-paths', '64', '--dump-outputs', str(tmp_path), '--full']
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, f'expected one stdout line, got {len(lines)}'
    j = json.loads(lines[0])
    for key, typ in (('metric', str), ('value', float), ('unit', str), ('n_gpus', int), ('steps', int), ('warmup', int),
                     ('ms_per_step', float), ('higher_is_better', bool), ('scaling', str), ('dtype', str), ('data', str),
                     ('config', dict), ('roofline', dict), ('cpu_baseline', dict)):
        assert isinstance(j[key], typ), key
    assert 'vs_baseline' in j and j['vs_baseline'] is None          # BASELINE.md holds no published number
    assert j['n_gpus'] == 1 and j['steps'] == 3 and j['warmup'] == 1 and j['scaling'] == 'weak' and j['dtype'] == 'bf16'
    f32 = j['heldout_eval_f32_same_schedule']                        # the same schedule replayed in exact fp32
    assert f32 is not None and f32['ms_per_step'] > 0 and abs(f32['mae_drift']) < 1.0
    assert j['higher_is_better'] is True and 'workload' in j['config'] and j['value'] > 0
    assert abs(j['value'] - 2 * 3 / (j['ms_per_step'] * 3 / 1e3)) / j['value'] < 1e-6      # designs / s over the timed steps
    r = j['roofline']
    assert r['bound'] in ('hbm', 'mfma') and r['unit'] in ('GB/s', 'TFLOP/s') and r['peak'] > 0
    assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-9 and 'traffic' in r
    c = j['cpu_baseline']
    assert c['kind'] in ('port', 'reference') and c['cores'] >= 1 and c['value'] > 0 and isinstance(c['sample'], str)
    # --dump-outputs: what the last timed step returned (2 designs x 64 sampled paths)
    import numpy as np
    assert sorted(os.listdir(tmp_path)) == ['endpoint_ids.npy', 'loss.npy', 'predictions.npy']
    loss, pred, ids = (np.load(tmp_path / f'{n}.npy') for n in ('loss', 'predictions', 'endpoint_ids'))
    assert loss.dtype == np.float32 and pred.dtype == np.float32 and ids.dtype == np.float64
    assert pred.shape == ids.shape == (2 * 64,) and np.isfinite(pred).all()
    assert float(loss) == j['loss_last_step']


def run_bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py')] + SMALL + ['--dump-outputs', str(out_dir)] + list(extra)
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, f'expected one stdout line, got {len(lines)}'
    return json.loads(lines[0])


def test_bench_plain_run_is_lean(dev, tmp_path):
    """Without --full the line carries the contract fields and nothing that needs runs of its own, and the timed steps
    compute what they compute in a --full run: same endpoints, same loss and predictions of the last timed step."""
    j = run_bench(tmp_path / 'plain')
    for key, typ in (('metric', str), ('value', float), ('unit', str), ('n_gpus', int), ('steps', int), ('warmup', int),
                     ('ms_per_step', float), ('higher_is_better', bool), ('scaling', str), ('dtype', str), ('data', str),
                     ('config', dict), ('loss_last_step', float), ('train_mae_last_step', float)):
        assert isinstance(j[key], typ), key
    assert j['metric'] == 'train-step samples/sec' and j['unit'] == 'designs/s' and j['higher_is_better'] is True
    assert j['n_gpus'] == 1 and j['steps'] == 3 and j['warmup'] == 1 and j['dtype'] == 'bf16' and j['full'] is False
    assert abs(j['value'] - 2 * 3 / (j['ms_per_step'] * 3 / 1e3)) / j['value'] < 1e-6
    for key in ('roofline', 'cpu_baseline', 'heldout_eval', 'heldout_eval_f32_same_schedule'):
        assert j[key] is None, key
    assert not any(k.startswith(('dropin', 'speedup')) for k in j)

    f = run_bench(tmp_path / 'full', '--full', '--no-cpu-baseline', '--no-dropin')
    assert f['full'] is True and isinstance(f['roofline'], dict) and isinstance(f['heldout_eval'], dict)
    got = {n: np.load(tmp_path / 'plain' / f'{n}.npy') for n in ('loss', 'predictions', 'endpoint_ids')}
    want = {n: np.load(tmp_path / 'full' / f'{n}.npy') for n in ('loss', 'predictions', 'endpoint_ids')}
    assert np.array_equal(got['endpoint_ids'], want['endpoint_ids'])
    for n in ('loss', 'predictions'):
        np.testing.assert_allclose(got[n], want[n], rtol=1e-5, atol=0, err_msg=n)
