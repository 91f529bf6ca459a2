"""mmft.epochs.EpochTrainer on the GPU: epochs over rotating design batches under one optimizer, and what it stands on -
TrainStep(optimizer=...), FlatAdam.state_dict() / load_state_dict(), validate(per_design=True).

Designs: synth_design(N=2048, L=12, tile=32), the size of the existing step tests.  At end_frac=0.5 every such design has
exactly 450 paths whatever its seed, so two of them could never differ in their batch count; the second design of each
group is therefore built with end_frac=0.25 (225 paths).  With batch_size=64 (64 sampled paths per design and step) the
first design of a group gives 7 batches per epoch and the second 3: it goes round twice and starts a third pass inside the
group's 7 steps, which is the wrap-around of EpochSchedule."""
import functools
import io

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import restatement as R

pytestmark = pytest.mark.gpu
BATCH = 64
STEPS_PER_EPOCH = 14


@functools.lru_cache(maxsize=None)
def _designs():
    from mmft.synth import synth_design
    return tuple(synth_design(N=2048, L=12, tile=32, end_frac=(0.5, 0.25)[i % 2], seed=930 + i) for i in range(4))


def _groups():
    d = _designs()
    assert [x.num_paths for x in d] == [450, 225, 450, 225]
    return [[d[0], d[1]], [d[2], d[3]]]


def _models(dev, seed=11):
    from mmft.train import build_models
    return build_models(map_size=_designs()[0].map_size, device=dev, seed=seed)


def _state(pmodel, cnn, optim):
    """Every entry of both state dicts (parameters, BatchNorm statistics and counters) and the optimizer's state, cloned."""
    torch.cuda.synchronize()
    out = {'pm.' + k: v.detach().clone() for k, v in pmodel.state_dict().items()}
    out.update({'cnn.' + k: v.detach().clone() for k, v in cnn.state_dict().items()})
    out.update(m=optim.m.clone(), v=optim.v.clone(), state=optim.state.clone())
    return out


def _assert_bitwise(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _trainer(dev, graphed, seed=11, **kw):
    from mmft.epochs import EpochTrainer
    pmodel, cnn = _models(dev, seed)
    return EpochTrainer(pmodel, cnn, _groups(), dev, batch_size=BATCH, graphed=graphed, seed=5, **kw)


@pytest.fixture(scope='module')
def straight(dev):
    """Two epochs straight through in bf16 mode, eagerly and replayed: the final state of each (shared, never modified)."""
    from mmft import lib
    out = {}
    with lib.math_mode('bf16'):
        for graphed in (False, True):
            tr = _trainer(dev, graphed)
            assert tr.steps_per_epoch == STEPS_PER_EPOCH
            assert tr.run_epoch() == STEPS_PER_EPOCH and tr.run_epoch() == STEPS_PER_EPOCH
            assert (tr.epoch, tr.step_in_epoch) == (2, 0)
            out[graphed] = _state(tr.pmodel, tr.cnn, tr.optim)
            assert tr.optim.device_step_count() == 2 * STEPS_PER_EPOCH == tr.optim.step_count
    return out


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_rotation_under_one_optimizer_equals_a_hand_rolled_loop(dev, mode):
    """Two groups of two designs, two epochs, eager: bitwise the loop one would write by hand from the public pieces - an
    evaluation-only TrainStep per group, ONE FlatAdam, forward / loss / zero_grad / backward / step per scheduled batch."""
    from mmft import lib
    from mmft.fusion import FlatAdam, unit_grad
    from mmft.train import TrainStep, trainable_parameters
    with lib.math_mode(mode):
        tr = _trainer(dev, graphed=False)
        plan = tr.schedule(0) + tr.schedule(1)
        assert len(plan) == 2 * STEPS_PER_EPOCH
        for _ in plan:
            tr.step()
        got = _state(tr.pmodel, tr.cnn, tr.optim)
        assert tr.optim.device_step_count() == len(plan) == tr.optim.step_count

        pmodel, cnn = _models(dev)
        steps = [TrainStep(pmodel, cnn, g, dev, with_optimizer=False) for g in _groups()]
        optim = FlatAdam(trainable_parameters(pmodel, cnn))
        for gi, ids in plan:
            ts = steps[gi]
            hats, ends_d, _ = ts.forward(ids)
            loss = ts.loss(hats, ends_d)
            optim.zero_grad()
            loss.backward(unit_grad(dev))
            optim.step()
        want = _state(pmodel, cnn, optim)
    _assert_bitwise(got, want)
    assert float(got['m'].abs().max()) > 0 and int(got['cnn.inc.double_conv.1.num_batches_tracked']) == 2 * len(plan)


def test_construction_leaves_the_model_as_it_was(dev):
    """graphed=True in bf16 mode: the captures' priming passes run a forward and a backward per group, yet parameters,
    BatchNorm statistics and counters are bitwise what they were, and the optimizer starts from zero moments and counters."""
    from mmft import lib
    from mmft.epochs import EpochTrainer
    with lib.math_mode('bf16'):
        pmodel, cnn = _models(dev)
        cnn.inc.double_conv[1].running_mean.add_(0.25)              # not the initial 0 / 1 / 0 everywhere
        cnn.inc.double_conv[1].num_batches_tracked.add_(3)
        before = {'pm.' + k: v.detach().clone() for k, v in pmodel.state_dict().items()}
        before.update({'cnn.' + k: v.detach().clone() for k, v in cnn.state_dict().items()})
        assert any(k.endswith('num_batches_tracked') for k in before)
        tr = EpochTrainer(pmodel, cnn, _groups(), dev, batch_size=BATCH, graphed=True, seed=5)
        assert tr.graphs is not None and len(tr.graphs) == 2 and all(g.graph is not None for g in tr.graphs)
        after = _state(pmodel, cnn, tr.optim)
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    assert float(after['m'].abs().max()) == 0.0 and float(after['v'].abs().max()) == 0.0
    assert int(after['state'].abs().max()) == 0 and tr.optim.step_count == 0
    assert (tr.epoch, tr.step_in_epoch) == (0, 0)


def test_replayed_rotation_follows_the_eager_one(dev, straight):
    """The same rotation replayed from the groups' graphs and stepped eagerly, bf16 mode: every floating-point entry of
    both state dicts within the 5e-4 of test_graphed_steps_without_host_sync_equal_eager (60 steps there, 28 here); a
    second replayed run is bitwise the first."""
    from mmft import lib
    for k, v in straight[False].items():
        if k.startswith(('pm.', 'cnn.')) and v.dtype.is_floating_point:
            e = rel_err(straight[True][k], v)
            print(f'{k}: {e:.3e}')
            assert e < 5e-4, (k, e)
    with lib.math_mode('bf16'):
        tr = _trainer(dev, graphed=True)
        for _ in range(2 * STEPS_PER_EPOCH):
            tr.step()                                   # no float(loss), no synchronize
        again = _state(tr.pmodel, tr.cnn, tr.optim)
    _assert_bitwise(again, straight[True])


def test_rotation_loss_trajectory_vs_oracle(dev):
    """Two groups of one design each, fp32 mode, two epochs against the fp64 oracle stepping one design at a time under
    one Adam in the schedule's order - the reference's own rotation.  Bound of test_training_trajectory_vs_oracle."""
    from mmft.epochs import EpochTrainer
    d = _designs()[:2]
    pmodel, cnn = _models(dev, seed=9294)
    oracle = R.OracleTrainer({k: v.detach().cpu().clone() for k, v in pmodel.state_dict().items()},
                             {k: v.detach().cpu().clone() for k, v in cnn.state_dict().items()}, dtype=torch.float64)
    csr = [R.design_csr(x) for x in d]
    tr = EpochTrainer(pmodel, cnn, [[d[0]], [d[1]]], dev, batch_size=BATCH, graphed=False, seed=3)
    plan = tr.schedule(0) + tr.schedule(1)
    assert [g for g, _ in plan] == ([0] * 7 + [1] * 3) * 2
    lo, lg = [], []
    for gi, ids in plan:
        lo.append(oracle.step(d[gi], csr[gi], ids[0].tolist())[0])
        loss, _, _ = tr.step()
        assert tr.last_group == gi
        lg.append(float(loss))
    print('oracle', lo)
    print('gpu   ', lg)
    np.testing.assert_allclose(lg, lo, rtol=2e-2, atol=1e-4)


@pytest.mark.parametrize('graphed', [False, True], ids=['eager', 'graphed'])
def test_resume_continues_where_the_saved_run_stood(dev, straight, graphed):
    """One epoch, torch.save / torch.load of state_dict() into freshly built models (another initialisation) and a freshly
    built trainer, the second epoch: bitwise the run that went straight through.  A state from another parameter layout
    is refused before anything is written."""
    from mmft import lib
    from mmft.fusion import FlatAdam
    with lib.math_mode('bf16'):
        first = _trainer(dev, graphed)
        first.run_epoch()
        f = io.BytesIO()
        torch.save(first.state_dict(), f)
        f.seek(0)
        del first
        second = _trainer(dev, graphed, seed=77)
        sd = torch.load(f)
        other = FlatAdam([torch.zeros(10, device=dev).requires_grad_(True), torch.zeros(3, device=dev).requires_grad_(True)])
        untouched = _state(second.pmodel, second.cnn, second.optim)
        with pytest.raises(ValueError, match='parameters'):
            second.load_state_dict(dict(sd, optim=other.state_dict()))
        _assert_bitwise(_state(second.pmodel, second.cnn, second.optim), untouched)
        second.load_state_dict(sd)
        assert (second.epoch, second.step_in_epoch) == (1, 0) and second.optim.step_count == STEPS_PER_EPOCH
        second.run_epoch()
        got = _state(second.pmodel, second.cnn, second.optim)
        assert second.optim.device_step_count() == 2 * STEPS_PER_EPOCH == second.optim.step_count
    _assert_bitwise(got, straight[graphed])


def _np_metrics(p, t, req, lab):
    """The formulas of mmft.evaluate.metrics_from_sums on float64 numpy sums."""
    p, t, req = p.astype(np.float64), t.astype(np.float64), req.astype(np.float64)
    d = p - t
    n, sy, syy, sse, sae = float(len(p)), t.sum(), (t * t).sum(), (d * d).sum(), np.abs(d).sum()
    nz = t != 0
    sape = (np.abs(d[nz]) / np.abs(t[nz])).sum()
    pc, ac = (req - p) < 0, lab != 0
    tp, fp, tn, fn = float((pc & ac).sum()), float((pc & ~ac).sum()), float((~pc & ~ac).sum()), float((~pc & ac).sum())
    ss_tot = syy - sy * sy / n
    recall = tp / (tp + fn) if tp else 0.0
    precision = tp / (tp + fp) if tp else 0.0
    f1 = 2 * recall * precision / (recall + precision) if (precision or recall) else 0.0
    return dict(n=int(n), loss=sse / n, r2=1.0 - sse / ss_tot, endpoint_slack_mae=sae / n, mape=sape / n, acc=(tp + tn) / n,
                recall=recall, precision=precision, f1=f1, tp=int(tp), fp=int(fp), tn=int(tn), fn=int(fn))


def test_per_design_metrics_from_one_pass(dev):
    """validate(per_design=True) on a batch of three designs against a float64 numpy recomputation from that call's own
    predictions: every metric of every design within 1e-9 relative (both sides add at most 450 terms in fp64, about
    n * 2^-53 apart); the per-design n add up to the pooled n; the call without per_design is unchanged; per design and
    level the n and the mean absolute error agree as well; EpochTrainer.validate()['overall'] is the mean of its cases."""
    from mmft.epochs import EpochTrainer
    from mmft.evaluate import validate
    from mmft.train import TrainStep
    designs = list(_designs()[:3])
    pmodel, cnn = _models(dev)
    ts = TrainStep(pmodel, cnn, designs, dev, with_optimizer=False)
    plain = validate(ts, frozen_stats=True)
    seen, forward = [], ts.forward

    def recording(*a, **k):
        seen.append(forward(*a, **k))
        return seen[-1]
    ts.forward = recording
    m = validate(ts, frozen_stats=True, per_design=True)
    ts.forward = forward
    assert len(seen) == 1
    hats, _, ends = seen[0]
    hats, ends = hats.detach().float().cpu().numpy().reshape(-1), np.asarray(ends)
    assert {k: v for k, v in m.items() if k != 'designs'} == plain
    assert validate(ts, frozen_stats=True) == plain
    assert len(m['designs']) == 3 and sum(c['n'] for c in m['designs']) == m['n'] == sum(d.num_paths for d in designs)
    which = np.searchsorted(ts.batch.node_off, ends, side='right') - 1           # endpoints come back as merged original ids
    full = validate(ts, frozen_stats=True, per_design=True, per_level=True)
    assert full['levels'] == validate(ts, frozen_stats=True, per_level=True)['levels']
    for i, d in enumerate(designs):
        rows = which == i
        local = ends[rows] - ts.batch.node_off[i]
        want = _np_metrics(hats[rows], d.arrival_time[local, 0], d.required_time[local, 0], d.label[local, 0])
        got = m['designs'][i]
        assert got.keys() == want.keys()
        for k, w in want.items():
            print(i, k, got[k], w)
            assert abs(got[k] - w) <= 1e-9 * abs(w), (i, k, got[k], w)
        assert {k: v for k, v in full['designs'][i].items() if k != 'levels'} == got
        level_of = {int(e): int(l) for e, l in zip(d.path2endpoint, d.path2level)}
        lv = np.array([level_of[int(e)] for e in local])
        assert sum(r['n'] for r in full['designs'][i]['levels']) == got['n']
        for r in full['designs'][i]['levels']:
            sel = lv == r['level']
            w = float(np.abs(hats[rows][sel].astype(np.float64) - d.arrival_time[local[sel], 0].astype(np.float64)).mean())
            assert r['n'] == int(sel.sum()) and abs(r['mae'] - w) <= 1e-9 * w
    tr = EpochTrainer(pmodel, cnn, [designs[:2], designs[2:]], dev, batch_size=BATCH, graphed=False)
    v = tr.validate(frozen_stats=True)
    assert [c['n'] for c in v['cases']] == [d.num_paths for d in designs]
    assert set(v['overall']) == {'loss', 'r2', 'acc', 'recall', 'precision', 'f1', 'endpoint_slack_mae', 'mape'}
    for k, o in v['overall'].items():
        assert o == float(np.mean([c[k] for c in v['cases']])), k
    held_out = tr.validate([[designs[2], designs[0]]], frozen_stats=True)        # other groups: evaluation-only steps
    assert [c['n'] for c in held_out['cases']] == [450, 450]


def _profiled_step(step):
    from mmft import lib
    lib.prof_reset()
    lib.prof_enable(True)
    try:
        step()
        torch.cuda.synchronize()
    finally:
        lib.prof_enable(False)
    return {r['name']: r['launches'] for r in lib.prof_report()}


def test_rotation_step_issues_the_launches_of_the_lone_step(dev):
    """The step is still the step: under the launch profiler an eager rotation step on a group - its second, the first
    uploads cached tables - issues the kernels of TrainStep(...).step on that group alone, name for name and count for
    count.  Checked on the first group and, after the rotation has moved on, on the second."""
    from mmft import lib
    from mmft.train import TrainStep
    with lib.math_mode('bf16'):
        tr = _trainer(dev, graphed=False)
        plan = tr.schedule(0)
        rotation = {}
        for k in range(9):
            if k in (1, 8):                                     # second step of group 0, second step of group 1
                rotation[plan[k][0]] = _profiled_step(tr.step)
            else:
                tr.step()
        assert sorted(rotation) == [0, 1]
        for gi, first in ((0, 0), (1, 7)):
            pmodel, cnn = _models(dev)
            ts = TrainStep(pmodel, cnn, _groups()[gi], dev, keep_grads=False)
            ts.step(plan[first][1])
            lone = _profiled_step(lambda: ts.step(plan[first + 1][1]))
            assert len(lone) > 20 and sum(lone.values()) > 100
            assert rotation[gi] == lone, {k: (rotation[gi].get(k), lone.get(k)) for k in set(lone) | set(rotation[gi])
                                          if rotation[gi].get(k) != lone.get(k)}


def test_shared_optimizer_argument_checks(dev):
    from mmft.fusion import FlatAdam
    from mmft.train import TrainStep, trainable_parameters
    d = [_designs()[1]]
    pmodel, cnn = _models(dev)
    stranger = FlatAdam([torch.zeros(12, device=dev).requires_grad_(True)])
    with pytest.raises(ValueError, match='trainable_parameters'):
        TrainStep(pmodel, cnn, d, dev, optimizer=stranger)
    some = FlatAdam(trainable_parameters(pmodel, cnn)[:-1])         # all but one of the right parameters
    with pytest.raises(ValueError, match='trainable_parameters'):
        TrainStep(pmodel, cnn, d, dev, optimizer=some)
    pmodel, cnn = _models(dev)
    shared = FlatAdam(trainable_parameters(pmodel, cnn))
    with pytest.raises(ValueError, match='world_size'):
        TrainStep(pmodel, cnn, d, dev, optimizer=shared, world_size=2)
    with pytest.raises(ValueError, match='fused_optimizer'):
        TrainStep(pmodel, cnn, d, dev, optimizer=shared, fused_optimizer=False)
    with pytest.raises(ValueError, match='with_optimizer'):
        TrainStep(pmodel, cnn, d, dev, optimizer=shared, with_optimizer=False)
    with pytest.raises(ValueError, match='FlatAdam'):
        TrainStep(pmodel, cnn, d, dev, optimizer=torch.optim.Adam(trainable_parameters(pmodel, cnn)))
    ts = TrainStep(pmodel, cnn, d, dev, optimizer=shared)
    assert ts.optim is shared
    other = TrainStep(pmodel, cnn, [_designs()[3]], dev, optimizer=shared)
    ts.step([np.arange(40)])
    other.step([np.arange(40)])
    assert shared.device_step_count() == 2 == shared.step_count


def test_per_design_metrics_of_the_classification_task(dev):
    """task 'cls' has no keyed sums kernel: validate(per_design=True) evaluates one design per call with the other designs'
    path lists empty.  With frozen statistics a row's logits do not depend on the other rows of the batch, so the per-design
    confusion counts add up to the pooled ones exactly and the per-design losses to the pooled loss (fp32 logits: 1e-5)."""
    from mmft.evaluate import validate
    from mmft.train import build_models, TrainStep
    designs = list(_designs()[:2])
    pmodel, cnn = build_models(map_size=designs[0].map_size, device=dev, seed=17, nlabels=2)
    ts = TrainStep(pmodel, cnn, designs, dev, with_optimizer=False, task='cls')
    plain = validate(ts, frozen_stats=True)
    m = validate(ts, frozen_stats=True, per_design=True)
    assert {k: v for k, v in m.items() if k != 'designs'} == plain
    assert [c['n'] for c in m['designs']] == [450, 225] and m['n'] == 675
    for k in ('tp', 'fp', 'tn', 'fn'):
        assert sum(c[k] for c in m['designs']) == m[k], k
    for c in m['designs']:
        assert c['tp'] + c['fp'] + c['tn'] + c['fn'] == c['n']
    total = sum(c['loss'] * c['n'] for c in m['designs'])
    assert abs(total - m['loss'] * m['n']) <= 1e-5 * m['loss'] * m['n']
    some = validate(ts, [np.arange(10), np.zeros(0, dtype=np.int64)], frozen_stats=True, per_design=True)
    assert some['n'] == 10 and some['designs'][0]['n'] == 10 and some['designs'][1] == dict(n=0)


def test_fit_validates_at_the_reference_cadence(dev):
    """fit(): validation after batch b of a group when b % validate_every == 0 and after the group's last batch
    (src/train.py:566-567), on evaluation-only steps over the validation groups; on_best exactly when the overall r2
    exceeds the best so far, which starts at 0 (src/train.py:449,572)."""
    from mmft.epochs import EpochTrainer
    d = _designs()
    pmodel, cnn = _models(dev)
    tr = EpochTrainer(pmodel, cnn, [[d[0]], [d[1]]], dev, batch_size=BATCH, graphed=False, seed=3)
    called = []
    history = tr.fit(1, [[d[2], d[3]]], validate_every=2, on_best=lambda t, m: called.append((t.best, m['overall']['r2'])))
    assert [(e, s) for e, s, _ in history] == [(0, 0), (0, 2), (0, 4), (0, 6), (0, 7), (0, 9)]      # 7 + 3 steps
    assert (tr.epoch, tr.step_in_epoch) == (1, 0) and tr.optim.device_step_count() == 10
    best, want = 0.0, []
    for _, _, m in history:
        assert [c['n'] for c in m['cases']] == [450, 225]
        assert m['overall']['r2'] == float(np.mean([c['r2'] for c in m['cases']]))
        if m['overall']['r2'] > best:
            best = m['overall']['r2']
            want.append((best, best))
    assert called == want and tr.best == best
    assert tr.state_dict()['best'] == best


@pytest.mark.parametrize('larger_first', [True, False])
def test_graphs_of_groups_of_different_size_live_side_by_side(dev, larger_first):
    """Two captured graphs of different size alive at once - two designs and 128 paths per step against one design and 64,
    in either order of capture, so the later capture once fits into and once outgrows the scratch of the earlier one: one
    epoch replayed follows the same epoch stepped eagerly (bf16 mode, the 5e-4 of
    test_replayed_rotation_follows_the_eager_one), optimizer state included."""
    from mmft import lib
    from mmft.epochs import EpochTrainer
    d = _designs()
    groups = [[d[0], d[1]], [d[3]]] if larger_first else [[d[3]], [d[0], d[1]]]
    out = {}
    with lib.math_mode('bf16'):
        for graphed in (False, True):
            pmodel, cnn = _models(dev)
            tr = EpochTrainer(pmodel, cnn, groups, dev, batch_size=BATCH, graphed=graphed, seed=9)
            assert tr.run_epoch() == 10 and tr.optim.device_step_count() == 10
            out[graphed] = _state(pmodel, cnn, tr.optim)
    for k, v in out[False].items():
        if v.dtype.is_floating_point:
            assert rel_err(out[True][k], v) < 5e-4, k
        else:
            assert torch.equal(out[True][k], v), k
