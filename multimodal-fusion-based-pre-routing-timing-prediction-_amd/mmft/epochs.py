"""Epoch training over rotating design batches under ONE optimizer (src/train.py:431-435,453-586).

The reference loops over epochs and, inside each, over its list of training designs with a single Adam state; every 50
batches and after the last batch of a design it validates per design and keeps the best model.  `EpochTrainer` is that loop
on the whole-sweep step: the designs are given as GROUPS, every group one resident `DesignBatch` with its own `TrainStep`
(and, replayed, its own captured HIP graph), all of them stepping the same `FlatAdam`.  `EpochSchedule` is its host half -
which paths of which design run in which step - and needs no GPU.
"""
import copy
import json
import time

import numpy as np
import torch

from . import gradsink, lib
from .evaluate import validate as _validate
from .fusion import FlatAdam
from .train import TrainStep, GraphedTrainStep, trainable_parameters

_OVERALL_KEYS = ('loss', 'r2', 'acc', 'recall', 'precision', 'f1', 'endpoint_slack_mae', 'mape')


def oversampled_paths(design, os_rate=1):
    """The path list of one training design (src/train.py:357-380): range(num_paths), plus its critical paths appended
    `os_rate` times when os_rate != 0 and (num_paths - n_crit) / n_crit - 1 > 1.  A design without critical paths is not
    oversampled (the reference would divide by zero there)."""
    paths = np.arange(design.num_paths, dtype=np.int64)
    crit = getattr(design, 'critical_paths', None)
    crit = np.zeros(0, dtype=np.int64) if crit is None else np.asarray(crit, dtype=np.int64).reshape(-1)
    n_crit = crit.shape[0]
    if os_rate != 0 and n_crit and (design.num_paths - n_crit) / n_crit - 1 > 1:
        paths = np.concatenate([paths] + [crit] * int(os_rate))
    return paths


class EpochSchedule:
    """Which paths of which design run in which step: a pure host function of (seed, epoch, the designs).

    Where the reference is defined it is followed.  A design's path list is `oversampled_paths`.  A list longer than
    `batch_size` gives len // batch_size batches of exactly batch_size paths per pass over it, the partial last batch
    dropped; a list no longer than batch_size gives one batch holding all of it (src/train.py:469-472); the batches of a
    pass are cut from a fresh permutation of the list.  Groups run in list order and all steps of a group run before the
    next group starts (src/train.py:461,475).

    Where several designs share a group the reference says nothing (it steps one design at a time): the group takes the
    MAXIMUM of its designs' batch counts as its number of steps per epoch, and a design that runs out of batches draws a
    fresh permutation and goes round again (the rotation proposal of its section 8), so every design
    contributes the same number of paths to every step of its group - the constant batch shape a replayed graph needs.

    Epoch e draws from numpy's default_rng([seed, e]), one permutation per design and pass, at the step that opens the
    pass; `schedule(e)` and the live cursor (`next()`) therefore agree, and the cursor's state - position, bit-generator
    state, the passes that are open - round-trips through state_dict()."""

    def __init__(self, groups, batch_size=1350, os_rate=1, seed=0):
        if not groups or any(len(g) == 0 for g in groups):
            raise ValueError('EpochSchedule: at least one group, and no empty group')
        if batch_size < 1:
            raise ValueError('EpochSchedule: batch_size must be positive')
        self.batch_size, self.os_rate, self.seed = int(batch_size), int(os_rate), int(seed)
        self.lists = [[oversampled_paths(d, self.os_rate) for d in g] for g in groups]
        for g in self.lists:
            if any(l.shape[0] == 0 for l in g):
                raise ValueError('EpochSchedule: a design without paths')
        # per design: paths per step and batches per pass
        self.per_step = [[min(l.shape[0], self.batch_size) for l in g] for g in self.lists]
        self.batches = [[max(l.shape[0] // self.batch_size, 1) for l in g] for g in self.lists]
        self.group_steps = [max(nb) for nb in self.batches]
        self.group_start = np.concatenate([[0], np.cumsum(self.group_steps)]).astype(np.int64)
        self.steps_per_epoch = int(self.group_start[-1])
        self._reset(0)

    def _reset(self, epoch):
        self.epoch, self.step = int(epoch), 0
        self.rng = np.random.default_rng([self.seed, self.epoch])
        self._open = None           # per design of the running group: [the pass's permuted paths, batches handed out]

    def position(self):
        """(group index, step inside the group, steps of the group) of the step that next() returns next."""
        gi = int(np.searchsorted(self.group_start, self.step, side='right')) - 1
        return gi, self.step - int(self.group_start[gi]), self.group_steps[gi]

    def next(self):
        """(group index, path_ids_per_design) of the next step; rolls over into the next epoch after the last one."""
        gi, local, _ = self.position()
        if local == 0:
            self._open = [None] * len(self.lists[gi])
        ids = []
        for j, paths in enumerate(self.lists[gi]):
            k, nb = self.per_step[gi][j], self.batches[gi][j]
            cur = self._open[j]
            if cur is None or cur[1] == nb:
                cur = self._open[j] = [paths[self.rng.permutation(paths.shape[0])][:nb * k], 0]
            ids.append(cur[0][cur[1] * k:(cur[1] + 1) * k])
            cur[1] += 1
        self.step += 1
        if self.step == self.steps_per_epoch:
            self._reset(self.epoch + 1)
        return gi, ids

    def schedule(self, epoch):
        """The ordered list of (group index, path_ids_per_design) of one epoch.  Leaves the live cursor alone."""
        c = copy.copy(self)
        c._reset(epoch)
        return [c.next() for _ in range(self.steps_per_epoch)]

    def example(self, gi):
        """Path ids with the shape of every step of group gi (what a graph capture is primed with); draws nothing."""
        return [paths[:k] for paths, k in zip(self.lists[gi], self.per_step[gi])]

    def _fingerprint(self):
        return dict(seed=self.seed, batch_size=self.batch_size, os_rate=self.os_rate,
                    lists=[[int(l.shape[0]) for l in g] for g in self.lists])

    def state_dict(self):
        """Plain python and torch tensors only (torch.save / torch.load with weights_only)."""
        open_ = None if self._open is None else [None if c is None else (torch.from_numpy(c[0].copy()), int(c[1]))
                                                 for c in self._open]
        return dict(epoch=self.epoch, step=self.step, rng=json.dumps(self.rng.bit_generator.state), open=open_,
                    config=self._fingerprint())

    def load_state_dict(self, sd):
        if sd['config'] != self._fingerprint():
            raise ValueError(f"EpochSchedule.load_state_dict: saved for {sd['config']}, this schedule is {self._fingerprint()}")
        self._reset(int(sd['epoch']))
        self.step = int(sd['step'])
        self.rng.bit_generator.state = json.loads(sd['rng'])
        self._open = None if sd['open'] is None else [None if c is None else [c[0].numpy().copy(), int(c[1])]
                                                      for c in sd['open']]


class EpochTrainer:
    """The reference's training loop (src/train.py:453-586) on the whole-sweep step: epochs over rotating design batches
    under one optimizer.

        trainer = EpochTrainer(pmodel, cnn, [[d0, d1], [d2, d3]], device, batch_size=1350)
        trainer.fit(num_epochs, [[v0, v1]], on_best=lambda t, m: torch.save(t.state_dict(), path))

    groups: list of lists of designs (mmft.synth / mmft.record designs, what TrainStep takes).  Each group becomes one
    resident DesignBatch and one TrainStep(optimizer=shared); with graphed=True each group's step is also captured once
    (GraphedTrainStep(warmup=0)) in the math mode that is set at construction, and step() replays it.  ALL groups stay
    resident.  The one FlatAdam is built first (it re-homes every parameter into its flat buffer), the steps after it, the
    graphs last - every group exists before the first optimizer step is taken.

    Constructing a trainer leaves the model as it was: parameters, BatchNorm running statistics and counters, Adam
    moments and step counters are bitwise what they were before (the capture's priming forward advances the running
    statistics; they are put back).  The modules end up in train mode, as TrainStep leaves them.

    The order of the steps is EpochSchedule's; see there for what happens when several designs share a group."""

    def __init__(self, pmodel, cnn, groups, device, batch_size=1350, lr=1e-3, weight_decay=0.0, task='reg', os_rate=1,
                 graphed=True, seed=0, cone=False, keep_grads=False):
        self.pmodel, self.cnn, self.device, self.task = pmodel, cnn, torch.device(device), task
        self.groups = [list(g) for g in groups]
        self.sched = EpochSchedule(self.groups, batch_size, os_rate, seed)
        self.math_mode = lib.get_math_mode()
        self.best = 0.0                     # max_r2 / max_F1_score start at 0 (src/train.py:449)
        self._eval = {}
        self.build_stats = [dict(seconds=0.0, bytes=0) for _ in self.groups]
        self.optim = FlatAdam(trainable_parameters(pmodel, cnn), lr=lr, weight_decay=weight_decay,
                              zero_after_step=not keep_grads)
        self.steps = [self._timed(gi, lambda g=g: TrainStep(pmodel, cnn, g, self.device, task=task, cone=cone,
                                                            optimizer=self.optim))
                      for gi, g in enumerate(self.groups)]
        self.graphs = None
        if graphed:
            saved = self._buffers()
            try:
                self.graphs = [self._timed(gi, lambda gi=gi, ts=ts: GraphedTrainStep(ts, self.sched.example(gi), warmup=0))
                               for gi, ts in enumerate(self.steps)]
            finally:
                self._restore_buffers(saved)

    def _timed(self, gi, build):
        torch.cuda.synchronize(self.device)
        t, m = time.perf_counter(), torch.cuda.memory_allocated(self.device)
        out = build()
        torch.cuda.synchronize(self.device)
        st = self.build_stats[gi]
        st['seconds'] += time.perf_counter() - t
        st['bytes'] += torch.cuda.memory_allocated(self.device) - m
        return out

    def _modules(self):
        return [m for m in (self.pmodel, self.cnn) if m is not None]

    def _buffers(self):
        """Copies of every module buffer (the BatchNorm running statistics and counters)."""
        return [{k: b.detach().clone() for k, b in m.named_buffers()} for m in self._modules()]

    def _restore_buffers(self, saved):
        # in place: the captured graphs hold the buffers' addresses (the U-Net may have re-homed its counters into one
        # vector meanwhile, so the buffers are looked up again by name)
        with torch.no_grad():
            for m, snap in zip(self._modules(), saved):
                for k, b in m.named_buffers():
                    b.copy_(snap[k])
        torch.cuda.synchronize(self.device)

    # ---------------------------------------------------------------- the schedule
    def schedule(self, epoch):
        return self.sched.schedule(epoch)

    @property
    def epoch(self):
        return self.sched.epoch

    @property
    def step_in_epoch(self):
        return self.sched.step

    @property
    def steps_per_epoch(self):
        return self.sched.steps_per_epoch

    # ---------------------------------------------------------------- training
    def step(self):
        """The next scheduled step: (loss, predictions, endpoints) as TrainStep.step returns them.  Replayed (graphed=True)
        it synchronises nothing: the loss and the predictions are the graph's static tensors, overwritten by the same
        group's next step."""
        if self.graphs is not None and lib.get_math_mode() != self.math_mode:
            raise RuntimeError(f'EpochTrainer: the graphs were captured in math mode {self.math_mode!r}, '
                               f'now {lib.get_math_mode()!r} is set')
        gi, ids = self.sched.next()
        self.last_group = gi
        return (self.graphs[gi] if self.graphs is not None else self.steps[gi]).step(ids)

    def run_epoch(self):
        """The rest of the current epoch; returns the number of steps taken."""
        e, n = self.sched.epoch, 0
        while self.sched.epoch == e:
            self.step()
            n += 1
        return n

    def _eval_steps(self, groups):
        """Evaluation-only steps over `groups`, sharing the modules (as bench.py does for its held-out design); built once
        per list of designs.  Never the training steps' own buffers: a captured graph has baked their addresses in."""
        key = tuple(tuple(id(d) for d in g) for g in groups)
        hit = self._eval.get(key)
        if hit is None:
            steps = [TrainStep(self.pmodel, self.cnn, list(g), self.device, with_optimizer=False, task=self.task) for g in groups]
            hit = self._eval[key] = (steps, [list(g) for g in groups])      # the designs are kept: the key holds their ids
        return hit[0]

    def validate(self, groups=None, frozen_stats=False, per_level=False):
        """dict(cases=[one metric dict per design], overall=mean over the designs) - the shape and the numbers of
        mmft.evaluate.validate_designs (src/train.py:280-290) - from ONE forward per group (validate(per_design=True)).
        groups=None: the training groups (replayed trainers evaluate them on evaluation-only steps of their own, a second
        resident copy of each group, built at the first call).  frozen_stats=False is the reference's behaviour (modules in train mode: the
        running statistics move)."""
        if groups is None:
            steps = self.steps if self.graphs is None else self._eval_steps(self.groups)
        else:
            steps = self._eval_steps(groups)
        cases = []
        for ts in steps:
            cases.extend(_validate(ts, per_level=per_level, frozen_stats=frozen_stats, per_design=True)['designs'])
        overall = {k: float(np.mean([c[k] for c in cases])) for k in _OVERALL_KEYS if cases and all(k in c for c in cases)}
        return dict(cases=cases, overall=overall)

    def fit(self, num_epochs, val_groups, validate_every=50, on_best=None):
        """num_epochs more epochs at the reference's cadence (src/train.py:566-586): after step b of a group (b counted
        from 0, as bidx) with b % validate_every == 0, and after the group's last step, the designs of `val_groups` are
        validated; a result is better when its overall r2 (task 'reg') or f1 ('cls') exceeds the best so far (0 at the
        start, as max_r2 / max_F1_score), and then on_best(trainer, metrics) is called.  Returns the validation results
        as a list of (epoch, step in epoch, metrics)."""
        key = 'r2' if self.task == 'reg' else 'f1'
        history = []
        for _ in range(num_epochs):
            e = self.sched.epoch
            while self.sched.epoch == e:
                _, b, n = self.sched.position()
                at = self.sched.step
                self.step()
                if b % validate_every == 0 or b == n - 1:
                    m = self.validate(val_groups)
                    history.append((e, at, m))
                    if m['overall'][key] > self.best:
                        self.best = float(m['overall'][key])
                        if on_best is not None:
                            on_best(self, m)
        return history

    # ---------------------------------------------------------------- save / resume
    def state_dict(self):
        """Everything a fresh process needs to continue where this run stands, storable with torch.save: both modules'
        state dicts (host copies), the optimizer's, the schedule's cursor (position as (epoch, step in epoch), numpy
        bit-generator state) and the best validation score."""
        host = lambda sd: {k: v.detach().cpu().clone() for k, v in sd.items()}
        return dict(pmodel=host(self.pmodel.state_dict()), cnn=host(self.cnn.state_dict()) if self.cnn is not None else None,
                    optim=self.optim.state_dict(), schedule=self.sched.state_dict(), best=float(self.best))

    def load_state_dict(self, sd):
        """In place: parameters, buffers and optimizer state keep their device addresses, so captured graphs stay valid.
        Refused before anything is written when the optimizer's parameter layout or the schedule's configuration differ,
        or when graphs are captured and the saved hyperparameters are not the ones baked into them."""
        self.optim.check_layout(sd['optim'])
        if self.graphs is not None and sd['optim']['hyper'] != self.optim.state_dict_hyper():
            raise ValueError(f"EpochTrainer.load_state_dict: saved with {sd['optim']['hyper']}, the captured graphs hold "
                             f"{self.optim.state_dict_hyper()}")
        if sd['schedule']['config'] != self.sched._fingerprint():
            raise ValueError(f"EpochTrainer.load_state_dict: saved for the schedule {sd['schedule']['config']}, "
                             f"this trainer runs {self.sched._fingerprint()}")
        torch.cuda.synchronize(self.device)
        self.pmodel.load_state_dict(sd['pmodel'])
        if self.cnn is not None:
            self.cnn.load_state_dict(sd['cnn'])
        self.optim.load_state_dict(sd['optim'])
        gradsink.params_changed()           # packed bf16 weights, the transposed fcn weight: rebuilt from the new values
        self.sched.load_state_dict(sd['schedule'])
        self.best = float(sd['best'])
        torch.cuda.synchronize(self.device)
