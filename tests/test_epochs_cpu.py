"""The host half of mmft.epochs: EpochSchedule decides which paths of which design run in which step of an epoch.  It is
a pure function of (seed, epoch, the designs) and needs no GPU; EpochTrainer.schedule() is this object's."""
import io

import numpy as np
import pytest
import torch

from mmft.epochs import EpochSchedule, oversampled_paths


class _Design:
    """What the schedule reads of a design: num_paths and critical_paths."""

    def __init__(self, num_paths, n_crit=0):
        self.num_paths = num_paths
        self.critical_paths = np.arange(n_crit, dtype=np.int64) * 2 % max(num_paths, 1)


def _groups():
    # batch_size 64: 450 paths -> 7 batches, 225 -> 3 (goes round again inside its group), 150 -> 2, 40 -> one batch of 40
    return [[_Design(450), _Design(225)], [_Design(150), _Design(40)], [_Design(64)]]


def _same(a, b):
    return len(a) == len(b) and all(ga == gb and len(ia) == len(ib) and all(np.array_equal(x, y) for x, y in zip(ia, ib))
                                    for (ga, ia), (gb, ib) in zip(a, b))


def test_same_seed_and_epoch_give_the_same_schedule():
    a, b = EpochSchedule(_groups(), 64, seed=3), EpochSchedule(_groups(), 64, seed=3)
    assert _same(a.schedule(2), b.schedule(2))
    assert _same(a.schedule(2), a.schedule(2))              # asking twice changes nothing
    a.next(); a.next()                                      # ... and neither does the live cursor's position
    assert _same(a.schedule(2), b.schedule(2))
    assert not _same(a.schedule(2), EpochSchedule(_groups(), 64, seed=4).schedule(2))


def test_schedule_differs_between_epochs():
    s = EpochSchedule(_groups(), 64, seed=0)
    assert not _same(s.schedule(0), s.schedule(1))
    assert [g for g, _ in s.schedule(0)] == [g for g, _ in s.schedule(1)]          # same shape, other paths


def test_batches_of_one_pass_are_disjoint_and_come_from_the_list():
    groups = [[_Design(450), _Design(225)], [_Design(1000, 100)]]                   # the last one is oversampled
    s = EpochSchedule(groups, 64, os_rate=2, seed=5)
    for gi, g in enumerate(groups):
        steps = [ids for k, ids in s.schedule(1) if k == gi]
        for j, d in enumerate(g):
            full = oversampled_paths(d, 2)
            nb = len(full) // 64
            for first in range(0, len(steps) - nb + 1, nb):                        # every complete pass
                got = np.concatenate([steps[t][j] for t in range(first, first + nb)])
                assert got.shape[0] == nb * 64
                # a sub-multiset of the list: no path more often than the list holds it (disjoint positions of the list)
                have = np.bincount(got, minlength=d.num_paths)
                assert (have <= np.bincount(full, minlength=d.num_paths)).all()
    assert len(oversampled_paths(groups[1][0], 2)) == 1200
    # the design of 225 paths makes two complete passes and a third of its third inside the seven steps of its group
    assert s.batches[0] == [7, 3] and s.group_steps[0] == 7


def test_short_design_gets_one_batch_holding_its_whole_list():
    s = EpochSchedule(_groups(), 64, seed=1)
    for epoch in (0, 1):
        sched = s.schedule(epoch)
        for gi, j, n in ((1, 1, 40), (2, 0, 64)):                                   # shorter than, and exactly, batch_size
            for ids in [ids for k, ids in sched if k == gi]:
                assert np.array_equal(np.sort(ids[j]), np.arange(n))                # every step: a permutation of all of it
    assert s.group_steps == [7, 2, 1]
    steps = [ids[1] for k, ids in s.schedule(0) if k == 1]
    assert not np.array_equal(steps[0], steps[1])                                   # a fresh permutation per pass


def test_paths_per_group_are_constant_over_its_steps():
    s = EpochSchedule(_groups(), 64, seed=2)
    for epoch in (0, 3):
        per_group = {}
        for gi, ids in s.schedule(epoch):
            per_group.setdefault(gi, set()).add(tuple(len(i) for i in ids))
        assert per_group == {0: {(64, 64)}, 1: {(64, 40)}, 2: {(64,)}}
    assert [[len(i) for i in s.example(g)] for g in range(3)] == [[64, 64], [64, 40], [64]]


def test_oversampling_rule_at_its_edges():
    """(num_paths - n_crit) / n_crit - 1 > 1 (src/train.py:359-361,377): 300 paths with 100 critical give exactly 1."""
    just_above, exactly, none = _Design(301, 100), _Design(300, 100), _Design(300, 0)
    assert len(oversampled_paths(just_above, 1)) == 401
    assert len(oversampled_paths(just_above, 3)) == 601
    assert np.array_equal(oversampled_paths(just_above, 1)[301:], just_above.critical_paths)
    assert len(oversampled_paths(just_above, 0)) == 301                              # os_rate 0: never
    assert len(oversampled_paths(exactly, 1)) == 300                                 # ratio == 1 is not > 1
    assert len(oversampled_paths(none, 1)) == 300                                    # no critical path: no division by zero
    s = EpochSchedule([[just_above]], 100, os_rate=1, seed=0)
    assert s.batches == [[4]] and s.per_step == [[100]]                              # 401 // 100, the partial batch dropped


def test_groups_run_in_order_and_each_in_one_piece():
    s = EpochSchedule(_groups(), 64, seed=7)
    for epoch in (0, 1):
        assert [g for g, _ in s.schedule(epoch)] == [0] * 7 + [1] * 2 + [2]
    assert s.steps_per_epoch == 10


def test_cursor_survives_a_state_dict_round_trip():
    """First half of an epoch from one object, torch.save / torch.load of its state into a fresh one, the rest from that:
    equal to the uninterrupted schedule, across the epoch's end."""
    whole = EpochSchedule(_groups(), 64, seed=11)
    want = whole.schedule(1) + whole.schedule(2)
    a = EpochSchedule(_groups(), 64, seed=11)
    for _ in range(a.steps_per_epoch):                                               # epoch 0
        a.next()
    got = [a.next() for _ in range(5)]                                               # epoch 1, stopped inside group 0
    f = io.BytesIO()
    torch.save(a.state_dict(), f)
    f.seek(0)
    b = EpochSchedule(_groups(), 64, seed=11)
    b.load_state_dict(torch.load(f))
    assert (b.epoch, b.step) == (1, 5)
    assert b.rng.bit_generator.state == a.rng.bit_generator.state
    got += [b.next() for _ in range(15)]
    assert (b.epoch, b.step) == (3, 0)
    assert _same(got, want)
    with pytest.raises(ValueError, match='saved for'):
        EpochSchedule(_groups(), 32, seed=11).load_state_dict(a.state_dict())
