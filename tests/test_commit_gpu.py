"""The commit of best moves on the GPU (include/mmft_commit.h, mmft.commit): mmft_commit_select against select_host on the
hand-built cases, mmft_commit_apply against apply_host, and Predictor.commit_moves / refine_moves against a twin's plain
search_moves, the host's selection, and the truth - predict() after the commit, and a placement=True Predictor given the
same coordinates through update()."""
import numpy as np
import pytest
import torch

import commit_cases as CC
import search_cases as SC
from mmft import commit as CM
from mmft import lib
from mmft import search as SE
from test_head_kernels_gpu import I32
from test_place_gpu import _live_models, _small_designs

pytestmark = pytest.mark.gpu
U32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
POISON = -(2 ** 63)          # an owner table full of it wins every bid, unless the kernel clears what it reads


# ------------------------------------------------------------------------------------------------ 1. select
def _select_on_device(dev, c):
    """(sel int32 [G], stats int64 [4]) of one mmft_commit_select call into fresh, poisoned buffers; the words behind sel and
    stats are checked here."""
    G, R, T = len(c['best_w']), len(c['grow_row']), c['T']
    sel = torch.full((G + 3,), -7, dtype=torch.int32, device=dev)
    stats = torch.full((6,), -7, dtype=torch.int64, device=dev)
    owner = torch.full(((CM.owner_bytes(T) + 7) // 8 + 1,), POISON, dtype=torch.int64, device=dev)
    best_dq = torch.from_numpy(c['best_dq']).to(dev)
    CM.abi('mmft_commit_select', I32(c['best_w'], dev), best_dq, G, c['radius'], I32(c['grow_ptr'], dev), I32(c['grow_row'], dev) if R else None,
           R, T, c['min_q'], sel, stats, owner, *lib.stream_args(sel))
    sel, stats, owner = sel.cpu().numpy(), stats.cpu().numpy(), owner.cpu().numpy()
    assert sel[G:].tolist() == [-7] * 3 and stats[4:].tolist() == [-7] * 2 and owner[-1] == POISON
    return sel[:G], stats[:4]


@pytest.mark.parametrize('name', list(CC.SELECT_CASES))
def test_commit_select_equals_select_host(dev, name):
    c, literal = CC.select_case(name)
    want, figures = CM.select_host(**c)
    assert (want.tolist(), *figures) == literal
    sel, stats = _select_on_device(dev, c)
    print(f'{name}: G {len(want)} R {len(c["grow_row"])} candidates {figures[2]} selected {figures[0]} rounds {int(stats[3])}')
    assert np.array_equal(sel, want) and tuple(int(v) for v in stats[:3]) == figures, (name, stats, figures)
    again = _select_on_device(dev, c)                                             # same inputs, same bits - the rounds too
    assert np.array_equal(again[0], sel) and np.array_equal(again[1], stats)
    rounds = int(stats[3])
    assert 1 <= rounds <= max(figures[2], 1)
    if name == 'chain_up':
        assert rounds >= 32
    if name == 'clique':
        assert rounds <= 3


def test_commit_select_without_candidates_runs_no_round(dev):
    c, _ = CC.select_case('ties')
    sel, stats = _select_on_device(dev, {**c, 'min_q': 10})
    assert not sel.any() and stats.tolist() == [0, 0, 0, 0]
    none = dict(c, grow_ptr=np.zeros(len(c['best_w']) + 1, dtype=np.int64), grow_row=c['grow_row'][:0])      # R == 0: everyone is taken
    sel, stats = _select_on_device(dev, none)
    assert sel.all() and stats.tolist() == [len(sel), -9 * len(sel), len(sel), 1]


# ------------------------------------------------------------------------------------------------ 2. apply
@pytest.mark.parametrize('radius', [1, 2])
def test_commit_apply_equals_apply_host_bitwise(dev, radius):
    c = CC.apply_case(radius)
    wx, wy = CM.apply_host(**c)
    lx, ly = CC.apply_literal(**c)
    assert wx.tolist() == lx and wy.tolist() == ly
    n, G, M = len(wx), len(c['sel']), len(c['mv_node'])
    x, y = torch.full((n + 2,), 77, dtype=torch.int32, device=dev), torch.full((n + 2,), 77, dtype=torch.int32, device=dev)
    x[:n], y[:n] = torch.from_numpy(c['loc_x']).to(dev), torch.from_numpy(c['loc_y']).to(dev)
    at = (x.data_ptr(), y.data_ptr())
    CM.abi('mmft_commit_apply', x, y, n, I32(c['sel'], dev), I32(c['best_w'], dev), radius, I32(c['mv_ptr'], dev), I32(c['mv_node'], dev), G, M,
           *lib.stream_args(x))
    gx, gy = x.cpu().numpy(), y.cpu().numpy()
    assert (x.data_ptr(), y.data_ptr()) == at
    assert np.array_equal(gx[:n], wx) and np.array_equal(gy[:n], wy) and gx[n:].tolist() == gy[n:].tolist() == [77, 77]
    # every element outside the selected groups' pins is as it was; the saturating pins are right
    mine = sorted({int(v) for g in range(G) if c['sel'][g] and 0 <= c['best_w'][g] < (2 * radius + 1) ** 2
                   for v in c['mv_node'][c['mv_ptr'][g]:c['mv_ptr'][g + 1]] if 0 <= v < n})
    rest = np.setdiff1d(np.arange(n), mine)
    assert mine == [0, 1, 2, 3, 10, 11, 12, 13, 14] and np.array_equal(gx[rest], c['loc_x'][rest]) and np.array_equal(gy[rest], c['loc_y'][rest])
    assert (gx[0], gy[2], gx[3], gy[1]) == (CC.I32_MAX, CC.I32_MAX, CC.I32_MIN, CC.I32_MIN)
    assert (gy[0], gx[2]) == (CC.I32_MIN + radius, CC.I32_MIN + radius)


# ------------------------------------------------------------------------------------------------ 3. - 5. the Predictor
def _setup(dev, eager_too=True):
    """truth (placement only), a twin for plain search_moves, and the Predictors under test - graphed and eager -, all on the
    same models and designs, after the predict() calls that make the graphed one replay."""
    from mmft.infer import Predictor
    designs = list(_small_designs())
    assert designs[0].map_size == 16 and len(designs) == 2 and int(designs[0].N) == 2048
    pmodel, cnn = _live_models(designs, dev)
    truth = Predictor(pmodel, cnn, designs, dev, placement=True)
    twin = Predictor(pmodel, cnn, designs, dev, placement=True, trials=True)
    objs = [Predictor(pmodel, cnn, designs, dev, placement=True, trials=True)]
    if eager_too:
        objs.append(Predictor(pmodel, cnn, designs, dev, placement=True, trials=True, graphed=False, overlap=False))
    first = truth.predict()[0].clone()
    for _ in range(3):
        objs[0].predict()
    assert objs[0]._replay.graph is not None and objs[0]._replay.calls == 3
    return designs, truth, twin, objs, first


def _set_required(first, seed, everyone):
    """Required times a hair above and below the resident predictions (test_search_gpu's rule; seed 0 alternates as it does,
    later seeds draw the signs): a prediction that moves changes who violates."""
    T = first.numel()
    if seed == 0:
        sign = torch.where(torch.arange(T, device=first.device) % 2 == 0, 1.0, -1.0)
    else:
        sign = torch.from_numpy(np.where(np.random.default_rng(seed).random(T) < 0.5, 1.0, -1.0).astype(np.float32)).to(first.device)
    near = (first + sign * first.abs().clamp_min(1e-3) * 2.0 ** -18).to(torch.float32)
    for q in everyone:
        q.required.copy_(near)
    return near.cpu().numpy()


def _violating_pins(state, node_off, i, N, rows_i, pred, required):
    """Every distinct pin (design i's own numbering, ascending) on a violating row of design i."""
    from mmft.report import reference_slack
    ptr, rows = state.rows_of_pin
    bad = np.zeros(pred.shape[0], dtype=bool)
    with np.errstate(invalid='ignore'):
        bad[rows_i] = reference_slack(pred[rows_i], required[rows_i]) < 0
    off = int(node_off[i])
    return np.array([n for n in range(N) if bad[rows[ptr[off + n]:ptr[off + n + 1]]].any()], dtype=np.int64)


def _pairwise_disjoint(plan, selected):
    rows, pins = set(), set()
    for g in np.flatnonzero(selected):
        r = set(plan.grow_row[plan.grow_ptr[g]:plan.grow_ptr[g + 1]].tolist())
        m = set(plan.mv_node[plan.mv_ptr[g]:plan.mv_ptr[g + 1]].tolist())
        if r & rows or m & pins:
            return False
        rows |= r
        pins |= m
    return True


def test_commit_moves_end_to_end_against_the_twin_the_host_and_the_truth(dev):
    with lib.math_mode('bf16'):
        designs, truth, twin, objs, first = _setup(dev)
        base_pred = first.cpu().numpy()
        rows_of = [np.flatnonzero(np.asarray(truth.row_design) == i) for i in range(len(designs))]
        several = rejected = False
        for seed in range(4):                                                     # seeds until the inputs show both
            required = _set_required(first, seed, [truth, twin] + objs)
            twin.predict()
            for i, d in enumerate(designs):
                N, off = int(d.N), int(twin._placed.node_off[i])
                pins = _violating_pins(twin._trial, twin._placed.node_off, i, N, rows_of[i], base_pred, required)
                assert pins.size >= 2
                home_x, home_y = np.asarray(d.pin_x), np.asarray(d.pin_y)
                twin_plan = twin.search_plan(i, pins)
                for radius in (1, 2):
                    want = twin.search_moves(twin_plan, radius=radius)
                    for q in objs:
                        plan = q.search_plan(i, pins)
                        out = q.predict()[0]                                    # (a replayed call's static buffer)
                        assert torch.equal(out, first)
                        lx, ly = q._placed.loc_x.clone(), q._placed.loc_y.clone()
                        at = (q._placed.loc_x.data_ptr(), q._placed.loc_y.data_ptr())
                        h, calls = q.h.clone(), (q._replay.calls if q._replay is not None else None)
                        # apply=False first: the same answer, and nothing another call reads is written
                        dry = q.commit_moves(plan, radius=radius, apply=False)
                        assert not q._trial.stale and torch.equal(q._placed.loc_x, lx) and torch.equal(q._placed.loc_y, ly) and torch.equal(q.h, h)
                        assert torch.equal(out, first) and torch.equal(q._trial.kept['pred'].reshape(-1), first.reshape(-1))
                        res = q.commit_moves(plan, radius=radius)
                        assert q._trial.stale and (q._placed.loc_x.data_ptr(), q._placed.loc_y.data_ptr()) == at
                        SC.same_tables(res, want, (seed, i, radius))              # (a) the search tables are the twin's
                        SC.same_tables(dry, want, (seed, i, radius, 'dry'))
                        assert res['base'] == want['base'] == SE.base_host(base_pred, required, rows_of[i])
                        T = base_pred.shape[0]
                        sel, (n_sel, total, n_cand) = CM.select_host(res['best_w'], res['best_dq'], radius, plan.grow_ptr, plan.grow_row, T, 1)
                        for r in (res, dry):                                      # (b) the selection is the host's on those tables
                            assert r['selected'].dtype == np.bool_ and np.array_equal(r['selected'], sel != 0)
                            assert (r['n_selected'], r['sum_dq'], r['n_candidates']) == (n_sel, total, n_cand)
                            assert r['predicted_nsum'] == r['base']['nsum'] + total and r['gain'] == -total * 2.0 ** -20
                            assert (r['rounds'] >= 1) == (n_cand > 0) and r['rounds'] <= max(n_cand, 1)
                        assert _pairwise_disjoint(plan, res['selected'])          # (c) no row and no pin twice
                        print(f'seed {seed} design {i} radius {radius} graphed {q.graphed}: G {plan.G} R {plan.R} candidates {n_cand} '
                              f'selected {n_sel} rounds {res["rounds"]} sum_dq {total}')
                        wx, wy = CM.apply_host(lx.cpu().numpy(), ly.cpu().numpy(), sel, res['best_w'], radius, plan.mv_ptr, plan.mv_node)
                        gx, gy = q._placed.loc_x.cpu().numpy(), q._placed.loc_y.cpu().numpy()
                        assert np.array_equal(gx, wx) and np.array_equal(gy, wy)  # (d) the resident pins
                        assert n_sel == 0 or not (np.array_equal(gx, lx.cpu().numpy()) and np.array_equal(gy, ly.cpu().numpy()))
                        pred = q.predict()[0].cpu().numpy()
                        assert not q._trial.stale
                        now = SE.base_host(pred, required, rows_of[i])
                        assert now['nsum'] == res['predicted_nsum'], (seed, i, radius, now, res['predicted_nsum'])      # (e) to the quantum
                        mine = np.zeros(T, dtype=bool)                            # (f) rows outside the selected groups' entries
                        for g in np.flatnonzero(sel):
                            mine[plan.grow_row[plan.grow_ptr[g]:plan.grow_ptr[g + 1]]] = True
                        assert np.array_equal(U32(pred[~mine]), U32(base_pred[~mine]))
                        truth.update(i, pin_x=gx[off:off + N], pin_y=gy[off:off + N])          # (g) the same coordinates through update()
                        assert np.array_equal(U32(truth.predict()[0].cpu().numpy()), U32(pred))
                        truth.update(i, pin_x=home_x, pin_y=home_y)
                        q.update(i, pin_x=home_x, pin_y=home_y)                   # back home for the next call
                        assert torch.equal(q.predict()[0], first) and torch.equal(q.h, h)
                        if calls is not None:                                     # no commit call captured or replayed a graph
                            assert q._replay.calls == calls + 2
                        several |= n_sel >= 2
                        rejected |= n_cand > n_sel
            if several and rejected:
                break
        assert several and rejected, (several, rejected)
        assert objs[1]._replay is None
        assert np.array_equal(U32(truth.predict()[0].cpu().numpy()), U32(base_pred))


def test_refine_moves_chains_its_passes_and_never_raises_the_sum(dev):
    with lib.math_mode('bf16'):
        designs, truth, twin, objs, first = _setup(dev, eager_too=False)
        p = objs[0]
        base_pred = first.cpu().numpy()
        required = _set_required(first, 0, [truth, twin, p])
        rows_of = [np.flatnonzero(np.asarray(truth.row_design) == i) for i in range(len(designs))]
        i = 0
        pins = _violating_pins(p._trial, p._placed.node_off, i, int(designs[i].N), rows_of[i], base_pred, required)
        plan = p.search_plan(i, pins)
        p.predict()
        out = p.refine_moves(plan, radius=1, passes=3)
        assert 1 <= len(out) <= 3 and not p._trial.stale
        assert out[0]['base'] == SE.base_host(base_pred, required, rows_of[i])
        for a, b in zip(out[:-1], out[1:]):
            assert a['n_selected'] > 0 and a['predicted_nsum'] == b['base']['nsum'] and b['base']['nsum'] <= a['base']['nsum']
        assert all(r['predicted_nsum'] <= r['base']['nsum'] for r in out)
        assert out[-1]['n_selected'] == 0 or len(out) == 3
        final = SE.base_host(p.predict()[0].cpu().numpy(), required, rows_of[i])
        assert final['nsum'] == out[-1]['predicted_nsum']
        print('refine_moves:', [(r['base']['nsum'], r['n_selected'], r['n_candidates'], r['rounds']) for r in out])
        one = p.refine_moves(plan, radius=1, passes=1)                              # `passes` bounds the loop
        assert len(one) == 1 and one[0]['base']['nsum'] == final['nsum']


def test_state_and_refusals(dev):
    from mmft.infer import Predictor
    designs = list(_small_designs())
    d = designs[0]
    on = [int(v) for v in d.path_nodes[int(np.flatnonzero(d.path_lens >= 2)[0]), :2]]
    pins = np.array(on, dtype=np.int64)
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        plain = Predictor(pmodel, cnn, designs, dev, placement=True)
        p = Predictor(pmodel, cnn, designs, dev, placement=True, trials=True)
        other = Predictor(pmodel, cnn, designs, dev, placement=True, trials=True)
        plan = p.search_plan(0, pins)
        with pytest.raises(RuntimeError, match='commit_moves\\(\\): built without trials=True'):
            plain.commit_moves(plan)
        with pytest.raises(RuntimeError, match='predict\\(\\) has not run'):
            p.commit_moves(plan)
        for _ in range(3):
            ref = p.predict()[0].clone()
            other.predict()
        calls = p._replay.calls
        # a plan of another Predictor, something that is no plan, a shared pin, bad arguments: nothing is written
        with pytest.raises(ValueError, match='commit_moves: the plan belongs to another Predictor'):
            other.commit_moves(plan)
        with pytest.raises(TypeError, match='commit_moves: plan must come from search_plan'):
            p.commit_moves(dict(G=1))
        shared = p.search_plan(0, np.array(on + on[:1], dtype=np.int64), np.array([0, 2, 3], dtype=np.int64))
        assert p.search_moves(shared)['dq'].shape == (2, 9)                         # searching accepts it, committing refuses
        for _ in range(2):
            with pytest.raises(ValueError, match=f'commit_moves: pin {on[0]} of design 0 belongs to groups 0 and 1'):
                p.commit_moves(shared)
        for kw in (dict(radius=0), dict(radius=9), dict(scale_log2=31), dict(max_rows=0), dict(min_gain=-1.0), dict(min_gain=float('nan')),
                   dict(min_gain=float('inf')), dict(min_gain=2.0 ** 42)):
            with pytest.raises(ValueError, match='commit_moves'):
                p.commit_moves(plan, **kw)
        assert not p._trial.stale and torch.equal(p.predict()[0], ref)
        # a threshold nobody reaches: no candidate, nothing selected, the pins stay - and the state is stale all the same
        lx = p._placed.loc_x.clone()
        res = p.commit_moves(plan, min_gain=1e6)
        assert (res['n_candidates'], res['n_selected'], res['rounds'], res['sum_dq'], res['gain']) == (0, 0, 0, 0, 0.0)
        assert not res['selected'].any() and res['predicted_nsum'] == res['base']['nsum'] and torch.equal(p._placed.loc_x, lx)
        # twice without a predict() in between
        for call in (p.commit_moves, p.search_moves, lambda pl: p.refine_moves(pl)):
            with pytest.raises(RuntimeError, match='update\\(\\) has run'):
                call(plan)
        assert torch.equal(p.predict()[0], ref)
        # under a stream capture
        graph, scratch = torch.cuda.CUDAGraph(), torch.zeros(4, device=dev)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match='commit_moves\\(\\) under an outer stream capture'):
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                scratch.add_(1.0)
                p.commit_moves(plan)
        torch.cuda.synchronize()
        assert torch.equal(p.predict()[0], ref) and torch.equal(p._placed.loc_x, lx)
        with lib.math_mode('f32'):
            with pytest.raises(ValueError, match='commit_moves: bf16 math mode only'):
                p.commit_moves(plan)
        # the replay counter: predict() alone counted; no commit call captured or replayed a graph
        assert p._replay.calls == calls + 3 and p._replay.graph is not None
