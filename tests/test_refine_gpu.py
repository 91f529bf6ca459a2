"""The patch of the kept head rows on the GPU (include/mmft_refine.h, mmft.refine): mmft_refine_rows bitwise against
mmft_search_rows and the resident rows, mmft_refine_patch against patch_host, and Predictor.commit_moves(patch=True) /
refine_moves(resident=True) against the truth - the predict() that follows, a twin that takes the unpatched route, and the
host loop of refine_moves."""
import numpy as np
import pytest
import torch

import search_cases as SC
from mmft import commit as CM
from mmft import lib
from mmft import refine as RF
from mmft import search as SE
from test_commit_gpu import _set_required, _setup, _violating_pins
from test_head_kernels_gpu import I32

pytestmark = pytest.mark.gpu
NAN = float('nan')
BITS = lambda t: (t.detach().cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)).view(np.int32)
same_bits = lambda a, b: np.array_equal(BITS(a), BITS(b))


def _rows_of(truth, designs):
    return [np.flatnonzero(np.asarray(truth.row_design) == i) for i in range(len(designs))]


def _entries(plan, selected):
    """bool [T']: the rows of the selected groups' entries, and their number."""
    mine, n = np.zeros(int(plan.grow_row.max()) + 1 if plan.R else 1, dtype=bool), 0
    for g in np.flatnonzero(selected):
        rows = plan.grow_row[plan.grow_ptr[g]:plan.grow_ptr[g + 1]]
        mine[rows] = True
        n += rows.shape[0]
    return mine, n


# ------------------------------------------------------------------------------------------------ 5. the kernels
def _disjoint_groups(state, off, N, want, skip=()):
    """`want` pins of a design (its own numbering) that lie on rows and whose row sets are pairwise disjoint."""
    ptr, rows = state.rows_of_pin
    taken, out = set(), []
    for n in range(N):
        mine = set(rows[ptr[off + n]:ptr[off + n + 1]].tolist())
        if n in skip or not mine or mine & taken:
            continue
        taken |= mine
        out.append(n)
        if len(out) == want:
            break
    assert len(out) == want
    return out


def test_refine_rows_and_patch_against_search_rows_and_patch_host_bitwise(dev):
    from mmft.infer import Predictor
    from test_place_gpu import _live_models, _small_designs
    designs = list(_small_designs())
    assert designs[0].map_size == 16 and len(designs) == 2 and int(designs[0].N) == 2048
    radius = 2
    W, side, centre = 25, 5, SE.centre(2)
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        p = Predictor(pmodel, cnn, designs, dev, placement=True, trials=True, graphed=False, overlap=False)
        i, d = 1, designs[1]                                                     # the second design: rows and nodes with offsets
        N, off = int(d.N), int(p._placed.node_off[1])
        far, *single = _disjoint_groups(p._trial, off, N, 6)
        pair = _disjoint_groups(p._trial, off, N, 8)[6:]                          # two more, one group of two pins
        px, py = np.asarray(d.pin_x).copy(), np.asarray(d.pin_y).copy()
        px[far] = SC.I32_MAX                                                      # + dx saturates here
        p.update(i, pin_x=px, pin_y=py)
        p.predict()
        # groups: 0 saturating, 1 selected, 2 not selected, 3 selected without an offset, 4 the centre, 5 selected (sel == 2,
        # the last offset), 6 two pins, selected; 7 shares group 1's pin and is not selected
        pins = np.array([far] + single + pair + [single[0]], dtype=np.int64)
        gptr = np.array([0, 1, 2, 3, 4, 5, 6, 8, 9], dtype=np.int64)
        plan = p.search_plan(i, pins, gptr)
        sel = np.array([1, 1, 0, 1, 1, 2, 1, 0], dtype=np.int32)
        best_w = np.array([(2 + 2) * side + 1, 3, 7, -1, centre, W - 1, 0, 11], dtype=np.int32)
        G, R = plan.G, plan.R
        assert G == 8 and R >= 8 and all(plan.grow_ptr[g + 1] > plan.grow_ptr[g] for g in range(G))
        assert best_w[0] // side - radius == 2 and int(p._placed.loc_x[off + far]) == SC.I32_MAX
        kept, placed, b = p._trial.kept, p._placed, p.batch
        x, GP, pred = kept['x'], kept['GP'], kept['pred'].reshape(-1)
        fcn, mods = pmodel.fcn, list(pmodel.mlp_fuse.layers)
        width, Dout, T, cnn_col = x.shape[1], fcn.weight.shape[0], pred.numel(), kept['cnn_col']
        d_gptr, d_grow, d_ggrp, d_mptr, d_node = plan.dev
        d_sel, d_w = I32(sel, dev), I32(best_w, dev)
        front = [placed.nodes, placed.lens, placed.maxlen, placed.loc_x, placed.loc_y, placed.map_x, placed.map_y, p._sel.paths,
                 p._sel.feat_off, T, d_grow, d_ggrp, R, d_mptr, d_node, G]
        ldxt = width + 4
        before = [t.clone() for t in (placed.loc_x, placed.loc_y, x, pred)]
        window = torch.full((W * R, ldxt), NAN, device=dev)
        SE.abi('mmft_search_rows', *front, radius, 0, W, GP, fcn.bias, x, x.stride(0), window, ldxt, width, cnn_col, Dout,
               b.masks.run_block, *lib.stream_args(x))

        def rows():
            xt = torch.full((R + 1, ldxt), NAN, device=dev)
            RF.abi('mmft_refine_rows', *front, d_sel, d_w, radius, GP, fcn.bias, x, x.stride(0), xt, ldxt, width, cnn_col, Dout,
                   b.masks.run_block, *lib.stream_args(x))
            return xt

        xt = rows()
        on = RF.selected_entries(sel, best_w, radius, plan.grow_ptr)
        assert on.sum() == sum(plan.grow_ptr[g + 1] - plan.grow_ptr[g] for g in (0, 1, 4, 5, 6)) and 0 < on.sum() < R
        want = RF.rows_host(x.cpu().numpy(), window.cpu().numpy().reshape(W, R, ldxt)[:, :, :width], sel, best_w, radius, plan.grow_ptr,
                            plan.grow_row)
        got = xt.cpu().numpy()
        assert same_bits(got[:R, :width], want)                                   # search_rows at best_w on the selected, x[row] on the others
        assert np.isnan(got[:R, width:]).all() and np.isnan(got[R]).all() and not np.isnan(got[:R, :width]).any()
        xh = x.cpu().numpy()
        assert same_bits(got[:R, :width][~on], xh[plan.grow_row[~on], :width])
        moved = [e for e in np.flatnonzero(on) if not same_bits(got[e, :width], xh[plan.grow_row[e], :width])]
        assert len(moved) >= 1                                                    # the offsets do move masks
        e4 = slice(int(plan.grow_ptr[4]), int(plan.grow_ptr[5]))                  # the centre: the resident row, recomputed
        assert same_bits(got[e4, :width], xh[plan.grow_row[e4], :width])
        assert same_bits(rows(), xt)                                              # same inputs, same bits
        # the head over xt: the resident prediction on every entry that was not moved
        pred_t = torch.full((R + 1,), NAN, device=dev)
        lib.head('mmft_head_mlp_fwd', xt, ldxt, mods[0].weight, mods[0].bias, mods[2].weight, mods[2].bias, None, pred_t, R,
                 mods[0].weight.shape[1], mods[0].weight.shape[0], 1, *lib.stream_args(x))
        ph, pth = pred.cpu().numpy(), pred_t.cpu().numpy()
        assert same_bits(pth[:R][~on], ph[plan.grow_row[~on]]) and same_bits(pth[e4], ph[plan.grow_row[e4]]) and np.isnan(pth[R])
        # the patch, into poisoned copies; a T below the largest selected row leaves entries out of range
        ldx = width + 8
        cut = int(plan.grow_row[on].max())
        assert cut >= 1 and (plan.grow_row[on] < cut).any()

        def patch(T_call):
            xc = torch.full((T + 1, ldx), NAN, device=dev)
            xc[:T, :width] = x
            pc = torch.full((T + 2,), NAN, device=dev)
            pc[:T] = pred
            stats = torch.full((4,), -7, dtype=torch.int64, device=dev)
            RF.abi('mmft_refine_patch', xc, ldx, pc, T_call, xt, ldxt, pred_t, d_sel, d_w, radius, d_grow, d_ggrp, R, G, cnn_col, Dout,
                   stats, *lib.stream_args(x))
            return xc.cpu().numpy(), pc.cpu().numpy(), stats.cpu().numpy()

        for T_call in (T, cut):
            xc, pc, stats = patch(T_call)
            wx, wp, counts = RF.patch_host(xh[:T_call], ph[:T_call], got[:R, :width], pth[:R], sel, best_w, radius, plan.grow_ptr,
                                           plan.grow_row, cnn_col, Dout)
            assert same_bits(xc[:T_call, :width], wx) and same_bits(pc[:T_call], wp) and tuple(stats[:2]) == counts
            assert same_bits(xc[T_call:T, :width], xh[T_call:]) and same_bits(pc[T_call:T], ph[T_call:])          # past T: as they were
            assert np.isnan(xc[:, width:]).all() and np.isnan(xc[T]).all() and np.isnan(pc[T:]).all() and stats[2:].tolist() == [-7, -7]
            assert counts[0] + counts[1] == on.sum() and (counts[1] > 0) == (T_call == cut)
            again = patch(T_call)
            assert same_bits(again[0], xc) and same_bits(again[1], pc) and np.array_equal(again[2], stats)
            rest = np.setdiff1d(np.arange(T_call), plan.grow_row[on])
            assert same_bits(xc[rest, :width], xh[rest]) and same_bits(pc[rest], ph[rest])
            assert same_bits(xc[:T, :cnn_col], xh[:, :cnn_col]) and same_bits(xc[:T, cnn_col + Dout:width], xh[:, cnn_col + Dout:])
        assert (ph[plan.grow_row[on]] != pth[:R][on]).any()                       # the patch is no identity
        # the tables, the pins and the kept state were read, never written
        assert all(torch.equal(a, c) for a, c in zip(before[:2], (placed.loc_x, placed.loc_y)))
        assert same_bits(before[2], x) and same_bits(before[3], pred)


# ------------------------------------------------------------------------------------------------ 6. the patched state is the truth
def test_the_patched_state_is_what_the_next_predict_writes(dev):
    with lib.math_mode('bf16'):
        designs, truth, twin, objs, first = _setup(dev)
        base_pred = first.cpu().numpy()
        rows_of = _rows_of(truth, designs)
        several = False
        for seed in range(4):                                                     # seeds until one selects two groups or more
            required = _set_required(first, seed, [truth, twin] + objs)
            for i, d in enumerate(designs):
                N = int(d.N)
                pins = _violating_pins(twin._trial, twin._placed.node_off, i, N, rows_of[i], base_pred, required)
                home_x, home_y = np.asarray(d.pin_x), np.asarray(d.pin_y)
                for radius in (1, 2):
                    for q in objs:
                        plan = q.search_plan(i, pins)
                        assert torch.equal(q.predict()[0], first)
                        kept = q._trial.kept
                        lx, ly = q._placed.loc_x.cpu().numpy(), q._placed.loc_y.cpu().numpy()
                        x0, calls = kept['x'].cpu().numpy(), (q._replay.calls if q._replay is not None else None)
                        res = q.commit_moves(plan, radius=radius, patch=True)
                        assert not q._trial.stale and (calls is None or q._replay.calls == calls)
                        kx, kp = q._trial.kept['x'].clone(), q._trial.kept['pred'].clone()
                        wx, wy = CM.apply_host(lx, ly, res['selected'], res['best_w'], radius, plan.mv_ptr, plan.mv_node)
                        assert np.array_equal(q._placed.loc_x.cpu().numpy(), wx) and np.array_equal(q._placed.loc_y.cpu().numpy(), wy)
                        mine, n = _entries(plan, res['selected'])
                        assert res['n_patched'] == n and (n > 0) == (res['n_selected'] > 0)
                        rest = np.setdiff1d(np.arange(base_pred.shape[0]), np.flatnonzero(mine))
                        assert same_bits(kx.cpu().numpy()[rest], x0[rest]) and same_bits(kp.cpu().numpy()[rest], base_pred[rest])
                        pred = q.predict()[0]
                        assert same_bits(q._trial.kept['x'], kx) and same_bits(q._trial.kept['pred'], kp) and same_bits(pred, kp)
                        assert SE.base_host(kp.cpu().numpy(), required, rows_of[i])['nsum'] == res['predicted_nsum']
                        print(f'seed {seed} design {i} radius {radius} graphed {q.graphed}: G {plan.G} R {plan.R} selected '
                              f'{res["n_selected"]} patched {n}')
                        several |= res['n_selected'] >= 2
                        q.update(i, pin_x=home_x, pin_y=home_y)                   # back home for the next call
                        assert torch.equal(q.predict()[0], first)
            if several:
                break
        assert several
        assert objs[1]._replay is None


# ------------------------------------------------------------------------------------------------ 7. - 9. the calls that follow
def _one_design(dev, seed=0, i=0):
    designs, truth, twin, objs, first = _setup(dev, eager_too=False)
    a = objs[0]
    base_pred = first.cpu().numpy()
    required = _set_required(first, seed, [truth, twin, a])
    rows_of = _rows_of(truth, designs)
    pins = _violating_pins(a._trial, a._placed.node_off, i, int(designs[i].N), rows_of[i], base_pred, required)
    twin.predict()
    a.predict()
    return designs, a, twin, pins, required, rows_of


def _same_trials(got, want):
    assert set(got) == set(want)
    for k in want:
        if k == 'base':
            assert {n: np.float64(v).tobytes() for n, v in got[k].items()} == {n: np.float64(v).tobytes() for n, v in want[k].items()}
        else:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


def test_a_second_search_and_trial_moves_need_no_predict(dev):
    with lib.math_mode('bf16'):
        designs, a, b, pins, required, rows_of = _one_design(dev)
        i, d = 0, designs[0]
        plans = [q.search_plan(i, pins) for q in (a, b)]
        moved = pins[:16]
        tx = np.asarray(d.pin_x)[moved].astype(np.int64) + 1
        ty = np.asarray(d.pin_y)[moved].astype(np.int64) - 1
        calls = a._replay.calls
        ra = a.commit_moves(plans[0], radius=1, patch=True)
        ta = a.trial_moves(i, moved, tx, ty)                                    # at once: no predict() since the commit
        sa = a.search_moves(plans[0], radius=2)
        assert a._replay.calls == calls and not a._trial.stale
        rb = b.commit_moves(plans[1], radius=1)
        assert b._trial.stale and ra['n_selected'] == rb['n_selected'] >= 1 and 'n_patched' not in rb
        SC.same_tables(ra, rb, 'the commit')
        b.predict()
        tb = b.trial_moves(i, moved, tx, ty)
        sb = b.search_moves(plans[1], radius=2)
        SC.same_tables(sa, sb, 'the second search')
        assert sa['base'] == sb['base'] and sa['base']['nsum'] == ra['predicted_nsum']
        _same_trials(ta, tb)
        assert torch.equal(a._placed.loc_x, b._placed.loc_x) and torch.equal(a._placed.loc_y, b._placed.loc_y)
        assert same_bits(a.predict()[0], b.predict()[0])


def test_the_resident_refinement_equals_the_host_loop(dev):
    with lib.math_mode('bf16'):
        designs, a, b, pins, required, rows_of = _one_design(dev)
        plans = [q.search_plan(0, pins) for q in (a, b)]
        calls = a._replay.calls
        out = a.refine_moves(plans[0], radius=1, passes=3, resident=True)
        assert a._replay.calls == calls + 1 and not a._trial.stale                 # the one predict() it leaves behind
        ref = b.refine_moves(plans[1], radius=1, passes=3)
        assert len(out) == len(ref) and 1 <= len(out) <= 3
        for k, (r, w) in enumerate(zip(out, ref)):
            SC.same_tables(r, w, k)
            assert np.array_equal(r['selected'], w['selected']) and r['base'] == w['base']
            assert (r['sum_dq'], r['predicted_nsum'], r['n_selected'], r['n_candidates']) == \
                (w['sum_dq'], w['predicted_nsum'], w['n_selected'], w['n_candidates'])
            assert r['n_patched'] == _entries(plans[0], r['selected'])[1]
        for r, nxt in zip(out[:-1], out[1:]):
            assert r['n_selected'] > 0 and r['predicted_nsum'] == nxt['base']['nsum']
        assert out[-1]['n_selected'] == 0 or len(out) == 3
        print('resident refine_moves:', [(r['base']['nsum'], r['n_selected'], r['n_patched']) for r in out])
        assert torch.equal(a._placed.loc_x, b._placed.loc_x) and torch.equal(a._placed.loc_y, b._placed.loc_y)
        pa, pb = a.predict()[0], b.predict()[0]
        assert same_bits(pa, pb)
        assert SE.base_host(pa.cpu().numpy(), required, rows_of[0])['nsum'] == out[-1]['predicted_nsum']
        one, ref1 = a.refine_moves(plans[0], radius=1, passes=1, resident=True), b.refine_moves(plans[1], radius=1, passes=1)
        assert len(one) == len(ref1) == 1                                         # `passes` bounds it
        SC.same_tables(one[0], ref1[0], 'one pass')
        assert one[0]['predicted_nsum'] == ref1[0]['predicted_nsum'] and same_bits(a.predict()[0], b.predict()[0])


def test_state_after_a_patched_commit(dev):
    with lib.math_mode('bf16'):
        designs, a, b, pins, required, rows_of = _one_design(dev)
        d = designs[0]
        plan = a.search_plan(0, pins)
        calls, graph = a._replay.calls, a._replay.graph
        with pytest.raises(ValueError, match='commit_moves: patch=True .* needs apply=True'):
            a.commit_moves(plan, patch=True, apply=False)
        with pytest.raises(ValueError, match='refine_moves: every pass applies'):
            a.refine_moves(plan, resident=True, apply=False)
        for kw in (dict(radius=0), dict(radius=9), dict(min_gain=-1.0), dict(max_rows=0)):          # once, before anything is launched
            with pytest.raises(ValueError, match='commit_moves'):
                a.refine_moves(plan, resident=True, **kw)
        assert not a._trial.stale
        held = a.predict()[0]                                                     # the static buffer of the replayed graph
        kept_before = held.clone()
        res = a.commit_moves(plan, patch=True)
        assert not a._trial.stale and res['n_patched'] > 0
        assert held.data_ptr() == a._trial.kept['pred'].data_ptr() and not torch.equal(held, kept_before)          # changed in place
        a.commit_moves(plan, patch=True)                                          # twice without a predict() in between
        a.search_moves(plan)
        assert a._replay.calls == calls + 1 and a._replay.graph is graph          # predict() alone counted
        a.commit_moves(plan)                                                      # the plain commit leaves the state stale
        assert a._trial.stale
        with pytest.raises(RuntimeError, match='update\\(\\) has run'):
            a.commit_moves(plan, patch=True)
        with pytest.raises(RuntimeError, match='update\\(\\) has run'):
            a.refine_moves(plan, resident=True)
        a.predict()
        a.commit_moves(plan, patch=True)
        assert not a._trial.stale
        a.update(0, pin_x=np.asarray(d.pin_x), pin_y=np.asarray(d.pin_y))          # update() after a patched commit: stale again
        assert a._trial.stale
        with pytest.raises(RuntimeError, match='update\\(\\) has run'):
            a.search_moves(plan)
        a.predict()
        assert not a._trial.stale and a._replay.calls == calls + 3
