"""The swaps on the GPU (include/mmft_swap.h, mmft.swap): mmft_swap_rows bitwise against mmft_trial_rows on the swaps written
out as explicit candidates, mmft_swap_score against score_host, mmft_swap_apply against apply_host, mmft_search_score after
the move of its accumulation into a shared header, and Predictor.swap_moves / commit_swaps against score_host fed with
trial_moves' predictions, the host's selection, and the truth - update() or the commit, then predict()."""
import functools

import numpy as np
import pytest
import torch

import place_cases as C
import search_cases as SC
import swap_cases as WC
from mmft import lib
from mmft import search as SE
from mmft import swap as SW
from mmft import trial as TR
from test_commit_gpu import _set_required, _setup, _violating_pins
from test_head_kernels_gpu import S, T_, I32
from test_search_gpu import _score_on_device

pytestmark = pytest.mark.gpu
NAN = float('nan')
U32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
ROW_CASES = ['single_block_8x8', 'edges_16x16', 'clamped_16x16', 'wide_32x64', 'long_walk_16x16']


# ------------------------------------------------------------------------------------------------ 1. the rows
@functools.lru_cache(maxsize=None)
def _case(name):
    """The tables, groups, pairs and - over every path and three of them twice - the plan and the pair tables of a case."""
    c = C.CASES[name]
    tabs, groups, (pair_a, pair_b, named) = WC.tables(c), WC.groups(c), WC.pairs(c)
    rng = np.random.default_rng(5)
    npaths = tabs[0].shape[0]
    sel = np.concatenate([rng.permutation(npaths), rng.integers(0, npaths, 3)])
    plan = WC.plan(c, sel)
    return tabs, groups, pair_a, pair_b, named, sel, plan, SW.pair_tables(plan[0], plan[1], pair_a, pair_b, sel.shape[0])


@pytest.mark.parametrize('Dout', [4, 128])
@pytest.mark.parametrize('name', ROW_CASES)
def test_swap_rows_equal_trial_rows_on_the_swaps_written_out_bitwise(dev, name, Dout):
    c = C.CASES[name]
    (nodes, lens, px, py, far, mate, twin), groups, pair_a, pair_b, named, sel, plan, ptabs = _case(name)
    grow_ptr, grow_row, grow_grp, mv_ptr, mv_node = plan
    prow_ptr, prow_row, prow_pair, _, _ = ptabs
    for must in [('same_row_a', 'same_row_b'), ('single', 'on_no_row'), ('saturating', 'single'), ('sixty_three', 'lone'),
                 ('thirty_two_a', 'thirty_two_b'), ('single', 'twin')] + ([('shared_by_two_stages', 'on_no_row')] if name == 'long_walk_16x16' else []):
        assert must in named
    if name == 'long_walk_16x16':
        assert nodes.shape[1] == 300 and dict(groups)['shared_by_two_stages'] == [int(nodes[0, 255])]
    T, P, G, K, RP = sel.shape[0], c.P, len(groups), len(named), prow_row.shape[0]
    paths = I32(sel, dev)
    tabs = [I32(nodes, dev), I32(lens, dev), I32(px, dev), I32(py, dev)]
    before = [t.clone() for t in tabs]
    d_prow, d_ppair, d_pa, d_pb = I32(prow_row, dev), I32(prow_pair, dev), I32(pair_a, dev), I32(pair_b, dev)
    d_mptr, d_node = I32(mv_ptr, dev), I32(mv_node, dev)
    cnn_col, after = 8, 12
    width = cnn_col + Dout + after
    ldx, ldxt = width + 4, width + 8
    x = T_((T, ldx), 7, dev)
    B = 2
    GP, bias = T_((B * P, Dout), 1, dev), T_((Dout,), 3, dev)
    foff = I32((np.arange(T) % B) * P, dev)
    # the reference: every swap written out as one trial-move candidate - the pins of a, then those of b, where the literal loop
    # puts them -, entry e = pair (prow_row[e], candidate prow_pair[e])
    e_ptr, e_node, e_x, e_y = WC.swapped_literal(px, py, mv_ptr, mv_node, pair_a, pair_b)
    want = torch.full((RP + 1, ldxt), NAN, device=dev)
    TR.abi('mmft_trial_rows', tabs[0], tabs[1], c.maxlen, tabs[2], tabs[3], c.map_x, c.map_y, paths, foff, T, d_prow, d_ppair, RP,
           I32(e_ptr, dev), I32(e_node, dev), I32(e_x, dev), I32(e_y, dev), K, GP, bias, x, ldx, want, ldxt, width, cnn_col, Dout, S,
           *lib.stream_args(GP))
    bits = lambda t: t.view(torch.int32)

    def rows(e0, e1):
        xt = torch.full((e1 - e0 + 1, ldxt), NAN, device=dev)
        SW.abi('mmft_swap_rows', tabs[0], tabs[1], c.maxlen, tabs[2], tabs[3], c.map_x, c.map_y, paths, foff, T, d_prow, d_ppair, RP,
               d_pa, d_pb, K, d_mptr, d_node, G, e0, e1, GP, bias, x, ldx, xt, ldxt, width, cnn_col, Dout, S, *lib.stream_args(GP))
        return xt

    full = rows(0, RP)
    assert torch.equal(bits(full), bits(want)), (name, Dout)                      # the poison beyond width and behind the last slot included
    assert bool(torch.isnan(full[:RP, width:]).all()) and bool(torch.isnan(full[RP]).all()) and not bool(torch.isnan(full[:RP, :width]).any())
    # the zero move of every entry's row: the centre of mmft_search_rows (one group, one offset)
    zero = torch.full((RP + 1, ldxt), NAN, device=dev)
    SE.abi('mmft_search_rows', tabs[0], tabs[1], c.maxlen, tabs[2], tabs[3], c.map_x, c.map_y, paths, foff, T, d_prow, I32(np.zeros(RP), dev), RP,
           I32([0, 1], dev), I32([mate], dev), 1, 1, 4, 5, GP, bias, x, ldx, zero, ldxt, width, cnn_col, Dout, S, *lib.stream_args(GP))
    k = named.index(('single', 'twin'))                                           # anchors that coincide: bitwise the zero move
    a, b = int(prow_ptr[k]), int(prow_ptr[k + 1])
    assert b > a and torch.equal(bits(full[a:b]), bits(zero[a:b]))
    moved = sum(int(not torch.equal(full[e, :width], zero[e, :width])) for e in range(RP))
    print(f'{name} Dout {Dout}: {moved} of {RP} entries differ from the zero move')
    assert moved >= 1                                                             # the swaps do move masks
    cut = RP // 3 + 1                                                             # an uneven split, single entries, no entry
    for e0, e1 in [(0, cut), (cut, RP), (cut, cut + 1), (RP - 1, RP), (0, 1), (2, 2)]:
        part = rows(e0, e1)
        assert torch.equal(bits(part[:e1 - e0]), bits(want[e0:e1])), (name, Dout, e0, e1)
        assert bool(torch.isnan(part[e1 - e0]).all())
    assert torch.equal(bits(rows(0, RP)), bits(full))                             # same inputs, same bits
    assert all(torch.equal(a, b) for a, b in zip(tabs, before))                   # the tables are read, never written


# ------------------------------------------------------------------------------------------------ 2. the scores
POISON = -7


def _swap_score_on_device(dev, pred_base, required, prow_ptr, prow_row, pred_trial, scale, cuts, design_rows):
    """mmft_swap_score over the pair ranges between `cuts` into poisoned tables that are one word longer at either end; the
    first call forms the base figures.  After each call the words outside everything written so far are still poison."""
    K, RP, T = len(prow_ptr) - 1, len(prow_row), len(pred_base)
    names = SW.TABLES + ('pick',)
    buf = {k: torch.full((K + 2,), POISON, dtype=torch.int64 if k == 'dq' else torch.int32, device=dev) for k in names}
    buf['worst'] = buf['worst'].view(torch.float32)
    tab = {k: v[1:K + 1] for k, v in buf.items()}
    base = torch.full((5,), POISON, dtype=torch.int64, device=dev)
    pb, rq = torch.from_numpy(np.asarray(pred_base, dtype=np.float32)).to(dev), torch.from_numpy(np.asarray(required, dtype=np.float32)).to(dev)
    d_ptr, d_row, d_rows = I32(prow_ptr, dev), I32(prow_row, dev), I32(design_rows, dev)
    done = np.zeros(K, dtype=bool)
    for k0, k1 in zip(cuts[:-1], cuts[1:]):
        e0 = int(prow_ptr[k0])
        pt = torch.from_numpy(np.ascontiguousarray(pred_trial[e0:int(prow_ptr[k1])] if RP else pred_trial)).to(dev)
        pt = pt if pt.numel() else torch.zeros(1, device=dev)                    # (a range without entries: never read)
        SW.abi('mmft_swap_score', pt if RP else None, pb, rq, T, d_ptr, d_row if RP else None, K, RP, k0, k1, scale, tab['dq'], tab['dviol'],
               tab['new_nan'], tab['capped'], tab['worst'], tab['worst_row'], tab['pick'], base[1:4] if k0 == cuts[0] else None, d_rows,
               len(design_rows), *lib.stream_args(pb))
        done[k0:k1] = True
        for k in names:                                                           # nothing outside the slices is written
            words = (buf[k].view(torch.int32) if k == 'worst' else buf[k]).cpu().numpy()
            assert words[0] == POISON and words[K + 1] == POISON and (words[1:K + 1][~done] == POISON).all(), (k, k0, k1)
    assert done.all() and base[0] == POISON and base[4] == POISON
    res = {k: v.cpu().numpy().copy() for k, v in tab.items()}
    res['eligible'] = res['pick'] == 0
    b = base[1:4].cpu().numpy()
    assert dict(nsum=int(b[0]), violations=int(b[1]), n_nan=int(b[2])) == SE.base_host(pred_base, required, design_rows, scale)
    return res


@pytest.mark.parametrize('name', list(WC.SCORE_CASES))
def test_swap_score_equals_score_host_bitwise(dev, name):
    pred_base, required, prow_ptr, prow_row, pred_trial, scale = WC.SCORE_CASES[name]()
    K, T = len(prow_ptr) - 1, len(pred_base)
    want = SW.score_host(pred_base, required, prow_ptr, prow_row, pred_trial, scale)
    WC.same_tables(want, WC.score_literal(pred_base, required, prow_ptr, prow_row, pred_trial, scale), name)
    rows = np.arange(T)
    one = _swap_score_on_device(dev, pred_base, required, prow_ptr, prow_row, pred_trial, scale, [0, K], rows)
    WC.same_tables(one, want, name)
    assert np.array_equal(one['pick'], want['pick']) and one['pick'].dtype == np.int32
    for cuts in ([0, K // 3 + 1, K], [0, 1, 2, K - 1, K], list(range(K + 1)) if K <= 9 else [0, 5, 6, 20, K]):
        part = _swap_score_on_device(dev, pred_base, required, prow_ptr, prow_row, pred_trial, scale, cuts, rows)
        WC.same_tables(part, one, (name, cuts))
        assert np.array_equal(part['pick'], one['pick'])
    if name == 'seeded':
        assert sorted(set(np.diff(prow_ptr).tolist())) == [0, 1, 257, 600] and T == 600
    if name == 'special_rows':
        assert one['pick'][0] == -1 and np.isnan(one['worst'][18:27]).all() and not one['dq'][18:27].any()        # a new NaN; pairs without entries
        out = prow_row.copy()                                                     # rows outside [0, T): in the score and in the base
        out[[0, 5]] = [17, -1]
        got = _swap_score_on_device(dev, pred_base, required, prow_ptr, out, pred_trial, scale, [0, K], np.array([0, 1, 2, 3, 4, 9, -2]))
        WC.same_tables(got, SW.score_host(pred_base, required, prow_ptr, out, pred_trial, scale), 'rows outside')
        none = _swap_score_on_device(dev, pred_base, required, np.zeros(4, dtype=np.int64), prow_row[:0], pred_trial[:0], scale, [0, 2, 3], rows)
        assert not none['dq'].any() and np.isnan(none['worst']).all() and (none['pick'] == 0).all()               # RP == 0


def test_search_score_still_equals_its_literal_definition_on_the_special_rows(dev):
    pred_base, required, grow_ptr, grow_row, trial, scale = SC.special_rows()
    want = SC.score_literal(pred_base, required, grow_ptr, grow_row, trial, 1, scale)
    SC.same_tables(_score_on_device(dev, pred_base, required, grow_ptr, grow_row, trial, 1, scale, [0, 9]), want, 'one call')
    SC.same_tables(_score_on_device(dev, pred_base, required, grow_ptr, grow_row, trial, 1, scale, [0, 4, 9]), want, 'two calls')


# ------------------------------------------------------------------------------------------------ 3. apply
def test_swap_apply_equals_apply_host_bitwise(dev):
    c = WC.apply_case()
    wx, wy = SW.apply_host(**c)
    lx, ly = WC.apply_literal(**c)
    assert wx.tolist() == lx and wy.tolist() == ly
    n, K, G, M = len(wx), len(c['sel']), len(c['mv_ptr']) - 1, len(c['mv_node'])
    x, y = torch.full((n + 2,), 77, dtype=torch.int32, device=dev), torch.full((n + 2,), 77, dtype=torch.int32, device=dev)
    x[:n], y[:n] = torch.from_numpy(c['loc_x']).to(dev), torch.from_numpy(c['loc_y']).to(dev)
    at = (x.data_ptr(), y.data_ptr())
    SW.abi('mmft_swap_apply', x, y, n, I32(c['sel'], dev), I32(c['pick'], dev), I32(c['pair_a'], dev), I32(c['pair_b'], dev), K,
           I32(c['mv_ptr'], dev), I32(c['mv_node'], dev), G, M, *lib.stream_args(x))
    gx, gy = x.cpu().numpy(), y.cpu().numpy()
    assert (x.data_ptr(), y.data_ptr()) == at
    assert np.array_equal(gx[:n], wx) and np.array_equal(gy[:n], wy) and gx[n:].tolist() == gy[n:].tolist() == [77, 77]
    mine = [0, 1, 4, 5, 6, 13, 14, 15]                                            # the pins of the two pairs that are written
    rest = np.setdiff1d(np.arange(n), mine)
    assert np.array_equal(gx[rest], c['loc_x'][rest]) and np.array_equal(gy[rest], c['loc_y'][rest])
    assert all((gx[v], gy[v]) != (c['loc_x'][v], c['loc_y'][v]) for v in mine)
    assert (gx[1], gy[1], gx[4], gy[4]) == (WC.I32_MAX, WC.I32_MIN, WC.I32_MIN, WC.I32_MAX)      # the saturating pair


# ------------------------------------------------------------------------------------------------ 4. - 6. the Predictor
def _groups_and_pairs(state, node_off, i, N, rows_i, pred, required, seed):
    """(pins, group_ptr, pair_a, pair_b) of design i: up to 24 single pins on violating rows, two groups of 8 pins on rows, three
    pins on no row; every idle pin paired with four singles (pairs that share a group which holds no row), 16 seeded pairs
    among the singles (pins of one path share its row), the two groups of 8 with each other and one of them with a single."""
    rng = np.random.default_rng(100 * seed + i)
    ptr, _ = state.rows_of_pin
    off = int(node_off[i])
    count = ptr[off + 1:off + N + 1] - ptr[off:off + N]
    bad = _violating_pins(state, node_off, i, N, rows_i, pred, required)
    singles = rng.choice(bad, min(24, bad.size), replace=False)
    rest = np.setdiff1d(np.flatnonzero(count > 0), singles)
    eights = rng.choice(rest, 16, replace=False).reshape(2, 8)
    idle = np.flatnonzero(count == 0)[:3]
    assert singles.size >= 8 and idle.size == 3
    sets = [[int(v)] for v in singles] + [e.tolist() for e in eights] + [[int(z)] for z in idle]
    n1 = singles.size
    pairs = [(n1 + 2 + z, int(s)) for z in range(3) for s in rng.choice(n1, 4, replace=False)]
    for _ in range(16):
        a, b = rng.choice(n1, 2, replace=False)
        pairs.append((int(a), int(b)))
    pairs += [(n1, n1 + 1), (n1 + 1, 0)]
    pins = np.array([v for s in sets for v in s], dtype=np.int64)
    gptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return pins, gptr, np.array([a for a, _ in pairs], dtype=np.int64), np.array([b for _, b in pairs], dtype=np.int64)


def _quanta_sum(pred, required, rows):
    return SE.base_host(pred, required, rows)['nsum']


def test_swap_moves_and_commit_swaps_against_trial_moves_the_host_and_the_truth(dev):
    with lib.math_mode('bf16'):
        designs, truth, twin, objs, first = _setup(dev)
        base_pred = first.cpu().numpy()
        T = base_pred.shape[0]
        rows_of = [np.flatnonzero(np.asarray(truth.row_design) == i) for i in range(len(designs))]
        shown = dict(improves=False, several=False, lost_by_row=False, lost_by_group=False, useless=False)
        for seed in range(4):                                                     # seeds until the inputs show all five
            required = _set_required(first, seed, [truth, twin] + objs)
            for i, d in enumerate(designs):
                N, off = int(d.N), int(twin._placed.node_off[i])
                home_x, home_y = np.asarray(d.pin_x), np.asarray(d.pin_y)
                pins, gptr, pair_a, pair_b = _groups_and_pairs(twin._trial, twin._placed.node_off, i, N, rows_of[i], base_pred, required, seed)
                base = SE.base_host(base_pred, required, rows_of[i])
                for q in objs:
                    plan = q.search_plan(i, pins, gptr)
                    splan = q.swap_plan(plan, pair_a, torch.from_numpy(pair_b))
                    K, G, RP = splan.K, plan.G, splan.RP
                    assert splan.ints.numel() == 2 * K + 2 * (K + 1) + 2 * RP + RP + 2 * K and K == len(pair_a)
                    out = q.predict()[0]                                        # (a replayed call's static buffer)
                    assert torch.equal(out, first)
                    lx, ly = q._placed.loc_x.clone(), q._placed.loc_y.clone()
                    at = (q._placed.loc_x.data_ptr(), q._placed.loc_y.data_ptr())
                    h, calls = q.h.clone(), (q._replay.calls if q._replay is not None else None)
                    res = q.swap_moves(splan)
                    # (a) the same swaps written out by the host, through trial_moves: its predictions feed score_host
                    c_ptr, c_node, c_x, c_y = SW.swapped_coords(lx.cpu().numpy(), ly.cpu().numpy(), plan.mv_ptr, plan.mv_node, pair_a, pair_b)
                    tm = q.trial_moves(i, c_node - off, c_x.astype(np.int64), c_y.astype(np.int64), c_ptr)
                    assert np.array_equal(tm['pair_ptr'], splan.prow_ptr) and np.array_equal(tm['rows'], splan.prow_row)
                    want = SW.score_host(base_pred, required, splan.prow_ptr, splan.prow_row, tm['pred'], 20)
                    WC.same_tables(res, want, (seed, i))
                    assert np.array_equal(res['gain'], want['gain']) and res['base'] == base
                    assert res['prow_ptr'] is splan.prow_ptr and res['rows'] is splan.prow_row
                    bp, bq = WC.best_pair_literal(res['dq'], res['eligible'], pair_a, pair_b, G)
                    assert np.array_equal(res['best_pair'], bp) and np.array_equal(res['best_pair_dq'], bq)
                    for max_rows in (1, RP // 3 + 1):                             # the chunking does not show
                        other = q.swap_moves(splan, max_rows=max_rows)
                        WC.same_tables(other, res, (seed, i, max_rows))
                        assert other['base'] == base
                    assert torch.equal(q._placed.loc_x, lx) and torch.equal(q._placed.loc_y, ly) and torch.equal(q.h, h) and torch.equal(out, first)
                    # (b) the truth of the best swap: written into the pins through update(), predicted, summed
                    k = int(np.lexsort((np.arange(K), np.where(res['eligible'], res['dq'], 2 ** 62)))[0])
                    nx, ny = home_x.copy(), home_y.copy()
                    at_k = slice(int(c_ptr[k]), int(c_ptr[k + 1]))
                    nx[c_node[at_k] - off], ny[c_node[at_k] - off] = c_x[at_k], c_y[at_k]
                    truth.update(i, pin_x=nx, pin_y=ny)
                    assert _quanta_sum(truth.predict()[0].cpu().numpy(), required, rows_of[i]) == base['nsum'] + int(res['dq'][k]), (seed, i, k)
                    truth.update(i, pin_x=home_x, pin_y=home_y)
                    # (c) the commit: apply=False first - the same answer, nothing moved, the state fresh
                    dry = q.commit_swaps(splan, apply=False)
                    assert not q._trial.stale and torch.equal(q._placed.loc_x, lx) and torch.equal(q._placed.loc_y, ly) and torch.equal(q.h, h)
                    got = q.commit_swaps(splan)
                    assert q._trial.stale and (q._placed.loc_x.data_ptr(), q._placed.loc_y.data_ptr()) == at
                    sel, (n_sel, total, n_cand) = SW.select_host(want['pick'], want['dq'], splan.sel_ptr, splan.sel_row, T, G, 1)
                    for r in (got, dry):
                        WC.same_tables(r, want, (seed, i, 'commit'))
                        assert r['selected'].dtype == np.bool_ and np.array_equal(r['selected'], sel != 0)
                        assert (r['n_selected'], r['sum_dq'], r['n_candidates']) == (n_sel, total, n_cand)
                        assert r['predicted_nsum'] == base['nsum'] + total and r['gain'] == -total * 2.0 ** -20
                        assert np.array_equal(r['pair_gain'], want['gain']) and (r['rounds'] >= 1) == (n_cand > 0)
                    wx, wy = SW.apply_host(lx.cpu().numpy(), ly.cpu().numpy(), sel, want['pick'], pair_a, pair_b, plan.mv_ptr, plan.mv_node)
                    gx, gy = q._placed.loc_x.cpu().numpy(), q._placed.loc_y.cpu().numpy()
                    assert np.array_equal(gx, wx) and np.array_equal(gy, wy)
                    assert n_sel == 0 or not (np.array_equal(gx, lx.cpu().numpy()) and np.array_equal(gy, ly.cpu().numpy()))
                    for call in (q.swap_moves, q.commit_swaps):                   # stale until a predict()
                        with pytest.raises(RuntimeError, match='update\\(\\) has run'):
                            call(splan)
                    pred = q.predict()[0].cpu().numpy()
                    assert not q._trial.stale
                    assert _quanta_sum(pred, required, rows_of[i]) == got['predicted_nsum'], (seed, i)               # to the quantum
                    q.update(i, pin_x=home_x, pin_y=home_y)                       # back home for the next call
                    assert torch.equal(q.predict()[0], first) and torch.equal(q.h, h)
                    if calls is not None:                                         # no swap call captured or replayed a graph
                        assert q._replay.calls == calls + 2
                    cand = want['eligible'] & (want['dq'] <= -1)
                    by_row, by_group = WC.lost_how(sel, cand, splan.prow_ptr, splan.prow_row, pair_a, pair_b)
                    shown['improves'] |= bool((want['dq'] < 0).any())
                    shown['several'] |= n_sel >= 2
                    shown['lost_by_row'] |= bool(by_row)
                    shown['lost_by_group'] |= bool(by_group)
                    shown['useless'] |= bool((~want['eligible'] | (want['dq'] >= 0)).any())
                    print(f'seed {seed} design {i} graphed {q.graphed}: K {K} G {G} RP {RP} candidates {n_cand} selected {n_sel} rounds {got["rounds"]} '
                          f'sum_dq {total} lost by row {by_row} by group alone {by_group} ineligible {int((~want["eligible"]).sum())}')
            if all(shown.values()):
                break
        assert all(shown.values()), shown
        assert objs[1]._replay is None
        assert np.array_equal(U32(truth.predict()[0].cpu().numpy()), U32(base_pred))


def test_state_and_refusals(dev):
    from mmft.infer import Predictor
    from test_place_gpu import _live_models, _small_designs
    designs = list(_small_designs())
    d = designs[0]
    on = [int(v) for v in d.path_nodes[int(np.flatnonzero(d.path_lens >= 2)[0]), :2]]
    pins, a, b = np.array(on, dtype=np.int64), np.array([0], dtype=np.int64), np.array([1], dtype=np.int64)
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        plain = Predictor(pmodel, cnn, designs, dev, placement=True)
        p = Predictor(pmodel, cnn, designs, dev, placement=True, trials=True)
        other = Predictor(pmodel, cnn, designs, dev, placement=True, trials=True)
        plan = p.search_plan(0, pins)
        with pytest.raises(RuntimeError, match='swap_plan\\(\\): built without trials=True'):
            plain.swap_plan(plan, a, b)
        with pytest.raises(ValueError, match='swap_plan: the plan belongs to another Predictor'):
            other.swap_plan(plan, a, b)
        splan = p.swap_plan(plan, a, b)                                           # host only: fine before the first predict()
        assert (splan.K, splan.G) == (1, 2) and splan.RP >= 1 and splan.owner is p
        for call, who in ((plain.swap_moves, 'swap_moves'), (plain.commit_swaps, 'commit_swaps')):
            with pytest.raises(RuntimeError, match=f'{who}\\(\\): built without trials=True'):
                call(splan)
        with pytest.raises(RuntimeError, match='predict\\(\\) has not run'):
            p.swap_moves(splan)
        for _ in range(3):
            ref = p.predict()[0].clone()
            other.predict()
        good = p.swap_moves(splan)
        assert good['dq'].shape == (1,) and good['best_pair'].tolist() == ([0, 0] if good['eligible'][0] else [-1, -1])
        with pytest.raises(ValueError, match='swap_moves: the plan belongs to another Predictor'):
            other.swap_moves(splan)
        with pytest.raises(TypeError, match='swap_moves: the plan must come from swap_plan'):
            p.swap_moves(plan)
        for kw in (dict(scale_log2=31), dict(scale_log2=-1), dict(max_rows=0)):
            with pytest.raises(ValueError, match='swap_moves'):
                p.swap_moves(splan, **kw)
        for kw in (dict(min_gain=-1.0), dict(min_gain=float('nan')), dict(min_gain=2.0 ** 42), dict(max_rows=0)):
            with pytest.raises(ValueError):
                p.commit_swaps(splan, **kw)
        assert not p._trial.stale
        # a threshold nobody reaches: no candidate, nothing selected, the pins stay - and the state is stale all the same
        lx = p._placed.loc_x.clone()
        res = p.commit_swaps(splan, min_gain=1e6)
        assert (res['n_candidates'], res['n_selected'], res['rounds'], res['sum_dq'], res['gain']) == (0, 0, 0, 0, 0.0)
        assert not res['selected'].any() and res['predicted_nsum'] == res['base']['nsum'] and torch.equal(p._placed.loc_x, lx)
        for call in (p.swap_moves, p.commit_swaps, p.search_moves):
            with pytest.raises(RuntimeError, match='update\\(\\) has run'):
                call(splan if call != p.search_moves else plan)
        assert torch.equal(p.predict()[0], ref)
        WC.same_tables(p.swap_moves(splan), good, 'after a commit and predict()')
        graph, scratch = torch.cuda.CUDAGraph(), torch.zeros(4, device=dev)      # under a stream capture
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match='commit_swaps\\(\\) under an outer stream capture'):
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                scratch.add_(1.0)
                p.commit_swaps(splan)
        torch.cuda.synchronize()
        assert torch.equal(p.predict()[0], ref) and torch.equal(p._placed.loc_x, lx)
        with lib.math_mode('f32'):
            with pytest.raises(ValueError, match='swap_moves: bf16 math mode only'):
                p.swap_moves(splan)
