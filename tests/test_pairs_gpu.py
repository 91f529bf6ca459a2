"""The near pairs on the GPU (include/mmft_pairs.h, mmft.pairs): the five entry points against near_pairs_host and
swap.pair_tables word for word, mmft_pairs_scan against np.cumsum, Predictor.near_swap_plan against swap_plan on the host's
pairs, commit_swaps(patch=True) against the predict() that follows, and refine_swaps(patch=True) against patch=False on a
twin.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import pairs_cases as PC
import swap_cases as WC
from mmft import lib
from mmft import pairs as PR
from mmft import search as SE
from mmft import swap as SW
from test_commit_gpu import _set_required, _setup
from test_head_kernels_gpu import I32
from test_swap_gpu import _groups_and_pairs

pytestmark = pytest.mark.gpu
POISON = -7
TABLE_NAMES = ('pair_a', 'pair_b', 'prow_ptr', 'prow_row', 'prow_pair', 'sel_ptr', 'sel_row')


def same_bits(a, b):
    a, b = (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v) for v in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _guarded(n, dev, dtype=torch.int32):
    """(the buffer of n + 2 words of poison, its inner n words): a kernel may write the inner ones only."""
    buf = torch.full((n + 2,), POISON, dtype=dtype, device=dev)
    return buf, buf[1:n + 1]


def _intact(buf):
    return int(buf[0]) == POISON and int(buf[-1]) == POISON


# ------------------------------------------------------------------------------------------------ 1. the tables
def _build_on_device(dev, case, reach, klass):
    """The order of a build (mmft_pairs.h) on a case's tables, every output between two words of poison: the words of the
    plan (int32, numpy), K and RP.  Every intermediate table is held against the host's on the way."""
    mv_ptr, mv_node, grow_ptr, grow_row = case['mv_ptr'], case['mv_node'], case['grow_ptr'], case['grow_row']
    G, M, R, T, n_nodes = len(mv_ptr) - 1, len(mv_node), len(grow_row), case['T'], len(case['px'])
    d_mptr, d_node, d_x, d_y = I32(mv_ptr, dev), I32(mv_node, dev) if M else None, I32(case['px'], dev), I32(case['py'], dev)
    d_gptr, d_grow = I32(grow_ptr, dev), I32(grow_row, dev) if R else None
    d_kl = None if klass is None else I32(klass, dev)
    frozen = [t.clone() for t in (d_mptr, d_x, d_y, d_gptr)]
    want_a, want_b = PR.near_pairs_host(mv_ptr, mv_node, case['px'], case['py'], reach, klass)
    g_cnt, cnt = _guarded(G, dev)
    g_off, off = _guarded(G + 1, dev)
    g_tot, tot = _guarded(2, dev, torch.int64)
    PR.abi('mmft_pairs_near_count', d_mptr, d_node, G, M, d_x, d_y, n_nodes, d_kl, reach, cnt, *lib.stream_args(d_x))
    PR.abi('mmft_pairs_scan', cnt, G, off, tot[:1], *lib.stream_args(d_x))
    K = int(tot[0])
    counts = np.bincount(want_a, minlength=G)
    assert K == len(want_a) and np.array_equal(cnt.cpu().numpy(), counts) and np.array_equal(off.cpu().numpy(), np.concatenate([[0], np.cumsum(counts)]))
    g_pa, pa = _guarded(K, dev)
    g_pb, pb = _guarded(K, dev)
    g_pc, pcnt = _guarded(K, dev)
    g_pp, pptr = _guarded(K + 1, dev)
    PR.abi('mmft_pairs_near_fill', d_mptr, d_node, G, M, d_x, d_y, n_nodes, d_kl, reach, off, K, pa if K else None, pb if K else None, *lib.stream_args(d_x))
    PR.abi('mmft_pairs_rows_count', pa if K else None, pb if K else None, K, d_gptr, d_grow, G, R, pcnt if K else None, *lib.stream_args(d_x))
    PR.abi('mmft_pairs_scan', pcnt if K else None, K, pptr if K else None, tot[1:] if K else None, *lib.stream_args(d_x))
    RP = int(tot[1]) if K else 0
    g_row, prow = _guarded(RP, dev)
    g_pair, ppair = _guarded(RP, dev)
    g_sp, sptr = _guarded(K + 1, dev)
    g_sr, srow = _guarded(RP + 2 * K, dev)
    PR.abi('mmft_pairs_rows_fill', pa if K else None, pb if K else None, pptr if K else None, K, RP, d_gptr, d_grow, G, R, T,
           prow if RP else None, ppair if RP else None, sptr if K else None, srow if K else None, *lib.stream_args(d_x))
    for name, buf in dict(cnt=g_cnt, off=g_off, pair_a=g_pa, pair_b=g_pb, pcnt=g_pc, prow_ptr=g_pp, prow_row=g_row, prow_pair=g_pair, sel_ptr=g_sp,
                          sel_row=g_sr).items():
        assert _intact(buf), name                                                # the poison in front of and behind every output
    assert int(g_tot[0]) == POISON and int(g_tot[3]) == POISON and (K > 0 or int(g_tot[2]) == POISON)
    assert all(torch.equal(a, b) for a, b in zip((d_mptr, d_x, d_y, d_gptr), frozen))      # the inputs are read, never written
    if K == 0:                                                                    # an empty call writes nothing at all
        assert all(bool((b == POISON).all()) for b in (g_pp, g_sp, g_sr))
        return np.zeros(0, dtype=np.int32), 0, 0
    return torch.cat([pa, pb, pptr, prow, ppair, sptr, srow]).cpu().numpy(), K, RP


def _check_case(dev, case, reach, klass, where):
    words, K, RP = _build_on_device(dev, case, reach, klass)
    a, b = PR.near_pairs_host(case['mv_ptr'], case['mv_node'], case['px'], case['py'], reach, klass)
    if len(a) == 0:
        assert K == 0, where
        return 0
    tabs, want = PC.expected(case, a, b)
    assert (K, RP) == (len(a), tabs[3].shape[0]) and words.dtype == want.dtype and np.array_equal(words, want), where
    again, _, _ = _build_on_device(dev, case, reach, klass)
    assert same_bits(again, words), where                                         # same inputs, same bits
    return K


@pytest.mark.parametrize('name', PC.KERNEL_CASES)
def test_the_device_tables_equal_the_hosts_on_the_kernel_cases(dev, name):
    case = PC.kernel_case(name)
    seen = 0
    for reach in (1, 2, 40, PC.MAX_REACH):
        for klass in (None, np.arange(len(case['tags'])) % 2):
            seen += _check_case(dev, case, reach, klass, (name, reach, klass is not None))
    assert seen > 0


@pytest.mark.parametrize('G', [1, 2, 255, 256, 257, 1025])
def test_the_device_tables_equal_the_hosts_on_seeded_grids(dev, G):
    """Group counts that cross the workgroup of 256 groups, the tile of 1024 partners and the pairing of the workgroups' blocks
    (one block, two, five with a middle one)."""
    case = PC.seeded(0 if G == 257 else G, G=G)
    for reach in (1, 2):
        with_class = _check_case(dev, case, reach, case['klass'], (G, reach, 'class'))
        one_class = _check_case(dev, case, reach, None, (G, reach))
        assert one_class >= with_class and (G < 255 or one_class > with_class > 0)
        print(f'G {G} reach {reach}: K {with_class} with classes, {one_class} without')


# ------------------------------------------------------------------------------------------------ 2. the scan
def _scan(dev, values):
    n = len(values)
    g_out, out = _guarded(n + 1, dev)
    g_tot, tot = _guarded(1, dev, torch.int64)
    d_in = I32(values, dev)
    keep = d_in.clone()
    PR.abi('mmft_pairs_scan', d_in, n, out, tot, *lib.stream_args(d_in))
    assert _intact(g_out) and _intact(g_tot) and torch.equal(d_in, keep)
    return out.cpu().numpy(), int(tot[0])


@pytest.mark.parametrize('n', [1, 2, 1023, 1024, 1025, 4095, 4096, 4097, 70000])
def test_scan_equals_cumsum_and_keeps_the_total_in_64_bits(dev, n):
    """The sizes cross the wave, the workgroup of 1024 threads and the round of 4096 elements; counts of 2^20 over 70 000
    elements pass 2^31, where the header defines the int32 words as the low 32 bits of the exact sums."""
    rng = np.random.default_rng(n)
    cases = [rng.integers(0, 6, n) * (rng.random(n) < 0.7), np.zeros(n, dtype=np.int64), rng.integers(-4, 5, n)]
    if n == 70000:
        big = np.full(n, 2 ** 20, dtype=np.int64)
        big[rng.random(n) < 0.1] = 0
        cases.append(big)
    for values in cases:
        values = np.asarray(values, dtype=np.int64)
        exact = np.concatenate([[0], np.cumsum(values, dtype=np.int64)])
        out, total = _scan(dev, values)
        assert total == int(exact[-1])
        assert out.dtype == np.int32 and np.array_equal(out, (exact & 0xffffffff).astype(np.uint32).view(np.int32))
        if abs(exact).max() < 2 ** 31:
            assert np.array_equal(out.astype(np.int64), exact)
        else:
            assert total > 2 ** 31 and int(out[-1]) != total and total == 2 ** 20 * int((values != 0).sum())
        again, total2 = _scan(dev, values)
        assert same_bits(again, out) and total2 == total


# ------------------------------------------------------------------------------------------------ 3. - 5. the Predictor
def _rows_of(truth, designs):
    return [np.flatnonzero(np.asarray(truth.row_design) == i) for i in range(len(designs))]


def _same_plan(got, want, where):
    assert (got.K, got.RP, got.G, got.T, got.i) == (want.K, want.RP, want.G, want.T, want.i), where
    for name in TABLE_NAMES:
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype == np.int64 and np.array_equal(g, w), (where, name)
    assert got.ints.dtype == torch.int32 and torch.equal(got.ints, want.ints), where
    assert len(got.dev) == 7 and all(torch.equal(a, b) for a, b in zip(got.dev, want.dev))


def _same_commit(got, want, where):
    WC.same_tables(got, want, where)
    for k in ('selected', 'pair_gain', 'best_pair', 'best_pair_dq'):
        assert np.array_equal(got[k], want[k]), (where, k)
    for k in ('n_selected', 'n_candidates', 'sum_dq', 'predicted_nsum', 'gain', 'base', 'rounds'):
        assert got[k] == want[k], (where, k)


def test_near_swap_plan_equals_swap_plan_on_the_hosts_pairs(dev):
    with lib.math_mode('bf16'):
        designs, truth, twin, objs, first = _setup(dev)
        base_pred = first.cpu().numpy()
        rows_of = _rows_of(truth, designs)
        required = _set_required(first, 0, [truth, twin] + objs)
        some = followed = 0
        for i, d in enumerate(designs):
            N, off = int(d.N), int(twin._placed.node_off[i])
            home_x, home_y = np.asarray(d.pin_x), np.asarray(d.pin_y)
            pins, gptr, _, _ = _groups_and_pairs(twin._trial, twin._placed.node_off, i, N, rows_of[i], base_pred, required, 0)
            for q in objs:
                plan = q.search_plan(i, pins, gptr)
                G = plan.G
                assert torch.equal(q.predict()[0], first)
                pins_now = lambda: (q._placed.loc_x.cpu().numpy(), q._placed.loc_y.cpu().numpy())
                calls = q._replay.calls if q._replay is not None else None
                for reach in (1, 2, 5):
                    for klass in (None, np.arange(G) % 3, torch.arange(G, dtype=torch.int32) % 2):
                        host_kl = klass.numpy() if torch.is_tensor(klass) else klass
                        a, b = PR.near_pairs_host(plan.mv_ptr, plan.mv_node, *pins_now(), reach, host_kl)
                        sp = q.near_swap_plan(plan, reach, klass)
                        if len(a) == 0:
                            assert sp is None
                            continue
                        want = q.swap_plan(plan, a, b)
                        _same_plan(sp, want, (i, reach))
                        some += 1
                sp, want = q.near_swap_plan(plan, 2), q.swap_plan(plan, *PR.near_pairs_host(plan.mv_ptr, plan.mv_node, *pins_now(), 2))
                WC.same_tables(q.swap_moves(sp), q.swap_moves(want), (i, 'swap_moves'))
                with pytest.raises(ValueError, match=f'near_swap_plan: K = {sp.K} near pairs exceed max_pairs = {sp.K - 1}'):
                    q.near_swap_plan(plan, 2, max_pairs=sp.K - 1)
                assert q.near_swap_plan(plan, 2, max_pairs=sp.K).K == sp.K
                # an anchor moves - update() - and a new call follows it: group g0 is put beside a group it was not near
                lx, ly = pins_now()
                anchor = plan.mv_node[plan.mv_ptr[:-1]]
                near = set(zip(sp.pair_a.tolist(), sp.pair_b.tolist()))
                g0, g1 = next((u, v) for u in range(G) for v in range(u + 1, G) if (u, v) not in near and plan.mv_ptr[u + 1] - plan.mv_ptr[u] == 1
                              and plan.mv_ptr[v + 1] - plan.mv_ptr[v] == 1 and max(abs(int(lx[anchor[u]]) - int(lx[anchor[v]])),
                                                                                  abs(int(ly[anchor[u]]) - int(ly[anchor[v]]))) > 2)
                nx, ny = home_x.copy(), home_y.copy()
                x1 = int(lx[anchor[g1]])
                nx[anchor[g0] - off], ny[anchor[g0] - off] = (x1 + 1 if x1 < 8 else x1 - 1), int(ly[anchor[g1]])
                q.update(i, pin_x=nx, pin_y=ny)
                moved = q.near_swap_plan(plan, 2)                                 # no predict(): it reads pins only
                assert q._trial.stale and (g0, g1) in set(zip(moved.pair_a.tolist(), moved.pair_b.tolist()))
                _same_plan(moved, q.swap_plan(plan, *PR.near_pairs_host(plan.mv_ptr, plan.mv_node, *pins_now(), 2)), (i, 'moved'))
                followed += 1
                q.update(i, pin_x=home_x, pin_y=home_y)
                assert torch.equal(q.predict()[0], first)
                if calls is not None:                                             # the two predict() calls alone
                    assert q._replay.calls == calls + 1
            # two pins far from each other, reach 1: nothing is near, and that is None
            q = objs[0]
            lx, ly = q._placed.loc_x.cpu().numpy()[off:off + N], q._placed.loc_y.cpu().numpy()[off:off + N]
            u = 0
            v = next(n for n in range(1, N) if max(abs(int(lx[n]) - int(lx[u])), abs(int(ly[n]) - int(ly[u]))) > 1)
            apart = q.search_plan(i, np.array([u, v], dtype=np.int64))
            assert q.near_swap_plan(apart, 1) is None
        assert some >= 8 and followed == 2 * len(designs)


def _entries(sp, selected):
    """bool [T]: the rows of the selected pairs' entries, and their number."""
    mine = np.zeros(sp.T, dtype=bool)
    n = 0
    for k in np.flatnonzero(selected):
        rows = sp.prow_row[sp.prow_ptr[k]:sp.prow_ptr[k + 1]]
        assert not mine[rows].any()                                               # the selected pairs share no row
        mine[rows] = True
        n += rows.shape[0]
    return mine, n


def test_the_patched_swap_commit_is_what_the_next_predict_writes(dev):
    with lib.math_mode('bf16'):
        designs, truth, twin, objs, first = _setup(dev)
        base_pred = first.cpu().numpy()
        T = base_pred.shape[0]
        rows_of = _rows_of(truth, designs)
        several = chunked = False
        for seed in range(4):                                                     # seeds until one selects two pairs or more
            required = _set_required(first, seed, [truth, twin] + objs)
            for i, d in enumerate(designs):
                N, off = int(d.N), int(twin._placed.node_off[i])
                home_x, home_y = np.asarray(d.pin_x), np.asarray(d.pin_y)
                pins, gptr, _, _ = _groups_and_pairs(twin._trial, twin._placed.node_off, i, N, rows_of[i], base_pred, required, seed)
                tplan = twin.search_plan(i, pins, gptr)
                for q in objs:
                    plan = q.search_plan(i, pins, gptr)
                    RP = q.near_swap_plan(plan, 3).RP
                    for max_rows in (65536, 1, RP // 3 + 1):
                        assert torch.equal(q.predict()[0], first) and torch.equal(twin.predict()[0], first)
                        sp = q.near_swap_plan(plan, 3)
                        tsp = twin.swap_plan(tplan, sp.pair_a, sp.pair_b)
                        n_chunks = len(SW.chunks(sp.prow_ptr, max_rows))
                        assert sp.RP == RP and (n_chunks == 1) == (max_rows == 65536)
                        kept = q._trial.kept
                        lx, ly = q._placed.loc_x.cpu().numpy(), q._placed.loc_y.cpu().numpy()
                        x0, calls = kept['x'].cpu().numpy(), (q._replay.calls if q._replay is not None else None)
                        res = q.commit_swaps(sp, patch=True, max_rows=max_rows)
                        assert not q._trial.stale and (calls is None or q._replay.calls == calls)
                        kx, kp = q._trial.kept['x'].clone(), q._trial.kept['pred'].clone()
                        ref = twin.commit_swaps(tsp)                              # patch=False on the twin: the same tables
                        assert twin._trial.stale and 'n_patched' not in ref
                        _same_commit(res, ref, (seed, i, max_rows))
                        wx, wy = SW.apply_host(lx, ly, res['selected'], np.where(res['eligible'], 0, -1), sp.pair_a, sp.pair_b, plan.mv_ptr, plan.mv_node)
                        assert np.array_equal(q._placed.loc_x.cpu().numpy(), wx) and np.array_equal(q._placed.loc_y.cpu().numpy(), wy)
                        assert torch.equal(q._placed.loc_x, twin._placed.loc_x) and torch.equal(q._placed.loc_y, twin._placed.loc_y)
                        mine, n = _entries(sp, res['selected'])
                        assert res['n_patched'] == n
                        rest = np.flatnonzero(~mine)
                        assert same_bits(kx.cpu().numpy()[rest], x0[rest]) and same_bits(kp.cpu().numpy().reshape(-1)[rest], base_pred[rest])
                        cnn_col, Dout = kept['cnn_col'], q.pmodel.fcn.weight.shape[0]
                        outside = np.r_[0:cnn_col, cnn_col + Dout:x0.shape[1]]
                        assert same_bits(kx.cpu().numpy()[:, outside], x0[:, outside])        # on the patched rows only the h_cnn columns moved
                        # the calls that follow at once equal the twin's after commit_swaps() + predict()
                        truth_pred = twin.predict()[0]
                        WC.same_tables(q.swap_moves(sp), twin.swap_moves(tsp), (seed, i, max_rows, 'swap_moves'))
                        c_ptr, c_node, c_x, c_y = SW.swapped_coords(wx, wy, plan.mv_ptr, plan.mv_node, sp.pair_a[:4], sp.pair_b[:4])
                        tm = [p.trial_moves(i, c_node - off, c_x.astype(np.int64), c_y.astype(np.int64), c_ptr) for p in (q, twin)]
                        assert np.array_equal(tm[0]['rows'], tm[1]['rows']) and same_bits(tm[0]['pred'], tm[1]['pred'])
                        assert calls is None or q._replay.calls == calls          # no swap call captured or replayed a graph
                        pred = q.predict()[0]
                        assert same_bits(q._trial.kept['x'], kx) and same_bits(q._trial.kept['pred'], kp) and same_bits(pred, kp)
                        assert same_bits(pred, truth_pred)
                        assert SE.base_host(kp.cpu().numpy().reshape(-1), required, rows_of[i])['nsum'] == res['predicted_nsum']
                        print(f'seed {seed} design {i} graphed {q.graphed} max_rows {max_rows}: K {sp.K} RP {sp.RP} chunks {n_chunks} '
                              f'selected {res["n_selected"]} patched {n}')
                        several |= res['n_selected'] >= 2
                        chunked |= n_chunks >= 3 and res['n_selected'] >= 1
                        q.commit_swaps(sp, patch=True, min_gain=1e6)              # nothing selected: the state stays fresh ...
                        assert not q._trial.stale
                        q.update(i, pin_x=home_x, pin_y=home_y)                   # ... and update() makes it stale again; back home
                        twin.update(i, pin_x=home_x, pin_y=home_y)
                        assert q._trial.stale
                        if calls is not None:
                            assert q._replay.calls == calls + 1                   # the predict() above alone
            if several and chunked:
                break
        assert several and chunked
        assert objs[1]._replay is None
        with pytest.raises(ValueError, match='commit_swaps: patch=True .*needs apply=True'):
            objs[0].commit_swaps(sp, patch=True, apply=False)


def _required_at(first, frac, everyone):
    """Required times at one quantile of the resident predictions, the same for every row: a share `frac` of the rows meets
    them, the others violate by as much as the predictions spread - slacks on which a swap has whole quanta to gain, pass after
    pass.  (The required times of _set_required lie a hair beside the predictions: a first pass takes what there is.)"""
    near = torch.full_like(first, float(torch.quantile(first.float(), frac)))
    for q in everyone:
        q.required.copy_(near)
    return near.cpu().numpy()


def test_refine_swaps_patched_equals_the_loop_with_a_predict_per_pass(dev):
    with lib.math_mode('bf16'):
        designs, truth, twin, objs, first = _setup(dev)
        base_pred = first.cpu().numpy()
        rows_of = _rows_of(truth, designs)
        repaired = None
        inputs = [('seed', s) for s in range(4)] + [('quantile', f) for f in (0.5, 0.25, 0.75)]
        for seed, (kind, value) in enumerate(inputs):                             # inputs until the re-pairing mattered
            everyone = [truth, twin] + objs
            required = _set_required(first, value, everyone) if kind == 'seed' else _required_at(first, value, everyone)
            for i, d in enumerate(designs):
                N = int(d.N)
                home_x, home_y = np.asarray(d.pin_x), np.asarray(d.pin_y)
                pins, gptr, _, _ = _groups_and_pairs(twin._trial, twin._placed.node_off, i, N, rows_of[i], base_pred, required, seed)
                tplan = twin.search_plan(i, pins, gptr)
                klass = np.arange(tplan.G) % 2 if seed % 2 else None
                for q in objs:
                    plan = q.search_plan(i, pins, gptr)
                    assert torch.equal(q.predict()[0], first) and torch.equal(twin.predict()[0], first)
                    calls = q._replay.calls if q._replay is not None else None
                    got = q.refine_swaps(plan, 3, passes=4, group_class=klass)
                    want = twin.refine_swaps(tplan, 3, passes=4, patch=False, group_class=klass)
                    assert len(got) == len(want) >= 1 and not q._trial.stale and not twin._trial.stale
                    for k, (g, w) in enumerate(zip(got, want)):
                        assert np.array_equal(g['pair_a'], w['pair_a']) and np.array_equal(g['pair_b'], w['pair_b']), (seed, i, k)
                        _same_commit(g, w, (seed, i, k))
                        assert 'n_patched' in g and 'n_patched' not in w and g['sum_dq'] <= 0
                        if k:
                            assert g['base']['nsum'] == got[k - 1]['predicted_nsum']          # the sums never increase
                    assert all(g['n_selected'] > 0 for g in got[:-1])
                    assert torch.equal(q._placed.loc_x, twin._placed.loc_x) and torch.equal(q._placed.loc_y, twin._placed.loc_y)
                    pq, pt = q.predict()[0], twin.predict()[0]
                    assert same_bits(pq, pt)
                    assert SE.base_host(pq.cpu().numpy(), required, rows_of[i])['nsum'] == got[-1]['predicted_nsum']
                    if calls is not None:                                         # one predict() behind the loop, and the one above
                        assert q._replay.calls == calls + 2
                    selecting = [g for g in got if g['n_selected'] > 0]
                    differ = len(selecting) >= 2 and any(not (np.array_equal(u['pair_a'], v['pair_a']) and np.array_equal(u['pair_b'], v['pair_b']))
                                                         for u, v in zip(selecting[:-1], selecting[1:]))
                    print(f'{kind} {value} design {i} graphed {q.graphed}: passes {len(got)} K {[len(g["pair_a"]) for g in got]} selected '
                          f'{[g["n_selected"] for g in got]} nsum {[g["predicted_nsum"] for g in got]} re-paired {differ}')
                    if differ and repaired is None:
                        repaired = (kind, value, i)
                    for p in (q, twin):
                        p.update(i, pin_x=home_x, pin_y=home_y)
            if repaired is not None:
                break
        assert repaired is not None                                               # two selecting passes whose pair lists differ
        print(f're-pairing mattered first at {repaired[0]} {repaired[1]}, design {repaired[2]}')
        q = objs[0]
        q.predict()
        cplan = q.search_plan(i, pins, gptr)
        graph, scratch = torch.cuda.CUDAGraph(), torch.zeros(4, device=dev)       # under a stream capture
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match='refine_swaps\\(\\) under an outer stream capture'):
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                scratch.add_(1.0)
                q.refine_swaps(cplan, 3)
        torch.cuda.synchronize()
        q.update(0, pin_x=np.asarray(designs[0].pin_x), pin_y=np.asarray(designs[0].pin_y))
        with pytest.raises(RuntimeError, match='refine_swaps\\(\\): update\\(\\) has run'):
            q.refine_swaps(q.search_plan(0, pins[:2]), 3)
