"""The critical cells on the GPU (include/mmft_cells.h, mmft.cells): the two entry points and the three scans between them
against cells.count_host / critical_host -> search.plan_tables word for word on synthetic tables, Predictor.critical_plan against
search_plan on the cells the host picks from the downloaded kept predictions - after predict(), after update() + predict() and
after a patched commit without a predict() -, and refine_cells(patch=True) against patch=False on a twin and against the
written-out host loop.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import cells_cases as KC
import search_cases as SC
from mmft import cells as CL
from mmft import lib
from mmft import pairs as PR
from mmft import search as SE
from test_commit_gpu import _set_required, _setup
from test_head_kernels_gpu import I32
from test_pairs_gpu import _guarded, _intact, _required_at, same_bits, POISON

pytestmark = pytest.mark.gpu
F32 = lambda a, dev: torch.as_tensor(np.asarray(a, dtype=np.float32)).to(dev)


# ------------------------------------------------------------------------------------------------ 1. the kernels
def _upload(dev, case):
    ptr, rows = case['inc']
    M, nnz = len(case['pins']), len(rows)
    return dict(cptr=I32(case['cell_ptr'], dev), cnode=I32(case['pins'] + KC.NODE_OFF, dev) if M else None, iptr=I32(ptr, dev),
                irow=I32(rows, dev) if nnz else None, pred=F32(case['pred'], dev), required=F32(case['required'], dev), M=M, nnz=nnz,
                N=len(ptr) - 1)


def _build_on_device(dev, case, thr, d=None):
    """The order of a build (mmft_cells.h) on a case's tables, every output between two words of poison: the words of the
    buffer (int32, numpy; None where nothing is selected).  Every intermediate table is held against the host's on the way."""
    d = d or _upload(dev, case)
    C, M, N, nnz, T, lo, span = case['C'], d['M'], d['N'], d['nnz'], case['T'], case['row_lo'], case['span']
    inputs = [t for t in (d['cptr'], d['cnode'], d['iptr'], d['irow'], d['pred'], d['required']) if t is not None]
    frozen = [t.clone() for t in inputs]
    g_sel, sel = _guarded(C, dev)
    g_nr, n_rows = _guarded(C, dev)
    g_np, n_pins = _guarded(C, dev)
    g_w, worst = _guarded(C, dev)
    g_off = [_guarded(C + 1, dev) for _ in range(3)]
    g_tot, tot = _guarded(3, dev, torch.int64)
    CL.abi('mmft_cells_count', d['cptr'], d['cnode'], C, M, d['iptr'], d['irow'], N, nnz, d['pred'], d['required'], T, lo, span,
           0 if thr is None else 1, 0.0 if thr is None else thr, sel, n_rows, n_pins, worst, *lib.stream_args(sel))
    for k, counts in enumerate((sel, n_rows, n_pins)):
        PR.abi('mmft_pairs_scan', counts, C, g_off[k][1], tot[k:k + 1], *lib.stream_args(sel))
    G, R, MP = (int(v) for v in tot.tolist())
    h_sel, h_rows, h_pins, h_worst = KC.host(case, thr)
    for got, want in ((sel, h_sel), (n_rows, h_rows), (n_pins, h_pins)):
        assert np.array_equal(got.cpu().numpy(), want.astype(np.int32))
    assert worst.cpu().numpy().tobytes() == h_worst.view(np.int32).tobytes()      # the bits, NaN included
    for (_, off), want in zip(g_off, (h_sel, h_rows, h_pins)):
        assert np.array_equal(off.cpu().numpy(), np.concatenate([[0], np.cumsum(want.astype(np.int64))]))
    chosen, tables, want_words = KC.expected(case, thr)
    assert G == len(chosen) and (G == 0 or (R, MP) == (tables[1].shape[0], tables[4].shape[0]))
    outs = [_guarded(n, dev) for n in (G + 1, R, R, G + 1, MP, G, G)]
    t = [inner for _, inner in outs]
    CL.abi('mmft_cells_fill', d['cptr'], d['cnode'], C, M, d['iptr'], d['irow'], N, nnz, lo, span, sel, worst, g_off[0][1], g_off[1][1], g_off[2][1],
           G, R, MP, t[0], t[1] if R else None, t[2] if R else None, t[3], t[4] if MP else None, t[5], t[6], *lib.stream_args(sel))
    for name, buf in dict(sel=g_sel, n_rows=g_nr, n_pins=g_np, worst=g_w, sel_off=g_off[0][0], row_off=g_off[1][0], pin_off=g_off[2][0],
                          grow_ptr=outs[0][0], grow_row=outs[1][0], grow_grp=outs[2][0], mv_ptr=outs[3][0], mv_node=outs[4][0], group_cell=outs[5][0],
                          group_worst=outs[6][0]).items():
        assert _intact(buf), name                                                # the poison in front of and behind every output
    assert int(g_tot[0]) == POISON and int(g_tot[4]) == POISON
    assert all(torch.equal(a, b) or (a.dtype == torch.float32 and same_bits(a, b)) for a, b in zip(inputs, frozen))      # read, never written
    if G == 0:                                                                    # a call that selects nothing writes no table word
        assert want_words is None and all(bool((buf == POISON).all()) for buf, _ in outs)
        return None
    words = torch.cat(t).cpu().numpy()
    assert words.dtype == want_words.dtype and np.array_equal(words, want_words)
    return words


@pytest.mark.parametrize('span', KC.SPANS)
def test_the_device_tables_equal_the_hosts_on_every_cell_count(dev, span):
    """Cell counts from one wave to many workgroups at every word edge of the bitmap; row_lo > 0; the crafted cells (a pin of 300
    rows, twin pins, rows at both ends of the range and outside it, cells of 0, 1, 8, 64 and 65 pins) as far as C reaches."""
    some = 0
    for C in KC.COUNTS:
        case = KC.make(C, span)
        assert case['row_lo'] > 0 and int(np.diff(case['inc'][0]).max()) == KC.LONG
        d = _upload(dev, case)
        for thr in (0.0, -0.25, None, -1e30):
            words = _build_on_device(dev, case, thr, d)
            assert words is None or thr != -1e30                                  # nothing lies below -1e30
            if words is not None:
                some += 1
                assert same_bits(_build_on_device(dev, case, thr, d), words)      # same inputs, same bits
    assert some >= 2 * len(KC.COUNTS)


def test_a_changed_prediction_changes_the_selection_as_the_host_says(dev):
    case = KC.make(63, 65)
    before = KC.expected(case, 0.0)[0]
    _build_on_device(dev, case, 0.0)
    lit = KC.literal(case, 0.0)
    c_in = next(c for c in before if len(lit[c]['rows']) == 1 and lit[c]['below'] >= 1)          # a cell selected through one row: it leaves
    c_out = next(c for c, v in enumerate(lit) if v['why'] == 'not_below' and v['rows'][0] != lit[c_in]['rows'][0])      # it enters
    moved = dict(case, pred=case['pred'].copy())
    moved['pred'][lit[c_in]['rows'][0]] = case['required'][lit[c_in]['rows'][0]] - np.float32(1.0)         # slack +1
    moved['pred'][lit[c_out]['rows'][0]] = case['required'][lit[c_out]['rows'][0]] + np.float32(1.0)       # slack -1
    after = KC.expected(moved, 0.0)[0]
    assert c_in in before and c_in not in after and c_out not in before and c_out in after
    assert _build_on_device(dev, moved, 0.0) is not None


# ------------------------------------------------------------------------------------------------ 2. the Predictor
def _partition(state, node_off, i, N, seed):
    """(pins, cell_ptr): a seeded partition of every node of design i into one cell of 64, eights and singles - the pins on a row -
    and the idle pins, each a cell of its own without a row."""
    ptr, _ = state.rows_of_pin
    off = int(node_off[i])
    deg = np.diff(ptr[off:off + N + 1])
    rng = np.random.default_rng(seed)
    busy, idle = rng.permutation(np.flatnonzero(deg > 0)), np.flatnonzero(deg == 0)
    assert busy.size >= 64 + 16 * 8 + 32 and idle.size > 0
    n8 = (busy.size - 64) // 24                                                   # a third of the rest in eights
    sizes = [64] + [8] * n8 + [1] * (busy.size - 64 - 8 * n8 + idle.size)
    pins = np.concatenate([busy, idle]).astype(np.int64)
    assert pins.size == N and np.unique(pins).size == N
    return pins, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _kept(q):
    return q._trial.kept['pred'].detach().cpu().numpy().reshape(-1).copy(), q.required.cpu().numpy()


def _host_plan(q, cs, thr):
    """(search_plan on the cells critical_host picks from the downloaded kept predictions, the cells, their worst); None."""
    pred, required = _kept(q)
    chosen, worst = CL.critical_host(q._trial.rows_of_pin, cs.node_off, cs.pins, cs.cell_ptr, pred, required, cs.row_lo, cs.span, thr)
    if chosen.size == 0:
        return None, chosen, worst
    return q.search_plan(cs.i, *CL.pins_of(cs.pins, cs.cell_ptr, chosen)), chosen, worst


def _same_plan(got, want, chosen, worst, where):
    assert (got.G, got.R, got.M, got.i, got.node_off) == (want.G, want.R, want.M, want.i, want.node_off), where
    for name in ('grow_ptr', 'grow_row', 'grow_grp', 'mv_ptr', 'mv_node'):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype == np.int64 and np.array_equal(g, w), (where, name)
    assert got.ints.dtype == torch.int32 and torch.equal(got.ints, want.ints), where             # bit for bit
    assert len(got.dev) == 5 and all(torch.equal(a, b) for a, b in zip(got.dev, want.dev))
    assert got.pins_distinct is True and got.owner is want.owner
    assert got.cell.dtype == np.int64 and np.array_equal(got.cell, chosen), where
    assert got.worst.dtype == np.float32 and got.worst.tobytes() == np.asarray(worst, dtype=np.float32).tobytes(), where


def _check_now(q, cs, thr, where):
    want, chosen, worst = _host_plan(q, cs, thr)
    got = q.critical_plan(cs, thr)
    if want is None:
        assert got is None, where
        return None, chosen
    _same_plan(got, want, chosen, worst, where)
    return got, chosen


def test_critical_plan_equals_search_plan_on_the_cells_the_host_picks(dev):
    with lib.math_mode('bf16'):
        designs, truth, twin, objs, first = _setup(dev)
        everyone = [truth, twin] + objs
        committed = changed = 0
        for i, d in enumerate(designs):
            N = int(d.N)
            home_x, home_y = np.asarray(d.pin_x), np.asarray(d.pin_y)
            pins, cptr = _partition(twin._trial, twin._placed.node_off, i, N, i)
            for q in objs:
                cs = q.cell_set(i, pins, cptr)
                rows = q.slack.rows_of(i)
                assert (cs.row_lo, cs.span) == (int(rows.min()), int(rows.max()) - int(rows.min()) + 1) and cs.span <= CL.MAX_SPAN
                calls = q._replay.calls if q._replay is not None else None
                if not getattr(q._trial, 'ready', False):                                         # (the eager one has not predicted yet)
                    with pytest.raises(RuntimeError, match='critical_plan\\(\\): predict\\(\\) has not run yet'):
                        q.critical_plan(cs, None)
                q.predict()
                # no threshold: every cell, and the plan of search_plan on the whole set, host tables included
                everything = q.critical_plan(cs, None)
                whole = q.search_plan(i, pins, cptr)
                _same_plan(everything, whole, np.arange(cs.C), CL.count_host(q._trial.rows_of_pin, cs.node_off, pins, cptr, *_kept(q), cs.row_lo,
                                                                             cs.span, None)[3], (i, 'None'))
                assert np.isnan(everything.worst).any() and (np.diff(whole.grow_ptr) == 0).any()  # the idle pins: cells without a row
                for seed in (0, 1):
                    _set_required(first, seed, everyone)
                    assert torch.equal(q.predict()[0], first)
                    plan, chosen = _check_now(q, cs, 0.0, (i, seed, 'predict'))                   # after predict()
                    assert plan is not None and 0 < plan.G < cs.C
                    want, _, _ = _host_plan(q, cs, 0.0)
                    SC.same_tables(q.search_moves(plan), q.search_moves(want), (i, seed, 'search_moves'))
                    with pytest.raises(ValueError, match=f'critical_plan: G = {plan.G} selected cells exceed max_groups = {plan.G - 1}'):
                        q.critical_plan(cs, 0.0, max_groups=plan.G - 1)
                    assert q.critical_plan(cs, 0.0, max_groups=plan.G).G == plan.G
                    # an update(): stale until predict(), then the selection of the moved pins
                    nx, ny = home_x.copy(), home_y.copy()
                    mv = pins[:64]
                    nx[mv], ny[mv] = (nx[mv] + 3) % 16, (ny[mv] + 5) % 16
                    q.update(i, pin_x=nx, pin_y=ny)
                    with pytest.raises(RuntimeError, match='critical_plan\\(\\): update\\(\\) has run'):
                        q.critical_plan(cs, 0.0)
                    q.predict()
                    plan_u, chosen_u = _check_now(q, cs, 0.0, (i, seed, 'update'))
                    q.update(i, pin_x=home_x, pin_y=home_y)
                    assert torch.equal(q.predict()[0], first)
                    # a patched commit and NO predict(): the case the feature exists for
                    before, _ = _kept(q)
                    res = q.commit_moves(plan, 1, patch=True)
                    assert not q._trial.stale
                    after, _ = _kept(q)
                    plan_c, chosen_c = _check_now(q, cs, 0.0, (i, seed, 'commit'))
                    committed += res['n_selected'] > 0
                    changed += not np.array_equal(chosen_c, chosen)
                    assert (res['n_selected'] > 0) == (not same_bits(before, after))
                    print(f'design {i} graphed {q.graphed} seed {seed}: C {cs.C} G {plan.G} R {plan.R} after update {len(chosen_u)} '
                          f'committed {res["n_selected"]} after commit {len(chosen_c)}')
                    if plan_c is not None:                                                        # an unpatched commit: stale
                        q.commit_moves(plan_c, 1)
                        if q._trial.stale:
                            with pytest.raises(RuntimeError, match='critical_plan\\(\\): update\\(\\) has run'):
                                q.critical_plan(cs, 0.0)
                    q.update(i, pin_x=home_x, pin_y=home_y)
                    assert torch.equal(q.predict()[0], first)
                for other in everyone:                                                            # no row violates: None
                    other.required.copy_(first + first.abs() + 1.0)
                assert q.critical_plan(cs, 0.0) is None and q.critical_plan(cs, None).G == cs.C
                assert q.critical_plan(cs, float('inf')).G == int((np.diff(whole.grow_ptr) > 0).sum())           # every cell with a row
                with pytest.raises(ValueError, match='the cell set belongs to another Predictor'):
                    twin.critical_plan(cs, 0.0)
                if calls is not None:                                                             # the predict() calls above alone
                    assert q._replay.calls == calls + 1 + 2 * 4
        assert committed >= 2 and changed >= 1
        q = objs[0]
        cs = q.cell_set(0, np.arange(8, dtype=np.int64))
        graph, scratch = torch.cuda.CUDAGraph(), torch.zeros(4, device=dev)                       # under a stream capture
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match='critical_plan\\(\\) under an outer stream capture'):
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                scratch.add_(1.0)
                q.critical_plan(cs, 0.0)
        torch.cuda.synchronize()


def test_refine_cells_patched_equals_a_predict_per_pass_and_the_host_loop(dev):
    with lib.math_mode('bf16'):
        designs, truth, twin, objs, first = _setup(dev)
        q, loop = objs                                                                            # graphed: refine_cells; eager: the host loop
        everyone = [truth, twin] + objs
        rows_of = [np.flatnonzero(np.asarray(truth.row_design) == i) for i in range(len(designs))]
        retargeted = None
        inputs = [('quantile', f) for f in (0.5, 0.25, 0.75)] + [('seed', s) for s in range(4)]
        for kind, value in inputs:                                                                # inputs until the re-targeting mattered
            required = _required_at(first, value, everyone) if kind == 'quantile' else _set_required(first, value, everyone)
            for i, d in enumerate(designs):
                N = int(d.N)
                home_x, home_y = np.asarray(d.pin_x), np.asarray(d.pin_y)
                pins, cptr = _partition(twin._trial, twin._placed.node_off, i, N, i)
                cs, tcs, lcs = (p.cell_set(i, pins, cptr) for p in (q, twin, loop))
                for p in (q, twin, loop):
                    assert torch.equal(p.predict()[0], first)
                calls = q._replay.calls
                got = q.refine_cells(cs, 1, passes=4)
                want = twin.refine_cells(tcs, 1, passes=4, patch=False)
                by_hand = []                                                                      # critical_host -> search_plan -> commit_moves(patch=True)
                for _ in range(4):
                    plan, chosen, _ = _host_plan(loop, lcs, 0.0)
                    if plan is None:
                        break
                    by_hand.append(dict(loop.commit_moves(plan, 1, patch=True), cell=chosen))
                    if by_hand[-1]['n_selected'] == 0:
                        break
                final = loop.predict()[0]
                assert len(got) == len(want) == len(by_hand) and not q._trial.stale and not twin._trial.stale
                assert q._replay.calls == calls + 1                                               # one predict() behind the loop
                for k, (g, w, h) in enumerate(zip(got, want, by_hand)):
                    for o in (w, h):
                        assert g['cell'].dtype == np.int64 and np.array_equal(g['cell'], o['cell']), (kind, value, i, k)
                        assert np.array_equal(g['selected'], o['selected']) and g['sum_dq'] == o['sum_dq'], (kind, value, i, k)
                        SC.same_tables(g, o, (kind, value, i, k))
                        assert g['base'] == o['base'] and g['predicted_nsum'] == o['predicted_nsum']
                    assert 'n_patched' in g and 'n_patched' not in w and g['sum_dq'] <= 0
                    if k:
                        assert g['base']['nsum'] == got[k - 1]['predicted_nsum']                  # each pass starts where the last one ended
                assert all(g['n_selected'] > 0 for g in got[:-1])
                for p in (twin, loop):
                    assert torch.equal(q._placed.loc_x, p._placed.loc_x) and torch.equal(q._placed.loc_y, p._placed.loc_y)
                pq, pt = q.predict()[0], twin.predict()[0]
                assert same_bits(pq, pt) and same_bits(pq, final)
                if got:
                    assert SE.base_host(pq.cpu().numpy(), required, rows_of[i])['nsum'] == got[-1]['predicted_nsum']
                selecting = [g for g in got if g['n_selected'] > 0]
                differ = len(selecting) >= 2 and any(not np.array_equal(u['cell'], v['cell']) for u, v in zip(selecting[:-1], selecting[1:]))
                print(f'{kind} {value} design {i}: passes {len(got)} cells {[len(g["cell"]) for g in got]} selected '
                      f'{[g["n_selected"] for g in got]} nsum {[g["predicted_nsum"] for g in got]} re-targeted {differ}')
                if differ and retargeted is None:
                    retargeted = (kind, value, i)
                for p in (q, twin, loop):
                    p.update(i, pin_x=home_x, pin_y=home_y)
            if retargeted is not None:
                break
        assert retargeted is not None                                                             # two selecting passes whose cell lists differ
        print(f're-targeting mattered first at {retargeted[0]} {retargeted[1]}, design {retargeted[2]}')
        q.predict()
        q.update(0, pin_x=np.asarray(designs[0].pin_x), pin_y=np.asarray(designs[0].pin_y))
        with pytest.raises(RuntimeError, match='refine_cells\\(\\): update\\(\\) has run'):
            q.refine_cells(q.cell_set(0, np.arange(2, dtype=np.int64)), 1)
