"""Trial pin moves on the GPU (include/mmft_trial.h, mmft.trial): mmft_trial_rows bitwise against mmft_placed_fc_fwd on pin
tables with the candidate written in, mmft_trial_reduce bitwise against its numpy restatement, and Predictor.trial_moves
against the truth - update() with the candidate's pins, predict(), report() - on a second Predictor."""
import functools

import numpy as np
import pytest
import torch

import place_cases as C
import trial_cases as TC
from mmft import lib
from mmft import trial as TR
from mmft.report import reference_slack
from test_head_kernels_gpu import S, T_, I32
from test_place_gpu import _live_models, _small_designs

pytestmark = pytest.mark.gpu
NAN = float('nan')
U32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the kernels
@functools.lru_cache(maxsize=None)
def _case(name):
    c = C.CASES[name]
    return TC.tables(c), TC.candidates(c)


def _placed(tabs, c, paths, foff, GP, bias, out, Dout):
    lib.place('mmft_placed_fc_fwd', tabs[0], tabs[1], c.maxlen, tabs[2], tabs[3], c.map_x, c.map_y, paths, foff, paths.numel(),
              GP, bias, out, Dout, Dout, S, None, *lib.stream_args(GP))


def _rows(tabs, c, paths, foff, T, pair_row, pair_cand, n_pairs, mv, K, GP, bias, x, ldx, xt, ldxt, width, cnn_col, Dout, block=S):
    TR.abi('mmft_trial_rows', tabs[0], tabs[1], c.maxlen, tabs[2], tabs[3], c.map_x, c.map_y, paths, foff, T, pair_row, pair_cand,
           n_pairs, mv[0], mv[1], mv[2], mv[3], K, GP, bias, x, ldx, xt, ldxt, width, cnn_col, Dout, block, *lib.stream_args(GP))


def _moves(cands, dev):
    ptr = np.concatenate([[0], np.cumsum([len(cd[1]) for cd in cands])])
    cat = lambda j: np.concatenate([np.asarray(cd[j], dtype=np.int64) for cd in cands])
    return [I32(ptr, dev), I32(cat(1), dev), I32(cat(2), dev), I32(cat(3), dev)]


@pytest.mark.parametrize('Dout', [4, 128])
@pytest.mark.parametrize('name', sorted(C.CASES))
def test_trial_rows_equal_placed_fc_on_moved_tables_bitwise(dev, name, Dout):
    c = C.CASES[name]
    (nodes, lens, px, py, rep), cands = _case(name)
    tags = [cd[0] for cd in cands]
    assert {'one_cell_x', 'jump0', 'off_the_map', 'int32_extremes', 'several_of_one_row', 'repeated_in_its_row', 'sixty_four',
            'on_no_row'} <= set(tags)
    assert max(len(cd[1]) for cd in cands) == 64 == TR.MAX_MOVES and all(len(set(cd[1])) == len(cd[1]) for cd in cands)
    assert TC.live(nodes, lens, rep).count(cands[tags.index('repeated_in_its_row')][1][0]) == 2
    if name == 'long_walk_16x16':
        assert nodes.shape[1] == 300 and 'shared_by_two_stages' in tags
        assert cands[tags.index('shared_by_two_stages')][1] == [int(nodes[0, 255])]
    npaths, P, K = nodes.shape[0], c.P, len(cands)
    rng = np.random.default_rng(5)
    sel = np.concatenate([rng.permutation(npaths), rng.integers(0, npaths, 3)])            # every path, some twice
    T = sel.shape[0]
    holds = np.array([[bool(set(cd[1]) & set(TC.live(nodes, lens, q))) for q in sel] for cd in cands])     # [K, T]
    assert not holds[tags.index('on_no_row')].any() and holds[tags.index('sixty_four')].any()
    paths = I32(sel, dev)
    tabs = [I32(nodes, dev), I32(lens, dev), I32(px, dev), I32(py, dev)]
    before = [t.clone() for t in tabs]
    mv = _moves(cands, dev)
    # every candidate against every row: the rows that hold none of its pins must come out as they are
    pair_cand, pair_row = np.repeat(np.arange(K), T), np.tile(np.arange(T), K)
    n_pairs = K * T
    d_row, d_cand = I32(pair_row, dev), I32(pair_cand, dev)
    cnn_col, after = 8, 12
    width = cnn_col + Dout + after
    ldx, ldxt = width + 4, width + 8
    x = T_((T, ldx), 7, dev)
    settings = [(2, True, True)] + ([(1, False, False)] if name == 'edges_16x16' else [])
    for B, with_off, with_bias in settings:
        GP = T_((B * P, Dout), 1, dev)
        bias = T_((Dout,), 3, dev) if with_bias else None
        foff = I32((np.arange(T) % B) * P, dev) if with_off else None
        xt = torch.full((n_pairs + 1, ldxt), NAN, device=dev)
        _rows(tabs, c, paths, foff, T, d_row, d_cand, n_pairs, mv, K, GP, bias, x, ldx, xt, ldxt, width, cnn_col, Dout)
        base = torch.full((T, Dout), NAN, device=dev)
        _placed(tabs, c, paths, foff, GP, bias, base, Dout)
        assert not bool(torch.isnan(base).any())
        differs = 0
        for k, cd in enumerate(cands):
            mx, my = TC.moved(px, py, cd)
            want = torch.full((T, Dout), NAN, device=dev)
            _placed([tabs[0], tabs[1], I32(mx, dev), I32(my, dev)], c, paths, foff, GP, bias, want, Dout)
            got = xt[k * T:(k + 1) * T, cnn_col:cnn_col + Dout]
            assert torch.equal(got, want), (name, Dout, cd[0])
            away = torch.from_numpy(~holds[k]).to(dev)
            assert torch.equal(got[away], base[away]), (name, Dout, cd[0])
            differs += int(not torch.equal(want, base))
        assert differs >= 3                                                       # the moves do move masks
        rows_d = d_row.long()
        assert torch.equal(xt[:n_pairs, :cnn_col], x[rows_d, :cnn_col])
        assert torch.equal(xt[:n_pairs, cnn_col + Dout:width], x[rows_d, cnn_col + Dout:width])
        assert bool(torch.isnan(xt[:n_pairs, width:]).all()) and bool(torch.isnan(xt[n_pairs]).all())
        again = torch.full((n_pairs + 1, ldxt), NAN, device=dev)
        _rows(tabs, c, paths, foff, T, d_row, d_cand, n_pairs, mv, K, GP, bias, x, ldx, again, ldxt, width, cnn_col, Dout)
        assert torch.equal(again[:n_pairs, :width], xt[:n_pairs, :width])
    assert all(torch.equal(a, b) for a, b in zip(tabs, before))                  # the tables are read, never written


def _reduce(pred_base, pred_trial, required, rows, pair_ptr, pair_row, dev):
    K, n_pairs = len(pair_ptr) - 1, len(pair_row)
    out = torch.full((K + 2, 6), -7.0, dtype=torch.float64, device=dev)
    pb, rq = torch.from_numpy(pred_base).to(dev), torch.from_numpy(required).to(dev)
    TR.abi('mmft_trial_reduce', pb, torch.from_numpy(pred_trial).to(dev) if n_pairs else None, rq, I32(rows, dev), len(rows), len(pred_base),
           I32(pair_ptr, dev) if K else None, I32(pair_row, dev) if n_pairs else None, n_pairs, K, out, *lib.stream_args(pb))
    h = out.cpu().numpy()
    assert (h[K + 1] == -7.0).all()
    return h[:K + 1]


def test_trial_reduce_equals_its_restatement_bitwise(dev):
    rng = np.random.default_rng(21)
    T = 1500
    required = rng.normal(0, 1, T).astype(np.float32)
    pred = (required + rng.normal(0, 10.0 ** rng.uniform(-6, 3, T))).astype(np.float32)
    pred[[3, 700, 1499]] = np.nan
    pred[10], required[10] = 0.0, -0.0                                             # slack -0.0
    pred[[20, 21, 900]], required[[20, 21, 900]] = 50.0, -1e6                      # three rows tie on the worst slack
    rows = np.flatnonzero(rng.random(T) < 0.8)
    rows = np.union1d(rows, [3, 10, 20, 21, 40, 900])
    K = 9
    sizes = [0, 1, 5, 300, 0, 40, 2, len(rows), 3]
    pair_ptr = np.concatenate([[0], np.cumsum(sizes)])
    pair_row = np.concatenate([np.sort(rng.permutation(rows)[:s]) for s in sizes])
    pred_trial = (required[pair_row] + rng.normal(0, 1, len(pair_row))).astype(np.float32)
    pred_trial[pair_ptr[7]:pair_ptr[8]] = np.nan                                   # candidate 7: no valid row
    pred_trial[pair_ptr[6]] = np.inf                                               # candidate 6: a slack of -inf is an ordinary value
    pair_row[pair_ptr[8]:pair_ptr[9]] = [20, 40, 900]                              # candidate 8 lifts two of the three tied rows
    pred_trial[pair_ptr[8]:pair_ptr[9]] = 0.0
    got = _reduce(pred, pred_trial, required, rows, pair_ptr, pair_row, dev)
    want = TR.reduce_host(pred, required, rows, pair_ptr, pair_row, pred_trial)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)
    lit = TC.reduce_literal(pred, required, rows, pair_ptr, pair_row, pred_trial)
    assert np.array_equal(got[:, :5], lit[:, :5], equal_nan=True)
    worst = float(np.float32(-1e6) - np.float32(50.0))
    assert got[K][3] == worst and got[K][4] == 20 and got[8][3] == worst and got[8][4] == 21
    assert got[6][3] == -np.inf and got[6][5] == -np.inf and np.isfinite(got[K][5]) and np.isfinite(got[3][5])
    assert got[7][0] == 0 and np.isnan(got[7][3]) and got[7][4] == -1 and got[7][5] == 0.0
    assert np.array_equal(got[0], got[K]) and np.array_equal(got[4], got[K])       # no pairs: the base's figures
    # the base alone, and a design of one row
    assert np.array_equal(_reduce(pred, pred_trial[:0], required, rows, pair_ptr[:1], pair_row[:0], dev).view(np.uint64), want[K:].view(np.uint64))
    one = _reduce(pred, pred_trial[:0], required, np.array([10]), pair_ptr[:1], pair_row[:0], dev)
    assert one[0].tolist() == [1, 0, 0, 0.0, 10, 0.0] and not np.signbit(one[0][3])
    assert np.array_equal(got.view(np.uint64), _reduce(pred, pred_trial, required, rows, pair_ptr, pair_row, dev).view(np.uint64))


# ------------------------------------------------------------------------------------------------ 2. bad arguments
def test_bad_arguments_launch_nothing(dev):
    c = C.CASES['edges_16x16']
    nodes, lens, px, py, _ = TC.tables(c)
    tabs = [I32(a, dev) for a in (nodes, lens, px, py)]
    Dout, T, K, n_pairs, width = 8, 3, 2, 3, 24
    paths = I32([2, 4, 5], dev)
    GP = torch.zeros((c.P, Dout), device=dev)
    bias = torch.zeros(Dout, device=dev)
    x = torch.ones((T, width), device=dev)
    xt = torch.full((n_pairs, width), 7.0, device=dev)
    d_row, d_cand = I32([0, 1, 2], dev), I32([0, 0, 1], dev)
    mv = _moves([('a', [int(nodes[2, 0])], [3], [4]), ('b', [int(nodes[5, 1])], [0], [9])], dev)
    d, st = lib.stream_args(GP)
    good = [tabs[0], tabs[1], c.maxlen, tabs[2], tabs[3], c.map_x, c.map_y, paths, None, T, d_row, d_cand, n_pairs, mv[0], mv[1], mv[2], mv[3],
            K, GP, None, x, width, xt, width, width, 8, Dout, S, d, st]
    TR.abi('mmft_trial_rows', *good)
    torch.cuda.synchronize()
    assert not bool((xt == 7.0).any())
    xt.fill_(7.0)
    wrong = {'P % 64': {5: 10, 6: 10}, 'P > 65536': {5: 512, 6: 256}, 'map_x = 0': {5: 0}, 'S': {27: 32}, 'Dout = 6': {26: 6}, 'Dout = 0': {26: 0},
             'Dout > 1024': {26: 1028, 21: 1040, 23: 1040, 24: 1040}, 'maxlen': {2: 0}, 'T = 0': {9: 0}, 'K = 0': {17: 0}, 'n_pairs < 0': {12: -1},
             'cnn_col % 4': {25: 6}, 'cnn_col < 0': {25: -4}, 'ldx % 4': {21: 26}, 'ldxt % 4': {23: 26}, 'width < cnn_col + Dout': {24: 12},
             'width > ldx': {21: 20}, 'width > ldxt': {23: 20},
             'null nodes': {0: None}, 'null lens': {1: None}, 'null loc_x': {3: None}, 'null loc_y': {4: None}, 'null paths': {7: None},
             'null pair_row': {10: None}, 'null pair_cand': {11: None}, 'null mv_ptr': {13: None}, 'null mv_node': {14: None},
             'null mv_x': {15: None}, 'null mv_y': {16: None}, 'null GP': {18: None}, 'null x': {20: None}, 'null xt': {22: None},
             'unaligned GP': {18: GP.data_ptr() + 4}, 'unaligned x': {20: x.data_ptr() + 4}, 'unaligned xt': {22: xt.data_ptr() + 4},
             'unaligned bias': {19: bias.data_ptr() + 8}}
    for what, change in wrong.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        with pytest.raises(RuntimeError, match=r'mmft_trial_rows failed \(-1\): trial_rows'):
            TR.abi('mmft_trial_rows', *args)
        torch.cuda.synchronize()
        assert bool((xt == 7.0).all()), what
    args = list(good)
    args[12] = 0                                                               # no pairs: fine, and nothing to write
    TR.abi('mmft_trial_rows', *args)
    torch.cuda.synchronize()
    assert bool((xt == 7.0).all())
    # the reduction
    pred, trial, req = torch.zeros(T, device=dev), torch.zeros(n_pairs, device=dev), torch.ones(T, device=dev)
    rows, pptr = I32([0, 1, 2], dev), I32([0, 2, 3], dev)
    summary = torch.full((K + 1, 6), 7.0, dtype=torch.float64, device=dev)
    good = [pred, trial, req, rows, T, T, pptr, d_row, n_pairs, K, summary, d, st]
    TR.abi('mmft_trial_reduce', *good)
    torch.cuda.synchronize()
    assert not bool((summary == 7.0).any())
    summary.fill_(7.0)
    wrong = {'n = 0': {4: 0}, 'n > 2^24': {4: (1 << 24) + 1}, 'T = 0': {5: 0}, 'T > 2^24': {5: (1 << 24) + 1}, 'K < 0': {9: -1}, 'n_pairs < 0': {8: -1},
             'null pred_base': {0: None}, 'null pred_trial': {1: None}, 'null required': {2: None}, 'null design_rows': {3: None},
             'null pair_ptr': {6: None}, 'null pair_row': {7: None}, 'null summary': {10: None}, 'unaligned summary': {10: summary.data_ptr() + 4}}
    for what, change in wrong.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        with pytest.raises(RuntimeError, match=r'mmft_trial_reduce failed \(-1\): trial_reduce'):
            TR.abi('mmft_trial_reduce', *args)
        torch.cuda.synchronize()
        assert bool((summary == 7.0).all()), what


# ------------------------------------------------------------------------------------------------ 3. / 4. the Predictor
def _candidates(state, designs, node_off, seed, singles, groups):
    """Per design (pins, pin_x, pin_y, cand_ptr): `singles` single pins that lie on selected rows, one that lies on none (where
    there is one), `groups` candidates of 8 pins, and one pin moved off the map; the new coordinates anywhere on the map."""
    ptr, _ = state.rows_of_pin
    out = []
    for i, d in enumerate(designs):
        rng = np.random.default_rng(seed * 10 + i)
        N, m, off = int(d.N), int(d.map_size), int(node_off[i])
        count = ptr[off + 1:off + N + 1] - ptr[off:off + N]
        on, idle = np.flatnonzero(count > 0), np.flatnonzero(count == 0)
        sets = [[int(v)] for v in rng.choice(on, singles, replace=False)]
        sets += [[int(idle[0])]] if idle.size else []
        sets += [[int(v) for v in rng.choice(on, 8, replace=False)] for _ in range(groups)]
        pins = np.array([v for s in sets for v in s], dtype=np.int64)
        x, y = rng.integers(0, m, pins.shape[0]), rng.integers(0, m, pins.shape[0])
        sets.append([int(on[0])])                                                 # off the map: below on one axis, beyond on the other
        pins, x, y = np.append(pins, on[0]), np.append(x, m + 9), np.append(y, -4)
        out.append((pins.astype(np.int64), x.astype(np.int64), y.astype(np.int32), np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)))
    return out


def _truth_of(truth, designs, calls):
    """Per design and candidate (pred as host fp32 [T], the design's report) from update() with the candidate written into the
    design's pins, predict(), report(); the pins are put back."""
    out = []
    for i, (pins, x, y, ptr) in enumerate(calls):
        d, per = designs[i], []
        for k in range(len(ptr) - 1):
            nx, ny = np.asarray(d.pin_x).copy(), np.asarray(d.pin_y).copy()
            a, b = int(ptr[k]), int(ptr[k + 1])
            nx[pins[a:b]], ny[pins[a:b]] = x[a:b], y[a:b]
            truth.update(i, pin_x=nx, pin_y=ny)
            pred = truth.predict()[0].clone().cpu().numpy()
            per.append((pred, truth.report()[i]))
            truth.update(i, pin_x=np.asarray(d.pin_x), pin_y=np.asarray(d.pin_y))
        out.append(per)
    return out


def _compare(res, truths, base_pred, base_report, required, rows_of_design):
    """One trial_moves result against the truth of its candidates; returns (candidates that changed a prediction's bits,
    candidates that changed violations or wns_row)."""
    K = len(truths)
    assert res['pair_ptr'].shape == (K + 1,) and res['pred'].dtype == np.float32 and res['pred'].shape == res['rows'].shape
    for f in ('wns', 'wns_row', 'tns', 'violations', 'n_nan', 'n'):
        assert res[f].shape == (K,)
    assert res['wns'].dtype == res['tns'].dtype == np.float64
    b = res['base']
    assert (b['n'], b['n_nan'], b['violations'], b['wns_row'], b['wns']) == tuple(base_report[f] for f in ('n', 'n_nan', 'violations', 'wns_row', 'wns'))
    moved, figures = 0, 0
    for k, (pred, rep) in enumerate(truths):
        rows = res['rows'][res['pair_ptr'][k]:res['pair_ptr'][k + 1]]
        assert (np.diff(rows) > 0).all()
        got = res['pred'][res['pair_ptr'][k]:res['pair_ptr'][k + 1]]
        assert np.array_equal(U32(got), U32(pred[rows])), k                       # bitwise the truth's rows
        changed = np.flatnonzero(U32(pred) != U32(base_pred))
        assert set(changed.tolist()) <= set(rows.tolist()), k                     # the expansion misses nothing
        assert (int(res['n'][k]), int(res['n_nan'][k]), int(res['violations'][k]), int(res['wns_row'][k])) == \
            (rep['n'], rep['n_nan'], rep['violations'], rep['wns_row']), k
        assert res['wns'][k] == rep['wns'], k
        s = reference_slack(pred[rows_of_design], required[rows_of_design]).astype(np.float64)
        neg = s[s < 0]
        # two fp64 summation orders of n terms can differ by no more than (n - 1) * 2^-52 * sum |slack|
        bound = max(neg.size - 1, 0) * 2.0 ** -52 * float(np.abs(neg).sum())
        print(f'candidate {k}: pairs {rows.size}, changed {changed.size}, tns {res["tns"][k]!r} vs {rep["tns"]!r}, bound {bound:.3e}')
        assert abs(res['tns'][k] - rep['tns']) <= bound, k
        if rows.size == 0:
            assert all(res[f][k] == b[f] for f in ('n', 'n_nan', 'violations', 'wns_row', 'wns', 'tns')), k
        moved += int(changed.size > 0)
        figures += int(rep['violations'] != base_report['violations'] or rep['wns_row'] != base_report['wns_row'])
    return moved, figures


def _trials_against_the_truth(designs, dev, singles, groups, eager_too):
    from mmft.infer import Predictor
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        truth = Predictor(pmodel, cnn, designs, dev, placement=True, report=dict(k=1))
        objs = [Predictor(pmodel, cnn, designs, dev, placement=True, trials=True)]
        if eager_too:
            objs.append(Predictor(pmodel, cnn, designs, dev, placement=True, trials=True, graphed=False, overlap=False))
        # required times a hair above and below the resident predictions: a prediction that moves changes who violates
        first = truth.predict()[0].clone()
        sign = torch.where(torch.arange(first.numel(), device=dev) % 2 == 0, 1.0, -1.0)
        near = (first + sign * first.abs().clamp_min(1e-3) * 2.0 ** -18).to(torch.float32)
        for q in [truth] + objs:
            assert q.required.shape == near.shape
            q.required.copy_(near)
        base_pred = truth.predict()[0].clone().cpu().numpy()
        assert np.array_equal(U32(base_pred), U32(first.cpu().numpy()))
        base_reports = truth.report()
        required = near.cpu().numpy()
        rows_of = [np.flatnonzero(np.asarray(truth.row_design) == i) for i in range(len(designs))]
        p = objs[0]
        for _ in range(3):
            p.predict()
        assert p._replay.graph is not None and p._replay.calls == 3 and p._trial in p._replay.keep
        befores = []
        for q in objs:
            befores.append((q.predict()[0].clone(), q._placed.loc_x.data_ptr(), q._placed.loc_y.data_ptr(), q._placed.loc_x.clone(),
                            q._placed.loc_y.clone(), q.h.clone()))
            assert np.array_equal(U32(befores[-1][0].cpu().numpy()), U32(base_pred))
        ok = False
        for seed in range(6):                                                     # seeds until the inputs show something
            calls = _candidates(p._trial, designs, p._placed.node_off, seed, singles, groups)
            truths = _truth_of(truth, designs, calls)
            tallies = []
            for q in objs:
                for i, (pins, x, y, ptr) in enumerate(calls):
                    res = q.trial_moves(i, pins, torch.from_numpy(x).to(dev) if i else x, y, ptr)
                    tallies.append(_compare(res, truths[i], base_pred, base_reports[i], required, rows_of[i]))
            ok = all(t[0] >= 1 for t in tallies) and any(t[1] >= 1 for t in tallies)
            if ok:
                break
        # in each design a candidate changes a prediction's bits; a candidate changes violations or wns_row
        assert ok, tallies
        # single moves, every move a candidate of its own (cand_ptr=None): the same figures as the same moves grouped one by one
        pins, x, y, ptr = calls[0]
        alone = p.trial_moves(0, pins[:3], x[:3], y[:3])
        grouped = p.trial_moves(0, pins[:3], x[:3], y[:3], np.arange(4, dtype=np.int64))
        assert all(np.array_equal(alone[f], grouped[f], equal_nan=True) for f in ('pair_ptr', 'rows', 'pred', 'wns', 'tns', 'violations'))
        for q, (pred, ax, ay, lx, ly, h) in zip(objs, befores):
            assert torch.equal(q.predict()[0], pred)
            assert (q._placed.loc_x.data_ptr(), q._placed.loc_y.data_ptr()) == (ax, ay)
            assert torch.equal(q._placed.loc_x, lx) and torch.equal(q._placed.loc_y, ly) and torch.equal(q.h, h)
        assert objs[0]._replay.calls == 5 and (not eager_too or objs[1]._replay is None)


def test_trial_moves_equal_update_predict_report(dev):
    designs = list(_small_designs())
    assert designs[0].map_size == 16 and len(designs) == 2
    _trials_against_the_truth(designs, dev, singles=7, groups=3, eager_too=True)


def test_trial_moves_on_a_128_x_128_map(dev):
    from mmft.synth import synth_design
    d = C.placed(synth_design(N=1024, L=8, tile=256, seed=33, end_frac=0.25), seed=34)
    assert d.map_size == 128
    _trials_against_the_truth([d], dev, singles=1, groups=1, eager_too=False)


def _same_bits(a, b, where='result'):
    """Decoded results compared bitwise: dicts key by key, sequences item by item, arrays by dtype, shape and bytes, floats by
    their fp64 bits (a NaN equals itself)."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), where
        for k in a:
            _same_bits(a[k], b[k], f'{where}[{k!r}]')
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), where
        for j, (x, y) in enumerate(zip(a, b)):
            _same_bits(x, y, f'{where}[{j}]')
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    elif isinstance(a, float):
        assert isinstance(b, float) and np.float64(a).tobytes() == np.float64(b).tobytes(), where
    else:
        assert type(a) is type(b) and a == b, where


def test_every_option_on_one_predictor_equals_each_option_alone(dev):
    """report=, criticality= (cells and sums), placement= and trials= on ONE Predictor against four Predictors with one of them
    each: after the same move of design 1's pins, the eager, the capturing and the replayed predict() give the same bits, and
    so do report(), criticality() and trial_moves().  update(pin_x=) needs placement=True, so each of the four has it; the
    option named is what it adds.  The options share the rows' slack inputs (Predictor.slack) and, here, the placement tables,
    and launch one after another on the same predictions: that they do not disturb one another is what this pins."""
    from mmft.infer import Predictor
    designs = list(_small_designs())
    assert len(designs) == 2 and designs[0].map_size ** 2 % 64 == 0
    report, crit = dict(k=8, hist=(-1.0, 1.0, 16)), dict(cells=True, sums=True)
    xy = C.move(designs[1], seed=75, frac=0.3)
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        combined = Predictor(pmodel, cnn, designs, dev, report=report, criticality=crit, placement=True, trials=True)
        alone = dict(report=Predictor(pmodel, cnn, designs, dev, placement=True, report=report),
                     criticality=Predictor(pmodel, cnn, designs, dev, placement=True, criticality=crit),
                     placement=Predictor(pmodel, cnn, designs, dev, placement=True),
                     trials=Predictor(pmodel, cnn, designs, dev, placement=True, trials=True))
        objs = [combined] + list(alone.values())
        assert combined._crit.placed is combined._placed and combined._report.slack is combined._crit.slack is combined.slack
        # required times a hair above and below the moved predictions: about every other row violates
        probe = Predictor(pmodel, cnn, designs, dev, placement=True, graphed=False)
        unmoved = probe.predict()[0].clone()
        probe.update(1, pin_x=xy[0], pin_y=xy[1])
        first = probe.predict()[0].clone()
        assert not torch.equal(first, unmoved)                                    # the move shows
        sign = torch.where(torch.arange(first.numel(), device=dev) % 2 == 0, 1.0, -1.0)
        near = (first + sign * first.abs().clamp_min(1e-3) * 2.0 ** -18).to(torch.float32)
        for q in objs:
            q.update(1, pin_x=xy[0], pin_y=xy[1])
            q.required.copy_(near)
        calls = _candidates(combined._trial, designs, combined._placed.node_off, 0, singles=3, groups=1)
        for call in range(3):                                                     # eager, the capturing call, a replay
            y, ends = combined.predict()
            assert np.array_equal(U32(y.cpu().numpy()), U32(first.cpu().numpy())), call
            for name, q in alone.items():
                yq, eq = q.predict()
                assert torch.equal(yq, y) and np.array_equal(eq, ends), (call, name)
            rep = combined.report()
            _same_bits(rep, alone['report'].report(), f'call {call}: report')
            _same_bits(combined.criticality(), alone['criticality'].criticality(), f'call {call}: criticality')
            assert all(0 < r['violations'] < r['n'] for r in rep)
            for i, (pins, x, py, ptr) in enumerate(calls):
                _same_bits(combined.trial_moves(i, pins, x, py, ptr), alone['trials'].trial_moves(i, pins, x, py, ptr),
                           f'call {call}: trial_moves({i})')
        assert combined._replay.graph is not None and combined._replay.calls == 3
        assert all(q._replay.graph is not None and q._replay.calls == 3 for q in alone.values())


# ------------------------------------------------------------------------------------------------ 5. state and refusals
def test_state_and_refusals(dev):
    from mmft.infer import Predictor
    from mmft.train import build_models
    designs = list(_small_designs())
    d = designs[0]
    pins = np.array([int(d.path_nodes[int(np.flatnonzero(d.path_lens >= 2)[0]), 0])], dtype=np.int64)
    x, y = np.array([3], dtype=np.int64), np.array([12], dtype=np.int64)
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        with pytest.raises(ValueError, match='trials=True needs placement=True'):
            Predictor(pmodel, cnn, designs, dev, trials=True)
        plain = Predictor(pmodel, cnn, designs, dev, placement=True)
        off = Predictor(pmodel, cnn, designs, dev, placement=True, trials=False)
        p = Predictor(pmodel, cnn, designs, dev, placement=True, trials=True)
        with pytest.raises(RuntimeError, match='predict\\(\\) has not run'):
            p.trial_moves(0, pins, x, y)
        # trials left off: the object of today - same bits, same replay bookkeeping; trials=True predicts the same bits
        for k in range(4):                                                    # eager, the capturing call, two replays
            a, b, c = plain.predict()[0].clone(), off.predict()[0].clone(), p.predict()[0].clone()
            assert torch.equal(a, b) and torch.equal(a, c), k
        for q in (plain, off, p):
            assert q._replay.graph is not None and q._replay.calls == 4 and q._placed in q._replay.keep
        assert plain._trial is None and off._trial is None and len(plain._replay.keep) == len(off._replay.keep) == len(p._replay.keep) - 1
        ref = p.predict()[0].clone()
        with pytest.raises(RuntimeError, match='without trials=True'):
            plain.trial_moves(0, pins, x, y)
        assert torch.equal(plain.predict()[0], ref)
        good = p.trial_moves(0, pins, x, y)
        assert good['pair_ptr'].tolist()[0] == 0 and good['rows'].size >= 1
        # after update() without predict(): refused, whatever was updated; the predict() that follows is the unmoved one
        p.update(0, pin_x=np.asarray(d.pin_x), pin_y=np.asarray(d.pin_y))
        with pytest.raises(RuntimeError, match='update\\(\\) has run'):
            p.trial_moves(0, pins, x, y)
        assert torch.equal(p.predict()[0], ref)
        again = p.trial_moves(0, pins, x, y)
        assert np.array_equal(U32(again['pred']), U32(good['pred'])) and again['tns'][0] == good['tns'][0]
        # bad arguments: validated on the host, nothing launched, nothing changed
        for exc, kw in ((TypeError, dict(pins=pins.astype(np.int32))), (IndexError, dict(pins=np.array([d.N], dtype=np.int64))),
                        (ValueError, dict(cand_ptr=np.array([0, 2], dtype=np.int64))), (ValueError, dict(pin_x=x[:0]))):
            with pytest.raises(exc, match='trial_moves'):
                p.trial_moves(**{**dict(i=0, pins=pins, pin_x=x, pin_y=y), **kw})
        with pytest.raises(IndexError):
            p.trial_moves(2, pins, x, y)
        assert torch.equal(p.predict()[0], ref)
        # under a stream capture: the pair list is host work done per call
        graph, scratch = torch.cuda.CUDAGraph(), torch.zeros(4, device=dev)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match='outer stream capture'):
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                scratch.add_(1.0)
                p.trial_moves(0, pins, x, y)
        torch.cuda.synchronize()
        assert torch.equal(p.predict()[0], ref)
        # a classification head
        two, cnn2 = build_models(map_size=designs[0].map_size, device=dev, seed=19, nlabels=2)
        with torch.no_grad():
            cnn2.outc.conv[0].bias.fill_(2.0)
        c2 = Predictor(two, cnn2, designs, dev, placement=True, trials=True)
        ref2 = [c2.predict()[0].clone() for _ in range(3)][-1]
        with pytest.raises(ValueError, match='regression head'):
            c2.trial_moves(0, pins, x, y)
        assert torch.equal(c2.predict()[0], ref2)
        # predict() in bf16 mode, trial_moves() in fp32 mode
        with lib.math_mode('f32'):
            with pytest.raises(ValueError, match='bf16 math mode only'):
                p.trial_moves(0, pins, x, y)
        assert torch.equal(p.predict()[0], ref)
    # fp32 mode throughout
    pmodel, cnn = _live_models(designs, dev)
    f = Predictor(pmodel, cnn, designs, dev, placement=True, trials=True)
    ref32 = f.predict()[0].clone()
    with pytest.raises(ValueError, match='bf16 math mode only'):
        f.trial_moves(0, pins, x, y)
    assert torch.equal(f.predict()[0], ref32) and f._replay is None
