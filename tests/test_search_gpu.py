"""The window search on the GPU (include/mmft_search.h, mmft.search): mmft_search_rows bitwise against mmft_trial_rows on the
window written out as explicit candidates, mmft_search_score + mmft_search_best bitwise against their numpy restatement, and
Predictor.search_moves against score_host fed with trial_moves' predictions of the same candidates - and against the truth
of its best moves: update(), predict(), the design's sum of quanta."""
import functools
import types

import numpy as np
import pytest
import torch

import place_cases as C
import search_cases as SC
from mmft import lib
from mmft import search as SE
from mmft import trial as TR
from mmft.criticality import reference_quanta
from mmft.report import reference_slack
from test_head_kernels_gpu import S, T_, I32
from test_place_gpu import _live_models, _small_designs

pytestmark = pytest.mark.gpu
NAN = float('nan')
U32 = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
ROW_CASES = ['single_block_8x8', 'edges_16x16', 'clamped_16x16', 'rows_of_24', 'wide_32x64', 'long_walk_16x16']


# ------------------------------------------------------------------------------------------------ 1. the rows
@functools.lru_cache(maxsize=None)
def _case(name):
    c = C.CASES[name]
    return SC.tables(c), SC.groups(c)


@pytest.mark.parametrize('Dout', [4, 128])
@pytest.mark.parametrize('radius', [1, 2])
@pytest.mark.parametrize('name', ROW_CASES)
def test_search_rows_equal_trial_rows_on_the_explicit_expansion_bitwise(dev, name, radius, Dout):
    c = C.CASES[name]
    (nodes, lens, px, py, rep, far), groups = _case(name)
    tags = [g[0] for g in groups]
    assert {'single', 'repeated_in_its_row', 'three_of_one_row', 'sixty_four', 'on_no_row', 'saturating'} <= set(tags)
    assert max(len(g[1]) for g in groups) == 64 == TR.MAX_MOVES and all(len(set(g[1])) == len(g[1]) for g in groups)
    assert (px[far], py[far]) == (SC.I32_MAX, SC.I32_MIN) and groups[tags.index('saturating')][1] == [far]
    if name == 'long_walk_16x16':
        assert nodes.shape[1] == 300 and groups[tags.index('shared_by_two_stages')][1] == [int(nodes[0, 255])]
    npaths, P, G = nodes.shape[0], c.P, len(groups)
    W = (2 * radius + 1) ** 2
    rng = np.random.default_rng(5)
    sel = np.concatenate([rng.permutation(npaths), rng.integers(0, npaths, 3)])            # every path, some twice
    T = sel.shape[0]
    # every group against every row: the rows that hold none of its pins must come out as they are
    grow_grp, grow_row = np.repeat(np.arange(G), T), np.tile(np.arange(T), G)
    R = G * T
    paths = I32(sel, dev)
    tabs = [I32(nodes, dev), I32(lens, dev), I32(px, dev), I32(py, dev)]
    before = [t.clone() for t in tabs]
    mv_ptr = np.concatenate([[0], np.cumsum([len(g[1]) for g in groups])])
    mv_node = np.concatenate([np.asarray(g[1], dtype=np.int64) for g in groups])
    d_row, d_grp, d_mptr, d_node = I32(grow_row, dev), I32(grow_grp, dev), I32(mv_ptr, dev), I32(mv_node, dev)
    cnn_col, after = 8, 12
    width = cnn_col + Dout + after
    ldx, ldxt = width + 4, width + 8
    x = T_((T, ldx), 7, dev)
    B = 2
    GP, bias = T_((B * P, Dout), 1, dev), T_((Dout,), 3, dev)
    foff = I32((np.arange(T) % B) * P, dev)
    # the reference: the whole window written out as G * W trial-move candidates, slot (w, e) = pair (grow_row[e], g * W + w)
    e_ptr, e_node, e_x, e_y = SC.explicit(px, py, [g[1] for g in groups], radius)
    pair_row = np.tile(grow_row, W)
    pair_cand = (grow_grp[None, :] * W + np.arange(W)[:, None]).reshape(-1)
    want = torch.full((W * R + 1, ldxt), NAN, device=dev)
    TR.abi('mmft_trial_rows', tabs[0], tabs[1], c.maxlen, tabs[2], tabs[3], c.map_x, c.map_y, paths, foff, T, I32(pair_row, dev),
           I32(pair_cand, dev), W * R, I32(e_ptr, dev), I32(e_node, dev), I32(e_x, dev), I32(e_y, dev), G * W, GP, bias, x, ldx, want, ldxt,
           width, cnn_col, Dout, S, *lib.stream_args(GP))
    bits = lambda t: t.view(torch.int32)

    def rows(w0, w1):
        xt = torch.full(((w1 - w0) * R + 1, ldxt), NAN, device=dev)
        SE.abi('mmft_search_rows', tabs[0], tabs[1], c.maxlen, tabs[2], tabs[3], c.map_x, c.map_y, paths, foff, T, d_row, d_grp, R,
               d_mptr, d_node, G, radius, w0, w1, GP, bias, x, ldx, xt, ldxt, width, cnn_col, Dout, S, *lib.stream_args(GP))
        return xt

    full = rows(0, W)
    assert torch.equal(bits(full), bits(want)), (name, radius, Dout)              # the poison beyond width and the last row included
    assert bool(torch.isnan(full[:W * R, width:]).all()) and bool(torch.isnan(full[W * R]).all())
    assert not bool(torch.isnan(full[:W * R, :width]).any())
    cw = SE.centre(radius)
    centre = full[cw * R:(cw + 1) * R, :width]
    moved = sum(int(not torch.equal(full[w * R:(w + 1) * R, :width], centre)) for w in range(W))
    assert moved >= W // 2                                                        # the offsets do move masks
    none = tags.index('on_no_row')                                                # a group on no row: every offset is the centre
    for w in (0, W - 1):
        assert torch.equal(full[w * R + none * T:w * R + (none + 1) * T, :width], centre[none * T:(none + 1) * T])
    cut = W // 3 + 1                                                              # an uneven split, and single offsets
    for w0, w1 in [(0, cut), (cut, W), (cw + 1, cw + 2), (W - 1, W), (0, 1)]:
        part = rows(w0, w1)
        n = (w1 - w0) * R
        assert torch.equal(bits(part[:n]), bits(want[w0 * R:w1 * R])), (name, radius, Dout, w0, w1)
        assert bool(torch.isnan(part[n]).all())
    assert torch.equal(bits(rows(0, W)), bits(full))                              # same inputs, same bits
    assert all(torch.equal(a, b) for a, b in zip(tabs, before))                   # the tables are read, never written


# ------------------------------------------------------------------------------------------------ 2. the scores
def _score_on_device(dev, pred_base, required, grow_ptr, grow_row, trial, radius, scale, cuts, design_rows=None):
    """mmft_search_score over the offset ranges between `cuts`, then mmft_search_best, decoded by search.fetch; the tables lie
    in search's own buffer layout, poisoned before the calls."""
    G, R, T = len(grow_ptr) - 1, len(grow_row), len(pred_base)
    W = (2 * radius + 1) ** 2
    trial = np.asarray(trial, dtype=np.float32).reshape(W, R)
    n64, n32 = G * W + G + 3, 5 * G * W + G
    raw = torch.full((n64 + (n32 + 1) // 2 + 1,), -7, dtype=torch.int64, device=dev)
    v = SE._views(raw[:-1], G, W, n64)
    pb, rq = torch.from_numpy(np.asarray(pred_base, dtype=np.float32)).to(dev), torch.from_numpy(np.asarray(required, dtype=np.float32)).to(dev)
    d_ptr, d_row = I32(grow_ptr, dev), I32(grow_row, dev)
    for w0, w1 in zip(cuts[:-1], cuts[1:]):
        pt = torch.from_numpy(np.ascontiguousarray(trial[w0:w1])).to(dev)
        SE.abi('mmft_search_score', pt if R else None, pb, rq, T, d_ptr, d_row if R else None, G, R, radius, w0, w1, scale, v['dq'],
               v['dviol'], v['new_nan'], v['capped'], v['worst'], v['worst_row'], *lib.stream_args(pb))
    rows = np.arange(T) if design_rows is None else design_rows
    SE.abi('mmft_search_best', v['dq'], v['new_nan'], G, radius, v['best_w'], v['best_dq'], pb, rq, I32(rows, dev), len(rows), T, scale,
           v['base'], *lib.stream_args(pb))
    assert int(raw[-1]) == -7                                                     # nothing behind the buffer is written
    plan = types.SimpleNamespace(G=G, grow_ptr=np.asarray(grow_ptr), grow_row=np.asarray(grow_row))
    res = SE.fetch(dict(plan=plan, W=W, radius=radius, scale_log2=scale, raw=raw[:-1], n64=n64))
    assert res['base'] == SE.base_host(pred_base, required, rows, scale)
    return res


def _scores(name):
    if name.startswith('seeded'):
        radius = int(name[-1])
        return SC.seeded_scores(radius=radius) + (radius,)
    args = getattr(SC, name)()
    return tuple(args[:6]) + (1,)


@pytest.mark.parametrize('name', ['special_rows', 'special_ties', 'special_ineligible', 'special_cap', 'seeded_r1', 'seeded_r2'])
def test_search_score_and_best_equal_their_restatement_bitwise(dev, name):
    pred_base, required, grow_ptr, grow_row, trial, scale, radius = _scores(name)
    W = (2 * radius + 1) ** 2
    want = SE.score_host(pred_base, required, grow_ptr, grow_row, trial, radius, scale)
    SC.same_tables(want, SC.score_literal(pred_base, required, grow_ptr, grow_row, trial, radius, scale), name)
    one = _score_on_device(dev, pred_base, required, grow_ptr, grow_row, trial, radius, scale, [0, W])
    SC.same_tables(one, want, name)
    two = _score_on_device(dev, pred_base, required, grow_ptr, grow_row, trial, radius, scale, [0, W // 3 + 1, W])
    SC.same_tables(two, one, f'{name}: two chunk calls')
    each = _score_on_device(dev, pred_base, required, grow_ptr, grow_row, trial, radius, scale, list(range(W + 1)))
    SC.same_tables(each, one, f'{name}: one call per offset')
    if name == 'special_rows':
        assert np.isnan(one['worst'][2]).all() and (one['worst_row'][2] == -1).all() and not one['dq'][2].any()     # a group without rows
        # rows outside [0, T) take part in nothing, in the score and in the base
        out = grow_row.copy()
        out[[0, 5]] = [17, -1]
        got = _score_on_device(dev, pred_base, required, grow_ptr, out, trial, radius, scale, [0, W], design_rows=np.array([0, 1, 2, 3, 4, 9, -2]))
        SC.same_tables(got, SE.score_host(pred_base, required, grow_ptr, out, trial, radius, scale), 'rows outside')
    if name.startswith('seeded'):
        assert np.diff(grow_ptr).tolist() == [0, 1, 257, 600] and len(pred_base) == 600
        none = _score_on_device(dev, pred_base, required, np.zeros(3, dtype=np.int64), grow_row[:0], trial[:, :0], radius, scale, [0, W])
        assert not none['dq'].any() and np.isnan(none['worst']).all() and (none['best_w'] == SE.centre(radius)).all()    # R == 0


# ------------------------------------------------------------------------------------------------ 3. / 4. the Predictor
def _groups(state, designs, node_off, seed, singles, eights, idle_too):
    """Per design (pins, group_ptr): `singles` single pins that lie on selected rows, with `idle_too` one that lies on none
    (where there is one), and `eights` groups of 8 pins."""
    ptr, _ = state.rows_of_pin
    out = []
    for i, d in enumerate(designs):
        rng = np.random.default_rng(seed * 10 + i)
        N, off = int(d.N), int(node_off[i])
        count = ptr[off + 1:off + N + 1] - ptr[off:off + N]
        on, idle = np.flatnonzero(count > 0), np.flatnonzero(count == 0)
        sets = [[int(v)] for v in rng.choice(on, singles, replace=False)]
        sets += [[int(idle[0])]] if idle_too and idle.size else []
        sets += [[int(v) for v in rng.choice(on, 8, replace=False)] for _ in range(eights)]
        out.append((np.array([v for s in sets for v in s], dtype=np.int64), np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)))
    return out


def _written_out(d, pins, gptr, radius):
    """The window of every group as explicit trial_moves candidates, candidate g * W + w: (pins, pin_x, pin_y, cand_ptr)."""
    dx, dy = SE.offsets(radius)
    px, py = np.asarray(d.pin_x), np.asarray(d.pin_y)
    ps, xs, ys, ptr = [], [], [], [0]
    for g in range(len(gptr) - 1):
        mine = pins[gptr[g]:gptr[g + 1]]
        for w in range(dx.shape[0]):
            ps.append(mine)
            xs.append(SE.moved_coords(px[mine], dx[w]))
            ys.append(SE.moved_coords(py[mine], dy[w]))
            ptr.append(ptr[-1] + mine.shape[0])
    return np.concatenate(ps).astype(np.int64), np.concatenate(xs).astype(np.int64), np.concatenate(ys).astype(np.int64), np.array(ptr, dtype=np.int64)


def _search_against_trial_moves(designs, dev, singles, eights, idle_too, radii, eager_too, seeds, must_show):
    from mmft.infer import Predictor
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        truth = Predictor(pmodel, cnn, designs, dev, placement=True)
        objs = [Predictor(pmodel, cnn, designs, dev, placement=True, trials=True)]
        if eager_too:
            objs.append(Predictor(pmodel, cnn, designs, dev, placement=True, trials=True, graphed=False, overlap=False))
        # required times a hair above and below the resident predictions: a prediction that moves changes who violates
        first = truth.predict()[0].clone()
        sign = torch.where(torch.arange(first.numel(), device=dev) % 2 == 0, 1.0, -1.0)
        near = (first + sign * first.abs().clamp_min(1e-3) * 2.0 ** -18).to(torch.float32)
        for q in [truth] + objs:
            q.required.copy_(near)
        base_pred, required = first.cpu().numpy(), near.cpu().numpy()
        rows_of = [np.flatnonzero(np.asarray(truth.row_design) == i) for i in range(len(designs))]
        p = objs[0]
        for _ in range(3):
            p.predict()
        assert p._replay.graph is not None and p._replay.calls == 3
        befores = []
        for q in objs:
            befores.append((q.predict()[0].clone(), q._placed.loc_x.data_ptr(), q._placed.loc_y.data_ptr(), q._placed.loc_x.clone(),
                            q._placed.loc_y.clone(), q.h.clone()))
            assert np.array_equal(U32(befores[-1][0].cpu().numpy()), U32(base_pred))
        moved = dviol = False
        for seed in range(seeds):                                                 # seeds until the inputs show something
            sets = _groups(p._trial, designs, p._placed.node_off, seed, singles, eights, idle_too)
            for i, (pins, gptr) in enumerate(sets):
                d = designs[i]
                plans = [q.search_plan(i, torch.from_numpy(pins) if i else pins, gptr) for q in objs]
                plan = plans[0]
                G, R = plan.G, plan.R
                assert G == len(gptr) - 1 and plan.grow_ptr.shape == (G + 1,) and plan.ints.numel() == 2 * (G + 1) + 2 * R + len(pins)
                base = SE.base_host(base_pred, required, rows_of[i])
                for radius in radii:
                    W, cw = (2 * radius + 1) ** 2, SE.centre(radius)
                    res = p.search_moves(plan, radius=radius)
                    # the same candidates written out by the host, through trial_moves: its pred feeds score_host
                    tm = p.trial_moves(i, *_written_out(d, pins, gptr, radius))
                    trial = np.zeros((W, R), dtype=np.float32)
                    for g in range(G):
                        a, b = int(plan.grow_ptr[g]), int(plan.grow_ptr[g + 1])
                        for w in range(W):
                            k = g * W + w
                            assert np.array_equal(tm['rows'][tm['pair_ptr'][k]:tm['pair_ptr'][k + 1]], plan.grow_row[a:b])
                            trial[w, a:b] = tm['pred'][tm['pair_ptr'][k]:tm['pair_ptr'][k + 1]]
                    want = SE.score_host(base_pred, required, plan.grow_ptr, plan.grow_row, trial, radius, 20)
                    SC.same_tables(res, want, (seed, i, radius))
                    assert res['base'] == base and res['grow_ptr'] is plan.grow_ptr and res['rows'] is plan.grow_row
                    assert not res['dq'][:, cw].any() and not res['dviol'][:, cw].any() and not res['new_nan'][:, cw].any()
                    assert (res['best_dq'] <= 0).all() and (res['best_w'] >= 0).all()
                    print(f'seed {seed} design {i} radius {radius}: G {G} R {R}, best_w {res["best_w"].tolist()}, best_dq {res["best_dq"].tolist()}, '
                          f'candidates with dviol {int(np.count_nonzero(res["dviol"]))}')
                    for q, pl in zip(objs, plans):                                # the chunking does not show; eager and graphed agree
                        for max_rows in (1, R + 1, 65536):
                            other = q.search_moves(pl, radius=radius, max_rows=max_rows)
                            SC.same_tables(other, res, (seed, i, radius, max_rows))
                            assert other['base'] == base
                    # the truth of each group's best move: written into the pins, predicted, summed
                    dx, dy = SE.offsets(radius)
                    for g in range(G):
                        w = int(res['best_w'][g])
                        mine = pins[gptr[g]:gptr[g + 1]]
                        nx, ny = np.asarray(d.pin_x).copy(), np.asarray(d.pin_y).copy()
                        nx[mine], ny[mine] = SE.moved_coords(nx[mine], dx[w]), SE.moved_coords(ny[mine], dy[w])
                        truth.update(i, pin_x=nx, pin_y=ny)
                        pred = truth.predict()[0].cpu().numpy()
                        truth.update(i, pin_x=np.asarray(d.pin_x), pin_y=np.asarray(d.pin_y))
                        quanta, _ = reference_quanta(reference_slack(pred[rows_of[i]], required[rows_of[i]]), 20)
                        assert int(quanta.sum()) == base['nsum'] + int(res['best_dq'][g]), (seed, i, radius, g, w)
                    moved |= bool((res['best_w'] != cw).any())
                    dviol |= bool(res['dviol'].any())
            if moved and dviol:
                break
        if must_show:                # some group has a move that helps; some candidate changes the number of violations
            assert moved and dviol, (moved, dviol)
        assert np.array_equal(U32(truth.predict()[0].cpu().numpy()), U32(base_pred))
        for q, (pred, ax, ay, lx, ly, h) in zip(objs, befores):
            assert torch.equal(q.predict()[0], pred)
            assert (q._placed.loc_x.data_ptr(), q._placed.loc_y.data_ptr()) == (ax, ay)
            assert torch.equal(q._placed.loc_x, lx) and torch.equal(q._placed.loc_y, ly) and torch.equal(q.h, h)
        assert objs[0]._replay.calls == 5 and (not eager_too or objs[1]._replay is None)      # no search call replayed or captured anything


def test_search_moves_equal_score_host_on_trial_moves_and_the_truth_of_their_best(dev):
    designs = list(_small_designs())
    assert designs[0].map_size == 16 and len(designs) == 2
    _search_against_trial_moves(designs, dev, singles=5, eights=2, idle_too=True, radii=(1, 2), eager_too=True, seeds=6, must_show=True)


def test_search_moves_on_a_128_x_128_map(dev):
    from mmft.synth import synth_design
    d = C.placed(synth_design(N=1024, L=8, tile=256, seed=33, end_frac=0.25), seed=34)
    assert d.map_size == 128
    _search_against_trial_moves([d], dev, singles=8, eights=0, idle_too=False, radii=(1,), eager_too=False, seeds=1, must_show=False)


# ------------------------------------------------------------------------------------------------ 5. state and refusals
def test_state_and_refusals(dev):
    from mmft.infer import Predictor
    designs = list(_small_designs())
    d = designs[0]
    pins = np.array([int(d.path_nodes[int(np.flatnonzero(d.path_lens >= 2)[0]), 0])], dtype=np.int64)
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        plain = Predictor(pmodel, cnn, designs, dev, placement=True)
        p = Predictor(pmodel, cnn, designs, dev, placement=True, trials=True)
        other = Predictor(pmodel, cnn, designs, dev, placement=True, trials=True)
        with pytest.raises(RuntimeError, match='search_plan\\(\\): built without trials=True'):
            plain.search_plan(0, pins)
        plan = p.search_plan(0, pins)                                             # host only: fine before the first predict()
        assert plan.G == 1 and plan.R >= 1 and plan.owner is p
        with pytest.raises(RuntimeError, match='search_moves\\(\\): built without trials=True'):
            plain.search_moves(plan)
        with pytest.raises(RuntimeError, match='predict\\(\\) has not run'):
            p.search_moves(plan)
        for k in range(3):
            ref = p.predict()[0].clone()
            other.predict()
        good = p.search_moves(plan)
        assert good['dq'].shape == (1, 9) and good['best_w'].shape == (1,)
        # after update() without predict(): refused; the predict() that follows is the unmoved one and the plan still holds
        p.update(0, pin_x=np.asarray(d.pin_x), pin_y=np.asarray(d.pin_y))
        with pytest.raises(RuntimeError, match='update\\(\\) has run'):
            p.search_moves(plan)
        assert torch.equal(p.predict()[0], ref)
        SC.same_tables(p.search_moves(plan), good, 'after update() and predict()')
        # a plan of another Predictor, something that is no plan, bad arguments
        with pytest.raises(ValueError, match='another Predictor'):
            other.search_moves(plan)
        with pytest.raises(TypeError, match='search_plan'):
            p.search_moves(dict(G=1))
        for kw in (dict(radius=0), dict(radius=9), dict(scale_log2=31), dict(scale_log2=-1), dict(max_rows=0)):
            with pytest.raises(ValueError, match='search_moves'):
                p.search_moves(plan, **kw)
        for exc, kw in ((TypeError, dict(pins=pins.astype(np.int32))), (IndexError, dict(pins=np.array([d.N], dtype=np.int64))),
                        (ValueError, dict(group_ptr=np.array([0, 2], dtype=np.int64))), (ValueError, dict(pins=pins[:0], group_ptr=np.array([0], dtype=np.int64)))):
            with pytest.raises(exc, match='search_plan'):
                p.search_plan(**{**dict(i=0, pins=pins), **kw})
        with pytest.raises(IndexError):
            p.search_plan(2, pins)
        # under a stream capture
        graph, scratch = torch.cuda.CUDAGraph(), torch.zeros(4, device=dev)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match='outer stream capture'):
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                scratch.add_(1.0)
                p.search_moves(plan)
        torch.cuda.synchronize()
        assert torch.equal(p.predict()[0], ref)
        # predict() in bf16 mode, search_moves() in fp32 mode
        with lib.math_mode('f32'):
            with pytest.raises(ValueError, match='search_moves: bf16 math mode only'):
                p.search_moves(plan)
        assert torch.equal(p.predict()[0], ref)
    # fp32 mode throughout
    pmodel, cnn = _live_models(designs, dev)
    f = Predictor(pmodel, cnn, designs, dev, placement=True, trials=True)
    ref32 = f.predict()[0].clone()
    fplan = f.search_plan(0, pins)
    with pytest.raises(ValueError, match='search_moves: bf16 math mode only'):
        f.search_moves(fplan)
    assert torch.equal(f.predict()[0], ref32) and f._replay is None
