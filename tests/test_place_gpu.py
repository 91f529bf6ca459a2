"""Masks that follow a placement, on the GPU: mmft_placed_fc_fwd (include/mmft_place.h) bitwise against
mmft_masked_fc_fwd_runs on masks rasterised on the host from the same pins, and Predictor(placement=True) bitwise against
Predictors built on those masks, before and after pins move."""
import copy
import functools

import numpy as np
import pytest
import torch

import place_cases as C
from mmft import fusion, lib
from mmft import placement as PL
from mmft.fusion import PathMasks
from test_head_kernels_gpu import TOL, EPS24, S, T_, I32, close
from test_infer_gpu import _models

pytestmark = pytest.mark.gpu
NAN = float('nan')


# ------------------------------------------------------------------------------------------------ 1. the kernel
@functools.lru_cache(maxsize=None)
def _host(name):
    """What the host derives from a case, once: CSR, runs, per-path (cells, runs), the dense 0/1 rows."""
    c = C.CASES[name]
    ip, cols = PL.rasterize_host(*c.arrays(), c.map_x, c.map_y)
    rp, rs, rl = PL.runs_host(*c.arrays(), c.map_x, c.map_y)
    M = np.zeros((len(ip) - 1, c.P))
    for q in range(len(ip) - 1):
        M[q, cols[ip[q]:ip[q + 1]]] = 1.0
    return ip, cols, np.stack([np.diff(ip), np.diff(rp)], 1).astype(np.int32), M


def _placed(tabs, c, paths, foff, GP, bias, out, ldo, Dout, stats, block=S):
    lib.place('mmft_placed_fc_fwd', tabs[0], tabs[1], c.maxlen, tabs[2], tabs[3], c.map_x, c.map_y, paths, foff, paths.numel(),
              GP, bias, out, ldo, Dout, block, stats, *lib.stream_args(GP))


@pytest.mark.parametrize('Dout', [4, 12, 128, 256])
@pytest.mark.parametrize('name', sorted(C.CASES))
def test_placed_fc_equals_the_run_kernel_bitwise(dev, name, Dout):
    c = C.CASES[name]
    ip, cols, counts, M = _host(name)
    P, npaths = c.P, len(ip) - 1
    tabs = [I32(a, dev) for a in c.arrays()]
    pmk = PathMasks(ip, cols, P, dev)
    assert pmk.run_block == S
    rng = np.random.default_rng(5)
    rows = np.concatenate([rng.permutation(npaths), rng.integers(0, npaths, npaths // 2 + 1)])       # every path, some twice
    w = T_((Dout, P), 2, dev, -0.05, 0.05)
    bias = T_((Dout,), 3, dev)
    d, st = lib.stream_args(w)
    wT = torch.empty((P, Dout), device=dev)
    lib.call('mmft_transpose', w, wT, Dout, P, d, st)
    for B in (1, 2):
        f = T_((B, P), 1, dev).reshape(-1).contiguous()
        GP = torch.empty((B * P, Dout), device=dev)
        lib.call('mmft_masked_fc_prefix', f, wT, GP, B, P, Dout, S, d, st)
        des = np.arange(rows.shape[0]) % B
        offs = [None, I32(np.zeros_like(rows), dev)] if B == 1 else [I32(np.zeros_like(rows), dev), I32(des * P, dev)]
        f64, w64 = f.double().cpu().numpy().reshape(B, P), w.double().cpu().numpy()
        m = float(f.abs().max() * w.abs().max())
        for foff in offs:
            des_h = np.zeros_like(rows) if foff is None else foff.cpu().numpy() // P
            for sel in (rows, rows[:1]):                                      # a permutation with repeats, and T = 1
                Tn = sel.shape[0]
                paths = I32(sel, dev)
                fo = None if foff is None else foff[:Tn].contiguous()
                for b in (bias, None):
                    want = torch.full((Tn, Dout), NAN, device=dev)
                    lib.call('mmft_masked_fc_fwd_runs', pmk.run_ptr, pmk.run_start, pmk.run_len, paths, fo, Tn, GP, b, want, Dout, S, d, st)
                    got = torch.full((Tn, Dout), NAN, device=dev)
                    stats = torch.full((Tn, 2), -7, dtype=torch.int32, device=dev)
                    _placed(tabs, c, paths, fo, GP, b, got, Dout, Dout, stats)
                    assert not bool(torch.isnan(want).any()) and torch.equal(got, want), (name, Dout, B, Tn)
                    assert np.array_equal(stats.cpu().numpy(), counts[sel])
                    again = torch.full((Tn, Dout), NAN, device=dev)
                    _placed(tabs, c, paths, fo, GP, b, again, Dout, Dout, None)
                    assert torch.equal(again, got)
                    # the fp64 dense product, under the bound test_masked_fc_kernels holds the run form to
                    ref = (M[sel] * f64[des_h[:Tn]]) @ w64.T + (b.double().cpu().numpy() if b is not None else 0.0)
                    bound = TOL * np.abs(ref).max() + float(M[sel].sum(1).max()) * S * m * EPS24
                    ok, err = close(got, ref, bound)
                    assert ok, (name, Dout, B, err, bound)
        # ldo > Dout: a column slice of a wider tensor; the columns around it are not written
        paths = I32(rows, dev)
        wide = torch.full((rows.shape[0], Dout + 8), NAN, device=dev)
        view = wide[:, 4:4 + Dout]
        assert view.data_ptr() % 16 == 0
        _placed(tabs, c, paths, offs[-1], GP, bias, view, Dout + 8, Dout, None)
        want = torch.empty((rows.shape[0], Dout), device=dev)
        lib.call('mmft_masked_fc_fwd_runs', pmk.run_ptr, pmk.run_start, pmk.run_len, paths, offs[-1], rows.shape[0], GP, bias, want, Dout, S, d, st)
        assert torch.equal(view, want) and bool(torch.isnan(wide[:, :4]).all()) and bool(torch.isnan(wide[:, 4 + Dout:]).all())
    # the device rasteriser agrees with the host rule on the same tables (what Predictor checks at construction)
    from mmft import prep
    dip, dcols = prep.rasterize_path_masks(*tabs, c.map_x, c.map_y)
    assert np.array_equal(dip.cpu().numpy(), ip) and np.array_equal(dcols.cpu().numpy(), cols)


# ------------------------------------------------------------------------------------------------ 2. bad arguments
def test_bad_arguments_launch_nothing(dev):
    c = C.CASES['edges_16x16']
    tabs = [I32(a, dev) for a in c.arrays()]
    Dout, Tn = 8, 3
    paths = I32([1, 2, 3], dev)
    GP = torch.zeros((c.P, Dout), device=dev)
    out = torch.full((Tn, Dout), 7.0, device=dev)
    d, st = lib.stream_args(GP)
    good = [tabs[0], tabs[1], c.maxlen, tabs[2], tabs[3], c.map_x, c.map_y, paths, None, Tn, GP, None, out, Dout, Dout, S, None, d, st]
    lib.place('mmft_placed_fc_fwd', *good)
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
    out.fill_(7.0)
    wrong = {'P % 64': {5: 10, 6: 10}, 'P > 65536': {5: 512, 6: 256}, 'S': {15: 32}, 'Dout = 6': {13: 8, 14: 6}, 'Dout = 0': {14: 0},
             'Dout > 1024': {13: 1028, 14: 1028}, 'maxlen': {2: 0}, 'T < 0': {9: -1}, 'ldo < Dout': {13: 4}, 'map_x = 0': {5: 0},
             'null nodes': {0: None}, 'null lens': {1: None}, 'null loc_x': {3: None}, 'null loc_y': {4: None}, 'null paths': {7: None},
             'null GP': {10: None}, 'null out': {12: None}, 'unaligned GP': {10: GP.data_ptr() + 4}, 'unaligned out': {12: out.data_ptr() + 4},
             'unaligned bias': {11: GP.data_ptr() + 8}}
    for what, change in wrong.items():
        args = list(good)
        for k, v in change.items():
            args[k] = v
        with pytest.raises(RuntimeError, match=r'mmft_placed_fc_fwd failed \(-1\): placed_fc_fwd'):
            lib.place('mmft_placed_fc_fwd', *args)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), what
    args = list(good)
    args[9] = 0                                                                # T = 0: fine, and nothing to write
    lib.place('mmft_placed_fc_fwd', *args)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ 3. - 6. Predictor
def _moved_copy(d, xy):
    """The design with its pins at xy and its masks rebuilt on the host: what a caller without placement mode would build."""
    return PL.attach_placement(copy.copy(d), d.path_nodes, d.path_lens, *xy)


def _live_models(designs, dev):
    """test_infer_gpu's models, with the U-Net's last bias raised: its single output channel ends in a ReLU, and with these
    seeds every cell of the map is negative in front of it - an all-zero feature map, on which no mask matters."""
    pmodel, cnn = _models(designs, dev)
    with torch.no_grad():
        cnn.outc.conv[0].bias.fill_(2.0)
    return pmodel, cnn


@functools.lru_cache(maxsize=None)
def _small_designs():
    from mmft.synth import synth_design
    return tuple(C.placed(synth_design(N=2048, L=12, tile=32, seed=700 + i, end_frac=0.25), seed=40 + i) for i in range(2))


def test_predictor_with_unmoved_pins_predicts_what_it_predicted(dev):
    from mmft.infer import Predictor
    designs = list(_small_designs())
    assert designs[0].map_size == 16
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        plain = Predictor(pmodel, cnn, designs, dev)
        moving = Predictor(pmodel, cnn, designs, dev, placement=True)
        for k in range(4):                                                    # eager, the capturing call, two replays
            a, b = plain.predict()[0].clone(), moving.predict()[0].clone()
            assert torch.equal(a, b), k
        assert moving._replay.graph is not None and moving._replay.calls == 4 and moving._placed in moving._replay.keep
        assert np.array_equal(plain.endpoints, moving.endpoints)
        for i, d in enumerate(designs):
            for p in (plain, moving):
                ip, cols = p.masks(i)
                assert np.array_equal(ip, d.mask_indptr) and np.array_equal(cols, d.mask_cols)


def test_predictor_batches_a_truncated_row_with_a_wider_design(dev):
    """A design 5 nodes wide with a truncated row (length 40) next to one 9 wide: the device clips lengths to the common
    width, 9, so the tables must hold that row's length as 5 - its columns 5..8 are padding, not pins."""
    from mmft.infer import Predictor
    from mmft.synth import synth_design
    a, b = (C.placed(synth_design(N=2048, L=12, tile=32, seed=710 + i, end_frac=0.25), seed=50 + i, maxlen=w) for i, w in enumerate((5, 9)))
    q = int(np.flatnonzero(a.path_lens == 5)[0])
    lens = a.path_lens.copy(); lens[q] = 40
    PL.attach_placement(a, a.path_nodes, lens, a.pin_x, a.pin_y)
    designs = [a, b]
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        plain = Predictor(pmodel, cnn, designs, dev)
        moving = Predictor(pmodel, cnn, designs, dev, placement=True)
        assert moving._placed.maxlen == 9 and int(moving._placed.lens.max()) <= 9 and int(moving._placed.lens[q]) == 5
        for k in range(3):
            assert torch.equal(plain.predict()[0], moving.predict()[0]), k
        for i, d in enumerate(designs):
            ip, cols = moving.masks(i)
            assert np.array_equal(ip, d.mask_indptr) and np.array_equal(cols, d.mask_cols)
        xy = C.move(a, seed=61, frac=0.5)
        moving.update(0, pin_x=xy[0], pin_y=xy[1])
        fresh = Predictor(pmodel, cnn, [_moved_copy(a, xy), b], dev).predict()[0].clone()
        assert torch.equal(moving.predict()[0], fresh)


def test_predictor_follows_moved_pins(dev):
    from mmft.infer import Predictor
    designs = list(_small_designs())
    xy = [C.move(d, seed=60 + i, frac=0.5) for i, d in enumerate(designs)]
    moved = [_moved_copy(d, p) for d, p in zip(designs, xy)]
    assert all(not np.array_equal(m.mask_cols, d.mask_cols) for m, d in zip(moved, designs))
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        p = Predictor(pmodel, cnn, designs, dev, placement=True)
        stale = [p.predict()[0].clone() for _ in range(3)]
        assert p._replay.graph is not None
        tables = lambda: [t.data_ptr() for t in (p._placed.nodes, p._placed.lens, p._placed.loc_x, p._placed.loc_y)]
        ptrs = tables()
        p.update(0, pin_x=xy[0][0], pin_y=torch.from_numpy(xy[0][1]).to(dev))
        half = p.predict()[0].clone()
        fresh_half = Predictor(pmodel, cnn, [moved[0], designs[1]], dev).predict()[0].clone()
        assert torch.equal(half, fresh_half)
        assert not torch.equal(half, stale[0]) and all(torch.equal(stale[0], y) for y in stale)
        of_design = np.searchsorted(p.batch.node_off, p.endpoints, side='right') - 1
        one = torch.from_numpy(of_design == 1).to(dev)
        assert bool(one.any()) and bool((~one).any()) and torch.equal(half[one], stale[0][one])
        assert np.array_equal(p.masks(0)[1], moved[0].mask_cols) and np.array_equal(p.masks(1)[1], designs[1].mask_cols)
        # design 1 moves between two replays: same tables, same graph
        calls = p._replay.calls
        p.update(1, pin_x=xy[1][0].astype(np.int32), pin_y=xy[1][1])
        full = p.predict()[0].clone()
        again = p.predict()[0].clone()
        assert tables() == ptrs and p._replay.calls == calls + 2
        fresh = Predictor(pmodel, cnn, moved, dev).predict()[0].clone()
        assert torch.equal(full, fresh) and torch.equal(again, fresh) and not torch.equal(full, half)
        eager = Predictor(pmodel, cnn, designs, dev, placement=True, graphed=False, overlap=False)
        assert torch.equal(eager.predict()[0], stale[0])
        for i in range(2):
            eager.update(i, pin_x=xy[i][0], pin_y=xy[i][1])
        assert torch.equal(eager.predict()[0], fresh) and eager._replay is None


def test_predictor_refuses_bad_placement_arguments_and_stays_as_it_was(dev):
    from mmft.infer import Predictor
    from mmft.synth import synth_design
    designs = list(_small_designs())
    bare = synth_design(N=2048, L=12, tile=32, seed=701, end_frac=0.25)
    x, y = C.move(designs[0], seed=9, frac=0.5)
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models(designs, dev)
        with pytest.raises(ValueError, match='design 1'):
            Predictor(pmodel, cnn, [designs[0], bare], dev, placement=True)
        liar = copy.copy(designs[1])                                         # pins moved, masks not rebuilt
        liar.pin_x, liar.pin_y = C.move(designs[1], seed=10, frac=0.5)
        with pytest.raises(ValueError, match='design 1'):
            Predictor(pmodel, cnn, [designs[0], liar], dev, placement=True)
        plain = Predictor(pmodel, cnn, designs, dev)
        p = Predictor(pmodel, cnn, designs, dev, placement=True)
        for q in (plain, p):
            for _ in range(3):
                q.predict()
        ref = p.predict()[0].clone()
        new_image = np.random.default_rng(1).random(designs[0].image.shape).astype(np.float32)
        refusals = [dict(pin_x=x), dict(pin_y=y), dict(pin_x=x[:-1], pin_y=y[:-1]), dict(pin_x=x, pin_y=y.astype(np.float32)),
                    dict(pin_x=x.astype(np.int16), pin_y=y), dict(pin_x=x.tolist(), pin_y=y),
                    dict(pin_x=x, pin_y=y, image=new_image[:, :-1]),              # good pins, bad image: the pins stay too
                    dict(pin_x=x[:-1], pin_y=y[:-1], image=new_image)]            # bad pins, good image: the image stays too
        for bad in refusals:
            with pytest.raises((ValueError, TypeError)):
                p.update(0, **bad)
            assert torch.equal(p.predict()[0], ref), sorted(bad)
        with pytest.raises(IndexError):
            p.update(2, pin_x=x, pin_y=y)
        with pytest.raises(ValueError, match='placement=True'):
            plain.update(0, pin_x=x, pin_y=y)
        assert torch.equal(plain.predict()[0], ref) and torch.equal(p.predict()[0], ref)


def test_predictor_follows_moved_pins_on_a_128_x_128_map(dev):
    """The bitmap (2 KB), the scan (256 blocks, one per thread) and the search depth of the benched configuration, once."""
    from mmft.infer import Predictor
    from mmft.synth import synth_design
    d = C.placed(synth_design(N=1024, L=8, tile=256, seed=33, end_frac=0.25), seed=34)
    assert d.map_size == 128
    xy = C.move(d, seed=35, frac=0.5)
    moved = _moved_copy(d, xy)
    with lib.math_mode('bf16'):
        pmodel, cnn = _live_models([d], dev)
        p = Predictor(pmodel, cnn, [d], dev, placement=True)
        stale = [p.predict()[0].clone() for _ in range(3)]
        assert torch.equal(stale[0], Predictor(pmodel, cnn, [d], dev).predict()[0])
        p.update(0, pin_x=xy[0], pin_y=xy[1])
        got = p.predict()[0].clone()
        assert p._replay.graph is not None and p._replay.calls == 4
        assert torch.equal(got, Predictor(pmodel, cnn, [moved], dev).predict()[0]) and not torch.equal(got, stale[0])
        assert np.array_equal(p.masks(0)[1], moved.mask_cols)
