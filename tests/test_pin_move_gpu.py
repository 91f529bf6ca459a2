"""Discrete pin sensitivity on the GPU (include/mmft_sens_pins.h): mmft_pin_move_rows / mmft_pin_move_sum on every case of
tests/pin_move_cases.py against the literal oracle of tests/pin_move_oracle.py, and Sensitivity(pins=True) end to end.

The bound per entry is  |got - ref| <= 2 (Dout + K + 1) 2^-24 A : the forward bound of an fp32 chain of that many operations
(the Dout-long dot product, the product with feat, K accumulations) on the fp64 sum of magnitudes A, the factor 2 for fma
contraction and the order of the sums.  For pin_move the K and A of the summed slots add, plus one operation per slot.  Entries
without a changed cell, later occurrences of a pin and padding are bitwise 0.0."""
import copy

import numpy as np
import pytest
import torch

from mmft import lib, ops, placement as PL
from pin_move_cases import CASES, DOUTS, PinCase, operands
from pin_move_oracle import bound, oracle

pytestmark = pytest.mark.gpu
SEED = 9294
GUARD = 64


def _bits(t):
    return t.contiguous().view(torch.int32)


def _tables(case, dev):
    nodes, lens, px, py = case.arrays()
    paths, f_off = case.selection()
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(dev)
    inc = PL.pin_incidence_host(nodes, lens, paths, px.shape[0])
    return dict(nodes=i32(nodes), lens=i32(lens), x=i32(px), y=i32(py), paths=i32(paths), f_off=None if f_off is None else i32(f_off),
                inc=(i32(inc[0]), i32(inc[1])))


def _guarded(shape, dev, fill):
    """(view of `shape`, the GUARD elements behind it) in one allocation; the view pre-filled with `fill`, the guard with 7.0."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), 7.0, device=dev)
    buf[:n] = fill
    return buf[:n].view(*shape), buf[n:]


def _check(case, Dout, got_row, got_pin, ref, what):
    row, pin = got_row.double().cpu().numpy(), got_pin.double().cpu().numpy()
    e_row, b_row = np.abs(row - ref['row_move']), bound(Dout, ref['K'], ref['A'])
    e_pin, b_pin = np.abs(pin - ref['pin_move']), bound(Dout, ref['pin_K'], ref['pin_A'], ref['pin_slots'])
    live = ref['K'] > 0
    print(f'{what} Dout {Dout}: {int(live.sum())} entries with changed cells, worst error / bound: row_move '
          f'{float((e_row[live] / b_row[live]).max()) if live.any() else 0.0:.3f}, pin_move '
          f'{float((e_pin[ref["pin_K"] > 0] / b_pin[ref["pin_K"] > 0]).max()) if (ref["pin_K"] > 0).any() else 0.0:.3f}')
    assert (e_row <= b_row).all() and (e_pin <= b_pin).all(), (case.name, Dout)
    zero = _bits(torch.zeros(1))[0].item()
    assert bool((_bits(got_row).cpu().numpy()[ref['K'] == 0] == zero).all())          # no changed cell, later occurrences, padding
    assert bool((_bits(got_pin).cpu().numpy()[ref['pin_K'] == 0] == zero).all())


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('name', list(CASES))
def test_kernels_vs_the_literal_oracle(dev, name):
    """Every case at Dout 4, 12 and 128: within the bound, exact zeros, a second call into NaN-filled buffers gives the same
    bits, the guard elements behind row_move / pin_move are untouched."""
    case = CASES[name]
    tb = _tables(case, dev)
    T, N = tb['paths'].numel(), tb['x'].numel()
    for Dout in DOUTS:
        feat, w, g = operands(case, Dout)
        ref = oracle(case, feat, w, g)
        f_d, wT_d, g_d = torch.from_numpy(feat).to(dev), torch.from_numpy(np.ascontiguousarray(w.T)).to(dev), torch.from_numpy(g).to(dev)
        outs = []
        for _ in range(2):
            row, row_guard = _guarded((T, case.maxlen, 4), dev, float('nan'))
            pin, pin_guard = _guarded((N, 4), dev, float('nan'))
            got = ops.pin_move_rows(tb['nodes'], tb['lens'], tb['x'], tb['y'], case.map_x, case.map_y, tb['paths'], tb['f_off'], f_d, wT_d,
                                    g_d, row_move=row)
            assert got is row
            assert ops.pin_move_sum(row, *tb['inc'], pin_move=pin) is pin
            torch.cuda.synchronize()
            assert bool((row_guard == 7.0).all()) and bool((pin_guard == 7.0).all())
            outs.append((row, pin))
        assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
        _check(case, Dout, outs[0][0], outs[0][1], ref, name)
        # without output buffers: the same bits
        row2 = ops.pin_move_rows(tb['nodes'], tb['lens'], tb['x'], tb['y'], case.map_x, case.map_y, tb['paths'], tb['f_off'], f_d, wT_d, g_d)
        assert torch.equal(_bits(row2), _bits(outs[0][0])) and torch.equal(_bits(ops.pin_move_sum(row2, *tb['inc'])), _bits(outs[0][1]))


@pytest.mark.parametrize('name', ['repeats_16x16', 'two_designs_16x16', 'seeded_128x128'])
def test_a_strided_g_gives_the_bits_of_a_dense_one(dev, name):
    """g as the column slice [:, 128:256] of a [T, 288] tensor - the h_cnn slice of the head's dx - against a dense copy."""
    case = CASES[name]
    tb = _tables(case, dev)
    feat, w, g = operands(case, 128)
    f_d, wT_d = torch.from_numpy(feat).to(dev), torch.from_numpy(np.ascontiguousarray(w.T)).to(dev)
    wide = torch.full((g.shape[0], 288), float('nan'), device=dev)
    wide[:, 128:256] = torch.from_numpy(g).to(dev)
    view = wide[:, 128:256]
    assert view.stride(0) == 288 and not view.is_contiguous()
    run = lambda gg: ops.pin_move_rows(tb['nodes'], tb['lens'], tb['x'], tb['y'], case.map_x, case.map_y, tb['paths'], tb['f_off'], f_d, wT_d, gg)
    a, b = run(view), run(view.contiguous())
    assert torch.equal(_bits(a), _bits(b)) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0.0


def test_the_wrappers_refuse_what_the_kernels_do_not_take(dev):
    case = CASES['repeats_16x16']
    tb = _tables(case, dev)
    feat, w, g = operands(case, 12)
    f_d, wT_d, g_d = torch.from_numpy(feat).to(dev), torch.from_numpy(np.ascontiguousarray(w.T)).to(dev), torch.from_numpy(g).to(dev)
    args = lambda **kw: {**dict(nodes=tb['nodes'], lens=tb['lens'], loc_x=tb['x'], loc_y=tb['y'], map_x=16, map_y=16, paths=tb['paths'],
                                f_off=None, feat=f_d, wT=wT_d, g=g_d), **kw}
    with pytest.raises(ValueError, match='B \\* 256 elements'):
        ops.pin_move_rows(**args(feat=f_d[:-1]))
    with pytest.raises(ValueError, match='g must be'):
        ops.pin_move_rows(**args(g=g_d[:-1]))
    with pytest.raises(TypeError, match='int32'):
        ops.pin_move_rows(**args(paths=tb['paths'].long()))
    with pytest.raises(ValueError, match='row_move must be'):
        ops.pin_move_rows(**args(row_move=torch.zeros(3, device=dev)))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.pin_move_rows(**args(nodes=tb['nodes'].cpu()))
    with pytest.raises(ValueError, match='1 .. 1024 nodes'):
        ops.pin_move_rows(**args(nodes=torch.zeros((2, 1025), dtype=torch.int32, device=dev), lens=torch.zeros(2, dtype=torch.int32, device=dev)))
    row = ops.pin_move_rows(**args())
    with pytest.raises(ValueError, match='pin_move must be'):
        ops.pin_move_sum(row, *tb['inc'], pin_move=torch.zeros((3, 4), device=dev))
    with pytest.raises(ValueError, match=r'\[T, maxlen, 4\]'):
        ops.pin_move_sum(row.reshape(-1, 4), *tb['inc'])
    # no selected row: nothing is launched, every pin is 0
    none = ops.pin_move_rows(**args(paths=tb['paths'][:0], g=g_d[:0]))
    assert tuple(none.shape) == (0, case.maxlen, 4)
    ptr0 = torch.zeros(tb['x'].numel() + 1, dtype=torch.int32, device=dev)
    assert float(ops.pin_move_sum(none, ptr0, tb['inc'][1][:0]).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ end to end
def _design(fanin, seed=SEED):
    from mmft.synth import synth_design
    from place_cases import placed
    return placed(synth_design(N=2048, L=16, tile=32, seed=SEED, fanin=fanin), seed)


def _models(d, dev):
    from mmft.train import build_models
    return build_models(map_size=d.map_size, device=dev, seed=SEED)


def _weights(T, seed=12):
    return torch.randn(T, generator=torch.Generator().manual_seed(seed))


def _case_of(s, name):
    """The object's own tables - path nodes, the pins as they are NOW, the selection - as a PinCase for the oracle."""
    p = s.placed
    c = PinCase(name, p.map_x, p.map_y, p.maxlen, B=p.B)
    c.px, c.py = p.loc_x.cpu().numpy().astype(np.int64).tolist(), p.loc_y.cpu().numpy().astype(np.int64).tolist()
    c.rows, c.lens = p.nodes.cpu().numpy().astype(np.int64).tolist(), p.lens.cpu().numpy().astype(np.int64).tolist()
    c.paths = s._sel[1].cpu().numpy().astype(np.int64)
    c.f_off = s._sel[2].cpu().numpy().astype(np.int64) if p.B > 1 else None
    return c


def _against_oracle(s, pmodel, grads, name):
    """grads[i]['pin_move'] and s.row_move against the oracle fed the object's own proj_grad, feat_map and fcn.weight."""
    case = _case_of(s, name)
    g = s.proj_grad.detach().cpu().numpy()
    ref = oracle(case, s.feat_map.detach().reshape(-1).cpu().numpy(), pmodel.fcn.weight.detach().cpu().numpy(), g)
    pin = torch.cat([gr['pin_move'] for gr in grads])
    assert pin.dtype == torch.float32 and tuple(pin.shape) == (len(case.px), 4) and tuple(s.row_move.shape) == ref['row_move'].shape
    assert int((ref['pin_K'] > 0).sum()) > 20 and float(np.abs(ref['pin_move']).max()) > 0.0
    _check(case, g.shape[1], s.row_move, pin, ref, name)
    return ref


def _same(a, b, keys=('cell_feat', 'net_feat')):
    return all(torch.equal(_bits(x[k]), _bits(y[k])) for x, y in zip(a, b) for k in keys)


@pytest.fixture(scope='module')
def resident(dev):
    """Per fan-in kind, made once: the placed design, the modules, and in bf16 mode a pins=False and a pins=True object with
    one run() each on the same seeded weights."""
    from mmft.sensitivity import Sensitivity
    cache = {}

    def get(fanin):
        if fanin not in cache:
            d = _design(fanin, seed=31)
            pmodel, cnn = _models(d, dev)
            w = _weights(d.num_paths)
            with lib.math_mode('bf16'):
                plain, pins = Sensitivity(pmodel, cnn, [d], dev), Sensitivity(pmodel, cnn, [d], dev, pins=True)
                r0, r1 = plain.run(weights=w), pins.run(weights=w)
            torch.cuda.synchronize()
            cache[fanin] = dict(d=d, pmodel=pmodel, cnn=cnn, w=w, plain=plain, pins=pins, r0=r0, r1=r1)
        return cache[fanin]
    return get


@pytest.mark.parametrize('fanin', ['regular', 'irregular'])
def test_sensitivity_returns_pin_move_and_changes_nothing_else(dev, resident, fanin):
    c = resident(fanin)
    (p0, e0, g0), (p1, e1, g1) = c['r0'], c['r1']
    assert 'pin_move' not in g0[0] and tuple(g1[0]['pin_move'].shape) == (c['d'].N, 4)
    assert torch.equal(_bits(p0), _bits(p1)) and np.array_equal(e0, e1) and _same(g0, g1)
    assert c['plain'].placed is None and c['plain'].row_move is None and c['plain'].proj_grad is None
    assert tuple(c['pins'].proj_grad.shape) == (c['pins'].T, c['pmodel'].fcn.weight.shape[0])
    _against_oracle(c['pins'], c['pmodel'], g1, f'e2e_{fanin}')
    # pins on no selected path: exactly 0
    on_a_row = np.zeros(c['d'].N, dtype=bool)
    nodes, lens = np.asarray(c['d'].path_nodes), np.asarray(c['d'].path_lens)
    for q in range(nodes.shape[0]):
        on_a_row[nodes[q, :min(int(lens[q]), nodes.shape[1])]] = True
    assert (~on_a_row).any() and float(g1[0]['pin_move'][torch.from_numpy(~on_a_row).to(dev)].abs().max()) == 0.0


def test_with_image_the_same_holds(dev, resident):
    from mmft.sensitivity import Sensitivity
    c = resident('regular')
    with lib.math_mode('bf16'):
        a = Sensitivity(c['pmodel'], c['cnn'], [c['d']], dev, image=True)
        b = Sensitivity(c['pmodel'], c['cnn'], [c['d']], dev, image=True, pins=True)
        (p0, _, g0), (p1, _, g1) = a.run(weights=c['w']), b.run(weights=c['w'])
        torch.cuda.synchronize()
        assert torch.equal(_bits(p0), _bits(p1)) and _same(g0, g1, ('cell_feat', 'net_feat', 'image'))
        assert torch.equal(_bits(p1), _bits(c['r1'][0]))
        _against_oracle(b, c['pmodel'], g1, 'e2e_regular_image')
        x = np.asarray(c['d'].pin_x)
        with pytest.raises(ValueError, match='image=True'):
            b.update(0, pin_x=x, pin_y=x)


def test_update_of_the_pins_then_run_equals_a_fresh_object_on_the_moved_design(dev, resident):
    from mmft.sensitivity import Sensitivity
    from place_cases import move
    c = resident('irregular')
    d, s = c['d'], c['pins']
    x, y = move(d, seed=32, frac=0.25)
    d2 = PL.attach_placement(copy.copy(d), d.path_nodes, d.path_lens, x, y)
    assert d2.mask_cols is not d.mask_cols
    with lib.math_mode('bf16'):
        with pytest.raises(ValueError, match='go together'):
            s.update(0, pin_x=x)
        with pytest.raises(ValueError, match='pins'):
            s.update(0, pin_x=x[:-1], pin_y=y[:-1])
        with pytest.raises(ValueError, match='pins=True'):
            c['plain'].update(0, pin_x=x, pin_y=y)
        s.update(0, pin_x=x, pin_y=y)
        pred_u, _, g_u = s.run(weights=c['w'])
        fresh = Sensitivity(c['pmodel'], c['cnn'], [d2], dev)
        pred_f, _, g_f = fresh.run(weights=c['w'])
        torch.cuda.synchronize()
        assert torch.equal(_bits(pred_u), _bits(pred_f)) and _same(g_u, g_f)
        assert not torch.equal(_bits(pred_u), _bits(c['r1'][0]))
        assert np.array_equal(s.placed.loc_x.cpu().numpy(), x) and np.array_equal(s.placed.loc_y.cpu().numpy(), y)
        _against_oracle(s, c['pmodel'], g_u, 'e2e_irregular_moved')
        s.update(0, pin_x=torch.from_numpy(np.asarray(d.pin_x)), pin_y=torch.from_numpy(np.asarray(d.pin_y)))      # back
        pred_b, _, g_b = s.run(weights=c['w'])
        assert torch.equal(_bits(pred_b), _bits(c['r1'][0])) and _same(g_b, c['r1'][2], ('cell_feat', 'net_feat', 'pin_move'))


def test_nothing_of_the_model_is_written_with_pins(dev, resident):
    from test_sens_gpu import _same_snapshot, _snapshot
    c = resident('regular')
    with lib.math_mode('bf16'):
        snap = _snapshot(c['pmodel'], c['cnn'])
        pred, _, g = c['pins'].run(weights=c['w'])
        torch.cuda.synchronize()
        _same_snapshot(snap, _snapshot(c['pmodel'], c['cnn']))
    assert torch.equal(_bits(pred), _bits(c['r1'][0])) and _same(g, c['r1'][2], ('cell_feat', 'net_feat', 'pin_move'))


def test_batch_of_two_designs(dev):
    """Two placed designs in one batch: f_off != 0 and a node offset, each design's pin_move in its own node order."""
    from mmft.sensitivity import Sensitivity
    designs = [_design('regular', seed=33), _design('irregular', seed=34)]
    pmodel, cnn = _models(designs[0], dev)
    with lib.math_mode('bf16'):
        s = Sensitivity(pmodel, cnn, designs, dev, pins=True)
        _, _, grads = s.run(weights=_weights(s.T, seed=13))
        torch.cuda.synchronize()
    assert [tuple(g['pin_move'].shape) for g in grads] == [(d.N, 4) for d in designs]
    ref = _against_oracle(s, pmodel, grads, 'e2e_two_designs')
    assert all(float(np.abs(ref['pin_move'][int(s.batch.node_off[i]):int(s.batch.node_off[i + 1])]).max()) > 0.0 for i in range(2))
