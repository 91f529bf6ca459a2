"""Discrete pin sensitivity without a GPU: mmft.placement.pin_move_host (the segment form) against the literal oracle of
tests/pin_move_oracle.py on every case, the conditions under which the cases bite, the ledger of include/mmft_sens_pins.h (the
rules test_sens_cpu.py applies to include/mmft_sens.h) with the host-side refusals of its two entry points, and the refusals of
Sensitivity(pins=True) that need no device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from abi_ledger import call_sites, declared as _declared, others
from mmft import lib, placement as PL
from pin_move_cases import CASES, DOUTS, HAND, PinCase, operands
from pin_move_oracle import FLAGS, geometry, oracle

NAMES = ['mmft_pin_move_rows', 'mmft_pin_move_sum']
NARGS = {'mmft_pin_move_rows': 18, 'mmft_pin_move_sum': 9}
OTHER_HEADERS = others('mmft_sens_pins.h')


# ------------------------------------------------------------------------------------------------ host form vs the definition
@pytest.mark.parametrize('name', list(CASES))
def test_host_segment_form_agrees_with_the_literal_oracle(name):
    """fp64 against fp64: 1e-12 A per entry; exactly 0 where no cell changes and at positions that are no first occurrence."""
    case = CASES[name]
    nodes, lens, px, py = case.arrays()
    paths, f_off = case.selection()
    for Dout in DOUTS:
        feat, w, g = operands(case, Dout)
        ref = oracle(case, feat, w, g)
        row, pin = PL.pin_move_host(nodes, lens, px, py, case.map_x, case.map_y, paths, f_off, feat, w, g)
        assert row.shape == ref['row_move'].shape == (paths.shape[0], case.maxlen, 4) and pin.shape == (px.shape[0], 4)
        assert (np.abs(row - ref['row_move']) <= 1e-12 * ref['A']).all(), (name, Dout)
        assert (row[ref['K'] == 0] == 0.0).all()
        assert (np.abs(pin - ref['pin_move']) <= 1e-12 * ref['pin_A']).all(), (name, Dout)
        assert (pin[ref['pin_slots'] == 0] == 0.0).all()
    # positions that are no first occurrence (later occurrences, padding, beyond the length) have no entry in the oracle at all
    firsts = {(t, j) for t, j, _, _, _ in geometry(case)}
    for t, q in enumerate(paths.tolist()):
        ids = nodes[q, :max(min(int(lens[q]), case.maxlen), 0)].tolist()
        assert {j for tt, j in firsts if tt == t} == {j for j, n in enumerate(ids) if n not in ids[:j]}


def test_incidence_csr_lists_first_occurrences_in_ascending_order():
    for case in CASES.values():
        nodes, lens, px, _ = case.arrays()
        paths, _ = case.selection()
        ptr, slot = PL.pin_incidence_host(nodes, lens, paths, px.shape[0])
        want = {}
        for t, j, d, _, _ in geometry(case):
            if d == 0:
                want.setdefault(int(nodes[paths[t], j]), []).append(t * case.maxlen + j)
        assert ptr[0] == 0 and ptr[-1] == slot.shape[0] == sum(len(v) for v in want.values())
        for n in range(px.shape[0]):
            assert slot[ptr[n]:ptr[n + 1]].tolist() == want.get(n, []), (case.name, n)
    with pytest.raises(ValueError, match='outside'):
        PL.pin_incidence_host(np.array([[0, 5]]), np.array([2]), np.array([0]), 3)


# ------------------------------------------------------------------------------------------------ the cases bite
def test_the_cases_bite():
    """Conditions on the INPUTS, under the unflagged rule alone: every flagged oracle differs from the true one on at least one
    entry; every direction has entries that gain cells and entries that lose cells; an entry keeps a proposed cell because a
    box the pin does not touch covers it; rows with a repeated pin, pins with several slots and a non-zero f_off exist."""
    feat_w_g = {c.name: operands(c, 4) for c in HAND}
    true = {c.name: oracle(c, *feat_w_g[c.name]) for c in HAND}
    for flag in FLAGS:
        differs = 0
        for c in HAND:
            o = oracle(c, *feat_w_g[c.name], flag=flag)
            differs += int((np.abs(o['row_move'] - true[c.name]['row_move']) > 1e-9 * (true[c.name]['A'] + o['A']) + 1e-300).sum())
        print(f'{flag}: {differs} entries differ')
        assert differs > 0, flag
    gains, loses, kept = np.zeros(4, dtype=int), np.zeros(4, dtype=int), 0
    for c in CASES.values():
        true_g = geometry(c)
        for t, j, d, gained, lost in true_g:
            gains[d] += bool(gained.any())
            loses[d] += bool(lost.any())
        if c in HAND:
            for (_, _, _, g0, l0), (_, _, _, g1, l1) in zip(true_g, geometry(c, 'ignore_coverage')):
                kept += int(((l1 > 0) & (l0 == 0)).any())               # a cell the pin's boxes lose, yet the mask keeps
    print('entries that gain cells per direction', gains, 'that lose cells', loses, 'with a cell kept by another box', kept)
    assert (gains > 0).all() and (loses > 0).all() and kept > 0
    rep = CASES['repeats_16x16']
    nodes, lens, _, _ = rep.arrays()
    assert any(len(set(r[:n])) < n for r, n in zip(nodes.tolist(), lens.tolist()))
    two = CASES['two_designs_16x16']
    assert two.selection()[1].max() == two.P and int(true[two.name]['pin_slots'].max()) > 1
    edge = true['edges_of_the_map_16x16']
    tags = CASES['edges_of_the_map_16x16'].tags
    assert edge['K'][tags.index('on_the_edge_moving_out'), 0, 0] == 0                 # x + 1 off the edge: clamped back
    assert edge['K'][tags.index('outside_moving_in_box_appears'), 0, 0] == 3          # the line x = 0, y in [5, 7]
    assert edge['K'][tags.index('single_cell_vanishes'), 0, 1] == 1 and edge['K'][tags.index('outside_moving_further_out'), 0, 1] == 0
    assert (edge['K'][tags.index('int32_extremes'), 0, 0] == 0) and (edge['K'][tags.index('int32_extremes'), 2, 1] == 0)


# ------------------------------------------------------------------------------------------------ the ledger
def test_pins_header_declares_exactly_the_two_names_and_overlaps_no_other_header():
    hd = _declared('mmft_sens_pins.h')
    decls = lib.pmove_decls()
    assert sorted(hd) == NAMES == sorted(decls)
    assert {n: len(decls[n][1]) for n in NAMES} == hd == NARGS
    for other in OTHER_HEADERS:
        assert not set(hd) & set(_declared(other)), other
    assert sorted(_declared('mmft_sens.h')) == ['mmft_mlp2_feat_dx_bf16'] and sorted(_declared('mmft_place.h')) == ['mmft_placed_fc_fwd']
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    assert decls['mmft_pin_move_rows'] == (I, [P, P, I, P, P, I, I, P, P, I, P, P, I, P, LL, P, I, P])
    assert decls['mmft_pin_move_sum'] == (I, [P, LL, P, P, LL, I, P, I, P])
    for foreign in ('mmft_version', 'mmft_placed_fc_fwd', 'mmft_mlp2_feat_dx_bf16'):
        with pytest.raises(RuntimeError, match='not declared'):
            lib.pmove(foreign)
    assert not set(NAMES) & (set(lib.place_decls()) | set(lib.sens_decls()) | set(lib.header_decls()))
    # the accessor's name is its own: the ledgers match call sites by attribute name
    assert lib.pmove not in (lib.call, lib.query, lib.ext, lib.place, lib.incr, lib.crit, lib.head, lib.csum, lib.sens, lib.simg)


def test_every_pmove_call_site_matches_the_header():
    protos = _declared('mmft_sens_pins.h')
    checked, bad, product = 0, [], set()
    for name, n, f, lineno in call_sites('pmove'):
        if n is None or name not in protos:                         # (a list built elsewhere; the refusal test above)
            continue
        checked += 1
        if os.sep + 'mmft' + os.sep in f:
            product.add(name)
        if protos.get(name) != n:
            bad.append((name, protos.get(name), n, f, lineno))
    assert checked >= 2 and product == set(NAMES) and not bad, bad


def _rows(**change):
    """A full argument list of mmft_pin_move_rows made of host integers: nothing can be launched on it, and nothing is."""
    a = dict(path_nodes=64, path_lens=64, maxlen=12, loc_x=64, loc_y=64, map_x=16, map_y=16, paths=64, f_off=None, T=5, feat=64, wT=64,
             Dout=128, g=64, ldg=288, row_move=64, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def _sum(**change):
    a = dict(row_move=64, slots=60, inc_ptr=64, inc_slot=64, nnz=7, N=9, pin_move=64, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def test_the_built_library_exports_the_names_and_refuses_bad_arguments_on_the_host():
    L = lib.load()
    assert not [n for n in NAMES if not hasattr(L, n)]
    assert L.mmft_version() >= 210
    assert len(_rows()) == NARGS['mmft_pin_move_rows'] and len(_sum()) == NARGS['mmft_pin_move_sum']
    refused = dict(null_nodes=dict(path_nodes=None), null_lens=dict(path_lens=None), null_x=dict(loc_x=None), null_y=dict(loc_y=None),
                   null_paths=dict(paths=None), null_feat=dict(feat=None), null_wT=dict(wT=None), null_g=dict(g=None),
                   null_out=dict(row_move=None), T_neg=dict(T=-1), maxlen0=dict(maxlen=0), maxlen_above_cap=dict(maxlen=1025),
                   cells_not_64=dict(map_x=10, map_y=10), cells_above_65536=dict(map_x=512, map_y=256), map0=dict(map_x=0),
                   Dout0=dict(Dout=0), Dout_odd=dict(Dout=6, ldg=8), Dout_above_1024=dict(Dout=1028, ldg=1028),
                   short_g_pitch=dict(ldg=124), odd_g_pitch=dict(ldg=130), odd_g=dict(g=68), odd_wT=dict(wT=72), odd_feat=dict(feat=68))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_pin_move_rows failed \(-1\): pin_move_rows'):
            lib.pmove('mmft_pin_move_rows', *_rows(**change))
    # T == 0 returns 0 and looks at no pointer - but its sizes are still judged
    assert lib.pmove('mmft_pin_move_rows', *_rows(T=0)) == 0
    assert lib.pmove('mmft_pin_move_rows', *_rows(T=0, path_nodes=None, path_lens=None, loc_x=None, loc_y=None, paths=None, feat=None,
                                                 wT=None, g=None, row_move=None)) == 0
    with pytest.raises(RuntimeError, match='bad sizes'):
        lib.pmove('mmft_pin_move_rows', *_rows(T=0, maxlen=1025))
    refused = dict(null_ptr=dict(inc_ptr=None), null_out=dict(pin_move=None), null_slot=dict(inc_slot=None), null_rows=dict(row_move=None),
                   N_neg=dict(N=-1), N_big=dict(N=1 << 29), slots_neg=dict(slots=-1), slots_big=dict(slots=1 << 29), nnz_neg=dict(nnz=-1),
                   nnz_big=dict(nnz=1 << 31), odd_rows=dict(row_move=68), odd_out=dict(pin_move=72))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_pin_move_sum failed \(-1\): pin_move_sum'):
            lib.pmove('mmft_pin_move_sum', *_sum(**change))
    assert lib.pmove('mmft_pin_move_sum', *_sum(N=0)) == 0
    assert lib.pmove('mmft_pin_move_sum', *_sum(N=0, row_move=None, inc_ptr=None, inc_slot=None, pin_move=None)) == 0
    with pytest.raises(RuntimeError, match='bad sizes'):
        lib.pmove('mmft_pin_move_sum', *_sum(N=0, slots=-1))


# ------------------------------------------------------------------------------------------------ host-side refusals
def test_sensitivity_pins_refusals_need_no_device():
    """check_pins_model and check_pin_update are plain functions, as check_model is: Sensitivity.__init__ / update() call them
    before a device is touched."""
    from mmft import sensitivity as S
    from mmft.synth import synth_design
    from mmft.train import build_models
    from place_cases import placed
    import model as M
    d = synth_design(N=256, L=8, tile=16, seed=3)
    pm, _ = build_models(map_size=d.map_size, device='cpu', seed=3, unet=False)
    cnn = torch.nn.Identity()
    with pytest.raises(ValueError, match='no placement data'):
        S.check_pins_model(pm, cnn, [d])
    placed(d, seed=4)
    assert PL.has_placement(d)
    S.check_pins_model(pm, cnn, [d])
    with pytest.raises(ValueError, match='design 1 carries no placement data'):
        S.check_pins_model(pm, cnn, [d, synth_design(N=256, L=8, tile=16, seed=5)])
    with pytest.raises(ValueError, match='no CNN'):
        S.check_pins_model(pm, None, [d])
    with pytest.raises(ValueError, match='no masked projection'):
        S.check_pins_model(M.PathModel(pm.gnn, None, None, None, None, pm.mlp_fuse), cnn, [d])
    with pytest.raises(ValueError, match='no CNN'):
        S.Sensitivity(pm, None, [d], 'cpu', pins=True)                  # refused before anything is built
    x = np.zeros(d.N, dtype=np.int64)
    assert S.check_pin_update(False, False, None, None) is False and S.check_pin_update(True, True, None, None) is False
    assert S.check_pin_update(True, False, x, x) is True
    with pytest.raises(ValueError, match='pins=True'):
        S.check_pin_update(False, False, x, x)
    with pytest.raises(ValueError, match='image=True'):
        S.check_pin_update(True, True, x, x)
    with pytest.raises(ValueError, match='go together'):
        S.check_pin_update(True, False, x, None)
    # the default is off, and a PinCase is what the helper says it is
    import inspect
    assert inspect.signature(S.Sensitivity.__init__).parameters['pins'].default is False
    assert isinstance(CASES['repeats_16x16'], PinCase)
