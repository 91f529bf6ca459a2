"""Masks that follow a placement, without a GPU: the ledger of include/mmft_place.h (the rules test_report_cpu.py applies to
include/mmft_report.h), mmft.placement's host side (rasterize_host, runs_host, attach_placement, the record round trip,
PlacedPaths' batching) against the oracle's mask rule, fusion._runs_from_csr and a literal restatement, and a mutation check:
each clause of the rule, broken in the literal form, must be noticed by the cases test_place_gpu.py feeds to the kernel."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import place_cases as C
from abi_ledger import call_sites, code_only as _code_only, declared as _declared
from mmft import fusion, lib
from mmft import placement as PL
from oracle.prep_restatement import path_mask_rows

HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------------------------------------ the header's ledger
def test_place_header_is_exported_and_the_other_headers_are_what_they_were():
    plc, ext, ref = _declared('mmft_place.h'), _declared('mmft_report.h'), _declared('mmft.h')
    assert sorted(plc) == ['mmft_placed_fc_fwd'] == sorted(lib.place_decls())
    assert not set(plc) & (set(ext) | set(ref))
    L = lib.load()
    assert not [n for n in plc if not hasattr(L, n)]
    assert L.mmft_version() >= 203
    assert lib.header_symbols() == sorted(ref) and set(lib.header_decls()) == set(ref)
    assert sorted(lib.ext_decls()) == sorted(ext) == ['mmft_timing_report', 'mmft_timing_report_workspace_bytes']
    assert len(lib.place_decls()['mmft_placed_fc_fwd'][1]) == plc['mmft_placed_fc_fwd'] == 19
    with pytest.raises(RuntimeError, match='not declared'):
        lib.place('mmft_version')
    # bad arguments are refused on the host, before anything touches a device
    with pytest.raises(RuntimeError, match=r'mmft_placed_fc_fwd failed \(-1\)'):
        lib.place('mmft_placed_fc_fwd', None, None, 1, None, None, 8, 8, None, None, 1, None, None, None, 4, 4, 64, None, 0, None)


def test_every_place_call_site_matches_the_header_and_the_kernel_test_names_the_entry_point():
    protos = _declared('mmft_place.h')
    checked, bad = 0, []
    for name, n, f, lineno in call_sites('place'):
        if n is None or name == 'mmft_version':                        # (the refusal test above)
            continue
        checked += 1
        if protos.get(name) != n:
            bad.append((name, protos.get(name, 'not declared'), n, f, lineno))
    assert checked >= 3 and not bad, bad
    src = open(os.path.join(HERE, 'test_place_gpu.py')).read()
    assert 'pytestmark = pytest.mark.gpu' in src
    assert re.search(r'(?<![A-Za-z0-9_])mmft_placed_fc_fwd(?![A-Za-z0-9_])', _code_only(src))


# ------------------------------------------------------------------------------------------------ the rule on the host
def test_the_cases_hold_every_edge_they_claim():
    tags = {t for c in C.HAND for t in c.tags}
    assert {'len0', 'len1', 'len2', 'one_cell', 'overlap', 'whole_map', 'rows_across_a_block_boundary', 'starts_a_block',
            'ends_a_block', 'below_and_above', 'outside_high', 'outside_low', 'garbage_after_len', 'len_above_maxlen',
            'row_across_64', 'serpentine'} <= tags
    assert {(c.map_x, c.map_y) for c in C.HAND} >= {(8, 8), (16, 16), (24, 24), (32, 64), (32, 32)}
    assert all(c.P % C.S == 0 for c in C.CASES.values()) and C.S == fusion.RUN_BLOCK
    assert [c.name for c in C.HAND if not c.in_range] == ['clamped_16x16', 'clipped_16x16']
    g = C.CASES['edges_16x16']
    rs = dict(zip(g.tags, C.run_rows(*PL.runs_host(*g.arrays(), g.map_x, g.map_y))))
    assert rs['len0'] == rs['len1'] == [] and rs['one_cell'] == [(3 * 16 + 3, 1)]
    assert rs['whole_map'] == [(0, 64), (64, 64), (128, 64), (192, 64)]
    assert rs['rows_across_a_block_boundary'] == [(48, 16), (64, 16)]
    assert rs['starts_a_block'] == [(64, 6)] and rs['ends_a_block'] == [(58, 6)]
    k = C.CASES['clamped_16x16']
    rows = dict(zip(k.tags, C.csr_rows(*PL.rasterize_host(*k.arrays(), 16, 16))))
    assert rows['outside_high'] == rows['outside_low'] == [] and rows['garbage_after_len1'] == []
    assert rows['below_and_above'] == [x * 16 + y for x in range(0, 5) for y in range(16)]
    assert rows['garbage_after_len'] == [x * 16 + y for x in (2, 3) for y in range(2, 7)]
    s = C.CASES['serpentine_32x32']
    rp = PL.runs_host(*s.arrays(), 32, 32)[0]
    assert 256 < rp[1] - rp[0] <= 1024                                 # more runs than the 256 entry lanes of Dout = 4
    s = C.CASES['serpentine_64x64']
    assert PL.runs_host(*s.arrays(), 64, 64)[0][1] > 1024              # more runs than the kernel lists: searched in the bitmap
    assert C.CASES['rows_of_24'].map_y % 32 != 0


@pytest.mark.parametrize('name', sorted(C.CASES))
def test_rasterize_and_runs_equal_the_oracle_the_csr_runs_and_the_literal_rule(name):
    c = C.CASES[name]
    ip, cols = PL.rasterize_host(*c.arrays(), c.map_x, c.map_y)
    assert ip.dtype == cols.dtype == np.int64 and ip[0] == 0 and ip[-1] == cols.shape[0]
    rows = C.csr_rows(ip, cols)
    if c.in_range:
        assert rows == path_mask_rows(*c.point_lists(), c.map_x, c.map_y)
    lit_rows, lit_runs = C.literal(c)
    assert rows == lit_rows
    got = PL.runs_host(*c.arrays(), c.map_x, c.map_y)
    want = fusion._runs_from_csr(ip, cols, fusion.RUN_BLOCK)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert C.run_rows(*got) == lit_runs
    assert sum(l for r in lit_runs for _, l in r) == cols.shape[0]


def test_runs_need_a_map_of_whole_blocks():
    with pytest.raises(ValueError, match='multiple'):
        PL.runs_host(np.zeros((1, 2), dtype=np.int64), np.array([0]), np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64), 10, 10)


@pytest.mark.parametrize('flag', ['exclusive_upper', 'no_block_split', 'no_clamp', 'len_unclipped', 'padding_counts'])
def test_the_cases_notice_each_broken_rule(flag):
    noticed = []
    for c in C.HAND:
        rows, runs = C.literal(c)
        b_rows, b_runs = C.literal(c, **{flag: True})
        if (rows, runs) != (b_rows, b_runs):
            noticed.append(c.name)
    expected = {'exclusive_upper': {'edges_16x16', 'single_block_8x8', 'rows_of_24', 'wide_32x64', 'serpentine_32x32'},
                'no_block_split': {'edges_16x16', 'rows_of_24', 'wide_32x64'}, 'no_clamp': {'clamped_16x16'},
                'len_unclipped': {'clipped_16x16'}, 'padding_counts': {'clamped_16x16'}}[flag]
    assert expected <= set(noticed), (flag, noticed)


# ------------------------------------------------------------------------------------------------ designs and records
def _design(seed=3):
    from mmft.synth import synth_design
    return synth_design(N=512, L=8, tile=32, seed=seed, end_frac=0.25)


def test_attach_placement_validates_and_rebuilds_the_masks():
    d = _design()
    old = d.mask_cols.copy()
    e = C.placed(copy.copy(d), seed=1)
    assert PL.has_placement(e) and not PL.has_placement(d)
    assert e.path_nodes.shape == (d.num_paths, 12) and e.path_lens.shape == (d.num_paths,) and e.pin_x.shape == e.pin_y.shape == (d.N,)
    assert e.path_lens[:3].tolist() == [0, 1, 12] and (e.path_nodes[np.arange(d.num_paths)[e.path_lens > 0], 0] == d.path2endpoint[e.path_lens > 0]).all()
    ip, cols = PL.rasterize_host(e.path_nodes, e.path_lens, e.pin_x, e.pin_y, e.map_size, e.map_size)
    assert np.array_equal(e.mask_indptr, ip) and np.array_equal(e.mask_cols, cols) and not np.array_equal(cols, old)
    loc = list(zip(e.pin_x.tolist(), e.pin_y.tolist()))
    assert C.csr_rows(ip, cols) == path_mask_rows([r[:n].tolist() for r, n in zip(e.path_nodes, e.path_lens)], loc, e.map_size, e.map_size)
    assert np.diff(ip).max() < e.map_size ** 2 // 2                    # local boxes, not the whole map
    good = (e.path_nodes, e.path_lens, e.pin_x, e.pin_y)
    f = copy.copy(d)

    def refused(i, value, exc=ValueError):
        args = list(good)
        args[i] = value
        with pytest.raises(exc):
            PL.attach_placement(f, *args)
        assert not PL.has_placement(f) and f.mask_cols is d.mask_cols
    refused(0, e.path_nodes[:-1])
    refused(0, e.path_nodes.astype(np.float32))
    refused(1, e.path_lens[:-1])
    refused(1, np.where(np.arange(d.num_paths) == 0, -1, e.path_lens))
    refused(2, e.pin_x[:-1])
    refused(3, e.pin_y.astype(np.float64))
    refused(3, e.pin_y.reshape(-1, 1))
    refused(2, np.where(np.arange(d.N) == 0, 2 ** 40, e.pin_x))
    bad = e.path_nodes.copy(); bad[2, 3] = d.N
    refused(0, bad)
    bad = e.path_nodes.copy(); bad[2, 3] = -1
    refused(0, bad)
    bad = e.path_nodes.copy(); bad[0, 5] = 7                          # beyond the length of row 0: must be -1
    refused(0, bad)
    # a truncated row (length above maxlen) and coordinates outside the map are data, not errors
    lens = e.path_lens.copy(); lens[2] = 40
    x = e.pin_x.copy(); x[::7] = -4; x[3::11] = 99
    h = PL.attach_placement(copy.copy(d), e.path_nodes, lens, x.astype(np.int32), e.pin_y)
    assert h.mask_cols.size and h.mask_cols.min() >= 0 and h.mask_cols.max() < h.map_size ** 2


def test_the_record_keeps_placement_data_and_a_design_without_it_is_what_it_was(tmp_path):
    from mmft.record import save_design, load_design
    d = _design()
    e = C.placed(copy.copy(d), seed=2)
    save_design(tmp_path / 'placed.npz', e)
    save_design(tmp_path / 'plain.npz', d)
    back, plain = load_design(tmp_path / 'placed.npz'), load_design(tmp_path / 'plain.npz')
    for k in PL.FIELDS:
        assert np.array_equal(getattr(back, k), getattr(e, k)) and getattr(plain, k, None) is None
    assert np.array_equal(back.mask_cols, e.mask_cols) and np.array_equal(plain.mask_cols, d.mask_cols)
    assert int(np.load(tmp_path / 'placed.npz')['version']) == 1
    assert set(np.load(tmp_path / 'placed.npz').files) - set(np.load(tmp_path / 'plain.npz').files) == set(PL.FIELDS)
    assert PL.has_placement(back) and not PL.has_placement(plain)


def test_placed_paths_batches_offsets_and_padding_on_the_host():
    a, b = C.placed(_design(3), seed=4, maxlen=5), C.placed(_design(4), seed=5, maxlen=9)
    node_off = np.array([0, a.N, a.N + b.N])
    pp = PL.PlacedPaths([a, b], node_off, 'cpu')
    assert pp.maxlen == 9 and pp.nodes.shape == (a.num_paths + b.num_paths, 9) and pp.nodes.dtype == torch.int32
    assert (pp.map_x, pp.map_y, pp.P, pp.B) == (16, 16, 256, 2) and pp.path_off.tolist() == [0, a.num_paths, a.num_paths + b.num_paths]
    na = pp.nodes[:a.num_paths].numpy()
    assert np.array_equal(na[:, :5], a.path_nodes) and (na[:, 5:] == -1).all()
    nb = pp.nodes[a.num_paths:].numpy()
    assert np.array_equal(nb, np.where(b.path_nodes >= 0, b.path_nodes + a.N, -1))
    assert np.array_equal(pp.lens.numpy(), np.concatenate([a.path_lens, b.path_lens]))
    assert np.array_equal(pp.loc_x.numpy(), np.concatenate([a.pin_x, b.pin_x])) and pp.loc_y.shape == (a.N + b.N,)
    # the batched tables rasterise to the designs' masks one after another
    ip, cols = PL.rasterize_host(pp.nodes.numpy(), pp.lens.numpy(), pp.loc_x.numpy(), pp.loc_y.numpy(), 16, 16)
    assert np.array_equal(cols, np.concatenate([a.mask_cols, b.mask_cols]))
    # set_pins: in place, one design's slice, validated first
    ptrs = (pp.loc_x.data_ptr(), pp.loc_y.data_ptr())
    x, y = C.move(b, seed=6, frac=0.3)
    before = pp.loc_x.clone(), pp.loc_y.clone()
    for bad in ((x[:-1], y), (x, y.astype(np.float32)), (x.astype(np.int16), y), (x.tolist(), y), (x, y.reshape(1, -1))):
        with pytest.raises((TypeError, ValueError)):
            pp.set_pins(1, *bad)
        assert torch.equal(pp.loc_x, before[0]) and torch.equal(pp.loc_y, before[1])
    with pytest.raises(IndexError):
        pp.set_pins(2, x, y)
    pp.set_pins(1, x, torch.from_numpy(y).to(torch.int32))
    assert ptrs == (pp.loc_x.data_ptr(), pp.loc_y.data_ptr())
    assert np.array_equal(pp.loc_x.numpy(), np.concatenate([a.pin_x, x])) and np.array_equal(pp.loc_y.numpy(), np.concatenate([a.pin_y, y]))
    with pytest.raises(ValueError, match='design 1'):
        PL.PlacedPaths([a, _design(4)], node_off, 'cpu')
    with pytest.raises(ValueError):
        PL.PlacedPaths([a, b], node_off[:-1], 'cpu')


def test_placed_paths_clips_a_truncated_row_to_its_own_designs_width():
    # design a is 5 nodes wide and holds a truncated row (length 40); b is 9 wide.  The device clips a length to the batch's
    # common maxlen, 9, only: unless PlacedPaths clips to a's own width first, columns 5..8 of that row - padding - count as nodes
    a, b = C.placed(_design(3), seed=4, maxlen=5), C.placed(_design(4), seed=5, maxlen=9)
    q = int(np.flatnonzero(a.path_lens == 5)[0])
    lens = a.path_lens.copy(); lens[q] = 40
    PL.attach_placement(a, a.path_nodes, lens, a.pin_x, a.pin_y)
    assert a.path_lens[q] == 40 and a.path_nodes.shape[1] == 5 and a.mask_indptr[q + 1] > a.mask_indptr[q]
    for designs in ([a, b], [b, a]):
        node_off = np.concatenate([[0], np.cumsum([d.N for d in designs])])
        pp = PL.PlacedPaths(designs, node_off, 'cpu')
        nodes, ln = pp.nodes.numpy(), pp.lens.numpy()
        assert pp.maxlen == 9 and ln.max() <= 9
        row = int(pp.path_off[designs.index(a)]) + q
        assert ln[row] == 5 and (nodes[row, :5] >= 0).all() and (nodes[row, 5:] == -1).all()
        # what the device takes for nodes - j < min(len, maxlen) - are pins of the row's own design, nothing else
        live = np.arange(9)[None, :] < np.minimum(ln, pp.maxlen)[:, None]
        lo, hi = np.repeat(node_off[:-1], [d.num_paths for d in designs]), np.repeat(node_off[1:], [d.num_paths for d in designs])
        assert ((nodes >= lo[:, None]) & (nodes < hi[:, None]))[live].all() and (nodes[~live] == -1).all()
        ip, cols = PL.rasterize_host(nodes, ln, pp.loc_x.numpy(), pp.loc_y.numpy(), 16, 16)
        assert np.array_equal(cols, np.concatenate([d.mask_cols for d in designs]))
        assert np.array_equal(np.diff(ip), np.concatenate([np.diff(d.mask_indptr) for d in designs]))
    # data set by hand, not through attach_placement, is checked as well: a padding entry inside a row's length
    c = copy.copy(a)
    c.path_nodes = a.path_nodes.copy(); c.path_nodes[q, 3] = -1
    with pytest.raises(ValueError, match='design 0'):
        PL.PlacedPaths([c, b], np.array([0, a.N, a.N + b.N]), 'cpu')


def test_pins_outside_32_bits_are_refused_before_anything_is_written():
    a = C.placed(_design(3), seed=4)
    pp = PL.PlacedPaths([a], np.array([0, a.N]), 'cpu')
    before = pp.loc_x.clone(), pp.loc_y.clone()
    x = a.pin_x.astype(np.int64)
    for bad in (2 ** 32 + 5, 2 ** 31, -2 ** 31 - 1):
        far = x.copy(); far[7] = bad
        for args in ((far, a.pin_y), (a.pin_x, torch.from_numpy(far))):
            with pytest.raises(ValueError, match='32-bit'):
                pp.set_pins(0, *args)
            assert torch.equal(pp.loc_x, before[0]) and torch.equal(pp.loc_y, before[1])
    far = x.copy(); far[7], far[8] = 2 ** 31 - 1, -2 ** 31                # the ends of the range are data: clamped to the map
    pp.set_pins(0, far, a.pin_y)
    assert pp.loc_x[7].item() == 2 ** 31 - 1 and pp.loc_x[8].item() == -2 ** 31 and pp.loc_x.dtype == torch.int32


def test_placed_fc_refuses_gradients_and_masks_without_a_run_form(monkeypatch):
    a = C.placed(_design(3), seed=4)
    pp = PL.PlacedPaths([a], np.array([0, a.N]), 'cpu')
    masks = fusion.PathMasks(a.mask_indptr, a.mask_cols, 256, 'cpu')
    paths = torch.arange(4, dtype=torch.int32)
    feat, w = torch.zeros(1, 256), torch.zeros(8, 256, requires_grad=True)
    with pytest.raises(RuntimeError, match='forward only'):
        PL.placed_fc(pp, paths, None, feat, w, None, masks)
    with torch.no_grad():
        monkeypatch.setattr(fusion, 'USE_RUNS', False)
        with pytest.raises(ValueError, match='no run form'):
            PL.placed_fc(pp, paths, None, feat, w, None, masks)
        monkeypatch.undo()
        with pytest.raises(ValueError):
            PL.placed_fc(pp, paths, None, feat, torch.zeros(6, 256), None, masks)
        with pytest.raises(ValueError):
            PL.placed_fc(pp, paths.long(), None, feat, w, None, masks)
