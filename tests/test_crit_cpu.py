"""Criticality per pin and per map cell, without a GPU: the ledger of include/mmft_crit.h (the rules test_report_cpu.py applies
to include/mmft_report.h), mmft.criticality's reference against a second, literal restatement of the header's words, a
mutation check - each clause, broken in the literal form, must be noticed by the inputs test_crit_gpu.py feeds to the kernel -
and the host-side validation of criticality() and of Predictor(criticality=...)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import crit_cases as C
import place_cases as PC
from abi_ledger import call_sites, code_only as _code_only, declared as _declared
from mmft import criticality as K
from mmft import lib
from mmft import placement as PL

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ['mmft_criticality', 'mmft_criticality_workspace_bytes']
F = np.float32


# ------------------------------------------------------------------------------------------------ the header's ledger
def test_crit_header_declares_two_symbols_and_the_other_headers_are_what_they_were():
    crt, inc, plc, ext, ref = (_declared(h) for h in ('mmft_crit.h', 'mmft_incr.h', 'mmft_place.h', 'mmft_report.h', 'mmft.h'))
    decls = lib.crit_decls()
    assert sorted(crt) == NAMES == sorted(decls)
    assert not set(crt) & (set(inc) | set(plc) | set(ext) | set(ref))
    assert sorted(inc) == sorted(lib.incr_decls()) == ['mmft_fanout_cone_step', 'mmft_mlp2_feat_fwd_bf16_masked', 'mmft_update_rows_diff']
    assert sorted(plc) == sorted(lib.place_decls()) == ['mmft_placed_fc_fwd']
    assert sorted(ext) == sorted(lib.ext_decls()) == ['mmft_timing_report', 'mmft_timing_report_workspace_bytes']
    assert lib.header_symbols() == sorted(ref) and set(lib.header_decls()) == set(ref)
    assert {n: len(decls[n][1]) for n in NAMES} == crt == {'mmft_criticality': 25, 'mmft_criticality_workspace_bytes': 3}
    res, args = decls['mmft_criticality']
    assert res is ctypes.c_int and args[-2:] == [ctypes.c_int, ctypes.c_void_p] and args[-3] is ctypes.c_longlong
    assert decls['mmft_criticality_workspace_bytes'] == (ctypes.c_longlong, [ctypes.c_int] * 3)
    with pytest.raises(RuntimeError, match='not declared'):
        lib.crit('mmft_version')
    # the accessor's name is its own: the other ledgers match call sites by attribute name
    assert lib.crit not in (lib.call, lib.query, lib.ext, lib.place, lib.incr)


def _args(**change):
    """A full argument list of mmft_criticality made of host integers: nothing can be launched on it, and nothing is - every
    refusal below comes before the device is looked at."""
    a = dict(pred=64, required=64, path_nodes=64, path_lens=64, maxlen=4, loc_x=64, loc_y=64, map_x=16, map_y=16, paths=64,
             row_design=None, T=5, N=10, B=1, node_slack=64, node_row=64, node_viol=64, node_crit=64, cell_slack=64, cell_viol=64,
             counts=64, workspace=64, workspace_bytes=1 << 20, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def test_the_built_library_exports_both_and_refuses_bad_arguments_on_the_host():
    L = lib.load()
    assert not [n for n in NAMES if not hasattr(L, n)]
    assert L.mmft_version() >= 205
    assert len(_args()) == 25
    refused = dict(null_pred=dict(pred=None), null_counts=dict(counts=None), null_paths=dict(paths=None), null_loc_with_cells=dict(loc_x=None),
                   T0=dict(T=0), T_above=dict(T=(1 << 24) + 1), N0=dict(N=0), B0=dict(B=0), maxlen0=dict(maxlen=0),
                   P96=dict(map_x=8, map_y=12), P_above=dict(map_x=512, map_y=256),
                   slack_without_viol=dict(cell_viol=None), viol_without_slack=dict(cell_slack=None),
                   null_workspace=dict(workspace=None), odd_workspace=dict(workspace=68), small_workspace=dict(workspace_bytes=8 * 10 + 8 + 4 * 256 - 1))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_criticality failed \(-1\): criticality'):
            lib.crit('mmft_criticality', *_args(**change))
    # the queries: sizes, and -1 outside the limits
    assert lib.crit('mmft_criticality_workspace_bytes', 10, 1, 256) == 8 * 10 + 8 + 4 * 256 == K.workspace_bytes(10, 1, 256)
    assert lib.crit('mmft_criticality_workspace_bytes', 10, 3, 0) == 8 * 10 + 16
    for bad in ((0, 1, 64), (10, 0, 64), (10, 1, 96), (10, 1, 65536 + 64), (10, 1, -64)):
        with pytest.raises(RuntimeError, match='criticality_workspace_bytes'):
            lib.crit('mmft_criticality_workspace_bytes', *bad)


def test_every_crit_call_site_matches_the_header_and_the_kernel_test_names_the_entry_point():
    protos = _declared('mmft_crit.h')
    checked, bad, seen = 0, [], set()
    for name, n, f, lineno in call_sites('crit'):
        if n is None or name == 'mmft_version':                        # (a list built elsewhere; the refusal test above)
            continue
        checked += 1
        seen.add(name)
        if protos.get(name) != n:
            bad.append((name, protos.get(name, 'not declared'), n, f, lineno))
    assert checked >= 4 and seen == set(NAMES) and not bad, bad
    src = open(os.path.join(HERE, 'test_crit_gpu.py')).read()
    assert 'pytestmark = pytest.mark.gpu' in src
    assert re.search(r'(?<![A-Za-z0-9_])mmft_criticality(?![A-Za-z0-9_])', _code_only(src))


# ------------------------------------------------------------------------------------------------ the rules, literally
def literal(b, cells=True, le_zero=False, tie_largest_row=False, nan_is_valid=False, negative_zero_violates=False,
            padding_counts=False, w_over_masked_rows=False):
    """include/mmft_crit.h word by word in plain Python, the masks cell by cell from place_cases.literal -> the seven arrays.
    Each flag breaks ONE clause."""
    masks = PC.literal(PC.CASES[b.name])[0] + [[]]                  # crit_cases appends an empty path
    P, inf = b.P, float('inf')
    best = [None] * b.N                                             # per pin (slack, tie-break, row)
    node_viol = [0] * b.N
    cell = [[inf] * P for _ in range(b.B)]
    cell_viol = [[0] * P for _ in range(b.B)]
    counts = [[0, 0] for _ in range(b.B)]
    worst = [inf] * b.B
    design = [0] * b.T if b.row_design is None else [int(x) for x in b.row_design]
    with np.errstate(invalid='ignore'):
        for t in range(b.T):
            s = F(F(b.required[t]) - F(b.pred[t]))
            if s == 0 and not negative_zero_violates:
                s = F(0.0)                                          # -0.0 becomes +0.0
            d, q = design[t], int(b.paths[t])
            if math.isnan(s):
                if not nan_is_valid:
                    counts[d][1] += 1
                    continue
                s = F(inf)
            counts[d][0] += 1
            viol = bool(s <= 0) if le_zero else bool(s < 0)
            if negative_zero_violates and np.signbit(s):
                viol = True
            row = [int(x) for x in b.nodes[q]]
            live = [x for x in row if x != -1] if padding_counts else row[:min(int(b.lens[q]), b.maxlen)]
            if not (w_over_masked_rows and not masks[q]):
                worst[d] = min(worst[d], float(s))
            for n in live:
                cand = (float(s), -t if tie_largest_row else t, t, s)
                if best[n] is None or cand[:2] < best[n][:2]:
                    best[n] = cand
                node_viol[n] += viol
            for c in masks[q] if cells else ():
                cell[d][c] = min(cell[d][c], float(s))
                cell_viol[d][c] += viol
    node_slack, node_row, node_crit = np.full(b.N, inf, dtype=F), np.full(b.N, -1, dtype=np.int32), np.zeros(b.N, dtype=F)
    for n, got in enumerate(best):
        if got is None:
            continue
        node_slack[n], node_row[n] = got[3], got[2]
        if got[0] < 0:
            w = F(worst[design[got[2]]])
            with np.errstate(invalid='ignore', divide='ignore'):
                node_crit[n] = F(1.0) if got[0] == float(w) else F(got[3]) / w
    return (node_slack, node_row, np.array(node_viol, dtype=np.int32), node_crit,
            np.array(cell, dtype=F).reshape(b.B, P) if cells else None, np.array(cell_viol, dtype=np.int32).reshape(b.B, P) if cells else None,
            np.array(counts, dtype=np.int32))


def test_the_patterns_hold_every_rule_they_claim():
    tags = set().union(*C.PATTERNS.values())
    assert {'equal_slack_shared_pin', 'nan_pred', 'plus_inf', 'minus_inf', 'required_equals_pred', 'tiny_negative',
            'design_without_violation', 'only_valid_row_has_an_empty_path', 'same_path_twice_different_slack'} <= tags
    assert set(C.NAMES) == set(PC.CASES) and {(PC.CASES[n].map_x, PC.CASES[n].map_y) for n in C.NAMES} >= {(8, 8), (128, 128), (32, 64)}
    assert PC.CASES['long_walk_16x16'].maxlen == 300
    for name in C.NAMES:
        b = C.batch(name, 'ties', 'three')
        assert b.B == 3 and set(b.row_design.tolist()) == {0, 2} and (np.diff(b.row_design) < 0).any()      # unsorted, design 1 empty
        assert b.lens[-1] == 0 and (b.paths[:b.T // 2] == b.paths[b.T // 2:]).all()
        s = K.reference_slack(b.pred, b.required)
        assert np.array_equal(s[:b.T // 2], s[b.T // 2:]) and (s < 0).any()
        b = C.batch(name, 'twice', 'one')
        s = K.reference_slack(b.pred, b.required)
        assert (s[:b.T // 2] != s[b.T // 2:]).all() and b.row_design is None
        b = C.batch(name, 'specials', 'three')
        s = K.reference_slack(b.pred, b.required)
        assert np.isnan(s).any() and (s == np.inf).any() and (s == -np.inf).any() and not np.signbit(s[s == 0]).any()
        if b.T // 2 >= len(C.SPECIALS):                                 # enough rows for every kind (the smallest case has three paths)
            with np.errstate(invalid='ignore'):
                raw = b.required - b.pred
            assert (s == -C.TINY).any() and np.signbit(raw)[s == 0].any() and (b.required == b.pred)[s == 0].any()
    assert sum(len(C.tables(n)[1]) >= len(C.SPECIALS) for n in C.NAMES) >= 3
    for name in C.NAMES:
        for layout in C.LAYOUTS:
            b = C.batch(name, 'nonneg_design', layout)
            d = np.zeros(b.T, dtype=int) if b.row_design is None else b.row_design
            assert (K.reference_slack(b.pred, b.required)[d == d.max()] >= 0).all()
            b = C.batch(name, 'lonely_empty', layout)
            s = K.reference_slack(b.pred, b.required)
            valid = np.flatnonzero(~np.isnan(s) & (d == d.max()))
            assert valid.tolist() == [b.T // 2 - 1] and b.lens[b.paths[valid[0]]] == 0 and s[valid[0]] == -2.0
            ref = C.reference(b)
            assert ref[6][d.max()].tolist() == [1, int((d == d.max()).sum()) - 1]


@pytest.mark.parametrize('name', C.NAMES)
def test_reference_criticality_equals_the_literal_restatement(name):
    for pattern in C.PATTERNS:
        for layout in C.LAYOUTS:
            b = C.batch(name, pattern, layout)
            ref = C.reference(b)
            assert [x.dtype for x in ref] == [np.float32, np.int32, np.int32, np.float32, np.float32, np.int32, np.int32]
            assert not C.differences(ref, literal(b)), (pattern, layout, C.differences(ref, literal(b)))
            assert ((ref[3] >= 0) & (ref[3] <= 1)).all() and (ref[3][ref[0] >= 0] == 0).all()
    b = C.batch(name, 'random', 'three')
    no_cells = C.reference(b, cells=False)
    assert no_cells[4] is None and no_cells[5] is None and not C.differences(no_cells, literal(b, cells=False))
    assert not C.differences(no_cells, C.reference(b), fields=('node_slack', 'node_row', 'node_viol', 'node_crit', 'counts'))
    # the masks may come from somebody else's rasteriser
    given = C.reference(b)
    from mmft.criticality import reference_criticality
    again = reference_criticality(b.pred, b.required, b.nodes, b.lens, None, None, b.map_x, b.map_y, b.paths, b.row_design, b.N, b.B,
                                  masks=PL.rasterize_host(b.nodes, b.lens, b.px, b.py, b.map_x, b.map_y))
    assert not C.differences(given, again)


@pytest.mark.parametrize('flag', ['le_zero', 'tie_largest_row', 'nan_is_valid', 'negative_zero_violates', 'padding_counts',
                                  'w_over_masked_rows'])
def test_the_cases_notice_each_broken_rule(flag):
    noticed = set()
    for name in [c.name for c in PC.HAND]:
        for pattern in C.PATTERNS:
            b = C.batch(name, pattern, 'three')
            if C.differences(C.reference(b), literal(b, **{flag: True})):
                noticed.add((name, pattern))
    expected = {'le_zero': {('edges_16x16', 'specials'), ('edges_16x16', 'nonneg_design')}, 'tie_largest_row': {('edges_16x16', 'ties')},
                'nan_is_valid': {('edges_16x16', 'specials'), ('edges_16x16', 'lonely_empty')},
                'negative_zero_violates': {('edges_16x16', 'specials')}, 'padding_counts': {('clamped_16x16', 'random')},
                'w_over_masked_rows': {('edges_16x16', 'worst_unmasked'), ('long_walk_16x16', 'worst_unmasked')}}[flag]
    assert expected <= noticed, (flag, sorted(noticed))


def test_a_division_that_is_not_exact_and_the_two_ends_of_the_scale():
    """One design, three paths through one pin each: w = -3, the others -1 and -inf-free; node_crit is the fp32 quotient."""
    nodes = np.array([[0, -1], [1, -1], [2, 3]])
    lens = np.array([1, 1, 2])
    z = np.zeros(4, dtype=np.int64)
    pred, required = np.array([3.0, 1.0, -1.0], dtype=F), np.zeros(3, dtype=F)
    out = K.reference_criticality(pred, required, nodes, lens, z, z, 8, 8, np.arange(3), None, 4, 1)
    assert out[0].tolist() == [-3.0, -1.0, 1.0, 1.0] and out[1].tolist() == [0, 1, 2, 2] and out[2].tolist() == [1, 1, 0, 0]
    assert out[3].tolist() == [1.0, float(F(-1.0) / F(-3.0)), 0.0, 0.0] and out[6].tolist() == [[3, 0]]
    assert out[4].shape == (1, 64) and out[4][0, 0] == 1.0 and np.isinf(out[4][0, 1:]).all() and not out[5].any()


# ------------------------------------------------------------------------------------------------ buffers, decoding
def test_crit_buffers_are_views_of_one_buffer_and_decode_splits_the_designs():
    bufs = K.CritBuffers(5, 2, 64, 'cpu')
    t = bufs.tensors()
    assert [tuple(x.shape) for x in t] == [(5,), (5,), (5,), (5,), (2, 64), (2, 64), (2, 2)]
    assert [x.dtype for x in t] == [torch.float32, torch.int32, torch.int32, torch.float32, torch.float32, torch.int32, torch.int32]
    lo, hi = bufs.raw.data_ptr(), bufs.raw.data_ptr() + 4 * bufs.raw.numel()
    assert all(lo <= x.data_ptr() < hi for x in t) and sum(x.numel() for x in t) == bufs.raw.numel()
    for i, x in enumerate(t):
        x.fill_(i + 1)
    h = bufs.host()
    assert all((a == i + 1).all() and a.shape == tuple(x.shape) for i, (a, x) in enumerate(zip(h, t)))
    d = K.decode(*h, node_off=[0, 2, 5], map_x=4, map_y=16)
    assert len(d) == 2 and d[0]['node_slack'].shape == (2,) and d[1]['node_crit'].shape == (3,) and d[1]['cell_viol'].shape == (4, 16)
    assert d[0]['n'] == 7 and d[0]['n_nan'] == 7 and sorted(d[0]) == sorted(K.FIELDS[:6] + ('n', 'n_nan'))
    plain = K.CritBuffers(5, 2, 64, 'cpu', cells=False)
    assert plain.tensors()[4] is None and plain.tensors()[5] is None and plain.raw.numel() == 4 * 5 + 4
    assert K.decode(*plain.host(), node_off=[0, 2, 5])[1]['cell_slack'] is None
    for bad in ((0, 1, 64), (5, 0, 64), (5, 1, 96), (5, 1, 65536 * 2)):
        with pytest.raises(ValueError):
            K.CritBuffers(*bad, 'cpu')


# ------------------------------------------------------------------------------------------------ host-side validation
def _placed_cpu():
    from mmft.synth import synth_design
    d = PC.placed(synth_design(N=512, L=8, tile=32, seed=3, end_frac=0.25), seed=4)
    return d, PL.PlacedPaths([d], np.array([0, d.N]), 'cpu')


def test_criticality_validates_on_the_host_before_anything_is_launched():
    d, pp = _placed_cpu()
    T = 6
    pred, required = torch.zeros(T), torch.ones(T)
    paths = torch.arange(T, dtype=torch.int32)
    good = dict(pred=pred, required=required, placed=pp, paths=paths, row_design=None, B=1)
    refusals = [(TypeError, dict(pred=pred.double())), (TypeError, dict(required=required.half())), (TypeError, dict(paths=paths.long())),
                (TypeError, dict(row_design=torch.zeros(T, dtype=torch.int64))), (TypeError, dict(pred=pred.numpy())),
                (ValueError, dict(pred=torch.zeros(2 * T)[::2])), (ValueError, dict(paths=torch.zeros(2 * T, dtype=torch.int32)[::2])),
                (ValueError, dict(required=torch.ones(T + 1))), (ValueError, dict(paths=paths[:-1].contiguous())),
                (ValueError, dict(row_design=torch.zeros(T - 1, dtype=torch.int32))), (ValueError, dict(pred=pred.reshape(2, 3))),
                (ValueError, dict(B=0)), (ValueError, dict(pred=torch.zeros(0), required=torch.zeros(0), paths=paths[:0]))]
    for exc, change in refusals:
        with pytest.raises(exc, match='criticality'):
            K.criticality(**{**good, **change})
    out = list(K.CritBuffers(d.N, 1, pp.P, 'cpu').tensors())
    for i, wrong in ((0, out[0].double()), (1, out[1][:-1]), (4, out[4].t()), (6, None)):
        bad = list(out)
        bad[i] = wrong
        with pytest.raises(ValueError, match='criticality'):
            K.criticality(**good, out=tuple(bad))
    with pytest.raises(ValueError, match='seven'):
        K.criticality(**good, out=tuple(out[:4]))
    # everything in order on the host: only then the device is looked at, and there is no CPU fallback
    with pytest.raises(RuntimeError, match='GPU only'):
        K.criticality(**good, out=tuple(out))
    with pytest.raises(RuntimeError, match='GPU only'):
        K.criticality(**good, cells=False)


def test_predictor_refuses_a_bad_criticality_option_before_it_touches_a_device():
    from mmft.infer import Predictor
    for bad in (dict(cell=True), dict(cells=True, k=3), 'yes', 3):
        with pytest.raises(ValueError, match='criticality='):
            Predictor(None, None, [], 'cpu', criticality=bad)
    assert Predictor._criticality_spec(None) is None and Predictor._criticality_spec(False) is None
    assert Predictor._criticality_spec(True) == {} and Predictor._criticality_spec(dict(cells=False)) == dict(cells=False)
