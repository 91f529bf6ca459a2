"""Negative-slack sums and TNS shares per pin and per cell, without a GPU: the ledger of include/mmft_crit_sums.h (the rules
test_crit_cpu.py applies to include/mmft_crit.h), the host-side refusals of the built library, mmft.criticality's
reference_criticality_sums against a second, literal restatement of the header's words, a mutation check - each new clause,
broken in the literal form, must be noticed by the inputs test_crit_sums_gpu.py feeds to the kernels - what those inputs must
hold, and the host side: buffers, decoding, validation, the Predictor's option."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import crit_cases as C
import crit_sums_cases as S
import place_cases as PC
from abi_ledger import call_sites, code_only as _code_only, declared as _declared, others
from mmft import criticality as K
from mmft import lib
from test_crit_cpu import _placed_cpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ['mmft_criticality_sums', 'mmft_criticality_sums_workspace_bytes']
OTHER_HEADERS = others('mmft_crit_sums.h')
F = np.float32


# ------------------------------------------------------------------------------------------------ the header's ledger
def test_sums_header_declares_two_symbols_of_its_own():
    new, decls = _declared('mmft_crit_sums.h'), lib.csum_decls()
    assert sorted(new) == NAMES == sorted(decls)
    for h in OTHER_HEADERS:
        assert not set(new) & set(_declared(h)), h
    # the argument list of mmft_criticality, scale_log2 and six outputs, the workspace pair, `int device, void* stream` last
    assert {n: len(decls[n][1]) for n in NAMES} == new == {'mmft_criticality_sums': 32, 'mmft_criticality_sums_workspace_bytes': 3}
    res, args = decls['mmft_criticality_sums']
    old = lib.crit_decls()['mmft_criticality'][1]
    assert res is ctypes.c_int and args[:21] == old[:21] and args[21] is ctypes.c_int and args[22:28] == [ctypes.c_void_p] * 6
    assert args[28:] == old[21:] == [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p]
    assert decls['mmft_criticality_sums_workspace_bytes'] == (ctypes.c_longlong, [ctypes.c_int] * 3)
    with pytest.raises(RuntimeError, match='not declared'):
        lib.csum('mmft_version')
    with pytest.raises(RuntimeError, match='not declared'):
        lib.csum('mmft_criticality')
    # the accessor's name is its own: the other ledgers match call sites by attribute name
    assert lib.csum not in (lib.call, lib.query, lib.ext, lib.place, lib.incr, lib.crit, lib.head)


def _args(**change):
    """A full argument list of mmft_criticality_sums made of host integers: nothing can be launched on it, and nothing is -
    every refusal below comes before the device is looked at."""
    a = dict(pred=64, required=64, path_nodes=64, path_lens=64, maxlen=4, loc_x=64, loc_y=64, map_x=16, map_y=16, paths=64,
             row_design=None, T=5, N=10, B=1, node_slack=64, node_row=64, node_viol=64, node_crit=64, cell_slack=64, cell_viol=64,
             counts=64, scale_log2=20, node_nsum=64, cell_nsum=64, design_nsum=64, saturated=64, node_share=64, cell_share=64,
             workspace=64, workspace_bytes=1 << 20, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def test_the_built_library_exports_both_and_refuses_bad_arguments_on_the_host():
    L = lib.load()
    assert not [n for n in NAMES if not hasattr(L, n)]
    assert L.mmft_version() >= 207
    assert len(_args()) == 32
    need = 8 * 10 + 8 + 4 * 256
    no_cells = dict(cell_slack=None, cell_viol=None, cell_nsum=None, cell_share=None)
    refused = dict(null_node_nsum=dict(node_nsum=None), null_design_nsum=dict(design_nsum=None), null_saturated=dict(saturated=None),
                   null_node_share=dict(node_share=None), null_cell_nsum=dict(cell_nsum=None), null_cell_share=dict(cell_share=None),
                   scale_below=dict(scale_log2=-1), scale_above=dict(scale_log2=31),
                   rows_times_maxlen=dict(T=16519105, maxlen=65), rows_times_maxlen_far=dict(T=1 << 24, maxlen=1 << 10),
                   cell_sums_without_cells={**no_cells, 'cell_nsum': 64, 'cell_share': 64}, cell_nsum_without_cells={**no_cells, 'cell_nsum': 64},
                   cell_share_without_cells={**no_cells, 'cell_share': 64},
                   odd_node_nsum=dict(node_nsum=68), odd_design_nsum=dict(design_nsum=68), odd_cell_nsum=dict(cell_nsum=68),
                   small_workspace=dict(workspace_bytes=need - 1),
                   # ... and those of mmft_criticality still hold
                   null_pred=dict(pred=None), null_counts=dict(counts=None), T0=dict(T=0), P96=dict(map_x=8, map_y=12),
                   slack_without_viol=dict(cell_viol=None), null_workspace=dict(workspace=None), odd_workspace=dict(workspace=68))
    assert 16519105 * 65 == (1 << 30) + 1 and 16519105 <= 1 << 24          # T * maxlen = 2^30 + 1 with T inside its own limit
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_criticality_sums failed \(-1\): criticality_sums'):
            lib.csum('mmft_criticality_sums', *_args(**change))
    # ... and 2^30 exactly is not refused for its size: the next check, the workspace's, is the one that speaks
    with pytest.raises(RuntimeError, match='workspace'):
        lib.csum('mmft_criticality_sums', *_args(T=1 << 20, maxlen=1 << 10, workspace_bytes=need - 1))
    # the queries: sizes, and -1 outside the limits
    assert lib.csum('mmft_criticality_sums_workspace_bytes', 10, 1, 256) == need == K.sums_workspace_bytes(10, 1, 256)
    assert lib.csum('mmft_criticality_sums_workspace_bytes', 10, 3, 0) == 8 * 10 + 16
    for bad in ((0, 1, 64), (10, 0, 64), (10, 1, 96), (10, 1, 65536 + 64), (10, 1, -64)):
        with pytest.raises(RuntimeError, match='criticality_sums_workspace_bytes'):
            lib.csum('mmft_criticality_sums_workspace_bytes', *bad)


def test_every_csum_call_site_matches_the_header_and_the_kernel_test_names_the_entry_point():
    protos = _declared('mmft_crit_sums.h')
    checked, bad, seen = 0, [], set()
    for name, n, f, lineno in call_sites('csum'):
        if n is None or name in ('mmft_version', 'mmft_criticality'):  # (a list built elsewhere; the refusal test above)
            continue
        checked += 1
        seen.add(name)
        if protos.get(name) != n:
            bad.append((name, protos.get(name, 'not declared'), n, f, lineno))
    assert checked >= 4 and seen == set(NAMES) and not bad, bad
    src = open(os.path.join(HERE, 'test_crit_sums_gpu.py')).read()
    assert 'pytestmark = pytest.mark.gpu' in src
    assert re.search(r'(?<![A-Za-z0-9_])mmft_criticality_sums(?![A-Za-z0-9_])', _code_only(src))


# ------------------------------------------------------------------------------------------------ the rules, literally
@functools.lru_cache(maxsize=None)
def _boxes(name):
    """Per path of the batch's tables the list of its boxes, each the set of cells it covers (THE MASK RULE of mmft_place.h,
    box by box; their union is the path's mask)."""
    b = S.hand() if name == 'repeat_8x8' else C.batch(name, 'ties', 'one')
    out = []
    done = lambda: out if name == 'repeat_8x8' else _same_union(name, out)
    for q in range(b.nodes.shape[0]):
        row, boxes = [int(x) for x in b.nodes[q][:min(int(b.lens[q]), b.maxlen)]], []
        for u, v in zip(row, row[1:]):
            x1, x2 = max(min(b.px[u], b.px[v]), 0), min(max(b.px[u], b.px[v]), b.map_x - 1)
            y1, y2 = max(min(b.py[u], b.py[v]), 0), min(max(b.py[u], b.py[v]), b.map_y - 1)
            boxes.append({int(x * b.map_y + y) for x in range(x1, x2 + 1) for y in range(y1, y2 + 1)})
        out.append(boxes)
    return done()


def _same_union(name, boxes):
    """The union of a path's boxes is the mask place_cases spells out (crit_cases appends an empty path)."""
    assert [sorted(set().union(*bx)) if bx else [] for bx in boxes[:-1]] == PC.literal(PC.CASES[name])[0] and not boxes[-1]
    return boxes


def _rint(x, half_up=False):
    """A non-negative exact fraction (Python float holding an fp32 times a power of two) to the nearest integer, ties to even."""
    lo = math.floor(x)
    if x - lo != 0.5:
        return lo + (x - lo > 0.5)
    return lo + 1 if half_up or lo % 2 else lo


def literal(b, L, cells=True, wrong_cap=False, half_up=False, pin_once_per_row=False, cell_once_per_box=False,
            design_skips_empty_paths=False, share_divides_by_zero=False, saturated_above_cap_only=False):
    """include/mmft_crit_sums.h word by word in plain Python, in Python's integers -> the six new arrays (node_nsum, cell_nsum,
    design_nsum, saturated, node_share, cell_share).  Each flag breaks ONE clause."""
    boxes = _boxes(b.name)
    design = [0] * b.T if b.row_design is None else [int(x) for x in b.row_design]
    cap = 2.0 ** ((33 if wrong_cap else 32) - L)
    node, cell, total, sat = [0] * b.N, [[0] * b.P for _ in range(b.B)], [0] * b.B, [0] * b.B
    best = [None] * b.N                                             # (slack, row): the row node_row names
    with np.errstate(invalid='ignore'):
        for t in range(b.T):
            s = F(F(b.required[t]) - F(b.pred[t]))
            if math.isnan(s):
                continue
            s, d, q = float(s), design[t], int(b.paths[t])
            live = [int(x) for x in b.nodes[q][:min(int(b.lens[q]), b.maxlen)]]
            for n in live:
                if best[n] is None or (s, t) < best[n]:
                    best[n] = (s, t)
            if not s < 0:
                continue
            quanta = _rint(min(-s, cap) * 2.0 ** L, half_up) if -s != math.inf else int(cap * 2.0 ** L)
            if not (design_skips_empty_paths and not live):
                total[d] += quanta
                sat[d] += (-s > cap) if saturated_above_cap_only else (-s >= cap)
            for n in set(live) if pin_once_per_row else live:
                node[n] += quanta
            if cells:
                for c in [c for bx in boxes[q] for c in bx] if cell_once_per_box else set().union(*boxes[q]):
                    cell[d][c] += quanta

    def share(x, tot):
        if tot == 0:
            return F(np.float64(x) / np.float64(tot)) if share_divides_by_zero else F(0)
        return F(np.float64(x) / np.float64(tot))
    with np.errstate(invalid='ignore', divide='ignore'):
        node_share = [F(0) if best[n] is None else share(node[n], total[design[best[n][1]]]) for n in range(b.N)]
        cell_share = [[share(cell[d][c], total[d]) for c in range(b.P)] for d in range(b.B)] if cells else None
    return (np.array(node, dtype=np.int64), np.array(cell, dtype=np.int64).reshape(b.B, b.P) if cells else None,
            np.array(total, dtype=np.int64), np.array(sat, dtype=np.int32), np.array(node_share, dtype=F),
            np.array(cell_share, dtype=F).reshape(b.B, b.P) if cells else None)


def _new_differences(ref13, lit6):
    return S.differences((None,) * 7 + tuple(ref13[7:]), (None,) * 7 + tuple(lit6))


@pytest.mark.parametrize('name', C.NAMES + ('repeat_8x8',))
def test_reference_sums_equal_the_literal_restatement(name):
    batches = [S.hand()] if name == 'repeat_8x8' else [C.batch(name, p, l) for p in C.PATTERNS for l in C.LAYOUTS]
    for b in batches:
        for L in S.SCALES:
            ref = S.reference(b, L)
            assert [x.dtype for x in ref[7:]] == [np.int64, np.int64, np.int64, np.int32, np.float32, np.float32]
            assert [x.shape for x in ref[7:]] == [(b.N,), (b.B, b.P), (b.B,), (b.B,), (b.N,), (b.B, b.P)]
            assert not _new_differences(ref, literal(b, L)), (b.pattern, b.layout, L, _new_differences(ref, literal(b, L)))
            # the seven old outputs are reference_criticality's
            old = K.reference_criticality(b.pred, b.required, b.nodes, b.lens, b.px, b.py, b.map_x, b.map_y, b.paths, b.row_design, b.N, b.B)
            assert not C.differences(ref[:7], old)
            assert (ref[7] >= 0).all() and (ref[8] >= 0).all() and (ref[8] <= ref[9][:, None]).all() and (ref[12] <= 1).all()
    b = batches[-1]
    pins = S.reference(b, 20, cells=False)
    assert all(pins[i] is None for i in (4, 5, 8, 12)) and not _new_differences(pins, literal(b, 20, cells=False))
    assert not S.differences(pins, S.reference(b, 20), fields=('node_nsum', 'design_nsum', 'saturated', 'node_share'))


MUTATION_CASES = ('edges_16x16', 'clamped_16x16', 'single_block_8x8')


@pytest.mark.parametrize('flag', ['wrong_cap', 'half_up', 'pin_once_per_row', 'cell_once_per_box', 'design_skips_empty_paths',
                                  'share_divides_by_zero', 'saturated_above_cap_only'])
def test_the_cases_notice_each_broken_clause(flag):
    noticed = set()
    batches = [C.batch(name, pattern, 'three') for name in MUTATION_CASES for pattern in C.PATTERNS] + [S.hand()]
    for b in batches:
        for L in S.SCALES:
            if _new_differences(S.reference(b, L), literal(b, L, **{flag: True})):
                noticed.add((b.name, b.pattern, L))
    expected = {'wrong_cap': {('edges_16x16', 'specials', 20), ('repeat_8x8', 'hand', 20)},                   # -inf; -8192 beyond 2^12
                'half_up': {('repeat_8x8', 'hand', 20), ('edges_16x16', 'ties', 0)},                          # 0.5 and 2.5 quanta; -0.5 at scale 0
                'pin_once_per_row': {('repeat_8x8', 'hand', 0)},
                'cell_once_per_box': {('repeat_8x8', 'hand', 0), ('edges_16x16', 'worst_unmasked', 20)},      # path 'overlap'
                'design_skips_empty_paths': {('edges_16x16', 'lonely_empty', 20), ('repeat_8x8', 'hand', 0)},
                'share_divides_by_zero': {('edges_16x16', 'nonneg_design', 20), ('repeat_8x8', 'hand', 20)},
                'saturated_above_cap_only': {('repeat_8x8', 'hand', 20), ('edges_16x16', 'worst_unmasked', 30)}}[flag]
    assert expected <= noticed, (flag, sorted(noticed))


def test_the_inputs_hold_what_the_kernels_must_be_shown():
    """Asserted on the reference, over the batches the GPU test runs (S.batches() at S.SCALES)."""
    seen = dict(pin_in_two_violating_rows=False, cell_in_two_violating_rows=False, design_with_sum_zero_and_rows=False, saturated_row=False,
                inexact_pin_share=False, row_on_the_cap=False, pin_repeated_in_a_row=False, zero_quanta_violation=False)
    for b in S.batches():
        if b.pattern not in ('random', 'specials', 'worst_unmasked', 'nonneg_design', 'hand') or b.layout == 'one' and b.pattern != 'nonneg_design':
            continue
        for L in S.SCALES:
            ref = S.reference(b, L)
            node_viol, cell_viol, counts = ref[2], ref[5], ref[6]
            node_nsum, cell_nsum, design_nsum, saturated, node_share = ref[7], ref[8], ref[9], ref[10], ref[11]
            seen['pin_in_two_violating_rows'] |= bool(((node_viol >= 2) & (node_nsum > 0)).any())
            seen['cell_in_two_violating_rows'] |= bool(((cell_viol >= 2) & (cell_nsum > 0)).any())
            seen['design_with_sum_zero_and_rows'] |= bool(((design_nsum == 0) & (counts[:, 0] > 0)).any())
            seen['saturated_row'] |= bool(saturated.any())
            hit = (node_nsum > 0) & (node_share > 0)
            d = np.zeros(b.T, dtype=np.int64) if b.row_design is None else b.row_design
            tot = design_nsum[d[np.maximum(ref[1], 0)]]
            seen['inexact_pin_share'] |= bool((node_share[hit].astype(np.float64) * tot[hit] != node_nsum[hit]).any())
            q, sat = K.reference_quanta(K.reference_slack(b.pred, b.required), L)
            seen['row_on_the_cap'] |= bool((sat & (-K.reference_slack(b.pred, b.required).astype(np.float64) == 2.0 ** (32 - L))).any())
            seen['zero_quanta_violation'] |= bool(((q == 0) & (K.reference_slack(b.pred, b.required) < 0)).any())
        live = [b.nodes[p][:min(int(b.lens[p]), b.maxlen)].tolist() for p in b.paths]
        seen['pin_repeated_in_a_row'] |= any(len(set(r)) < len(r) for r in live)
    assert all(seen.values()), seen


def test_half_quanta_round_to_even_and_the_cap_saturates():
    quantum = 2.0 ** -20
    q, sat = K.reference_quanta(np.array([-0.5 * quantum, -1.5 * quantum, -2.5 * quantum, 0.5 * quantum, 0.0, np.nan], dtype=F), 20)
    assert q.tolist() == [0, 2, 2, 0, 0, 0] and q.dtype == np.int64 and not sat.any()
    q, sat = K.reference_quanta(np.array([-4096.0, -np.inf, -4095.99951171875, -1e30, np.inf, -1e-45], dtype=F), 20)
    assert q.tolist() == [1 << 32, 1 << 32, (1 << 32) - 512, 1 << 32, 0, 0] and sat.tolist() == [True, True, False, True, False, False]
    for L in range(31):                                                 # 0 <= q <= 2^32 at every scale; the largest finite slack saturates
        q, sat = K.reference_quanta(np.array([-3.4028235e38, -2.0 ** (32 - L), -np.nextafter(F(2.0 ** (32 - L)), F(0)), -2.0 ** -L], dtype=F), L)
        assert q.tolist() == [1 << 32, 1 << 32, (1 << 32) - 256, 1] and sat.tolist() == [True, True, False, False], L
    # through the whole reference: the hand-built batch at scale 20, rows 1, 2, 3 on paths 0, 1 and 4
    ref = S.reference(S.hand(), 20)
    assert ref[7][0] == 2 * (int(0.75 * 2 ** 20) + 2) and ref[7][2] == 0 + 2 + (1 << 32) and ref[10].tolist() == [2, 0]


def test_many_saturated_rows_and_single_quanta_sum_exactly_where_fp32_would_not():
    """5000 saturated rows and 7 rows of one quantum through one pin: 5000 * 2^32 + 7, which no fp32 (and no fp64 sum of fp32
    terms accumulated in fp32) holds."""
    T = 5007
    slack = np.full(T, -np.inf, dtype=F)
    slack[::716] = F(-(2.0 ** -20))                                     # rows 0, 716, ..., 4296: seven of them
    assert (slack > -np.inf).sum() == 7
    nodes, lens = np.array([[0]], dtype=np.int64), np.array([1], dtype=np.int64)
    z = np.zeros(1, dtype=np.int64)
    ref = K.reference_criticality_sums(-slack, np.zeros(T, dtype=F), nodes, lens, z, z, 8, 8, np.zeros(T, dtype=np.int64), None, 1, 1,
                                       scale_log2=20, cells=False)
    exact = 5000 * (1 << 32) + 7
    assert int(ref[7][0]) == exact == int(ref[9][0]) and ref[10].tolist() == [5000] and ref[11][0] == 1.0 and ref[2][0] == T
    acc = F(0)
    for q in K.reference_quanta(slack, 20)[0]:
        acc = F(acc + F(q))
    assert int(acc) != exact and int(F(exact)) != exact


# ------------------------------------------------------------------------------------------------ buffers, decoding
def test_sums_buffers_are_views_of_one_buffer_with_aligned_int64_fields_and_decode_sums_splits_the_designs():
    for N in (5, 6):                                                    # an odd and an even number of 4-byte fields in front of nothing
        bufs = K.CritSumsBuffers(N, 3, 64, 'cpu')
        t = bufs.tensors()
        assert len(t) == 13 == len(K.FIELDS + K.SUM_FIELDS)
        assert [tuple(x.shape) for x in t] == [(N,)] * 4 + [(3, 64), (3, 64), (3, 2), (N,), (3, 64), (3,), (3,), (N,), (3, 64)]
        assert [x.dtype for x in t] == [torch.float32, torch.int32, torch.int32, torch.float32, torch.float32, torch.int32, torch.int32,
                                        torch.int64, torch.int64, torch.int64, torch.int32, torch.float32, torch.float32]
        lo, hi = bufs.raw.data_ptr(), bufs.raw.data_ptr() + 4 * bufs.raw.numel()
        assert all(lo <= x.data_ptr() and x.data_ptr() + x.numel() * x.element_size() <= hi for x in t)
        assert sum(x.numel() * x.element_size() for x in t) == 4 * bufs.raw.numel()
        spans = sorted((x.data_ptr(), x.data_ptr() + x.numel() * x.element_size()) for x in t)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))      # no two fields overlap
        assert lo % 8 == 0 and all(x.data_ptr() % 8 == 0 for x in t if x.dtype == torch.int64)
        for i, x in enumerate(t):
            x.fill_(i + 1)
        h = bufs.host()
        assert all((a == i + 1).all() and a.shape == tuple(x.shape) for i, (a, x) in enumerate(zip(h, t)))
        assert [a.dtype for a in h[7:]] == [np.int64, np.int64, np.int64, np.int32, np.float32, np.float32]
    h = [np.asarray(a) for a in K.CritSumsBuffers(5, 2, 64, 'cpu').host()]
    for i, a in enumerate(h):
        a[...] = i + 1
    d = K.decode_sums(*h, node_off=[0, 2, 5], scale_log2=3, map_x=4, map_y=16)
    assert len(d) == 2 and sorted(d[0]) == sorted(K.FIELDS[:6] + ('n', 'n_nan', 'node_tns', 'cell_tns', 'tns', 'node_share', 'cell_share', 'saturated'))
    assert d[0]['node_tns'].shape == (2,) and d[1]['node_tns'].shape == (3,) and d[1]['node_tns'].dtype == np.float64
    assert (d[1]['node_tns'] == -8.0 / 8).all() and d[1]['cell_tns'].shape == (4, 16) and (d[1]['cell_tns'] == -9.0 / 8).all()
    assert d[0]['tns'] == -10.0 / 8 and d[0]['saturated'] == 11 and (d[0]['node_share'] == 12).all() and d[1]['cell_share'].shape == (4, 16)
    assert d[1]['node_slack'].shape == (3,) and d[1]['cell_viol'].shape == (4, 16) and d[0]['n'] == 7
    zero = K.decode_sums(*[np.zeros_like(a) for a in h], node_off=[0, 2, 5], scale_log2=20, map_x=4, map_y=16)[0]
    assert zero['tns'] == 0.0 and not np.signbit(zero['node_tns']).any() and not np.signbit(zero['cell_tns']).any()
    plain = K.CritSumsBuffers(5, 2, 64, 'cpu', cells=False)
    assert [plain.tensors()[i] for i in (4, 5, 8, 12)] == [None] * 4 and plain.raw.numel() == 2 * 5 + 2 * 2 + 4 * 5 + 4 + 2 + 5
    got = K.decode_sums(*plain.host(), node_off=[0, 2, 5], scale_log2=20)[1]
    assert got['cell_tns'] is None and got['cell_share'] is None and got['cell_slack'] is None
    for bad in ((0, 1, 64), (5, 0, 64), (5, 1, 96), (5, 1, 65536 * 2)):
        with pytest.raises(ValueError):
            K.CritSumsBuffers(*bad, 'cpu')


# ------------------------------------------------------------------------------------------------ host-side validation
def test_criticality_sums_validates_on_the_host_before_anything_is_launched():
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
                (ValueError, dict(B=0)), (ValueError, dict(pred=torch.zeros(0), required=torch.zeros(0), paths=paths[:0])),
                (ValueError, dict(scale_log2=-1)), (ValueError, dict(scale_log2=31)), (ValueError, dict(scale_log2=20.0)),
                (ValueError, dict(scale_log2=True)), (ValueError, dict(scale_log2=None))]
    for exc, change in refusals:
        with pytest.raises(exc, match='criticality_sums'):
            K.criticality_sums(**{**good, **change})
    out = list(K.CritSumsBuffers(d.N, 1, pp.P, 'cpu').tensors())
    for i, wrong in ((0, out[0].double()), (1, out[1][:-1]), (4, out[4].t()), (6, None), (7, out[7].to(torch.int32)), (8, out[8].t()),
                     (9, out[9].double()), (10, out[10].long()), (11, out[11][:-1]), (12, None)):
        bad = list(out)
        bad[i] = wrong
        with pytest.raises(ValueError, match='criticality_sums'):
            K.criticality_sums(**good, out=tuple(bad))
    with pytest.raises(ValueError, match='thirteen'):
        K.criticality_sums(**good, out=tuple(out[:7]))
    # everything in order on the host: only then the device is looked at, and there is no CPU fallback
    with pytest.raises(RuntimeError, match='GPU only'):
        K.criticality_sums(**good, out=tuple(out))
    with pytest.raises(RuntimeError, match='GPU only'):
        K.criticality_sums(**good, cells=False, scale_log2=0)


def test_the_row_limit_is_checked_on_the_host(monkeypatch):
    d, pp = _placed_cpu()
    monkeypatch.setattr(K, 'MAX_ROW_PINS', 6 * int(pp.maxlen) - 1)
    T = 6
    with pytest.raises(ValueError, match=r'criticality_sums: T \* maxlen'):
        K.criticality_sums(torch.zeros(T), torch.ones(T), pp, torch.arange(T, dtype=torch.int32), None, 1)
    monkeypatch.setattr(K, 'MAX_ROW_PINS', 6 * int(pp.maxlen))
    with pytest.raises(RuntimeError, match='GPU only'):
        K.criticality_sums(torch.zeros(T), torch.ones(T), pp, torch.arange(T, dtype=torch.int32), None, 1)
    assert K.MAX_ROW_PINS == 6 * int(pp.maxlen)
    monkeypatch.undo()
    assert K.MAX_ROW_PINS == 1 << 30


def test_predictor_refuses_a_bad_sums_option_before_it_touches_a_device():
    from mmft.infer import Predictor
    for bad in (dict(scale_log2=20), dict(sums=False, scale_log2=20), dict(sums=True, scale_log2=-1), dict(sums=True, scale_log2=31),
                dict(sums=True, scale_log2=20.0), dict(sums=True, scale_log2='20'), dict(sums=True, scale_log2=True),
                dict(sums=True, scale=20), dict(cells=True, sum=True), dict(cell=True)):
        with pytest.raises(ValueError, match='criticality='):
            Predictor(None, None, [], 'cpu', criticality=bad)
    spec = Predictor._criticality_spec
    assert spec(None) is None and spec(False) is None and spec(True) == {} and spec(dict(cells=False)) == dict(cells=False)
    assert spec(dict(sums=True)) == dict(sums=True) and spec(dict(cells=False, sums=True, scale_log2=0)) == dict(cells=False, sums=True, scale_log2=0)
    assert spec(dict(sums=True, scale_log2=30))['scale_log2'] == 30 and spec(dict(sums=False)) == dict(sums=False)
