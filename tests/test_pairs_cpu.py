"""The near pairs without a GPU: the ledger of include/mmft_pairs.h (bound by mmft.pairs.abi, outside the table of mmft.lib),
the host-side refusals of the built library, near_pairs_host against a literal double loop on the kernel cases of
swap_cases.py and on a seeded grid, and the host validation of near_swap_plan, refine_swaps and commit_swaps(patch=True)."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import pairs_cases as PC
from abi_ledger import HEADERS, ROOT, code_only, declared
from mmft import commit as CM
from mmft import lib
from mmft import pairs as PR
from mmft import refine as RF
from mmft import search as SE
from mmft import swap as SW
from mmft import trial as TR
from test_search_cpu import _abi_call_sites
from test_swap_cpu import _fake

NAMES = ['mmft_pairs_near_count', 'mmft_pairs_near_fill', 'mmft_pairs_rows_count', 'mmft_pairs_rows_fill', 'mmft_pairs_scan']
NARGS = {'mmft_pairs_near_count': 12, 'mmft_pairs_scan': 6, 'mmft_pairs_near_fill': 15, 'mmft_pairs_rows_count': 10, 'mmft_pairs_rows_fill': 16}
I64 = PC.I64
SEED = 0                                  # of pairs_cases.seeded: the one whose 257 groups show every exclusion below


# ------------------------------------------------------------------------------------------------ the header's ledger
def test_pairs_header_declares_exactly_its_names_and_overlaps_no_other_header():
    new, decls = declared('mmft_pairs.h'), PR.abi.decls()
    assert sorted(new) == NAMES == sorted(decls) and new == NARGS
    assert {n: len(decls[n][1]) for n in NAMES} == NARGS
    for h in ['mmft.h', 'mmft_trial.h', 'mmft_search.h', 'mmft_commit.h', 'mmft_refine.h', 'mmft_swap.h'] + list(HEADERS.values()):
        assert not set(new) & set(declared(h)), h
    for n in NAMES:
        res, args = decls[n]
        assert res is ctypes.c_int and args[-2:] == [ctypes.c_int, ctypes.c_void_p]    # `int device, void* stream` last
    for other in ('mmft_version', 'mmft_swap_rows', 'mmft_commit_select', 'mmft_refine_patch'):
        with pytest.raises(RuntimeError, match='not declared'):
            PR.abi(other)
    for acc in [getattr(lib, a) for a in HEADERS] + [TR.abi, SE.abi, CM.abi, RF.abi, SW.abi]:
        for n in NAMES:
            with pytest.raises(RuntimeError, match='not declared'):
                acc(n)


def test_the_header_is_bound_by_the_module_and_lib_still_holds_its_nine():
    found = {k: v for k, v in vars(lib).items() if isinstance(v, lib.Header)}
    assert set(found) == set(HEADERS) and len(found) == 9
    assert isinstance(PR.abi, lib.Header) and all(PR.abi is not v for v in found.values()) and PR.abi not in (TR.abi, SE.abi, CM.abi, RF.abi, SW.abi)
    assert PR.abi.path.replace('\\', '/').endswith('include/mmft_pairs.h') and PR.abi_decls == PR.abi.decls
    assert not hasattr(lib, 'pairs') and not any('mmft_pairs' in str(getattr(v, 'path', '')) for v in vars(lib).values())
    assert sorted(declared('mmft_swap.h')) == ['mmft_swap_apply', 'mmft_swap_rows', 'mmft_swap_score']      # the swaps keep their three


def test_every_pairs_call_site_has_the_headers_argument_count():
    seen, bad = set(), []
    for name, n, f, lineno in _abi_call_sites():
        if name not in NARGS or n is None:        # (a list built elsewhere: the refusal tests)
            continue
        seen.add((name, os.path.basename(f)))
        if NARGS[name] != n:
            bad.append((name, NARGS[name], n, f, lineno))
    assert not bad, bad
    assert {(n, 'pairs.py') for n in NAMES} <= seen and {(n, 'test_pairs_gpu.py') for n in NAMES} <= seen


def test_the_kernel_test_names_the_five_entry_points():
    src = open(os.path.join(ROOT, 'tests', 'test_pairs_gpu.py')).read()
    assert 'pytestmark = pytest.mark.gpu' in src
    code = code_only(src)
    assert all(f"'{n}'" in code for n in NAMES)


# ------------------------------------------------------------------------------------------------ the built library
def _args(base, change):
    assert not set(change) - set(base)
    return list({**base, **change}.values())


NEAR = dict(mv_ptr=64, mv_node=64, G=3, M=5, loc_x=64, loc_y=64, n_nodes=9, klass=None, reach=2)
COUNT = dict(NEAR, cnt=64, device=0, stream=None)
FILL = dict(NEAR, off=64, K=4, pair_a=64, pair_b=64, device=0, stream=None)
SCAN = dict(inp=64, n=5, out=256, total=64, device=0, stream=None)
RCOUNT = dict(pair_a=64, pair_b=64, K=2, grow_ptr=64, grow_row=64, G=3, R=6, cnt=64, device=0, stream=None)
RFILL = dict(pair_a=64, pair_b=64, prow_ptr=64, K=2, RP=6, grow_ptr=64, grow_row=64, G=3, R=6, T=5, prow_row=64, prow_pair=64, sel_ptr=64,
             sel_row=64, device=0, stream=None)


def test_the_built_library_exports_the_five_and_refuses_bad_arguments_on_the_host():
    """Every argument list below is made of host integers: nothing can be launched on it, and nothing is - each refusal comes
    before the device is looked at."""
    L = lib.load()
    assert not [n for n in NAMES if not hasattr(L, n)]
    assert [len(v) for v in (COUNT, SCAN, FILL, RCOUNT, RFILL)] == [12, 6, 15, 10, 16]
    near_bad = dict(G0=dict(G=0), G_above=dict(G=(1 << 24) + 1), M_negative=dict(M=-1), n0=dict(n_nodes=0), reach0=dict(reach=0),
                    reach_negative=dict(reach=-3), null_mv_ptr=dict(mv_ptr=None), null_mv_node=dict(mv_node=None), null_loc_x=dict(loc_x=None),
                    null_loc_y=dict(loc_y=None))
    for what, change in {**near_bad, 'null_cnt': dict(cnt=None)}.items():
        with pytest.raises(RuntimeError, match=r'mmft_pairs_near_count failed \(-1\): pairs_near_count'):
            PR.abi('mmft_pairs_near_count', *_args(COUNT, change))
    for what, change in {**near_bad, 'K_negative': dict(K=-1), 'null_off': dict(off=None), 'null_pair_a': dict(pair_a=None),
                         'null_pair_b': dict(pair_b=None)}.items():
        with pytest.raises(RuntimeError, match=r'mmft_pairs_near_fill failed \(-1\): pairs_near_fill'):
            PR.abi('mmft_pairs_near_fill', *_args(FILL, change))
    for what, change in dict(n_negative=dict(n=-1), null_in=dict(inp=None), null_out=dict(out=None), null_total=dict(total=None),
                             odd_total=dict(total=68), overlap=dict(out=72), overlap_behind=dict(inp=256, out=240)).items():
        with pytest.raises(RuntimeError, match=r'mmft_pairs_scan failed \(-1\): pairs_scan'):
            PR.abi('mmft_pairs_scan', *_args(SCAN, change))
    for what, change in dict(K_negative=dict(K=-1), G0=dict(G=0), R_negative=dict(R=-1), null_pair_a=dict(pair_a=None), null_pair_b=dict(pair_b=None),
                             null_grow_ptr=dict(grow_ptr=None), null_grow_row=dict(grow_row=None), null_cnt=dict(cnt=None)).items():
        with pytest.raises(RuntimeError, match=r'mmft_pairs_rows_count failed \(-1\): pairs_rows_count'):
            PR.abi('mmft_pairs_rows_count', *_args(RCOUNT, change))
    for what, change in dict(K_negative=dict(K=-1), RP_negative=dict(RP=-1), G0=dict(G=0), R_negative=dict(R=-1), T0=dict(T=0),
                             total_does_not_fit=dict(RP=2 ** 31 - 4, K=2), total_does_not_fit_K=dict(RP=0, K=2 ** 30),
                             rows_do_not_fit=dict(T=(1 << 24) - 2), null_pair_a=dict(pair_a=None), null_pair_b=dict(pair_b=None),
                             null_prow_ptr=dict(prow_ptr=None), null_grow_ptr=dict(grow_ptr=None), null_grow_row=dict(grow_row=None),
                             null_prow_row=dict(prow_row=None), null_prow_pair=dict(prow_pair=None), null_sel_ptr=dict(sel_ptr=None),
                             null_sel_row=dict(sel_row=None)).items():
        with pytest.raises(RuntimeError, match=r'mmft_pairs_rows_fill failed \(-1\): pairs_rows_fill'):
            PR.abi('mmft_pairs_rows_fill', *_args(RFILL, change))
    assert PR.abi('mmft_pairs_rows_fill', *_args(RFILL, dict(RP=2 ** 31 - 5, K=0))) == 0        # the largest total that fits, and no pair
    # the empty calls: fine once the sizes are in order, and no pointer is looked at
    none = dict(mv_ptr=None, mv_node=None, loc_x=None, loc_y=None, off=None, pair_a=None, pair_b=None)
    assert PR.abi('mmft_pairs_near_fill', *_args(FILL, dict(none, K=0))) == 0
    assert PR.abi('mmft_pairs_scan', *_args(SCAN, dict(inp=None, out=None, total=None, n=0))) == 0
    assert PR.abi('mmft_pairs_rows_count', *_args(RCOUNT, dict(pair_a=None, pair_b=None, grow_ptr=None, grow_row=None, cnt=None, K=0))) == 0
    assert PR.abi('mmft_pairs_rows_fill', *_args(RFILL, dict(pair_a=None, pair_b=None, prow_ptr=None, grow_ptr=None, grow_row=None, prow_row=None,
                                                             prow_pair=None, sel_ptr=None, sel_row=None, K=0, RP=0))) == 0
    with pytest.raises(RuntimeError, match='pairs_near_fill'):                  # ... but the sizes are looked at first
        PR.abi('mmft_pairs_near_fill', *_args(FILL, dict(none, K=0, reach=0)))
    with pytest.raises(RuntimeError, match='pairs_rows_count'):
        PR.abi('mmft_pairs_rows_count', *_args(RCOUNT, dict(K=0, G=0)))


# ------------------------------------------------------------------------------------------------ the rule
def _same_pairs(case, reach, klass):
    a, b, no = PC.near_literal(case['mv_ptr'], case['mv_node'], case['px'], case['py'], reach, klass)
    ha, hb = PR.near_pairs_host(case['mv_ptr'], case['mv_node'], case['px'], case['py'], reach, klass)
    assert ha.dtype == hb.dtype == np.int64 and np.array_equal(ha, a) and np.array_equal(hb, b), (reach, ha, a, hb, b)
    assert (ha < hb).all() and (np.diff(ha * (len(case['mv_ptr']) - 1) + hb) > 0).all()          # ascending (a, b), each once
    return a, b, no


@pytest.mark.parametrize('name', PC.KERNEL_CASES)
def test_near_pairs_host_equals_a_literal_double_loop_on_the_kernel_cases(name):
    c = PC.kernel_case(name)
    tags, px, py, far = c['tags'], c['px'], c['py'], c['far']
    size = dict(zip(tags, np.diff(c['mv_ptr']).tolist()))
    assert (size['single'], size['sixty_three'], size['lone'], size['thirty_two_a'], size['thirty_two_b']) == (1, 63, 1, 32, 32)
    assert (px[far], py[far]) == (PC.I32_MAX, PC.I32_MIN) and (px[c['twin']], py[c['twin']]) == (px[c['mate']], py[c['mate']])
    g_on_no_row = tags.index('on_no_row')
    assert c['grow_ptr'][g_on_no_row + 1] == c['grow_ptr'][g_on_no_row]            # a group on no row
    for reach in (1, 2, 40, PC.MAX_REACH):
        for klass in (None, np.arange(len(tags)) % 2):
            _same_pairs(c, reach, klass)
    a, b, no = _same_pairs(c, PC.MAX_REACH, None)
    pairs = set(zip(a.tolist(), b.tolist()))
    t = tags.index
    key = lambda u, v: (min(t(u), t(v)), max(t(u), t(v)))
    assert no[key('single', 'twin')] == {'coincide'}                              # anchors that coincide: the zero move, no pair
    assert key('sixty_three', 'lone') in pairs and key('thirty_two_a', 'thirty_two_b') in pairs      # 63 + 1 and 32 + 32: at the limit
    # the saturating pin at (INT32_MAX, INT32_MIN): its partners are those whose true distance - Python integers - stays
    # within 2^31 - 1, while a difference formed in 32 bits would wrap and pair it with singles that lie farther away
    sat = t('saturating')
    singles = [g for g in range(len(tags)) if size[tags[g]] == 1 and g != sat]
    anchor = lambda g: int(c['mv_node'][c['mv_ptr'][g]])
    wrap = lambda v: (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31
    true = {g for g in singles
            if max(abs(int(px[anchor(g)]) - PC.I32_MAX), abs(int(py[anchor(g)]) - PC.I32_MIN)) <= PC.MAX_REACH}
    assert {g for g in singles if (min(g, sat), max(g, sat)) in pairs} == true
    assert any(1 <= max(abs(wrap(int(px[anchor(g)]) - PC.I32_MAX)), abs(wrap(int(py[anchor(g)]) - PC.I32_MIN))) <= PC.MAX_REACH
               for g in singles if g not in true)
    for g in singles:                                                             # every other single does pair with something
        assert any(g in p for p in pairs), tags[g]
    if name in ('single_block_8x8', 'wide_32x64', 'long_walk_16x16'):             # every pin of these lies at y >= 0: 2^31 and more away
        assert not true and not any(sat in p for p in pairs)
    else:                                                                         # the idle pin at y == -1 lies exactly 2^31 - 1 away
        assert true == {g_on_no_row} and int(py[anchor(g_on_no_row)]) == -1


def test_near_pairs_host_equals_a_literal_double_loop_on_a_seeded_grid():
    c = PC.seeded(SEED)
    G = len(c['mv_ptr']) - 1
    size = np.diff(c['mv_ptr'])
    assert G == 257 and set(size.tolist()) == set(PC.SIZES) and set(c['klass'].tolist()) == set(PC.CLASSES)
    anchors = c['mv_node'][c['mv_ptr'][:-1][size > 0]]
    assert ((c['px'][anchors] >= 0) & (c['px'][anchors] < PC.GRID) & (c['py'][anchors] >= 0) & (c['py'][anchors] < PC.GRID)).all()
    for reach in (1, 2):
        a, b, no = _same_pairs(c, reach, c['klass'])
        alone = {w: [p for p, why in no.items() if why == {w}] for w in ('size', 'class', 'coincide', 'empty')}
        assert any(size[u] == 40 and size[v] == 40 for u, v in alone['size'])      # excluded by size alone: 40 + 40
        assert alone['class'] and alone['coincide'] and alone['empty']             # by class alone, by coinciding anchors alone, by an empty group
        paired = set(a.tolist()) | set(b.tolist())
        assert [g for g in range(G) if size[g] > 0 and g not in paired]            # a non-empty group without a partner
        assert len(a) > 0
        one_class = _same_pairs(c, reach, None)[0]
        assert len(one_class) > len(a)                                            # the class table does exclude pairs
    tabs, words = PC.expected(c, a, b)
    assert words.dtype == np.int32 and words.shape[0] == 6 * len(a) + 2 + 3 * tabs[3].shape[0]
    assert (np.diff(tabs[2]) == 0).any() and int(np.diff(tabs[2]).max()) >= 8      # pairs on no row, and pairs of many


# ------------------------------------------------------------------------------------------------ host validation
def test_near_swap_plan_and_refine_swaps_validate_on_the_host():
    from mmft.infer import Predictor
    assert callable(Predictor.near_swap_plan) and callable(Predictor.refine_swaps)

    class NoTrials:
        _trial = None
    for call, name in ((PR.near_swap_plan, 'near_swap_plan'), (PR.refine_swaps, 'refine_swaps')):
        with pytest.raises(RuntimeError, match=f'{name}\\(\\): built without trials=True'):
            call(NoTrials(), None, 1)
    p, plan = _fake()
    G = plan.G
    for who, call in (('near_swap_plan', PR.near_swap_plan), ('refine_swaps', PR.refine_swaps)):
        for reach in (0, -1, 2 ** 31, 1.0, True, None, '2'):
            with pytest.raises(ValueError, match=f'{who}: reach must be an integer in'):
                call(p, plan, reach)
        other, _ = _fake()
        with pytest.raises(ValueError, match=f'{who}: the plan belongs to another Predictor'):
            call(other, plan, 1)
        with pytest.raises(TypeError, match=f'{who}: plan must come from search_plan'):
            call(p, dict(G=3), 1)
        q, shared = _fake(groups=([0, 1], [2], [1]))
        with pytest.raises(ValueError, match='pin 1 of design 0 belongs to groups 0 and 2'):
            call(q, shared, 1)
        big, bplan = _fake(T=(1 << 24) - 6)
        with pytest.raises(ValueError, match=f'{who}: .*groups do not fit'):
            call(big, bplan, 1)
    for bad, match in ((np.zeros(G), 'integers'), ([0] * G, 'integers'), (np.zeros(G + 1, dtype=np.int64), 'one class per group'),
                       (np.zeros((G, 1), dtype=np.int32), 'one class per group'), (torch.zeros(G), 'integers'),
                       (np.full(G, 2 ** 31, dtype=np.int64), 'fit int32')):
        with pytest.raises(ValueError, match=f'near_swap_plan: group_class .*{match}'):
            PR.near_swap_plan(p, plan, 1, bad)
    assert PR.check_class(torch.arange(G), G).dtype == np.int32 and PR.check_class(None, G) is None
    assert PR.check_reach(np.int64(2 ** 31 - 1)) == 2 ** 31 - 1
    for max_pairs in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='near_swap_plan: max_pairs'):
            PR.near_swap_plan(p, plan, 1, None, max_pairs)
    for passes in (0, -1, 1.5, True):                                             # as refine_moves validates it
        with pytest.raises(ValueError, match='refine_swaps: passes must be an integer of at least 1'):
            PR.refine_swaps(p, plan, 1, passes=passes)
    with pytest.raises(ValueError, match='refine_swaps: every pass applies'):
        PR.refine_swaps(p, plan, 1, apply=False)


def test_commit_swaps_refuses_a_patch_without_apply_before_anything_else():
    with pytest.raises(ValueError, match='commit_swaps: patch=True .*needs apply=True'):
        SW.commit_swaps(types.SimpleNamespace(_trial=None), None, apply=False, patch=True)


def test_a_plan_decoded_from_device_words_is_an_ordinary_swap_plan():
    """SwapPlan.from_device on the words of a host-built plan (the CPU stands in for the device): the same tables, dtypes and
    views as swap_plan's."""
    p, plan = _fake()
    want = SW.swap_plan(p, plan, I64([0, 1, 4]), I64([1, 3, 5]))
    got = SW.SwapPlan.from_device(p, plan, want.ints.clone(), want.K, want.RP, want.T)
    assert (got.K, got.RP, got.G, got.T, got.i) == (want.K, want.RP, want.G, want.T, want.i) and got.owner is p and got.plan is plan
    for name in ('pair_a', 'pair_b', 'prow_ptr', 'prow_row', 'prow_pair', 'sel_ptr', 'sel_row'):
        assert getattr(got, name).dtype == np.int64 and np.array_equal(getattr(got, name), getattr(want, name)), name
    assert len(got.dev) == 7 and all(torch.equal(g, w) for g, w in zip(got.dev, want.dev))
