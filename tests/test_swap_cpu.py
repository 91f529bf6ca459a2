"""The swaps without a GPU: the ledger of include/mmft_swap.h (bound by mmft.swap.abi, outside the table of mmft.lib), the
host-side refusals of the built library, swapped_coords and pair_tables against literal loops, score_host against a literal
per-pair loop, the select table through commit.select_host, apply_host, and the host validation of swap_plan's arguments."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import place_cases as C
import swap_cases as WC
from abi_ledger import HEADERS, ROOT, code_only, declared
from mmft import commit as CM
from mmft import lib
from mmft import search as SE
from mmft import swap as SW
from mmft import trial as TR
from test_search_cpu import _abi_call_sites

NAMES = ['mmft_swap_apply', 'mmft_swap_rows', 'mmft_swap_score']
NARGS = {'mmft_swap_rows': 33, 'mmft_swap_score': 23, 'mmft_swap_apply': 14}
KERNEL_CASES = ['single_block_8x8', 'edges_16x16', 'clamped_16x16', 'wide_32x64', 'long_walk_16x16']
I64 = WC.I64


# ------------------------------------------------------------------------------------------------ the header's ledger
def test_swap_header_declares_exactly_its_names_and_overlaps_no_other_header():
    new, decls = declared('mmft_swap.h'), SW.abi.decls()
    assert sorted(new) == NAMES == sorted(decls) and new == NARGS
    assert {n: len(decls[n][1]) for n in NAMES} == NARGS
    for h in ['mmft.h', 'mmft_trial.h', 'mmft_search.h', 'mmft_commit.h', 'mmft_refine.h'] + list(HEADERS.values()):
        assert not set(new) & set(declared(h)), h
    for n in NAMES:
        res, args = decls[n]
        assert res is ctypes.c_int and args[-2:] == [ctypes.c_int, ctypes.c_void_p]    # `int device, void* stream` last
    for other in ('mmft_version', 'mmft_search_rows', 'mmft_commit_select'):
        with pytest.raises(RuntimeError, match='not declared'):
            SW.abi(other)
    for acc in [getattr(lib, a) for a in HEADERS] + [TR.abi, SE.abi, CM.abi]:
        for n in NAMES:
            with pytest.raises(RuntimeError, match='not declared'):
                acc(n)


def test_the_header_is_bound_by_the_module_and_lib_still_holds_its_nine():
    found = {k: v for k, v in vars(lib).items() if isinstance(v, lib.Header)}
    assert set(found) == set(HEADERS) and len(found) == 9
    assert isinstance(SW.abi, lib.Header) and all(SW.abi is not v for v in found.values()) and SW.abi not in (TR.abi, SE.abi, CM.abi)
    assert SW.abi.path.replace('\\', '/').endswith('include/mmft_swap.h') and SW.abi_decls == SW.abi.decls
    assert not hasattr(lib, 'swap') and not any('mmft_swap' in str(getattr(v, 'path', '')) for v in vars(lib).values())


def test_every_swap_call_site_has_the_headers_argument_count():
    seen, bad = set(), []
    for name, n, f, lineno in _abi_call_sites():
        if name not in NARGS or n is None:        # (a list built elsewhere: the refusal tests)
            continue
        seen.add((name, os.path.basename(f)))
        if NARGS[name] != n:
            bad.append((name, NARGS[name], n, f, lineno))
    assert not bad, bad
    assert {(n, 'swap.py') for n in NAMES} <= seen and {(n, 'test_swap_gpu.py') for n in NAMES} <= seen


def test_the_kernel_test_names_the_three_entry_points():
    src = open(os.path.join(ROOT, 'tests', 'test_swap_gpu.py')).read()
    assert 'pytestmark = pytest.mark.gpu' in src
    code = code_only(src)
    assert all(f"'{n}'" in code for n in NAMES)


# ------------------------------------------------------------------------------------------------ the built library
def _rows_args(**change):
    """A full argument list of mmft_swap_rows made of host integers: nothing can be launched on it, and nothing is - every
    refusal below comes before the device is looked at."""
    a = dict(path_nodes=64, path_lens=64, maxlen=4, loc_x=64, loc_y=64, map_x=16, map_y=16, paths=64, f_off=None, T=5,
             prow_row=64, prow_pair=64, RP=6, pair_a=64, pair_b=64, K=2, mv_ptr=64, mv_node=64, G=3, e0=0, e1=6, GP=64, bias=None,
             x=64, ldx=288, xt=64, ldxt=288, width=288, cnn_col=128, Dout=128, S=64, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def _score_args(**change):
    a = dict(pred_trial=64, pred_base=64, required=64, T=5, prow_ptr=64, prow_row=64, K=2, RP=6, k0=0, k1=2, scale_log2=20,
             dq=64, dviol=64, new_nan=64, capped=64, worst=64, worst_row=64, pick=64, base=64, design_rows=64, n=5, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def _apply_args(**change):
    a = dict(loc_x=64, loc_y=64, n_nodes=9, sel=64, pick=64, pair_a=64, pair_b=64, K=2, mv_ptr=64, mv_node=64, G=3, M=5, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def test_the_built_library_exports_the_three_and_refuses_bad_arguments_on_the_host():
    L = lib.load()
    assert not [n for n in NAMES if not hasattr(L, n)]
    assert len(_rows_args()) == 33 and len(_score_args()) == 23 and len(_apply_args()) == 14
    refused = dict(S=dict(S=32), P_not_64=dict(map_x=10, map_y=10), P_above=dict(map_x=512, map_y=256), Dout6=dict(Dout=6, width=300, ldx=300, ldxt=300),
                   Dout0=dict(Dout=0), maxlen0=dict(maxlen=0), T0=dict(T=0), G0=dict(G=0), K0=dict(K=0), RP_negative=dict(RP=-1, e0=0, e1=0),
                   cnn_col_odd=dict(cnn_col=126), ldx_odd=dict(ldx=290), ldxt_odd=dict(ldxt=290), width_above_ldx=dict(ldx=284),
                   width_above_ldxt=dict(ldxt=284), e0_negative=dict(e0=-1), e0_above_e1=dict(e0=5, e1=4), e1_above_RP=dict(e1=7),
                   null_nodes=dict(path_nodes=None), null_lens=dict(path_lens=None), null_loc_x=dict(loc_x=None), null_loc_y=dict(loc_y=None),
                   null_paths=dict(paths=None), null_prow_row=dict(prow_row=None), null_prow_pair=dict(prow_pair=None),
                   null_pair_a=dict(pair_a=None), null_pair_b=dict(pair_b=None), null_mv_ptr=dict(mv_ptr=None), null_mv_node=dict(mv_node=None),
                   null_GP=dict(GP=None), null_x=dict(x=None), null_xt=dict(xt=None), odd_GP=dict(GP=68), odd_x=dict(x=72), odd_xt=dict(xt=68),
                   odd_bias=dict(bias=72))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_swap_rows failed \(-1\): swap_rows'):
            SW.abi('mmft_swap_rows', *_rows_args(**change))
    # no entries in the call: fine once the sizes are in order, and no pointer is looked at
    nothing = dict(path_nodes=None, path_lens=None, loc_x=None, loc_y=None, paths=None, prow_row=None, prow_pair=None, pair_a=None,
                   pair_b=None, mv_ptr=None, mv_node=None, GP=None, x=None, xt=None)
    assert SW.abi('mmft_swap_rows', *_rows_args(**nothing, e0=3, e1=3)) == 0
    assert SW.abi('mmft_swap_rows', *_rows_args(**nothing, RP=0, e0=0, e1=0)) == 0
    with pytest.raises(RuntimeError, match=r'swap_rows'):
        SW.abi('mmft_swap_rows', *_rows_args(**nothing, e0=3, e1=3, S=32))
    refused = dict(T0=dict(T=0), T_above=dict(T=(1 << 24) + 1), K0=dict(K=0, k1=0), RP_negative=dict(RP=-1), k0_negative=dict(k0=-1),
                   empty=dict(k0=1, k1=1), k1_above_K=dict(k1=3), scale_negative=dict(scale_log2=-1), scale_above=dict(scale_log2=31),
                   null_pred_trial=dict(pred_trial=None), null_pred_base=dict(pred_base=None), null_required=dict(required=None),
                   null_prow_ptr=dict(prow_ptr=None), null_prow_row=dict(prow_row=None), null_dq=dict(dq=None), null_dviol=dict(dviol=None),
                   null_new_nan=dict(new_nan=None), null_capped=dict(capped=None), null_worst=dict(worst=None), null_worst_row=dict(worst_row=None),
                   null_pick=dict(pick=None), odd_dq=dict(dq=68), odd_base=dict(base=68), base_n0=dict(n=0), base_n_above=dict(n=(1 << 24) + 1),
                   base_null_rows=dict(design_rows=None))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_swap_score failed \(-1\): swap_score'):
            SW.abi('mmft_swap_score', *_score_args(**change))
    refused = dict(n0=dict(n_nodes=0), K0=dict(K=0), G0=dict(G=0), M_negative=dict(M=-1), null_loc_x=dict(loc_x=None), null_loc_y=dict(loc_y=None),
                   null_sel=dict(sel=None), null_pick=dict(pick=None), null_pair_a=dict(pair_a=None), null_pair_b=dict(pair_b=None),
                   null_mv_ptr=dict(mv_ptr=None), null_mv_node=dict(mv_node=None))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_swap_apply failed \(-1\): swap_apply'):
            SW.abi('mmft_swap_apply', *_apply_args(**change))
    assert SW.abi('mmft_swap_apply', *_apply_args(M=0, mv_node=None)) == 0           # no pin at all: nothing to write


# ------------------------------------------------------------------------------------------------ the rule and the tables
@pytest.mark.parametrize('name', KERNEL_CASES)
def test_swapped_coords_and_pair_tables_equal_literal_loops_on_the_kernel_cases(name):
    c = C.CASES[name]
    nodes, lens, px, py, far, mate, twin = WC.tables(c)
    groups = WC.groups(c)
    pair_a, pair_b, named = WC.pairs(c)
    tags = [g[0] for g in groups]
    sizes = {t: len(g) for t, g in groups}
    assert {'single', 'three_of_one_row', 'on_no_row', 'saturating', 'sixty_three', 'lone', 'thirty_two_a', 'thirty_two_b'} <= set(tags)
    assert (sizes['single'], sizes['sixty_three'], sizes['thirty_two_a'], sizes['thirty_two_b']) == (1, 63, 32, 32)
    assert (px[far], py[far]) == (WC.I32_MAX, WC.I32_MIN) and groups[tags.index('saturating')][1] == [far]
    assert (px[twin], py[twin]) == (px[mate], py[mate]) and twin != mate
    rng = np.random.default_rng(5)
    paths = np.concatenate([rng.permutation(nodes.shape[0]), rng.integers(0, nodes.shape[0], 3)])      # every path, some twice
    T = paths.shape[0]
    grow_ptr, grow_row, grow_grp, mv_ptr, mv_node = WC.plan(c, paths)
    assert grow_ptr[tags.index('on_no_row') + 1] == grow_ptr[tags.index('on_no_row')]       # a group on no row
    for a, b in zip(pair_a, pair_b):                                            # what a pair joins holds distinct pins
        assert not set(groups[a][1]) & set(groups[b][1])
    a, b = SW.check_pairs(mv_ptr, pair_a, pair_b)
    got = SW.swapped_coords(px, py, mv_ptr, mv_node, a, b)
    want = WC.swapped_literal(px, py, mv_ptr, mv_node, a, b)
    assert got[0].dtype == got[1].dtype == np.int64 and got[2].dtype == got[3].dtype == np.int32
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), (name, got, want)
    assert int(np.diff(got[0]).max()) == 64 == SW.MAX_PINS
    # the saturating pin paired with an ordinary one: the 64-bit difference exceeds int32, and the ordinary pin lands on the ends
    k = named.index(('saturating', 'single'))
    at = slice(int(got[0][k]), int(got[0][k + 1]))
    assert max(abs(int(px[mate]) - int(px[far])), abs(int(py[mate]) - int(py[far]))) > WC.I32_MAX and got[1][at].tolist() == [far, mate]
    assert (got[2][at].tolist(), got[3][at].tolist()) == ([int(px[mate]), WC.I32_MAX], [int(py[mate]), WC.I32_MIN])
    k = named.index(('single', 'twin'))                                         # anchors that coincide: the zero move
    at = slice(int(got[0][k]), int(got[0][k + 1]))
    assert got[2][at].tolist() == [int(px[mate])] * 2 and got[3][at].tolist() == [int(py[mate])] * 2
    tabs = SW.pair_tables(grow_ptr, grow_row, a, b, T)
    lit = WC.pair_tables_literal(grow_ptr, grow_row, a, b, T)
    assert all(g.dtype == np.int64 and np.array_equal(g, w) for g, w in zip(tabs, lit)), (name, tabs, lit)
    prow_ptr, prow_row, prow_pair, sel_ptr, sel_row = tabs
    k = named.index(('same_row_a', 'same_row_b'))                               # a row that holds pins of both groups: once
    ra, rb = (set(grow_row[grow_ptr[g]:grow_ptr[g + 1]].tolist()) for g in (a[k], b[k]))
    assert ra & rb and prow_ptr[k + 1] - prow_ptr[k] == len(ra | rb) < len(ra) + len(rb)
    assert np.array_equal(np.diff(sel_ptr), np.diff(prow_ptr) + 2) and sel_row.max() < T + len(groups)
    assert (np.diff(prow_ptr) == 0).any()                                       # a pair without entries


def test_pair_tables_on_hand_built_rows():
    grow_ptr, grow_row, pair_a, pair_b, pick, dq, T, min_q, want, n_cand = WC.select_case()
    prow_ptr, prow_row, prow_pair, sel_ptr, sel_row = SW.pair_tables(grow_ptr, grow_row, pair_a, pair_b, T)
    assert prow_ptr.tolist() == [0, 1, 2, 5, 8, 10, 12, 14] and prow_row.tolist() == [0, 1, 2, 3, 4, 3, 5, 6, 7, 8, 9, 10, 11, 12]
    assert prow_pair.tolist() == [0, 1, 2, 2, 2, 3, 3, 3, 4, 4, 5, 5, 6, 6]
    assert sel_row[:6].tolist() == [0, T + 0, T + 1, 1, T + 0, T + 2] and sel_ptr.tolist() == [0, 3, 6, 11, 16, 20, 24, 28]
    # the same pair twice and (a, b) beside (b, a): allowed, the same entries
    twice = SW.pair_tables(grow_ptr, grow_row, I64([3, 3, 4]), I64([4, 4, 3]), T)
    assert twice[0].tolist() == [0, 3, 6, 9] and twice[1].tolist() == [2, 3, 4] * 3
    assert all(np.array_equal(g, w) for g, w in zip(twice, WC.pair_tables_literal(grow_ptr, grow_row, [3, 3, 4], [4, 4, 3], T)))


# ------------------------------------------------------------------------------------------------ the scores
@pytest.mark.parametrize('name', list(WC.SCORE_CASES))
def test_score_host_equals_a_literal_per_pair_loop(name):
    pred_base, required, prow_ptr, prow_row, pred_trial, scale = WC.SCORE_CASES[name]()
    got = SW.score_host(pred_base, required, prow_ptr, prow_row, pred_trial, scale)
    want = WC.score_literal(pred_base, required, prow_ptr, prow_row, pred_trial, scale)
    WC.same_tables(got, want, name)
    K = len(prow_ptr) - 1
    assert all(got[k].shape == (K,) for k in SW.TABLES + ('pick', 'eligible', 'gain')) and got['dq'].dtype == np.int64
    assert got['pick'].dtype == np.int32 and np.array_equal(got['pick'], want['pick']) and np.array_equal(got['pick'] == 0, got['new_nan'] == 0)
    assert np.array_equal(got['gain'], -got['dq'] * 2.0 ** -scale) and not np.signbit(got['worst'][got['worst'] == 0]).any()
    if name == 'special_rows':                                                  # pair g * 9 + w of the window case: its edges, by name
        q1 = 2 ** scale
        assert got['new_nan'][0] == 1 and got['pick'][0] == -1 and got['pick'][1:].tolist() == [0] * (K - 1)      # a new NaN
        assert got['dq'][1] == 2 ** 32 - q1 and got['capped'][1] == 1 and got['worst'][1] == -np.inf            # slack -inf: the cap
        assert got['dq'][2] == -q1 and got['worst'][2] == 0.0 and got['worst_row'][2] == 2                     # slack +inf cures; rows 2, 3 tie at +0
        assert got['dq'][3] == 0 and got['worst'][3] == -1.0                                                    # -0.0 changes nothing
        assert not got['new_nan'][9:18].any() and np.isnan(got['worst'][9 + 4]) and got['worst_row'][9 + 4] == -1      # a NaN base row
        assert not got['dq'][18:27].any() and np.isnan(got['worst'][18:27]).all() and (got['worst_row'][18:27] == -1).all()      # no entries
        assert got['worst'][27 + 7] == -0.5 and got['worst_row'][27 + 7] == 0                                  # equal worst slack: the smallest row
        out = prow_row.copy()                                                   # rows outside pred take part in nothing
        out[[0, 5]] = [17, -1]
        WC.same_tables(SW.score_host(pred_base, required, prow_ptr, out, pred_trial, scale),
                       WC.score_literal(pred_base, required, prow_ptr, out, pred_trial, scale), 'rows outside')
    if name == 'special_cap':
        assert scale == 30 and got['capped'].tolist() == [2, 1, 1, 1, 1, 1, 1, 1, 1] and got['dq'][0] == 2 ** 32 - 2 ** 30
    if name == 'seeded':
        assert sorted(set(np.diff(prow_ptr).tolist())) == [0, 1, 257, 600] and (~got['eligible']).any() and got['capped'].any() and (got['dq'] < 0).any()


def test_best_pair_host_equals_a_literal_loop():
    _, _, pair_a, pair_b, pick, dq, _, _, _, _ = WC.select_case()
    got = SW.best_pair_host(dq, pick == 0, pair_a, pair_b, 13)
    want = WC.best_pair_literal(dq, pick == 0, pair_a, pair_b, 13)
    assert all(g.dtype == np.int64 and np.array_equal(g, w) for g, w in zip(got, want))
    assert got[0].tolist() == [1, 0, 1, 2, 2, 3, 3, 4, 4, -1, -1, 6, 6] and got[1][[0, 9]].tolist() == [-7, 0]       # group 0: pair 1 beats pair 0
    tie = SW.best_pair_host(I64([-4, -4, -9]), np.array([True, True, False]), I64([0, 0, 0]), I64([1, 2, 3]), 4)      # equal dq: the smaller k
    assert tie[0].tolist() == [0, 0, 1, -1] and tie[1].tolist() == [-4, -4, -4, 0]
    big = I64([-2 ** 61, 5, -2 ** 61, 2 ** 61])                                  # keys that do not fit one int64 together with k
    got = SW.best_pair_host(big, np.ones(4, dtype=bool), I64([0, 1, 0, 3]), I64([1, 2, 2, 2]), 4)
    assert all(np.array_equal(g, w) for g, w in zip(got, WC.best_pair_literal(big, np.ones(4, dtype=bool), [0, 1, 0, 3], [1, 2, 2, 2], 4)))
    assert got[0].tolist() == [0, 0, 2, 3] and got[1].tolist() == [-2 ** 61, -2 ** 61, -2 ** 61, 2 ** 61]
    rng = np.random.default_rng(9)
    for _ in range(20):
        K, G = int(rng.integers(1, 40)), int(rng.integers(2, 12))
        a = rng.integers(0, G, K)
        b = (a + rng.integers(1, G, K)) % G
        dq, ok = rng.integers(-5, 3, K), rng.random(K) < 0.7
        assert all(np.array_equal(g, w) for g, w in zip(SW.best_pair_host(dq, ok, a, b, G), WC.best_pair_literal(dq, ok, a, b, G)))


# ------------------------------------------------------------------------------------------------ selection and write
def test_the_select_table_makes_pairs_conflict_on_a_row_or_a_group():
    grow_ptr, grow_row, pair_a, pair_b, pick, dq, T, min_q, want, n_cand = WC.select_case()
    G = len(grow_ptr) - 1
    prow_ptr, prow_row, _, sel_ptr, sel_row = SW.pair_tables(grow_ptr, grow_row, pair_a, pair_b, T)
    sel, (n_sel, total, cands) = SW.select_host(pick, dq, sel_ptr, sel_row, T, G, min_q)
    assert sel.tolist() == want and (n_sel, total, cands) == (3, -19, n_cand)
    cand = (pick == 0) & (dq <= -min_q)
    by_row, by_group = WC.lost_how(sel, cand, prow_ptr, prow_row, pair_a, pair_b)
    assert by_row == [3] and by_group == [0]          # pair 3 loses on row 3; pair 0 on group 0 alone, which holds no row
    assert not set(prow_row[prow_ptr[0]:prow_ptr[1]].tolist()) & set(prow_row[prow_ptr[1]:prow_ptr[2]].tolist()) and grow_ptr[1] == grow_ptr[0]
    assert sel[4] == 1                                # disjoint from every other pair: taken beside them
    assert sel[5] == 0 and dq[5] == dq.min()          # ineligible: never selected, whatever its dq
    assert sel[6] == 0 and pick[6] == 0 and -min_q < dq[6] < 0      # does not reach the threshold
    # on the plan's rows alone - without the pseudo-rows - pairs 0 and 1 would both be taken: the table is what separates them
    rows_only, _ = CM.select_host(pick, dq, 1, prow_ptr, prow_row, T, min_q)
    assert rows_only.tolist() == [1, 1, 1, 0, 1, 0, 0]
    # the same pair twice, (a, b) beside (b, a): they conflict, the smaller k wins on equal dq
    t = SW.pair_tables(grow_ptr, grow_row, I64([7, 8, 7]), I64([8, 7, 8]), T)
    assert SW.select_host(np.zeros(3, dtype=np.int32), I64([-4, -4, -4]), t[3], t[4], T, G)[0].tolist() == [1, 0, 0]


def test_apply_host_equals_a_literal_loop():
    c = WC.apply_case()
    gx, gy = SW.apply_host(**c)
    lx, ly = WC.apply_literal(**c)
    assert gx.dtype == gy.dtype == np.int32 and gx.tolist() == lx and gy.tolist() == ly
    moved = sorted(set(np.flatnonzero((gx != c['loc_x']) | (gy != c['loc_y'])).tolist()))
    assert moved == [0, 1, 4, 5, 6, 13, 14, 15]       # pairs 0 and 3 alone; ids -1, 99 and 40 skipped
    assert (gx[1], gy[1]) == (WC.I32_MAX, WC.I32_MIN) and (gx[0], gy[0]) == (-3, 7)          # the anchors exchanged positions
    assert gx[4] == WC.I32_MIN and gy[4] == WC.I32_MAX                                        # the saturating pin's companion: clamped
    assert (gx[15], gy[15]) == (c['loc_x'][13], c['loc_y'][13]) and (gx[13], gy[13]) == (c['loc_x'][15], c['loc_y'][15])
    assert gx[14] - gx[13] == int(c['loc_x'][14]) - int(c['loc_x'][13])                        # a pin keeps its offset from its own anchor


# ------------------------------------------------------------------------------------------------ host validation
def _fake(T=20, groups=([0], [1, 2], [], [3], list(range(10, 42)), list(range(50, 82)), [4])):
    """A stand-in Predictor and a real SearchPlan on the CPU: swap_plan is host work.  Every non-empty group lies on one row of
    its own, in order; an empty one on none."""
    p = types.SimpleNamespace(_trial=object(), _sel=types.SimpleNamespace(paths=types.SimpleNamespace(numel=lambda: T)), device='cpu')
    has = np.array([len(g) > 0 for g in groups])
    tables = (I64(np.concatenate([[0], np.cumsum(has)])), I64(np.arange(has.sum())), I64(np.flatnonzero(has)),
              I64(np.concatenate([[0], np.cumsum([len(g) for g in groups])])), I64([v for g in groups for v in g]))
    return p, SE.SearchPlan(p, 0, tables, 'cpu')


def test_swap_plan_validates_its_arguments_on_the_host():
    p, plan = _fake()
    a, b = I64([0, 1]), I64([1, 3])
    sp = SW.swap_plan(p, plan, a, torch.from_numpy(b))
    assert isinstance(sp, SW.SwapPlan) and (sp.K, sp.RP, sp.G, sp.T) == (2, 4, 7, 20) and sp.owner is p and sp.plan is plan
    assert sp.ints.dtype == torch.int32 and sp.ints.numel() == 26 and len(sp.dev) == 7
    assert sp.prow_row.tolist() == [0, 1, 1, 2] and sp.sel_row.tolist() == [0, 1, 20, 21, 1, 2, 21, 23]
    assert SW.swap_plan(p, plan, I64([4]), I64([5])).K == 1                     # 32 + 32 pins: at the limit
    refusals = [
        (ValueError, 'with itself', dict(pair_a=I64([0, 1]), pair_b=I64([1, 1]))),                # a == b
        (ValueError, 'empty group', dict(pair_a=I64([0]), pair_b=I64([2]))),
        (ValueError, '33 \\+ 32 pins', dict(pair_a=I64([4]), pair_b=I64([5]), groups=([0], [1], [2], [3], list(range(10, 43)), list(range(50, 82))))),
        (IndexError, 'outside the plan', dict(pair_a=I64([0]), pair_b=I64([7]))),                 # an id equal to G
        (IndexError, 'outside the plan', dict(pair_a=I64([-1]), pair_b=I64([1]))),
        (ValueError, 'int64', dict(pair_a=a.astype(np.int32))), (ValueError, 'int64', dict(pair_b=[1, 3])),       # a wrong dtype, a list
        (ValueError, '1-D', dict(pair_a=a.reshape(1, 2))),
        (ValueError, 'same number', dict(pair_a=I64([0]))), (ValueError, 'at least one', dict(pair_a=I64([]), pair_b=I64([]))),
    ]
    for exc, match, change in refusals:
        q, pl = _fake(groups=change.pop('groups')) if 'groups' in change else (p, plan)
        with pytest.raises(exc, match=f'swap_plan: .*{match}'):
            SW.swap_plan(q, pl, **{**dict(pair_a=a, pair_b=b), **change})
    other, _ = _fake()
    with pytest.raises(ValueError, match='swap_plan: the plan belongs to another Predictor'):
        SW.swap_plan(other, plan, a, b)
    with pytest.raises(TypeError, match='swap_plan: plan must come from search_plan'):
        SW.swap_plan(p, dict(G=3), a, b)
    with pytest.raises(RuntimeError, match='swap_plan\\(\\): built without trials=True'):
        SW.swap_plan(types.SimpleNamespace(_trial=None), plan, a, b)
    q, shared = _fake(groups=([0, 1], [2], [1]))                                # pin 1 in two groups: commit.check_plan's verdict, cached
    for _ in range(2):
        with pytest.raises(ValueError, match='pin 1 of design 0 belongs to groups 0 and 2'):
            SW.swap_plan(q, shared, I64([0]), I64([1]))
    assert isinstance(shared.pins_distinct, str) and plan.pins_distinct is True
    big, bplan = _fake(T=(1 << 24) - 6)                                         # T + G one above 2^24
    with pytest.raises(ValueError, match='swap_plan: .*groups do not fit'):
        SW.swap_plan(big, bplan, a, b)
    # exactly 64 pins together is fine
    q, pl = _fake(groups=(list(range(32)), list(range(40, 72)), [90], list(range(100, 163))))
    assert SW.swap_plan(q, pl, I64([0, 3]), I64([1, 2])).K == 2


def test_predictor_methods_exist_and_refuse_without_trials_before_a_device_is_touched():
    from mmft.infer import Predictor
    assert callable(Predictor.swap_plan) and callable(Predictor.swap_moves) and callable(Predictor.commit_swaps)

    class NoTrials:
        _trial = None
    for call, name in ((SW.swap_moves, 'swap_moves'), (SW.commit_swaps, 'commit_swaps')):
        with pytest.raises(RuntimeError, match=f'{name}\\(\\): built without trials=True'):
            call(NoTrials(), None)
    assert SW.chunks([0, 3, 3, 10, 12, 12], 4) == [(0, 2), (2, 3), (3, 5)]      # cut at pair boundaries; a larger pair goes alone
    assert SW.chunks([0, 0, 0], 1) == [(0, 2)] and SW.chunks([0, 5, 6, 7], 2) == [(0, 1), (1, 3)] and SW.chunks([0, 2, 4], 65536) == [(0, 2)]
