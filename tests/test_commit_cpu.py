"""The commit of best moves without a GPU: the ledger of include/mmft_commit.h (bound by mmft.commit.abi, outside the table of
mmft.lib), the host-side refusals of the built library, select_host and apply_host against literal loops on the hand-built
cases of commit_cases.py, check_plan, min_quanta, and the Predictor's methods."""
import ctypes
import os
import types

import numpy as np
import pytest

import commit_cases as CC
from abi_ledger import HEADERS, ROOT, code_only, declared
from mmft import commit as CM
from mmft import lib
from mmft import search as SE
from mmft import trial as TR
from test_search_cpu import _abi_call_sites

NAMES = ['mmft_commit_apply', 'mmft_commit_select']
NARGS = {'mmft_commit_select': 14, 'mmft_commit_apply': 12}


# ------------------------------------------------------------------------------------------------ the header's ledger
def test_commit_header_declares_exactly_its_names_and_overlaps_no_other_header():
    new, decls = declared('mmft_commit.h'), CM.abi.decls()
    assert sorted(new) == NAMES == sorted(decls) and new == NARGS
    assert {n: len(decls[n][1]) for n in NAMES} == NARGS
    for h in ['mmft.h', 'mmft_trial.h', 'mmft_search.h'] + list(HEADERS.values()):
        assert not set(new) & set(declared(h)), h
    for n in NAMES:
        res, args = decls[n]
        assert res is ctypes.c_int and args[-2:] == [ctypes.c_int, ctypes.c_void_p]    # `int device, void* stream` last
    assert decls['mmft_commit_select'][1][8] is ctypes.c_longlong                      # min_q
    for foreign in ('mmft_version', 'mmft_search_best', 'mmft_trial_rows'):
        with pytest.raises(RuntimeError, match='not declared'):
            CM.abi(foreign)
    for acc in list(HEADERS) + ['trial', 'search']:
        for n in NAMES:
            with pytest.raises(RuntimeError, match='not declared'):
                {'trial': TR.abi, 'search': SE.abi}.get(acc, getattr(lib, acc, None))(n)


def test_the_header_is_bound_by_the_module_and_absent_from_lib():
    found = {k: v for k, v in vars(lib).items() if isinstance(v, lib.Header)}
    assert set(found) == set(HEADERS)
    assert isinstance(CM.abi, lib.Header) and all(CM.abi is not v for v in found.values()) and CM.abi is not TR.abi and CM.abi is not SE.abi
    assert CM.abi.path.replace('\\', '/').endswith('include/mmft_commit.h') and CM.abi_decls == CM.abi.decls
    assert not hasattr(lib, 'commit') and not any('mmft_commit' in str(getattr(v, 'path', '')) for v in vars(lib).values())


def test_every_commit_call_site_has_the_headers_argument_count():
    seen, bad = set(), []
    for name, n, f, lineno in _abi_call_sites():
        if name not in NARGS or n is None:        # (a list built elsewhere: the refusal tests)
            continue
        seen.add((name, os.path.basename(f)))
        if NARGS[name] != n:
            bad.append((name, NARGS[name], n, f, lineno))
    assert not bad, bad
    assert {(n, 'commit.py') for n in NAMES} <= seen


# ------------------------------------------------------------------------------------------------ the built library
def _select_args(**change):
    """A full argument list of mmft_commit_select made of host integers: nothing can be launched on it, and nothing is - every
    refusal below comes before the device is looked at."""
    a = dict(best_w=64, best_dq=64, G=2, radius=1, grow_ptr=64, grow_row=64, R=3, T=5, min_q=1, sel=64, stats=64, owner=64,
             device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def _apply_args(**change):
    a = dict(loc_x=64, loc_y=64, n_nodes=9, sel=64, best_w=64, radius=1, mv_ptr=64, mv_node=64, G=2, M=3, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def test_the_built_library_exports_the_two_and_refuses_bad_arguments_on_the_host():
    L = lib.load()
    assert not [n for n in NAMES if not hasattr(L, n)]
    assert L.mmft_version() >= 213
    assert len(_select_args()) == 14 and len(_apply_args()) == 12
    refused = dict(G0=dict(G=0), G_negative=dict(G=-1), radius0=dict(radius=0), radius9=dict(radius=9), min_q0=dict(min_q=0),
                   min_q_negative=dict(min_q=-2 ** 40), R_negative=dict(R=-1), T0=dict(T=0), T_above=dict(T=(1 << 24) + 1),
                   null_best_w=dict(best_w=None), null_best_dq=dict(best_dq=None), null_grow_ptr=dict(grow_ptr=None),
                   null_grow_row=dict(grow_row=None), null_sel=dict(sel=None), null_stats=dict(stats=None), null_owner=dict(owner=None),
                   odd_best_dq=dict(best_dq=68), odd_stats=dict(stats=68), odd_owner=dict(owner=68))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_commit_select failed \(-1\): commit_select'):
            CM.abi('mmft_commit_select', *_select_args(**change))
    with pytest.raises(RuntimeError, match='commit_select: null pointer'):         # grow_row may be NULL only without entries
        CM.abi('mmft_commit_select', *_select_args(grow_row=None, R=1))
    refused = dict(n0=dict(n_nodes=0), G0=dict(G=0), M_negative=dict(M=-1), radius0=dict(radius=0), radius9=dict(radius=9),
                   null_loc_x=dict(loc_x=None), null_loc_y=dict(loc_y=None), null_sel=dict(sel=None), null_best_w=dict(best_w=None),
                   null_mv_ptr=dict(mv_ptr=None), null_mv_node=dict(mv_node=None))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_commit_apply failed \(-1\): commit_apply'):
            CM.abi('mmft_commit_apply', *_apply_args(**change))
    assert CM.abi('mmft_commit_apply', *_apply_args(mv_node=None, M=0)) == 0           # no pins: fine, and nothing is launched
    with pytest.raises(RuntimeError, match='commit_apply'):
        CM.abi('mmft_commit_apply', *_apply_args(mv_node=None, M=0, radius=0))
    assert CM.owner_bytes(5) == 60 and 'MMFT_COMMIT_OWNER_BYTES(T) (12ll' in open(CM.abi.path).read()


# ------------------------------------------------------------------------------------------------ select_host
@pytest.mark.parametrize('name', list(CC.SELECT_CASES))
def test_select_host_equals_the_literal_loop(name):
    c, (sel, n_sel, total, n_cand) = CC.select_case(name)
    got, stats = CM.select_host(**c)
    assert got.dtype == np.int32 and got.tolist() == sel and stats == (n_sel, total, n_cand), name
    assert all(isinstance(v, int) for v in stats)
    G = len(sel)
    if name == 'chain_up':
        assert sel == [1, 0] * 32 and n_cand == 64
    if name == 'chain_down':
        assert sel == [0, 1] * 32 and n_cand == 64
    if name == 'clique':
        assert n_sel == 1 and n_cand == 40 and sel[int(np.argmin(c['best_dq']))] == 1
    if name == 'ties':
        assert sel == [1, 0, 0, 0, 0, 0] + [1, 0, 1, 0, 1, 0, 1] + [1, 0]
    if name == 'thresholds':                     # -1, the centre, 0 and -min_q + 1 are no candidates; -min_q - 1 beats -min_q
        assert sel == [0, 0, 0, 0, 1, 1, 0, 1] and n_cand == 4 and total == -17
    if name == 'edges':                          # rows outside conflict with nothing; the non-candidate on rows 2, 3 blocks nobody
        assert sel == [1, 1, 1, 1, 0, 0] and n_cand == 5
    if name == 'big':
        b = 2 ** 56
        assert sel == [0, 1, 0, 0, 1, 0, 0] and total == -2 * b - 2 and n_cand == 5
    if name == 'seeded':
        assert G == 300 and c['T'] == 600 and len(c['grow_row']) > 4096 and 2 <= n_sel < n_cand < G
    if name == 'wide':
        assert G == 2500 and n_sel >= 100 and n_cand - n_sel >= 100


def test_select_host_refuses_a_bad_threshold_and_radius():
    c, _ = CC.select_case('ties')
    with pytest.raises(ValueError, match='min_q'):
        CM.select_host(**{**c, 'min_q': 0})
    with pytest.raises(ValueError, match='radius'):
        CM.select_host(**{**c, 'radius': 9})


# ------------------------------------------------------------------------------------------------ apply_host
@pytest.mark.parametrize('radius', [1, 2])
def test_apply_host_equals_the_literal_loop_and_saturates(radius):
    c = CC.apply_case(radius)
    before = (c['loc_x'].copy(), c['loc_y'].copy())
    x, y = CM.apply_host(**c)
    wx, wy = CC.apply_literal(**c)
    assert x.dtype == y.dtype == np.int32 and x.tolist() == wx and y.tolist() == wy
    assert np.array_equal(c['loc_x'], before[0]) and np.array_equal(c['loc_y'], before[1])        # copies: the inputs stay
    r = radius
    # group 0 moves by (+r, +r), group 1 by (-r, -r): the pins at the ends of int32 stay there
    assert (x[0], y[0]) == (CC.I32_MAX, CC.I32_MIN + r) and (x[2], y[2]) == (CC.I32_MIN + r, CC.I32_MAX)
    assert (x[1], y[1]) == (CC.I32_MAX - 1 - r, CC.I32_MIN) and (x[3], y[3]) == (CC.I32_MIN, CC.I32_MAX - 1 - r)
    moved = np.flatnonzero((x != before[0]) | (y != before[1])).tolist()
    # not selected (4 - 6), best_w outside the window (7; 8, 9), the centre (12) and the ids outside the arrays change nothing
    assert moved == [0, 1, 2, 3, 10, 11, 13, 14]


# ------------------------------------------------------------------------------------------------ check_plan, min_quanta
def _plan(groups, node_off=0, i=0):
    ptr = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    return types.SimpleNamespace(mv_ptr=ptr, mv_node=np.array([v + node_off for g in groups for v in g], dtype=np.int64), node_off=node_off,
                                 i=i, pins_distinct=None)


def test_check_plan_names_the_first_shared_pin_and_remembers_its_verdict():
    good = _plan([[3, 4], [5], [], [6, 7]])
    CM.check_plan(good)
    assert good.pins_distinct is True
    good.mv_node[:] = 3                                     # decided once: the remembered verdict holds
    CM.check_plan(good)
    bad = _plan([[3, 4], [9, 5], [4], [6, 9], [3]], node_off=100, i=1)
    with pytest.raises(ValueError, match='commit_moves: pin 3 of design 1 belongs to groups 0 and 4'):
        CM.check_plan(bad)
    assert isinstance(bad.pins_distinct, str)
    with pytest.raises(ValueError, match='pin 3 of design 1'):
        CM.check_plan(bad)
    with pytest.raises(ValueError, match='pin 4 of design 0 belongs to groups 1 and 2'):
        CM.check_plan(_plan([[3], [4], [4]]))
    # search_plan's own validation accepts a pin in two groups: only committing refuses
    pins, ptr = SE.check_groups(10, np.array([3, 4, 4], dtype=np.int64), np.array([0, 1, 2, 3], dtype=np.int64))
    assert pins.tolist() == [3, 4, 4] and ptr.tolist() == [0, 1, 2, 3]


def test_min_quanta_edges():
    assert CM.min_quanta(0.0) == 1 and CM.min_quanta(0) == 1 and CM.min_quanta(-0.0) == 1
    assert CM.min_quanta(2.0 ** -20) == 1 and CM.min_quanta(np.nextafter(2.0 ** -20, 1.0)) == 2 and CM.min_quanta(2.0 ** -21) == 1
    assert CM.min_quanta(1.0) == 2 ** 20 and CM.min_quanta(1.5, 0) == 2 and CM.min_quanta(3, 30) == 3 * 2 ** 30
    assert CM.min_quanta(np.float32(0.5), np.int64(4)) == 8 and CM.min_quanta(0.1, 20) == 104858
    assert CM.min_quanta(2.0 ** 41, 20) == 2 ** 61 and CM.min_quanta(np.nextafter(2.0 ** 42, 0.0), 20) < 2 ** 62
    for bad in (-1e-30, -1, float('nan'), float('inf'), -float('inf'), 2.0 ** 42, 1e300, None, '1', True):
        with pytest.raises(ValueError, match='commit_moves: min_gain'):
            CM.min_quanta(bad, 20)
    assert CM.min_quanta(2.0 ** 61, 0) == 2 ** 61
    with pytest.raises(ValueError, match='62 bits'):
        CM.min_quanta(2.0 ** 62, 0)


# ------------------------------------------------------------------------------------------------ the Predictor
def test_predictor_methods_exist_and_refuse_without_trials_before_a_device_is_touched():
    from mmft.infer import Predictor
    assert callable(Predictor.commit_moves) and callable(Predictor.refine_moves)

    class NoTrials:
        _trial = None
        commit_moves, refine_moves = Predictor.commit_moves, Predictor.refine_moves
    with pytest.raises(RuntimeError, match='commit_moves\\(\\): built without trials=True'):
        NoTrials().commit_moves(None)
    with pytest.raises(RuntimeError, match='commit_moves\\(\\): built without trials=True'):
        NoTrials().refine_moves(None)
    with pytest.raises(ValueError, match='refine_moves: passes'):
        NoTrials().refine_moves(None, passes=0)
    with pytest.raises(ValueError, match='refine_moves: every pass applies'):
        NoTrials().refine_moves(None, apply=False)
    # search_moves' own messages keep its name
    with pytest.raises(ValueError, match='search_moves: radius'):
        SE.check_call(10, radius=0)
    with pytest.raises(ValueError, match='commit_moves: radius'):
        SE.check_call(10, radius=0, who='commit_moves')


def test_the_kernel_test_names_the_two_entry_points():
    src = open(os.path.join(ROOT, 'tests', 'test_commit_gpu.py')).read()
    assert 'pytestmark = pytest.mark.gpu' in src
    code = code_only(src)
    assert all(f"'{n}'" in code for n in NAMES)
