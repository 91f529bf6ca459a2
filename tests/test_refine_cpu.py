"""The patch of the kept head rows without a GPU: the ledger of include/mmft_refine.h (bound by mmft.refine.abi, outside the table
of mmft.lib), the host-side refusals of the built library, patch_host and rows_host against literal loops on a hand-built case,
and the refusals of the Predictor's methods that come before a device is touched."""
import ctypes
import os

import numpy as np
import pytest

from abi_ledger import HEADERS, ROOT, code_only, declared
from mmft import commit as CM
from mmft import lib
from mmft import refine as RF
from mmft import search as SE
from mmft import trial as TR
from test_search_cpu import _abi_call_sites

NAMES = ['mmft_refine_patch', 'mmft_refine_rows']
NARGS = {'mmft_refine_rows': 31, 'mmft_refine_patch': 19}


# ------------------------------------------------------------------------------------------------ the header's ledger
def test_refine_header_declares_exactly_its_names_and_overlaps_no_other_header():
    new, decls = declared('mmft_refine.h'), RF.abi.decls()
    assert sorted(new) == NAMES == sorted(decls) and new == NARGS
    assert {n: len(decls[n][1]) for n in NAMES} == NARGS
    for h in ['mmft.h', 'mmft_trial.h', 'mmft_search.h', 'mmft_commit.h'] + list(HEADERS.values()):
        assert not set(new) & set(declared(h)), h
    for n in NAMES:
        res, args = decls[n]
        assert res is ctypes.c_int and args[-2:] == [ctypes.c_int, ctypes.c_void_p]    # `int device, void* stream` last
    assert [decls['mmft_refine_patch'][1][k] for k in (1, 5)] == [ctypes.c_longlong] * 2           # ldx, ldxt
    assert [decls['mmft_refine_rows'][1][k] for k in (22, 24)] == [ctypes.c_longlong] * 2
    for foreign in ('mmft_version', 'mmft_search_rows', 'mmft_commit_apply'):
        with pytest.raises(RuntimeError, match='not declared'):
            RF.abi(foreign)
    for acc in list(HEADERS) + ['trial', 'search', 'commit']:
        for n in NAMES:
            with pytest.raises(RuntimeError, match='not declared'):
                {'trial': TR.abi, 'search': SE.abi, 'commit': CM.abi}.get(acc, getattr(lib, acc, None))(n)


def test_the_header_is_bound_by_the_module_and_absent_from_lib():
    found = {k: v for k, v in vars(lib).items() if isinstance(v, lib.Header)}
    assert set(found) == set(HEADERS)
    assert isinstance(RF.abi, lib.Header) and all(RF.abi is not v for v in list(found.values()) + [TR.abi, SE.abi, CM.abi])
    assert RF.abi.path.replace('\\', '/').endswith('include/mmft_refine.h') and RF.abi_decls == RF.abi.decls
    assert not hasattr(lib, 'refine') and not any('mmft_refine' in str(getattr(v, 'path', '')) for v in vars(lib).values())


def test_every_refine_call_site_has_the_headers_argument_count():
    seen, bad = set(), []
    for name, n, f, lineno in _abi_call_sites():
        if name not in NARGS or n is None:        # (a list built elsewhere: the refusal tests)
            continue
        seen.add((name, os.path.basename(f)))
        if NARGS[name] != n:
            bad.append((name, NARGS[name], n, f, lineno))
    assert not bad, bad
    assert {(n, 'refine.py') for n in NAMES} <= seen


# ------------------------------------------------------------------------------------------------ the built library
def _rows_args(**change):
    """A full argument list of mmft_refine_rows made of host integers: nothing can be launched on it, and nothing is - every
    refusal below comes before the device is looked at."""
    a = dict(path_nodes=64, path_lens=64, maxlen=4, loc_x=64, loc_y=64, map_x=8, map_y=8, paths=64, f_off=None, T=5, grow_row=64,
             grow_grp=64, R=3, mv_ptr=64, mv_node=64, G=2, sel=64, best_w=64, radius=1, GP=64, bias=None, x=64, ldx=24, xt=64, ldxt=24,
             width=24, cnn_col=8, Dout=8, S=64, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def _patch_args(**change):
    a = dict(x=64, ldx=24, pred=64, T=5, xt=64, ldxt=24, pred_t=64, sel=64, best_w=64, radius=1, grow_row=64, grow_grp=64, R=3, G=2,
             cnn_col=8, Dout=8, stats=64, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def test_the_built_library_exports_the_two_and_refuses_bad_arguments_on_the_host():
    L = lib.load()
    assert not [n for n in NAMES if not hasattr(L, n)]
    assert L.mmft_version() >= 214
    assert len(_rows_args()) == 31 and len(_patch_args()) == 19
    refused = dict(radius0=dict(radius=0), radius9=dict(radius=9), R_negative=dict(R=-1), T0=dict(T=0), T_above=dict(T=(1 << 24) + 1),
                   G0=dict(G=0), S32=dict(S=32), map_odd=dict(map_x=3), Dout6=dict(Dout=6), Dout0=dict(Dout=0), cnn_col_odd=dict(cnn_col=6),
                   cnn_col_negative=dict(cnn_col=-4), narrow=dict(width=12), ldx_short=dict(ldx=20), ldxt_odd=dict(ldxt=26),
                   maxlen0=dict(maxlen=0), null_path_nodes=dict(path_nodes=None), null_loc_x=dict(loc_x=None), null_loc_y=dict(loc_y=None),
                   null_paths=dict(paths=None), null_grow_row=dict(grow_row=None), null_grow_grp=dict(grow_grp=None),
                   null_mv_ptr=dict(mv_ptr=None), null_mv_node=dict(mv_node=None), null_sel=dict(sel=None), null_best_w=dict(best_w=None),
                   null_GP=dict(GP=None), null_x=dict(x=None), null_xt=dict(xt=None), odd_x=dict(x=68), odd_xt=dict(xt=72), odd_GP=dict(GP=68),
                   odd_bias=dict(bias=68))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_refine_rows failed \(-1\): refine_rows'):
            RF.abi('mmft_refine_rows', *_rows_args(**change))
    assert RF.abi('mmft_refine_rows', *_rows_args(R=0, x=None, xt=None, sel=None)) == 0        # no entries: fine, no pointer is looked at
    with pytest.raises(RuntimeError, match='refine_rows: radius'):
        RF.abi('mmft_refine_rows', *_rows_args(R=0, radius=9))
    refused = dict(radius0=dict(radius=0), radius9=dict(radius=9), R_negative=dict(R=-1), T0=dict(T=0), T_negative=dict(T=-3),
                   T_above=dict(T=(1 << 24) + 1), G0=dict(G=0), Dout6=dict(Dout=6), Dout_above=dict(Dout=1028), cnn_col_odd=dict(cnn_col=2),
                   cnn_col_negative=dict(cnn_col=-4), ldx_short=dict(ldx=12), ldxt_short=dict(ldxt=12), ldx_odd=dict(ldx=22),
                   null_x=dict(x=None), null_pred=dict(pred=None), null_xt=dict(xt=None), null_pred_t=dict(pred_t=None),
                   null_sel=dict(sel=None), null_best_w=dict(best_w=None), null_grow_row=dict(grow_row=None),
                   null_grow_grp=dict(grow_grp=None), null_stats=dict(stats=None), odd_x=dict(x=72), odd_xt=dict(xt=68),
                   odd_stats=dict(stats=68))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_refine_patch failed \(-1\): refine_patch'):
            RF.abi('mmft_refine_patch', *_patch_args(**change))
    for null in ('x', 'pred', 'sel', 'best_w', 'stats'):                                   # R == 0 excuses the entries' pointers alone
        with pytest.raises(RuntimeError, match='refine_patch: null pointer'):
            RF.abi('mmft_refine_patch', *_patch_args(R=0, grow_row=None, grow_grp=None, xt=None, pred_t=None, **{null: None}))


# ------------------------------------------------------------------------------------------------ the restatements
def _hand_case():
    """Radius 1 (W = 9, centre 4), T = 6 rows of width 12 with h_cnn in columns [4, 8), five groups:
        0   selected, best_w 2       rows 0, 3
        1   not selected, best_w 5   rows 1, 3      (shares row 3 with group 0: it is not selected, so nothing of it is written)
        2   selected, best_w -1      row 2          (no eligible offset: not SELECTED in the header's sense)
        3   selected, best_w 8       rows 4, 6, -1  (rows 6 and -1 lie outside [0, T): skipped and counted)
        4   selected, best_w 9       row 5          (an offset outside the window)"""
    T, width, cnn_col, Dout = 6, 12, 4, 4
    grow_ptr = np.array([0, 2, 4, 5, 8, 9], dtype=np.int64)
    grow_row = np.array([0, 3, 1, 3, 2, 4, 6, -1, 5], dtype=np.int64)
    sel = np.array([1, 0, 1, 2, 1], dtype=np.int32)
    best_w = np.array([2, 5, -1, 8, 9], dtype=np.int64)
    rng = np.random.default_rng(17)
    x = rng.normal(size=(T, width)).astype(np.float32)
    pred = rng.normal(size=T).astype(np.float32)
    xt = rng.normal(size=(grow_row.shape[0], width)).astype(np.float32)
    pred_t = rng.normal(size=grow_row.shape[0]).astype(np.float32)
    return dict(x=x, pred=pred, xt=xt, pred_t=pred_t, sel=sel, best_w=best_w, radius=1, grow_ptr=grow_ptr, grow_row=grow_row,
                cnn_col=cnn_col, Dout=Dout)


def _patch_literal(x, pred, xt, pred_t, sel, best_w, radius, grow_ptr, grow_row, cnn_col, Dout):
    x, pred = x.copy(), pred.copy()
    W, patched, skipped = (2 * radius + 1) ** 2, 0, 0
    for g in range(len(sel)):
        if sel[g] == 0 or not 0 <= best_w[g] < W:
            continue
        for e in range(int(grow_ptr[g]), int(grow_ptr[g + 1])):
            r = int(grow_row[e])
            if not 0 <= r < len(pred):
                skipped += 1
                continue
            for c in range(cnn_col, cnn_col + Dout):
                x[r, c] = xt[e, c]
            pred[r] = pred_t[e]
            patched += 1
    return x, pred, (patched, skipped)


def test_patch_host_equals_the_literal_double_loop():
    c = _hand_case()
    before = (c['x'].copy(), c['pred'].copy())
    x, pred, counts = RF.patch_host(**c)
    wx, wpred, wcounts = _patch_literal(**c)
    assert x.dtype == pred.dtype == np.float32
    assert np.array_equal(x.view(np.uint32), wx.view(np.uint32)) and np.array_equal(pred.view(np.uint32), wpred.view(np.uint32))
    assert counts == wcounts == (3, 2) and all(isinstance(v, int) for v in counts)
    assert np.array_equal(c['x'], before[0]) and np.array_equal(c['pred'], before[1])              # copies: the inputs stay
    assert RF.selected_entries(c['sel'], c['best_w'], 1, c['grow_ptr']).tolist() == [True, True, False, False, False, True, True, True, False]
    # rows 0, 3 (group 0) and 4 (group 3) changed, in h_cnn and the prediction alone; rows 1, 2 and 5 are as they were
    changed = np.flatnonzero((x != before[0]).any(axis=1)).tolist()
    assert changed == [0, 3, 4] == np.flatnonzero(pred != before[1]).tolist()
    assert np.array_equal(x[:, :4], before[0][:, :4]) and np.array_equal(x[:, 8:], before[0][:, 8:])
    assert np.array_equal(x[3, 4:8], c['xt'][1, 4:8]) and pred[3] == c['pred_t'][1]                # entry 1, not entry 3 of group 1
    with pytest.raises(ValueError, match='radius'):
        RF.patch_host(**{**c, 'radius': 9})


def test_rows_host_takes_the_best_offset_of_the_selected_and_the_resident_row_of_the_others():
    c = _hand_case()
    R, width = c['grow_row'].shape[0], c['x'].shape[1]
    window = np.random.default_rng(18).normal(size=(9, R, width)).astype(np.float32)
    xt = RF.rows_host(c['x'], window, c['sel'], c['best_w'], 1, c['grow_ptr'], c['grow_row'])
    want = np.zeros((R, width), dtype=np.float32)
    for g in range(5):
        for e in range(int(c['grow_ptr'][g]), int(c['grow_ptr'][g + 1])):
            r = int(c['grow_row'][e])
            if not 0 <= r < 6:
                continue                                                                  # outside the tables: zeros
            want[e] = window[c['best_w'][g], e] if c['sel'][g] != 0 and 0 <= c['best_w'][g] < 9 else c['x'][r]
    assert xt.dtype == np.float32 and np.array_equal(xt.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(xt[0], window[2, 0]) and np.array_equal(xt[2], c['x'][1]) and np.array_equal(xt[4], c['x'][2])
    assert np.array_equal(xt[5], window[8, 5]) and not xt[6].any() and not xt[7].any() and np.array_equal(xt[8], c['x'][5])


# ------------------------------------------------------------------------------------------------ the Predictor
def test_predictor_methods_refuse_before_a_device_is_touched():
    import inspect

    from mmft.infer import Predictor
    assert inspect.signature(Predictor.commit_moves).parameters['patch'].default is False
    assert inspect.signature(Predictor.refine_moves).parameters['resident'].default is False

    class NoTrials:
        _trial = None
        commit_moves, refine_moves = Predictor.commit_moves, Predictor.refine_moves
    with pytest.raises(ValueError, match='commit_moves: patch=True .* needs apply=True'):
        NoTrials().commit_moves(None, patch=True, apply=False)
    with pytest.raises(ValueError, match='refine_moves: every pass applies'):
        NoTrials().refine_moves(None, resident=True, apply=False)
    with pytest.raises(ValueError, match='refine_moves: passes'):
        NoTrials().refine_moves(None, passes=0, resident=True)
    with pytest.raises(ValueError, match='refine_moves: resident=True patches every pass'):
        NoTrials().refine_moves(None, resident=True, patch=False)
    with pytest.raises(RuntimeError, match='commit_moves\\(\\): built without trials=True'):
        NoTrials().commit_moves(None, patch=True)
    with pytest.raises(RuntimeError, match='commit_moves\\(\\): built without trials=True'):
        NoTrials().refine_moves(None, resident=True)


def test_the_kernel_test_names_the_two_entry_points():
    src = open(os.path.join(ROOT, 'tests', 'test_refine_gpu.py')).read()
    assert 'pytestmark = pytest.mark.gpu' in src
    code = code_only(src)
    assert all(f"'{n}'" in code for n in NAMES)
