"""The window search without a GPU: the ledger of include/mmft_search.h (bound by mmft.search.abi, outside the table of
mmft.lib), the host-side refusals of the built library, the window's arithmetic, search_plan's tables against a literal loop,
score_host against a literal definition, and the host validation of search_plan's and search_moves' arguments."""
import ast
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import search_cases as SC
import trial_cases as TC
from abi_ledger import HEADERS, PKG, ROOT, code_only, declared
from mmft import lib
from mmft import search as SE
from mmft import trial as TR
from mmft.criticality import reference_quanta

NAMES = ['mmft_search_best', 'mmft_search_rows', 'mmft_search_score']
NARGS = {'mmft_search_rows': 31, 'mmft_search_score': 20, 'mmft_search_best': 15}
F = np.float32


# ------------------------------------------------------------------------------------------------ the header's ledger
def test_search_header_declares_exactly_its_names_and_overlaps_no_other_header():
    new, decls = declared('mmft_search.h'), SE.abi.decls()
    assert sorted(new) == NAMES == sorted(decls) and new == NARGS
    assert {n: len(decls[n][1]) for n in NAMES} == NARGS
    for h in ['mmft.h', 'mmft_trial.h'] + list(HEADERS.values()):
        assert not set(new) & set(declared(h)), h
    for n in NAMES:
        res, args = decls[n]
        assert res is ctypes.c_int and args[-2:] == [ctypes.c_int, ctypes.c_void_p]    # `int device, void* stream` last
    with pytest.raises(RuntimeError, match='not declared'):
        SE.abi('mmft_version')
    with pytest.raises(RuntimeError, match='not declared'):
        SE.abi('mmft_placed_fc_fwd')
    for acc in list(HEADERS) + ['trial']:
        for n in NAMES:
            with pytest.raises(RuntimeError, match='not declared'):
                (TR.abi if acc == 'trial' else getattr(lib, acc))(n)


def test_the_header_is_bound_by_the_module_and_absent_from_lib():
    found = {k: v for k, v in vars(lib).items() if isinstance(v, lib.Header)}
    assert set(found) == set(HEADERS)
    assert isinstance(SE.abi, lib.Header) and all(SE.abi is not v for v in found.values()) and SE.abi is not TR.abi
    assert SE.abi.path.replace('\\', '/').endswith('include/mmft_search.h') and SE.abi_decls == SE.abi.decls
    assert not hasattr(lib, 'search') and not any('mmft_search' in str(getattr(v, 'path', '')) for v in vars(lib).values())


def _abi_call_sites():
    """(name, nargs, file, lineno) of every `abi('mmft_...', ...)` / `something.abi('mmft_...', ...)` call under the package,
    tests/ and tools/; nargs as abi_ledger.call_sites counts them (a starred `stream_args(...)` as its two)."""
    files = glob.glob(os.path.join(PKG, '**', '*.py'), recursive=True)
    files += glob.glob(os.path.join(ROOT, 'tests', '*.py')) + glob.glob(os.path.join(ROOT, 'tools', '*.py'))
    for f in files:
        for node in ast.walk(ast.parse(open(f).read())):
            if not isinstance(node, ast.Call) or not node.args:
                continue
            fn, a0 = node.func, node.args[0]
            if not ((isinstance(fn, ast.Name) and fn.id == 'abi') or (isinstance(fn, ast.Attribute) and fn.attr == 'abi')):
                continue
            if not (isinstance(a0, ast.Constant) and isinstance(a0.value, str) and a0.value.startswith('mmft_')):
                continue
            n = 0
            for a in node.args[1:]:
                if not isinstance(a, ast.Starred):
                    n += 1
                elif isinstance(a.value, ast.Call) and getattr(a.value.func, 'attr', '') == 'stream_args':
                    n += 2
                else:
                    n = None
                    break
            yield a0.value, n, f, node.lineno


def test_every_search_call_site_has_the_headers_argument_count():
    seen, bad = set(), []
    for name, n, f, lineno in _abi_call_sites():
        if name not in NARGS or n is None:        # (a list built elsewhere: the refusal tests)
            continue
        seen.add((name, os.path.basename(f)))
        if NARGS[name] != n:
            bad.append((name, NARGS[name], n, f, lineno))
    assert not bad, bad
    assert {(n, 'search.py') for n in NAMES} <= seen


# ------------------------------------------------------------------------------------------------ the built library
def _rows_args(**change):
    """A full argument list of mmft_search_rows made of host integers: nothing can be launched on it, and nothing is - every
    refusal below comes before the device is looked at."""
    a = dict(path_nodes=64, path_lens=64, maxlen=4, loc_x=64, loc_y=64, map_x=16, map_y=16, paths=64, f_off=None, T=5,
             grow_row=64, grow_grp=64, R=3, mv_ptr=64, mv_node=64, G=2, radius=1, w0=0, w1=9, GP=64, bias=None,
             x=64, ldx=288, xt=64, ldxt=288, width=288, cnn_col=128, Dout=128, S=64, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def _score_args(**change):
    a = dict(pred_trial=64, pred_base=64, required=64, T=5, grow_ptr=64, grow_row=64, G=2, R=3, radius=1, w0=0, w1=9, scale_log2=20,
             dq=64, dviol=64, new_nan=64, capped=64, worst=64, worst_row=64, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def _best_args(**change):
    a = dict(dq=64, new_nan=64, G=2, radius=1, best_w=64, best_dq=64, pred_base=64, required=64, design_rows=64, n=5, T=5,
             scale_log2=20, base=64, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def test_the_built_library_exports_the_three_and_refuses_bad_arguments_on_the_host():
    L = lib.load()
    assert not [n for n in NAMES if not hasattr(L, n)]
    assert L.mmft_version() >= 212
    assert len(_rows_args()) == 31 and len(_score_args()) == 20 and len(_best_args()) == 15
    refused = dict(S=dict(S=32), P_not_64=dict(map_x=10, map_y=10), P_above=dict(map_x=512, map_y=256), map_x0=dict(map_x=0),
                   Dout6=dict(Dout=6, width=300, ldx=300, ldxt=300), Dout0=dict(Dout=0), Dout_above=dict(Dout=1028, width=1200, ldx=1200, ldxt=1200),
                   maxlen0=dict(maxlen=0), T0=dict(T=0), G0=dict(G=0), R_negative=dict(R=-1),
                   cnn_col_odd=dict(cnn_col=126), cnn_col_negative=dict(cnn_col=-4), ldx_odd=dict(ldx=290), ldxt_odd=dict(ldxt=290),
                   width_below=dict(width=252, ldx=252, ldxt=252), width_above_ldx=dict(ldx=284), width_above_ldxt=dict(ldxt=284),
                   radius0=dict(radius=0), radius9=dict(radius=9, w1=361), w0_negative=dict(w0=-1), w0_above_w1=dict(w0=5, w1=4),
                   w1_above_W=dict(w1=10), slots=dict(R=2 ** 31 - 1, radius=8, w1=289),
                   null_nodes=dict(path_nodes=None), null_lens=dict(path_lens=None), null_loc_x=dict(loc_x=None), null_loc_y=dict(loc_y=None),
                   null_paths=dict(paths=None), null_grow_row=dict(grow_row=None), null_grow_grp=dict(grow_grp=None),
                   null_mv_ptr=dict(mv_ptr=None), null_mv_node=dict(mv_node=None), null_GP=dict(GP=None), null_x=dict(x=None), null_xt=dict(xt=None),
                   odd_GP=dict(GP=68), odd_x=dict(x=72), odd_xt=dict(xt=68), odd_bias=dict(bias=72))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_search_rows failed \(-1\): search_rows'):
            SE.abi('mmft_search_rows', *_rows_args(**change))
    # no entries, or no offsets: fine once the sizes are in order, and no pointer is looked at
    nothing = dict(path_nodes=None, path_lens=None, loc_x=None, loc_y=None, paths=None, grow_row=None, grow_grp=None, mv_ptr=None,
                   mv_node=None, GP=None, x=None, xt=None)
    assert SE.abi('mmft_search_rows', *_rows_args(**nothing, R=0)) == 0
    assert SE.abi('mmft_search_rows', *_rows_args(**nothing, w0=3, w1=3)) == 0
    with pytest.raises(RuntimeError, match=r'search_rows'):
        SE.abi('mmft_search_rows', *_rows_args(**nothing, R=0, S=32))
    refused = dict(T0=dict(T=0), T_above=dict(T=(1 << 24) + 1), G0=dict(G=0), R_negative=dict(R=-1), radius0=dict(radius=0),
                   radius9=dict(radius=9), w0_negative=dict(w0=-1), empty=dict(w0=4, w1=4), w1_above_W=dict(w1=10),
                   slots=dict(R=2 ** 31 - 1, radius=8, w1=289), scale_negative=dict(scale_log2=-1), scale_above=dict(scale_log2=31),
                   null_pred_trial=dict(pred_trial=None), null_pred_base=dict(pred_base=None), null_required=dict(required=None),
                   null_grow_ptr=dict(grow_ptr=None), null_grow_row=dict(grow_row=None), null_dq=dict(dq=None), null_dviol=dict(dviol=None),
                   null_new_nan=dict(new_nan=None), null_capped=dict(capped=None), null_worst=dict(worst=None),
                   null_worst_row=dict(worst_row=None), odd_dq=dict(dq=68))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_search_score failed \(-1\): search_score'):
            SE.abi('mmft_search_score', *_score_args(**change))
    refused = dict(G0=dict(G=0), n0=dict(n=0), n_above=dict(n=(1 << 24) + 1), T0=dict(T=0), T_above=dict(T=(1 << 24) + 1),
                   radius0=dict(radius=0), radius9=dict(radius=9), scale_negative=dict(scale_log2=-1), scale_above=dict(scale_log2=31),
                   null_dq=dict(dq=None), null_new_nan=dict(new_nan=None), null_best_w=dict(best_w=None), null_best_dq=dict(best_dq=None),
                   null_pred_base=dict(pred_base=None), null_required=dict(required=None), null_rows=dict(design_rows=None),
                   null_base=dict(base=None), odd_dq=dict(dq=68), odd_best_dq=dict(best_dq=68), odd_base=dict(base=68))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_search_best failed \(-1\): search_best'):
            SE.abi('mmft_search_best', *_best_args(**change))


# ------------------------------------------------------------------------------------------------ the window
def test_offsets_the_centre_and_the_saturating_add():
    for r in range(1, 9):
        dx, dy = SE.offsets(r)
        W = (2 * r + 1) ** 2
        assert dx.dtype == dy.dtype == np.int32 and dx.shape == dy.shape == (W,)
        assert list(zip(dx.tolist(), dy.tolist())) == SC.window(r)
        c = SE.centre(r)
        assert c == 2 * r * (r + 1) and (dx[c], dy[c]) == (0, 0) and np.count_nonzero((dx == 0) & (dy == 0)) == 1
        assert dx.min() == dy.min() == -r and dx.max() == dy.max() == r
        assert (dx[0], dy[0]) == (-r, -r) and (dx[1], dy[1]) == (-r, -r + 1)         # y runs fastest: x is the first map axis
    for r in (0, 9, -1):
        with pytest.raises(ValueError, match='radius'):
            SE.offsets(r)
    loc = np.array([SC.I32_MAX, SC.I32_MAX - 1, SC.I32_MIN, SC.I32_MIN + 1, 0, 7], dtype=np.int32)
    assert SE.moved_coords(loc, 1).tolist() == [SC.I32_MAX, SC.I32_MAX, SC.I32_MIN + 1, SC.I32_MIN + 2, 1, 8]
    assert SE.moved_coords(loc, -1).tolist() == [SC.I32_MAX - 1, SC.I32_MAX - 2, SC.I32_MIN, SC.I32_MIN, -1, 6]
    assert SE.moved_coords(loc, 8).tolist()[:2] == [SC.I32_MAX] * 2 and SE.moved_coords(loc, -8).tolist()[2:4] == [SC.I32_MIN] * 2
    assert SE.moved_coords(loc, 1).dtype == np.int32
    assert SE.moved_coords(loc.astype(np.int64), np.array([1, 1, -1, -1, 0, 0])).tolist() == [SC.I32_MAX, SC.I32_MAX, SC.I32_MIN, SC.I32_MIN, 0, 7]
    assert [SC.sat32(int(v) + 1) for v in loc] == SE.moved_coords(loc, 1).tolist()


# ------------------------------------------------------------------------------------------------ the plan
def _plan_both(inc, i, pins, group_ptr):
    nodes, lens, paths, maxlen, node_off, n_nodes = inc
    table = TR.rows_of_pin(nodes, lens, paths, maxlen, n_nodes)
    pins, group_ptr = np.asarray(pins, dtype=np.int64), np.asarray(group_ptr, dtype=np.int64)
    got = SE.plan_tables(table, node_off[i], pins, group_ptr)
    want = SC.plan_literal(nodes, lens, paths, node_off[i], pins, group_ptr)
    assert len(got) == len(want) == 5 and all(g.dtype == np.int64 for g in got)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), (got, want)
    return got


def test_plan_tables_equal_a_literal_loop_on_hand_built_rows():
    inc = TC.hand_incidence()
    # design 0.  group 0: pin 0, twice in row 0 -> the row once.  1: pin 4, on no selected row.  2: pins 1 and 2 share rows 0, 1,
    # 2 and 5 -> each once.  3: empty.  4: pin 3 -> row 2 alone
    gptr, grow, ggrp, mptr, mnode = _plan_both(inc, 0, [0, 4, 1, 2, 3], [0, 1, 2, 4, 4, 5])
    assert gptr.tolist() == [0, 1, 1, 5, 5, 6] and grow.tolist() == [0, 0, 1, 2, 5, 2] and ggrp.tolist() == [0, 2, 2, 2, 2, 4]
    assert mptr.tolist() == [0, 1, 2, 4, 4, 5] and mnode.tolist() == [0, 4, 1, 2, 3]
    # design 1: the same ids mean other pins (offset 5)
    gptr, grow, ggrp, mptr, mnode = _plan_both(inc, 1, [0, 3, 1, 2], [0, 1, 2, 4])
    assert gptr.tolist() == [0, 2, 2, 4] and grow.tolist() == [3, 4, 3, 4] and mnode.tolist() == [5, 8, 6, 7]
    _plan_both(inc, 0, [0, 1, 2, 3, 4], np.arange(6))                     # every pin a group of its own
    inc = TC.truncated_incidence()                                        # a row truncated by maxlen: only its first maxlen nodes count
    gptr, grow, _, _, _ = _plan_both(inc, 0, [0, 3, 2], [0, 1, 2, 3])
    assert gptr.tolist() == [0, 2, 3, 4] and grow.tolist() == [0, 1, 1, 0]
    rng = np.random.default_rng(6)
    for _ in range(20):                                                   # and seeded groups over the hand-built rows
        inc = TC.hand_incidence()
        i = int(rng.integers(2))
        n = int(inc[4][i + 1] - inc[4][i])
        sizes = rng.integers(0, n + 1, int(rng.integers(1, 6)))
        pins = np.concatenate([rng.permutation(n)[:s] for s in sizes]) if sizes.sum() else np.zeros(0, dtype=np.int64)
        _plan_both(inc, i, pins, np.concatenate([[0], np.cumsum(sizes)]))


# ------------------------------------------------------------------------------------------------ the scores
def _check_scores(pred_base, required, grow_ptr, grow_row, trial, scale, radius=1):
    got = SE.score_host(pred_base, required, grow_ptr, grow_row, trial, radius, scale)
    want = SC.score_literal(pred_base, required, grow_ptr, grow_row, trial, radius, scale)
    SC.same_tables(got, want)
    G, W = len(grow_ptr) - 1, (2 * radius + 1) ** 2
    assert all(got[k].shape == (G, W) for k in SE.TABLES) and all(got[k].shape == (G,) for k in ('best_w', 'best_dx', 'best_dy', 'best_dq', 'best_gain'))
    assert got['dq'].dtype == got['best_dq'].dtype == np.int64 and got['best_gain'].dtype == np.float64
    assert not np.signbit(got['worst'][got['worst'] == 0]).any()           # a worst slack of zero is +0.0
    return got


def test_score_host_equals_the_literal_definition_on_the_special_rows():
    pred_base, required, grow_ptr, grow_row, trial, scale = SC.special_rows()
    got = _check_scores(pred_base, required, grow_ptr, grow_row, trial, scale)
    c, q1 = SE.centre(1), 2 ** scale
    assert c == 4 and not got['dq'][:, c].any() and not got['dviol'][:, c].any() and not got['new_nan'][:, c].any()
    # group 0: a new NaN; slack -inf hits the cap and is the worst of all; slack +inf cures the row; -0.0 changes nothing
    assert got['new_nan'][0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0] and got['dq'][0, 0] == -q1 and got['dviol'][0, 0] == -1
    assert got['dq'][0, 1] == 2 ** 32 - q1 and got['capped'][0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0]
    assert got['worst'][0, 1] == -np.inf and got['worst_row'][0, 1] == 0
    assert got['dq'][0, 2] == -q1 and got['dviol'][0, 2] == -1 and got['worst'][0, 2] == 0.0 and got['worst_row'][0, 2] == 2
    assert got['dq'][0, 3] == 0 and got['worst'][0, 3] == -1.0
    assert got['dq'][0, 5] == q1 // 2 and got['dviol'][0, 5] == 1
    assert got['dq'][0, 6] == 0 and got['dviol'][0, 6] == 0 and got['worst'][0, 6] == -1.0 and got['worst_row'][0, 6] == 2
    assert got['best_w'][0] == 2 and got['best_dq'][0] == -q1 and got['best_gain'][0] == 1.0      # w = 0 has the same dq but a new NaN
    # group 1: a NaN base row - no worst at the centre, never a NEW NaN; a number makes it valid again
    assert not got['new_nan'][1].any() and np.isnan(got['worst'][1, c]) and got['worst_row'][1, c] == -1
    assert got['dq'][1, 0] == 4 * q1 and got['dviol'][1, 0] == 1 and got['worst'][1, 8] == 1.0 and got['best_w'][1] == c
    # group 2: no rows
    assert not got['dq'][2].any() and not got['dviol'][2].any() and not got['capped'][2].any() and np.isnan(got['worst'][2]).all()
    assert (got['worst_row'][2] == -1).all() and got['best_w'][2] == c and got['best_dq'][2] == 0
    # group 3: rows 0 and 4 tie on the worst slack: the smallest row
    assert got['worst'][3, c] == -1.0 and got['worst_row'][3, c] == 0 and got['worst'][3, 7] == -0.5 and got['worst_row'][3, 7] == 0
    assert got['dq'][3, 7] == -q1 and got['best_w'][3] == 7 and (got['best_dx'][3], got['best_dy'][3]) == (1, 0)


def test_score_host_breaks_ties_by_distance_then_by_offset_and_skips_an_ineligible_minimum():
    *args, want = SC.special_ties()
    got = _check_scores(*args)
    assert got['best_w'].tolist() == want == [1, 0] and got['best_dq'].tolist() == [-2 ** 19, -3 * 2 ** 18]
    assert (got['dq'][0, [0, 1, 3, 7]] == -2 ** 19).all() and (got['dq'][1, [0, 8]] == -3 * 2 ** 18).all()
    *args, want = SC.special_ineligible()
    got = _check_scores(*args)
    assert got['best_w'].tolist() == want and got['new_nan'][0, 2] == 1 and got['dq'][0, 2] == got['dq'][0].min() < got['best_dq'][0] < 0
    # nothing eligible at all (tables of another origin): -1 and zeros
    none = SE.best_host(np.zeros((1, 9), dtype=np.int64), np.ones((1, 9), dtype=np.int32), 1)
    assert none['best_w'].tolist() == [-1] and none['best_dq'].tolist() == [0] and none['best_dx'].tolist() == [0]


def test_score_host_at_the_cap_and_on_seeded_rows():
    pred_base, required, grow_ptr, grow_row, trial, scale = SC.special_cap()
    got = _check_scores(pred_base, required, grow_ptr, grow_row, trial, scale)
    assert scale == 30 and got['capped'][0].tolist() == [2, 1, 1, 1, 1, 1, 1, 1, 1]
    assert got['dq'][0, 0] == 2 ** 32 - 2 ** 30 and got['dq'][0, 1] == 2 ** 32 - 256 - 2 ** 30 and got['dq'][0, 2] == 2 ** 29 - 2 ** 32
    assert reference_quanta(np.array([-4.0, np.nextafter(F(-4.0), F(0.0))], dtype=F), 30)[0].tolist() == [2 ** 32, 2 ** 32 - 256]
    for radius in (1, 2):
        args = SC.seeded_scores(radius=radius)
        got = _check_scores(*args, radius=radius)
        sizes = np.diff(args[2]).tolist()
        assert sizes == [0, 1, 257, 600] and got['new_nan'].any() and got['capped'].any() and (got['best_dq'] <= 0).all()
        assert (got['best_w'] != SE.centre(radius)).any()
    # an entry whose row lies outside pred takes part in nothing
    pred_base, required, grow_ptr, grow_row, trial, scale = SC.special_rows()
    out = grow_row.copy()
    out[[0, 5]] = [17, -1]
    _check_scores(pred_base, required, grow_ptr, out, trial, scale)
    base = SE.base_host(pred_base, required, np.array([0, 1, 2, 3, 4, 9]), scale)
    assert base == dict(nsum=2 * 2 ** scale, violations=2, n_nan=2)


# ------------------------------------------------------------------------------------------------ host validation
def test_check_groups_validates_like_check_moves_under_its_own_name():
    n = 10
    pins, ptr = np.array([1, 2, 3, 1], dtype=np.int64), np.array([0, 3, 4], dtype=np.int64)
    p, gp = SE.check_groups(n, pins, ptr)
    assert p.dtype == gp.dtype == np.int64 and p.tolist() == [1, 2, 3, 1] and gp.tolist() == [0, 3, 4]
    assert SE.check_groups(n, torch.from_numpy(pins), None)[1].tolist() == [0, 1, 2, 3, 4]
    assert SE.check_groups(n, pins[:0], np.array([0, 0], dtype=np.int64))[1].tolist() == [0, 0]
    many = np.arange(64, dtype=np.int64)
    assert SE.check_groups(100, many, np.array([0, 64], dtype=np.int64))[0].shape == (64,)
    refusals = [
        (TypeError, dict(pins=pins.astype(np.int32))), (TypeError, dict(pins=pins.tolist())), (TypeError, dict(pins=pins.astype(np.float64))),
        (TypeError, dict(group_ptr=ptr.astype(np.int32))), (TypeError, dict(group_ptr=[0, 3, 4])),
        (ValueError, dict(pins=pins.reshape(2, 2))), (ValueError, dict(group_ptr=ptr.reshape(1, 3))),
        (IndexError, dict(pins=np.array([1, 2, 3, 10], dtype=np.int64))), (IndexError, dict(pins=np.array([-1, 2, 3, 1], dtype=np.int64))),
        (ValueError, dict(group_ptr=np.zeros(0, dtype=np.int64))),                                  # no entry at all
        (ValueError, dict(group_ptr=np.array([1, 3, 4], dtype=np.int64))),                          # does not start at 0
        (ValueError, dict(group_ptr=np.array([0, 3, 2, 4], dtype=np.int64))),                       # decreases
        (ValueError, dict(group_ptr=np.array([0, 3], dtype=np.int64))),                             # does not end at M
        (ValueError, dict(group_ptr=np.array([0, 3, 5], dtype=np.int64))),
        (ValueError, dict(group_ptr=np.array([0, 4], dtype=np.int64))),                             # pin 1 twice in one group
    ]
    good = dict(pins=pins, group_ptr=ptr)
    for exc, change in refusals:
        with pytest.raises(exc, match='search_plan') as e:
            SE.check_groups(n, **{**good, **change})
        assert 'trial_moves' not in str(e.value) and 'cand_ptr' not in str(e.value)
        kw = {**good, **change}                                           # the same exception type as check_moves gives
        m = np.zeros(np.asarray(kw['pins']).reshape(-1).shape[0], dtype=np.int64)
        with pytest.raises(exc, match='trial_moves'):
            TR.check_moves(n, kw['pins'], m, m, kw['group_ptr'])
    many = np.arange(65, dtype=np.int64)
    with pytest.raises(ValueError, match='65 pins'):
        SE.check_groups(100, many, np.array([0, 65], dtype=np.int64))


def test_check_call_validates_search_moves_arguments():
    assert SE.check_call(10) == (9, 9) and SE.check_call(10, radius=2, max_rows=35) == (25, 3)
    assert SE.check_call(10, radius=8, max_rows=1) == (289, 1) and SE.check_call(0, radius=1, max_rows=1) == (9, 1)
    assert SE.check_call(7, radius=1, max_rows=8) == (9, 1) and SE.check_call(7, np.int64(2), np.int32(0), np.int64(14)) == (25, 2)
    for kw in (dict(radius=0), dict(radius=9), dict(radius=-1), dict(radius=1.0), dict(radius=True), dict(scale_log2=-1), dict(scale_log2=31),
               dict(scale_log2=20.0), dict(max_rows=0), dict(max_rows=-5), dict(max_rows=None)):
        with pytest.raises(ValueError, match='search_moves'):
            SE.check_call(10, **kw)
    assert SE.check_call((2 ** 31 - 1) // 9, radius=1)[0] == 9
    with pytest.raises(ValueError, match='2\\^31'):
        SE.check_call((2 ** 31 - 1) // 9 + 1, radius=1)


def test_predictor_methods_exist_and_refuse_without_trials_before_a_device_is_touched():
    from mmft.infer import Predictor
    assert callable(Predictor.search_plan) and callable(Predictor.search_moves)

    class NoTrials:
        _trial = None
    pins = np.array([0], dtype=np.int64)
    with pytest.raises(RuntimeError, match='search_plan\\(\\): built without trials=True'):
        SE.search_plan(NoTrials(), 0, pins)
    with pytest.raises(RuntimeError, match='search_moves\\(\\): built without trials=True'):
        SE.search_moves(NoTrials(), None)


def test_the_kernel_test_names_the_three_entry_points():
    src = open(os.path.join(ROOT, 'tests', 'test_search_gpu.py')).read()
    assert 'pytestmark = pytest.mark.gpu' in src
    code = code_only(src)
    assert all(f"'{n}'" in code for n in NAMES)
