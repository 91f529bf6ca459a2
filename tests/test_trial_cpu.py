"""Trial pin moves without a GPU: the ledger of include/mmft_trial.h (bound by mmft.trial.abi, outside the table of mmft.lib),
the host-side refusals of the built library, expand_candidates against a literal loop, the reduction's numpy restatement
against a literal definition, and the host validation of trial_moves' arguments."""
import ast
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import trial_cases as TC
from abi_ledger import HEADERS, PKG, ROOT, declared, others
from mmft import lib
from mmft import trial as TR

NAMES = ['mmft_trial_reduce', 'mmft_trial_rows']
NARGS = {'mmft_trial_rows': 30, 'mmft_trial_reduce': 13}
F = np.float32


# ------------------------------------------------------------------------------------------------ the header's ledger
def test_trial_header_declares_exactly_its_names_and_overlaps_no_other_header():
    new, decls = declared('mmft_trial.h'), TR.abi.decls()
    assert sorted(new) == NAMES == sorted(decls) and new == NARGS
    assert {n: len(decls[n][1]) for n in NAMES} == NARGS
    for h in ['mmft.h'] + list(HEADERS.values()):
        assert not set(new) & set(declared(h)), h
    assert others('mmft_trial.h') == ['mmft.h'] + list(HEADERS.values())          # the shared table does not know this header
    for n in NAMES:
        res, args = decls[n]
        assert res is ctypes.c_int and args[-2:] == [ctypes.c_int, ctypes.c_void_p]    # `int device, void* stream` last
    with pytest.raises(RuntimeError, match='not declared'):
        TR.abi('mmft_version')
    with pytest.raises(RuntimeError, match='not declared'):
        TR.abi('mmft_placed_fc_fwd')
    for acc in HEADERS:
        for n in NAMES:
            with pytest.raises(RuntimeError, match='not declared'):
                getattr(lib, acc)(n)


def test_lib_still_has_exactly_its_nine_header_attributes():
    found = {k: v for k, v in vars(lib).items() if isinstance(v, lib.Header)}
    assert set(found) == set(HEADERS) and len(found) == 9
    assert isinstance(TR.abi, lib.Header) and all(TR.abi is not v for v in found.values())
    assert TR.abi.path.replace('\\', '/').endswith('include/mmft_trial.h') and TR.abi_decls == TR.abi.decls
    assert not hasattr(lib, 'trial') and not hasattr(lib, 'abi')


def _abi_call_sites():
    """(name, nargs, file, lineno) of every `abi('mmft_...', ...)` / `something.abi('mmft_...', ...)` call under the package,
    tests/ and tools/; nargs as abi_ledger.call_sites counts them."""
    files = glob.glob(os.path.join(PKG, '**', '*.py'), recursive=True)
    files += glob.glob(os.path.join(ROOT, 'tests', '*.py')) + glob.glob(os.path.join(ROOT, 'tools', '*.py'))
    for f in files:
        for node in ast.walk(ast.parse(open(f).read())):
            if not isinstance(node, ast.Call) or not node.args:
                continue
            fn = node.func
            if not ((isinstance(fn, ast.Name) and fn.id == 'abi') or (isinstance(fn, ast.Attribute) and fn.attr == 'abi')):
                continue
            a0 = node.args[0]
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


def test_every_abi_call_site_has_the_headers_argument_count():
    checked, bad, seen = 0, [], set()
    for name, n, f, lineno in _abi_call_sites():
        if n is None or name not in NARGS:        # (a list built elsewhere; the names the ledger test feeds to be refused)
            continue
        checked += 1
        seen.add((name, os.path.basename(f)))
        if NARGS[name] != n:
            bad.append((name, NARGS[name], n, f, lineno))
    assert not bad, bad
    assert {('mmft_trial_rows', 'trial.py'), ('mmft_trial_reduce', 'trial.py')} <= seen and checked >= 2


# ------------------------------------------------------------------------------------------------ the built library
def _rows_args(**change):
    """A full argument list of mmft_trial_rows made of host integers: nothing can be launched on it, and nothing is - every
    refusal below comes before the device is looked at."""
    a = dict(path_nodes=64, path_lens=64, maxlen=4, loc_x=64, loc_y=64, map_x=16, map_y=16, paths=64, f_off=None, T=5,
             pair_row=64, pair_cand=64, n_pairs=3, mv_ptr=64, mv_node=64, mv_x=64, mv_y=64, K=2, GP=64, bias=None,
             x=64, ldx=288, xt=64, ldxt=288, width=288, cnn_col=128, Dout=128, S=64, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def _reduce_args(**change):
    a = dict(pred_base=64, pred_trial=64, required=64, design_rows=64, n=5, T=5, pair_ptr=64, pair_row=64, n_pairs=3, K=2,
             summary=64, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def test_the_built_library_exports_both_and_refuses_bad_arguments_on_the_host():
    L = lib.load()
    assert not [n for n in NAMES if not hasattr(L, n)]
    assert L.mmft_version() >= 211
    assert len(_rows_args()) == 30 and len(_reduce_args()) == 13
    refused = dict(S=dict(S=32), P_not_64=dict(map_x=10, map_y=10), P_above=dict(map_x=512, map_y=256), map_x0=dict(map_x=0),
                   Dout6=dict(Dout=6, width=300, ldx=300, ldxt=300), Dout0=dict(Dout=0), Dout_above=dict(Dout=1028, width=1200, ldx=1200, ldxt=1200),
                   maxlen0=dict(maxlen=0), T0=dict(T=0), K0=dict(K=0), pairs_negative=dict(n_pairs=-1),
                   cnn_col_odd=dict(cnn_col=126), cnn_col_negative=dict(cnn_col=-4), ldx_odd=dict(ldx=290), ldxt_odd=dict(ldxt=290),
                   width_below=dict(width=252, ldx=252, ldxt=252), width_above_ldx=dict(ldx=284), width_above_ldxt=dict(ldxt=284),
                   null_nodes=dict(path_nodes=None), null_lens=dict(path_lens=None), null_loc_x=dict(loc_x=None), null_loc_y=dict(loc_y=None),
                   null_paths=dict(paths=None), null_pair_row=dict(pair_row=None), null_pair_cand=dict(pair_cand=None),
                   null_mv_ptr=dict(mv_ptr=None), null_mv_node=dict(mv_node=None), null_mv_x=dict(mv_x=None), null_mv_y=dict(mv_y=None),
                   null_GP=dict(GP=None), null_x=dict(x=None), null_xt=dict(xt=None),
                   odd_GP=dict(GP=68), odd_x=dict(x=72), odd_xt=dict(xt=68), odd_bias=dict(bias=72))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_trial_rows failed \(-1\): trial_rows'):
            TR.abi('mmft_trial_rows', *_rows_args(**change))
    # no pairs: fine once the sizes are in order, and no pointer is looked at
    nothing = dict(n_pairs=0, path_nodes=None, path_lens=None, loc_x=None, loc_y=None, paths=None, pair_row=None, pair_cand=None,
                   mv_ptr=None, mv_node=None, mv_x=None, mv_y=None, GP=None, x=None, xt=None)
    assert TR.abi('mmft_trial_rows', *_rows_args(**nothing)) == 0
    with pytest.raises(RuntimeError, match=r'trial_rows'):
        TR.abi('mmft_trial_rows', *_rows_args(**nothing, S=32))
    refused = dict(n0=dict(n=0), n_above=dict(n=(1 << 24) + 1), T0=dict(T=0), T_above=dict(T=(1 << 24) + 1), K_negative=dict(K=-1),
                   pairs_negative=dict(n_pairs=-1), null_pred_base=dict(pred_base=None), null_required=dict(required=None),
                   null_design_rows=dict(design_rows=None), null_summary=dict(summary=None), null_pair_ptr=dict(pair_ptr=None),
                   null_pair_row=dict(pair_row=None), null_pred_trial=dict(pred_trial=None), odd_summary=dict(summary=68))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_trial_reduce failed \(-1\): trial_reduce'):
            TR.abi('mmft_trial_reduce', *_reduce_args(**change))


# ------------------------------------------------------------------------------------------------ expansion
def _expand_both(inc, i, pins, cand_ptr):
    nodes, lens, paths, maxlen, node_off, n_nodes = inc
    table = TR.rows_of_pin(nodes, lens, paths, maxlen, n_nodes)
    pins, cand_ptr = np.asarray(pins, dtype=np.int64), np.asarray(cand_ptr, dtype=np.int64)
    got = TR.expand_candidates(table, node_off[i], pins, cand_ptr)
    want = TC.expand_literal(nodes, lens, paths, node_off[i], pins, cand_ptr)
    assert all(g.dtype == np.int64 for g in got)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), (got, want)
    return got


def test_expand_candidates_equals_a_literal_loop_on_hand_built_rows():
    inc = TC.hand_incidence()
    # design 0.  candidate 0: pin 0, twice in row 0 -> the row once.  1: pin 4, on no selected row.  2: pins 1 and 2 share rows
    # 0, 1, 2 and 5 -> each once.  3: empty.  4: pin 3 -> row 2 alone
    ptr, row, cand = _expand_both(inc, 0, [0, 4, 1, 2, 3], [0, 1, 2, 4, 4, 5])
    assert ptr.tolist() == [0, 1, 1, 5, 5, 6] and row.tolist() == [0, 0, 1, 2, 5, 2] and cand.tolist() == [0, 2, 2, 2, 2, 4]
    # design 1: the same ids mean other pins (offset 5): pin 0 is table pin 5 -> rows 3 and 4; pin 3 is table pin 8, on no path
    ptr, row, cand = _expand_both(inc, 1, [0, 3, 1, 2], [0, 1, 2, 4])
    assert ptr.tolist() == [0, 2, 2, 4] and row.tolist() == [3, 4, 3, 4]
    # every move a candidate of its own, and no move at all
    _expand_both(inc, 0, [0, 1, 2, 3, 4], np.arange(6))
    ptr, row, cand = _expand_both(inc, 0, [], [0])
    assert ptr.tolist() == [0] and row.size == 0 and cand.size == 0
    ptr, row, cand = _expand_both(inc, 0, [], [0, 0, 0])
    assert ptr.tolist() == [0, 0, 0]
    # a row truncated by maxlen: only its first maxlen nodes count
    inc = TC.truncated_incidence()
    ptr, row, cand = _expand_both(inc, 0, [0, 3, 2], [0, 1, 2, 3])
    assert ptr.tolist() == [0, 2, 3, 4] and row.tolist() == [0, 1, 1, 0]
    rng = np.random.default_rng(4)
    for _ in range(20):                                                  # and seeded candidates over the hand-built rows
        inc = TC.hand_incidence()
        i = int(rng.integers(2))
        n = int(inc[4][i + 1] - inc[4][i])
        sizes = rng.integers(0, n + 1, int(rng.integers(1, 6)))
        pins = np.concatenate([rng.permutation(n)[:s] for s in sizes]) if sizes.sum() else np.zeros(0, dtype=np.int64)
        _expand_both(inc, i, pins, np.concatenate([[0], np.cumsum(sizes)]))


def test_expand_candidates_has_no_python_loop():
    import inspect
    tree = ast.parse(inspect.getsource(TR.expand_candidates))
    assert not [n for n in ast.walk(tree) if isinstance(n, (ast.For, ast.While, ast.ListComp, ast.GeneratorExp, ast.DictComp, ast.SetComp))]


# ------------------------------------------------------------------------------------------------ reduction
def _check_reduction(pred_base, required, design_rows, pair_ptr, pair_row, pred_trial):
    got = TR.reduce_host(pred_base, required, design_rows, pair_ptr, pair_row, pred_trial)
    want = TC.reduce_literal(pred_base, required, design_rows, pair_ptr, pair_row, pred_trial)
    assert got.shape == want.shape == (len(pair_ptr), 6) and got.dtype == np.float64
    assert np.array_equal(got[:, :5], want[:, :5], equal_nan=True), (got, want)
    assert not np.signbit(got[:, 3][got[:, 3] == 0]).any()               # a worst slack of zero is +0.0
    for k in range(got.shape[0]):
        # two fp64 summation orders of n terms differ by at most (n - 1) * 2^-52 * sum |term| (here: from the exact sum)
        n, mag = int(got[k, 2]), abs(want[k, 5])
        assert abs(got[k, 5] - want[k, 5]) <= max(n - 1, 0) * 2.0 ** -52 * mag, k
    return got


def test_reduce_host_equals_the_literal_definition_on_the_special_rows():
    nan = np.nan
    #            row:  0     1     2     3     4     5     6     7
    required = np.array([1.0, 1.0, 2.0, 0.5, 0.5, 3.0, 1.0, 9.0], dtype=F)
    pred_base = np.array([2.0, nan, 2.0, 1.5, 1.5, 1.0, 1.0, 9.5], dtype=F)   # slacks -1, NaN, +0, -1, -1, 2, +0, -0.5
    design_rows = np.array([0, 1, 2, 3, 4, 6, 7])                          # row 5 belongs to another design
    # the base: rows 0, 3 and 4 tie on the worst slack, -1: the smallest row, 0, wins
    # candidate 0: row 2 gets a NaN prediction -> one more NaN row; row 6 keeps its slack of zero
    # candidate 1: row 0 is improved to +1; rows 3 and 4 still tie: row 3 wins
    # candidate 2: no pairs - the base's figures
    # candidate 3: every row NaN - no valid row
    pair_ptr = np.array([0, 2, 3, 3, 10])
    pair_row = np.array([2, 6, 0, 0, 1, 2, 3, 4, 6, 7])
    pred_trial = np.array([nan, 1.0, 0.0, nan, nan, nan, nan, nan, nan, nan], dtype=F)
    got = _check_reduction(pred_base, required, design_rows, pair_ptr, pair_row, pred_trial)
    base = got[4]
    assert base.tolist()[:5] == [6, 1, 4, -1.0, 0] and base[5] == -3.5
    assert got[0].tolist()[:5] == [5, 2, 4, -1.0, 0]
    assert got[1].tolist()[:5] == [6, 1, 3, -1.0, 3] and got[1][5] == -2.5
    assert np.array_equal(got[2], base)
    assert got[3].tolist()[:3] == [0, 7, 0] and np.isnan(got[3][3]) and got[3][4] == -1 and got[3][5] == 0.0
    # -0.0: required -0.0 and pred +0.0 give -0.0 - 0.0 = -0.0 in fp32; it must come out as +0.0, not violate, and tie with +0.0
    required = np.array([-0.0, 0.0, 5.0], dtype=F)
    pred_base = np.array([0.0, 0.0, 1.0], dtype=F)
    assert np.signbit(F(required[0]) - F(pred_base[0]))
    got = _check_reduction(pred_base, required, np.arange(3), np.array([0]), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=F))
    assert got[0].tolist() == [3, 0, 0, 0.0, 0, 0.0] and not np.signbit(got[0][3])
    # a row index outside pred counts like a NaN row
    got = _check_reduction(pred_base, required, np.array([0, 7, 2, -1]), np.array([0]), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=F))
    assert got[0].tolist()[:3] == [2, 2, 0]


def test_reduce_host_sums_in_the_kernels_order():
    """Thread j of 256 takes rows j, j + 256, ...; lanes by xor 32 .. 1; waves in order: on terms chosen so that the order
    shows (a large term cancels only when it meets its negative first)."""
    rng = np.random.default_rng(8)
    n = 1000
    slack = -(10.0 ** rng.uniform(-6, 6, n)).astype(F)
    required, pred = np.zeros(n, dtype=F), -slack                          # slack = 0 - pred
    got = TR.reduce_host(pred, required, np.arange(n), np.array([0]), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=F))[0]
    per = np.zeros(256)
    for j in range(256):
        acc = 0.0
        for v in slack[j::256]:
            acc += float(v)
        per[j] = acc
    waves = []
    for w in range(4):
        v = per[64 * w:64 * w + 64].copy()
        for o in (32, 16, 8, 4, 2, 1):
            v = np.array([v[l] + v[l ^ o] for l in range(64)])
        assert len(set(v.tolist())) == 1                                   # every lane holds the same bits
        waves.append(v[0])
    want = 0.0
    for w in waves:
        want += w
    assert got[5] == want and got[2] == n
    _check_reduction(pred, required, np.arange(n), np.array([0]), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=F))


def test_decode_splits_the_summary_into_typed_fields():
    s = np.array([[3, 1, 2, -0.5, 7, -0.75], [0, 4, 0, np.nan, -1, 0.0]])
    d = TR.decode(s)
    assert sorted(d) == sorted(TR.FIELDS)
    assert d['n'].tolist() == [3, 0] and d['n_nan'].tolist() == [1, 4] and d['violations'].tolist() == [2, 0] and d['wns_row'].tolist() == [7, -1]
    assert d['wns'][0] == -0.5 and np.isnan(d['wns'][1]) and d['tns'].tolist() == [-0.75, 0.0]
    assert all(d[k].dtype == np.int64 for k in ('n', 'n_nan', 'violations', 'wns_row')) and d['wns'].dtype == d['tns'].dtype == np.float64


# ------------------------------------------------------------------------------------------------ host validation
def test_check_moves_validates_on_the_host():
    n = 10
    pins = np.array([1, 2, 3, 1], dtype=np.int64)
    x, y = np.array([0, 1, 2, 3], dtype=np.int64), np.array([4, 5, 6, 7], dtype=np.int32)
    ptr = np.array([0, 3, 4], dtype=np.int64)
    p, gx, gy, gp = TR.check_moves(n, pins, x, y, ptr)
    assert p.dtype == np.int64 and gx.dtype == gy.dtype == np.int32 and gp.dtype == np.int64
    assert p.tolist() == [1, 2, 3, 1] and gx.tolist() == [0, 1, 2, 3] and gy.tolist() == [4, 5, 6, 7] and gp.tolist() == [0, 3, 4]
    # tensors, int32 extremes, every move a candidate of its own (the same pin in two candidates is fine)
    p, gx, gy, gp = TR.check_moves(n, torch.from_numpy(pins), torch.tensor([-2 ** 31, 2 ** 31 - 1, 0, 5]), y, None)
    assert gp.tolist() == [0, 1, 2, 3, 4] and gx.tolist() == [-2 ** 31, 2 ** 31 - 1, 0, 5]
    assert TR.check_moves(n, pins[:0], x[:0], y[:0], None)[3].tolist() == [0]
    assert TR.check_moves(n, pins[:0], x[:0], y[:0], np.array([0, 0], dtype=np.int64))[3].tolist() == [0, 0]
    many = np.arange(64, dtype=np.int64)
    assert TR.check_moves(100, many, many, many, np.array([0, 64], dtype=np.int64))[0].shape == (64,)
    refusals = [
        (TypeError, dict(pins=pins.astype(np.int32))), (TypeError, dict(pins=pins.tolist())), (TypeError, dict(pins=pins.astype(np.float64))),
        (TypeError, dict(pin_x=x.astype(np.float32))), (TypeError, dict(pin_y=y.astype(np.int16))), (TypeError, dict(pin_x=x.tolist())),
        (TypeError, dict(cand_ptr=ptr.astype(np.int32))), (TypeError, dict(cand_ptr=[0, 3, 4])),
        (ValueError, dict(pins=pins.reshape(2, 2))), (ValueError, dict(pin_x=x[:-1])), (ValueError, dict(pin_y=y.reshape(2, 2))),
        (ValueError, dict(cand_ptr=ptr.reshape(1, 3))), (ValueError, dict(pin_x=np.array([0, 1, 2, 2 ** 31], dtype=np.int64))),
        (ValueError, dict(pin_y=np.array([0, 1, 2, -2 ** 31 - 1], dtype=np.int64))),
        (IndexError, dict(pins=np.array([1, 2, 3, 10], dtype=np.int64))), (IndexError, dict(pins=np.array([-1, 2, 3, 1], dtype=np.int64))),
        (ValueError, dict(cand_ptr=np.array([0, 4, 4][:0], dtype=np.int64))),                      # no entry at all
        (ValueError, dict(cand_ptr=np.array([1, 3, 4], dtype=np.int64))),                          # does not start at 0
        (ValueError, dict(cand_ptr=np.array([0, 3, 2, 4], dtype=np.int64))),                       # decreases
        (ValueError, dict(cand_ptr=np.array([0, 3], dtype=np.int64))),                             # does not end at M
        (ValueError, dict(cand_ptr=np.array([0, 3, 5], dtype=np.int64))),
        (ValueError, dict(cand_ptr=np.array([0, 4], dtype=np.int64))),                             # pin 1 twice in one candidate
    ]
    good = dict(pins=pins, pin_x=x, pin_y=y, cand_ptr=ptr)
    for exc, change in refusals:
        with pytest.raises(exc, match='trial_moves'):
            TR.check_moves(n, **{**good, **change})
    many = np.arange(65, dtype=np.int64)
    with pytest.raises(ValueError, match='65 moves'):
        TR.check_moves(100, many, many, many, np.array([0, 65], dtype=np.int64))


def test_predictor_refuses_trials_without_placement_before_it_touches_a_device():
    from mmft.infer import Predictor
    with pytest.raises(ValueError, match='trials=True needs placement=True'):
        Predictor(None, None, [], 'cpu', trials=True)
    with pytest.raises(ValueError, match='trials=True needs placement=True'):
        Predictor(None, None, [], 'cpu', trials=True, placement=False, report=dict(k=1))


def test_the_kernel_test_names_both_entry_points():
    src = open(os.path.join(ROOT, 'tests', 'test_trial_gpu.py')).read()
    assert 'pytestmark = pytest.mark.gpu' in src
    from abi_ledger import code_only
    code = code_only(src)
    assert all(f"'{n}'" in code for n in NAMES)
