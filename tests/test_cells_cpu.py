"""The critical cells without a GPU: the ledger of include/mmft_cells.h (bound by mmft.cells.abi, outside the table of mmft.lib),
the host-side refusals of the built library, cells.critical_host against a literal triple loop on the crafted cells of
cells_cases.py and on a seeded input of 257 cells, the host validation of cell_set, critical_plan and refine_cells, and
SearchPlan.from_device on words made by the host."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import cells_cases as KC
from abi_ledger import HEADERS, ROOT, code_only, declared
from mmft import cells as CL
from mmft import commit as CM
from mmft import lib
from mmft import pairs as PR
from mmft import refine as RF
from mmft import search as SE
from mmft import swap as SW
from mmft import trial as TR
from test_search_cpu import _abi_call_sites
from test_swap_cpu import _fake

NAMES = ['mmft_cells_count', 'mmft_cells_fill']
NARGS = {'mmft_cells_count': 21, 'mmft_cells_fill': 27}
I64 = KC.I64


# ------------------------------------------------------------------------------------------------ the header's ledger
def test_cells_header_declares_exactly_its_names_and_overlaps_no_other_header():
    new, decls = declared('mmft_cells.h'), CL.abi.decls()
    assert sorted(new) == NAMES == sorted(decls) and new == NARGS
    assert {n: len(decls[n][1]) for n in NAMES} == NARGS
    for h in ['mmft.h', 'mmft_trial.h', 'mmft_search.h', 'mmft_commit.h', 'mmft_refine.h', 'mmft_swap.h', 'mmft_pairs.h'] + list(HEADERS.values()):
        assert not set(new) & set(declared(h)), h
    for n in NAMES:
        res, args = decls[n]
        assert res is ctypes.c_int and args[-2:] == [ctypes.c_int, ctypes.c_void_p]    # `int device, void* stream` last
    assert decls['mmft_cells_count'][1][14] is ctypes.c_float                          # slack_below: the one fp32 argument
    assert ctypes.c_float not in decls['mmft_cells_fill'][1]
    for other in ('mmft_version', 'mmft_pairs_scan', 'mmft_search_rows', 'mmft_commit_select'):
        with pytest.raises(RuntimeError, match='not declared'):
            CL.abi(other)
    for acc in [getattr(lib, a) for a in HEADERS] + [TR.abi, SE.abi, CM.abi, RF.abi, SW.abi, PR.abi]:
        for n in NAMES:
            with pytest.raises(RuntimeError, match='not declared'):
                acc(n)


def test_the_header_is_bound_by_the_module_and_lib_still_holds_its_nine():
    found = {k: v for k, v in vars(lib).items() if isinstance(v, lib.Header)}
    assert set(found) == set(HEADERS) and len(found) == 9
    assert isinstance(CL.abi, lib.Header) and all(CL.abi is not v for v in found.values())
    assert CL.abi not in (TR.abi, SE.abi, CM.abi, RF.abi, SW.abi, PR.abi)
    assert CL.abi.path.replace('\\', '/').endswith('include/mmft_cells.h') and CL.abi_decls == CL.abi.decls
    assert not hasattr(lib, 'cells') and not any('mmft_cells' in str(getattr(v, 'path', '')) for v in vars(lib).values())
    assert sorted(declared('mmft_pairs.h')) == ['mmft_pairs_near_count', 'mmft_pairs_near_fill', 'mmft_pairs_rows_count', 'mmft_pairs_rows_fill',
                                                'mmft_pairs_scan']                     # the pairs keep their five: the scan is used as it stands
    assert (CL.MAX_SPAN, CL.MAX_PINS) == (65536, 64)
    hdr = open(CL.abi.path).read()
    assert '#define MMFT_CELLS_MAX_SPAN 65536' in hdr and '#define MMFT_CELLS_MAX_PINS 64' in hdr


def test_every_cells_call_site_has_the_headers_argument_count():
    seen, bad = set(), []
    for name, n, f, lineno in _abi_call_sites():
        if name not in NARGS or n is None:        # (a list built elsewhere: the refusal tests)
            continue
        seen.add((name, os.path.basename(f)))
        if NARGS[name] != n:
            bad.append((name, NARGS[name], n, f, lineno))
    assert not bad, bad
    assert {(n, 'cells.py') for n in NAMES} <= seen and {(n, 'test_cells_gpu.py') for n in NAMES} <= seen


def test_the_kernel_test_names_the_two_entry_points_and_the_scan():
    src = open(os.path.join(ROOT, 'tests', 'test_cells_gpu.py')).read()
    assert 'pytestmark = pytest.mark.gpu' in src
    code = code_only(src)
    assert all(f"'{n}'" in code for n in NAMES + ['mmft_pairs_scan'])


# ------------------------------------------------------------------------------------------------ the built library
def _args(base, change):
    assert not set(change) - set(base)
    return list({**base, **change}.values())


SET = dict(cell_ptr=64, cell_node=64, C=3, M=5, inc_ptr=64, inc_row=64, N=9, nnz=7)
COUNT = dict(SET, pred=64, required=64, T=40, row_lo=2, span=33, use_threshold=1, slack_below=0.0, sel=64, n_rows=64, n_pins=64, worst=64,
             device=0, stream=None)
FILL = dict(SET, row_lo=2, span=33, sel=64, worst=64, sel_off=64, row_off=64, pin_off=64, G=2, R=6, MP=4, grow_ptr=64, grow_row=64, grow_grp=64,
            mv_ptr=64, mv_node=64, group_cell=64, group_worst=64, device=0, stream=None)


def test_the_built_library_exports_the_two_and_refuses_bad_arguments_on_the_host():
    """Every argument list below is made of host numbers: nothing can be launched on it, and nothing is - each refusal comes
    before the device is looked at."""
    L = lib.load()
    assert not [n for n in NAMES if not hasattr(L, n)]
    assert [len(v) for v in (COUNT, FILL)] == [21, 27]
    sizes_bad = dict(C_negative=dict(C=-1), C_above=dict(C=(1 << 24) + 1), M_negative=dict(M=-1), N0=dict(N=0), nnz_negative=dict(nnz=-1),
                     row_lo_negative=dict(row_lo=-1), span0=dict(span=0), span_above=dict(span=65537), null_cell_ptr=dict(cell_ptr=None),
                     null_cell_node=dict(cell_node=None), null_inc_ptr=dict(inc_ptr=None), null_inc_row=dict(inc_row=None), null_sel=dict(sel=None),
                     null_worst=dict(worst=None))
    count_bad = dict(T0=dict(T=0), range_past_T=dict(T=34), use2=dict(use_threshold=2), use_negative=dict(use_threshold=-1),
                     nan_threshold=dict(slack_below=float('nan')), null_pred=dict(pred=None), null_required=dict(required=None),
                     null_n_rows=dict(n_rows=None), null_n_pins=dict(n_pins=None))
    for what, change in {**sizes_bad, **count_bad}.items():
        with pytest.raises(RuntimeError, match=r'mmft_cells_count failed \(-1\): cells_count'):
            CL.abi('mmft_cells_count', *_args(COUNT, change))
    fill_bad = dict(C0=dict(C=0), G_negative=dict(G=-1), G_above_C=dict(G=4), R_negative=dict(R=-1), MP_negative=dict(MP=-1),
                    range_past_int=dict(row_lo=2 ** 31 - 10), null_sel_off=dict(sel_off=None), null_row_off=dict(row_off=None),
                    null_pin_off=dict(pin_off=None), null_grow_ptr=dict(grow_ptr=None), null_grow_row=dict(grow_row=None),
                    null_grow_grp=dict(grow_grp=None), null_mv_ptr=dict(mv_ptr=None), null_mv_node=dict(mv_node=None),
                    null_group_cell=dict(group_cell=None), null_group_worst=dict(group_worst=None))
    for what, change in {**sizes_bad, **fill_bad}.items():
        with pytest.raises(RuntimeError, match=r'mmft_cells_fill failed \(-1\): cells_fill'):
            CL.abi('mmft_cells_fill', *_args(FILL, change))
    # the empty calls: fine once the sizes are in order, and no pointer is looked at
    none = dict(cell_ptr=None, cell_node=None, inc_ptr=None, inc_row=None, sel=None, worst=None)
    assert CL.abi('mmft_cells_count', *_args(COUNT, dict(none, C=0, pred=None, required=None, n_rows=None, n_pins=None))) == 0
    assert CL.abi('mmft_cells_count', *_args(COUNT, dict(none, C=0, pred=None, required=None, n_rows=None, n_pins=None, use_threshold=0,
                                                        slack_below=float('nan')))) == 0          # (no threshold: the value is not looked at)
    assert CL.abi('mmft_cells_fill', *_args(FILL, dict(none, G=0, sel_off=None, row_off=None, pin_off=None, grow_ptr=None, grow_row=None, grow_grp=None,
                                                      mv_ptr=None, mv_node=None, group_cell=None, group_worst=None))) == 0
    assert CL.abi('mmft_cells_count', *_args(COUNT, dict(none, C=0, pred=None, required=None, n_rows=None, n_pins=None, span=65536, T=65538))) == 0
    with pytest.raises(RuntimeError, match='cells_count'):                      # ... but the sizes are looked at first
        CL.abi('mmft_cells_count', *_args(COUNT, dict(none, C=0, span=0)))
    with pytest.raises(RuntimeError, match='cells_fill'):
        CL.abi('mmft_cells_fill', *_args(FILL, dict(none, G=0, span=65537)))


# ------------------------------------------------------------------------------------------------ the rule
def _same_as_the_loop(case, thr):
    lit = KC.literal(case, thr)
    sel, n_rows, n_pins, worst = KC.host(case, thr)
    chosen, cw = CL.critical_host(case['inc'], KC.NODE_OFF, case['pins'], case['cell_ptr'], case['pred'], case['required'], case['row_lo'],
                                  case['span'], thr)
    assert chosen.dtype == np.int64 and cw.dtype == np.float32 and worst.dtype == np.float32
    assert chosen.tolist() == [c for c, v in enumerate(lit) if v['sel']], thr
    size = np.diff(case['cell_ptr'])
    for c, v in enumerate(lit):
        assert bool(sel[c]) == v['sel'] and n_rows[c] == (len(v['rows']) if v['sel'] else 0) and n_pins[c] == (size[c] if v['sel'] else 0), (thr, c)
        want = np.float32(np.nan) if v['worst'] is None else v['worst']
        assert np.float32(worst[c]).tobytes() == np.float32(want).tobytes(), (thr, c)                # the bits: NaN is 0x7fc00000
    assert cw.tobytes() == worst[sel].tobytes()
    if chosen.size:                                                               # the rows of the tables are the loop's, all of them
        tabs = CL.plan_host(case['inc'], KC.NODE_OFF, case['pins'], case['cell_ptr'], chosen, case['row_lo'], case['span'])
        for g, c in enumerate(chosen):
            assert tabs[1][tabs[0][g]:tabs[0][g + 1]].tolist() == lit[c]['rows'] and (tabs[2][tabs[0][g]:tabs[0][g + 1]] == g).all()
            assert (tabs[4][tabs[3][g]:tabs[3][g + 1]] - KC.NODE_OFF).tolist() == case['pins'][case['cell_ptr'][c]:case['cell_ptr'][c + 1]].tolist()
    return lit


def _shows_every_edge(case):
    """Each situation the rule distinguishes occurs in the case: asserted one by one."""
    t = case['tags']
    at0, quarter, none = (_same_as_the_loop(case, thr) for thr in (0.0, -0.25, None))
    assert np.float32(CL.NAN_BITS).dtype == np.float32 and np.array([np.nan], dtype=np.float32).view(np.uint32)[0] == CL.NAN_BITS
    assert at0[t['no_pins']]['why'] == 'no_pins' and none[t['no_pins']]['why'] == 'no_pins'          # excluded by having no pins
    assert at0[t['sixty_five']]['why'] == 'many_pins' and none[t['sixty_five']]['why'] == 'many_pins'  # ... by having 65 pins
    assert np.diff(case['cell_ptr'])[t['sixty_five']] == 65 and np.diff(case['cell_ptr'])[t['sixty_four']] == 64
    assert none[t['sixty_four']]['sel']                                            # 64 pins: at the limit
    assert at0[t['no_rows']]['why'] == 'no_rows' and at0[t['outside_only']]['why'] == 'no_rows'      # ... by having no rows
    assert at0[t['nan_only']]['why'] == 'nan_only' and at0[t['nan_only']]['rows']                     # ... by having only NaN rows
    v = quarter[t['quarter']]                                                      # ... by a slack exactly equal to the threshold
    assert v['why'] == 'not_below' and v['worst'] == np.float32(-0.25)
    v = at0[t['zero']]
    assert v['why'] == 'not_below' and v['worst'] == 0.0
    v, r = at0[t['minus_zero']], at0[t['minus_zero']]['rows'][0]                   # ... by a -0.0 slack at threshold 0
    raw = np.float32(case['required'][r]) - np.float32(case['pred'][r])
    assert v['why'] == 'not_below' and raw == 0.0 and np.signbit(raw) and not np.signbit(v['worst'])
    v = at0[t['quarter']]                                                          # selected through a single row of a single pin
    assert v['sel'] and v['below'] == 1 and v['visits'] == 1 and np.diff(case['cell_ptr'])[t['quarter']] == 1
    v = at0[t['sharing']]                                                          # pins that share rows: the union is shorter than the sum
    assert v['sel'] and len(v['rows']) < v['visits']
    v = at0[t['long']]
    assert v['longest'] == KC.LONG > 64 and v['sel']                               # a pin with more than 64 rows
    assert v['outside'] >= 2 and at0[t['outside_only']]['outside'] == 2            # rows outside the span, ignored
    assert case['row_lo'] in at0[t['ends']]['rows'] and case['row_lo'] + case['span'] - 1 in at0[t['ends']]['rows']
    for name in ('no_rows', 'outside_only'):                                       # slack_below=None selects cells without rows
        assert none[t[name]]['sel'] and not none[t[name]]['rows']
    assert none[t['nan_only']]['sel'] and none[t['nan_only']]['worst'] is None
    return at0


@pytest.mark.parametrize('span', [64, 65, 2049])
def test_critical_host_equals_a_literal_triple_loop_on_the_crafted_cells(span):
    case = KC.make(12, span)
    assert len(case['tags']) == 12 and case['row_lo'] > 0
    _shows_every_edge(case)
    for thr in (-1e30, 1e30, float('inf'), -float('inf'), -0.0, 1.0):
        _same_as_the_loop(case, thr)


def test_critical_host_equals_a_literal_triple_loop_on_a_seeded_input_of_257_cells():
    case = KC.make(257, 2049, row_lo=11, seed=3)
    size = np.diff(case['cell_ptr'])
    assert case['C'] == 257 and set(KC.SIZES) <= set(size.tolist())
    at0 = _shows_every_edge(case)
    whys = [v['why'] for v in at0[12:]]                                            # the seeded cells show the exclusions too
    assert {'no_pins', 'many_pins', 'not_below', None} <= set(whys)
    chosen, tables, words = KC.expected(case, 0.0)
    G, R, MP = len(chosen), tables[1].shape[0], tables[4].shape[0]
    assert 0 < G < 257 and words.dtype == np.int32 and words.shape[0] == 4 * G + 2 + 2 * R + MP
    assert KC.expected(case, -1e30)[2] is None


# ------------------------------------------------------------------------------------------------ host validation
def _predictor(N=100, T=20, rows_of_design=None):
    """A stand-in Predictor on the CPU with what cell_set reads: one design of N nodes behind 7 of another, T rows."""
    design = np.zeros(T, dtype=np.int64) if rows_of_design is None else rows_of_design

    def check(i, what):
        if not 0 <= i < 2:
            raise IndexError(f'{what}: design {i} of 2')
    return types.SimpleNamespace(_trial=object(), _check_design=check, slack=types.SimpleNamespace(design=design),
                                 _placed=types.SimpleNamespace(node_off=[0, 7, 7 + N]), device='cpu')


def test_cell_set_validates_once_on_the_host():
    from mmft.infer import Predictor
    assert callable(Predictor.cell_set) and callable(Predictor.critical_plan) and callable(Predictor.refine_cells)
    design = np.array([0, 0, 1, 1, 0, 1, 1, 0], dtype=np.int64)
    p = _predictor(rows_of_design=design)
    cs = CL.cell_set(p, 1, I64([4, 9, 2, 30]), I64([0, 2, 2, 3, 4]))
    assert isinstance(cs, CL.CellSet) and (cs.C, cs.M, cs.i, cs.node_off, cs.row_lo, cs.span) == (4, 4, 1, 7, 2, 5) and cs.owner is p
    assert cs.ints.dtype == torch.int32 and cs.ints.tolist() == [0, 2, 2, 3, 4, 11, 16, 9, 37]
    assert cs.dev[0].tolist() == [0, 2, 2, 3, 4] and cs.dev[1].tolist() == [11, 16, 9, 37]
    assert CL.cell_set(p, 1, torch.tensor([5, 6])).cell_ptr.tolist() == [0, 1, 2]                   # None: every pin a cell of its own
    with pytest.raises(RuntimeError, match='cell_set\\(\\): built without trials=True'):
        CL.cell_set(types.SimpleNamespace(_trial=None), 0, I64([1]))
    with pytest.raises(IndexError, match='cell_set: design 2 of 2'):
        CL.cell_set(p, 2, I64([1]))
    with pytest.raises(ValueError, match='cell_set: design 0 has no selected path'):
        CL.cell_set(_predictor(rows_of_design=np.ones(4, dtype=np.int64)), 0, I64([1]))
    refusals = [
        (TypeError, 'pins must be a numpy array or tensor of int64', dict(pins=[1, 2])),
        (TypeError, 'pins must be a numpy array or tensor of int64', dict(pins=np.array([1, 2], dtype=np.int32))),
        (TypeError, 'cell_ptr must be a numpy array or tensor of int64', dict(cell_ptr=[0, 2])),
        (ValueError, 'pins must be 1-D', dict(pins=I64([[1, 2]]))),
        (IndexError, 'pins outside the design\'s 100 nodes', dict(pins=I64([1, 100]))),
        (IndexError, 'pins outside', dict(pins=I64([-1, 2]))),
        (ValueError, 'cell_ptr must start at 0', dict(cell_ptr=I64([1, 2]))),
        (ValueError, 'cell_ptr must not decrease', dict(cell_ptr=I64([0, 2, 1, 2]))),
        (ValueError, 'cell_ptr must end at the number of pins, 2', dict(cell_ptr=I64([0, 1]))),
        (ValueError, 'a cell holds 65 pins, at most 64', dict(pins=I64(np.arange(65)), cell_ptr=I64([0, 65]))),
        (ValueError, 'the same pin twice in one cell', dict(pins=I64([3, 3]), cell_ptr=I64([0, 2]))),
        (ValueError, 'cell_set: no cell', dict(pins=I64([]), cell_ptr=I64([0]))),
        (ValueError, 'cell_set: pin 5 belongs to cells 0 and 3; the cells of a set must hold distinct pins',
         dict(pins=I64([5, 8, 6, 8, 5]), cell_ptr=I64([0, 2, 2, 3, 5]))),           # a pin in two cells: the first such pin, its two cells
        (ValueError, 'cell_set: pin 4 belongs to cells 0 and 1', dict(pins=I64([4, 4]))),
    ]
    for exc, match, change in refusals:
        args = dict(dict(pins=I64([1, 2]), cell_ptr=None), **change)
        with pytest.raises(exc, match=f'cell_set: .*{match}' if not match.startswith('cell_set') else match):
            CL.cell_set(p, 1, args['pins'], args['cell_ptr'])
    assert CL.cell_set(p, 1, I64(np.arange(64)), I64([0, 64])).C == 1                                # 64 pins: at the limit


def test_critical_plan_and_refine_cells_validate_on_the_host():
    p, other = _predictor(), _predictor()
    cs = CL.cell_set(p, 0, I64([1, 2, 3]))

    class NoTrials:
        _trial = None
    for who, call in (('critical_plan', CL.critical_plan), ('refine_cells', CL.refine_cells)):
        with pytest.raises(RuntimeError, match=f'{who}\\(\\): built without trials=True'):
            call(NoTrials(), cs)
        for bad in (dict(C=3), None, _fake()[1], I64([1, 2])):
            with pytest.raises(TypeError, match=f'{who}: cells must come from cell_set'):
                call(p, bad)
        with pytest.raises(ValueError, match=f'{who}: the cell set belongs to another Predictor'):   # a foreign cell set
            call(other, cs)
        for bad in (float('nan'), np.float32('nan'), np.nan):
            with pytest.raises(ValueError, match=f'{who}: slack_below must not be NaN'):
                call(p, cs, slack_below=bad)
        for bad in ('0', True, [0.0], 1j, torch.zeros(1)):
            with pytest.raises(ValueError, match=f'{who}: slack_below must be a number or None'):
                call(p, cs, slack_below=bad)
    for max_groups in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match='critical_plan: max_groups must be an integer of at least 1'):
            CL.critical_plan(p, cs, 0.0, max_groups)
    for passes in (0, -1, 1.5, True):                                             # as refine_moves validates it
        with pytest.raises(ValueError, match='refine_cells: passes must be an integer of at least 1'):
            CL.refine_cells(p, cs, passes=passes)
    with pytest.raises(ValueError, match='refine_cells: every pass applies'):
        CL.refine_cells(p, cs, apply=False)
    assert CL.check_threshold(None) is None and CL.check_threshold(np.int64(2)) == 2.0 and CL.check_threshold(-0.0) == 0.0
    assert CL.check_threshold(0.1) == float(np.float32(0.1)) != 0.1               # the threshold is an fp32
    assert CL.check_threshold(float('inf')) == float('inf') and CL.check_threshold(1e300) == float('inf')


# ------------------------------------------------------------------------------------------------ the plan
def test_a_plan_decoded_from_device_words_is_an_ordinary_search_plan():
    """SearchPlan.from_device on the words of a host-built plan (the CPU stands in for the device): the same tables, dtypes and
    views as SearchPlan(...)'s, with and without words behind the tables."""
    p, want = _fake()
    extra = torch.tensor([7, -3, 0x7fc00000], dtype=torch.int32)
    for buf, tail in ((want.ints.clone(), []), (torch.cat([want.ints, extra]), extra.tolist())):
        got = SE.SearchPlan.from_device(p, 0, buf, want.G, want.R, want.M, node_off=want.node_off, pins_distinct=True)
        assert isinstance(got, SE.SearchPlan) and (got.G, got.R, got.M, got.i, got.node_off) == (want.G, want.R, want.M, want.i, want.node_off)
        assert got.owner is p and got.pins_distinct is True and got.tail.dtype == np.int32 and got.tail.tolist() == tail
        for name in ('grow_ptr', 'grow_row', 'grow_grp', 'mv_ptr', 'mv_node'):
            assert getattr(got, name).dtype == np.int64 and np.array_equal(getattr(got, name), getattr(want, name)), name
        assert got.ints.dtype == torch.int32 and torch.equal(got.ints, want.ints)
        assert len(got.dev) == 5 and all(torch.equal(g, w) for g, w in zip(got.dev, want.dev))
        assert got.ints.data_ptr() == buf.data_ptr()                               # views of the buffer, no second copy
        CM.check_plan(got)                                                         # the verdict it was given: no np.unique per plan
    assert SE.SearchPlan.from_device(p, 0, want.ints.clone(), want.G, want.R, want.M).pins_distinct is None
    q, shared = _fake(groups=([0, 1], [2], [1]))
    again = SE.SearchPlan.from_device(q, 0, shared.ints.clone(), shared.G, shared.R, shared.M)
    with pytest.raises(ValueError, match='pin 1 of design 0 belongs to groups 0 and 2'):              # undecided: check_plan decides as ever
        CM.check_plan(again)
