"""Incremental re-prediction without a GPU: the numpy cone test_incr_gpu.py checks the device against is a closure, the ledger of
include/mmft_incr.h (the rules test_place_cpu.py applies to include/mmft_place.h), and the host validation of update(rows=)."""
import os
import re

import numpy as np
import pytest
import torch

import incr_cases as C
from abi_ledger import call_sites, code_only as _code_only, declared as _declared
from mmft import lib
from mmft.infer import check_rows

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ['mmft_fanout_cone_step', 'mmft_mlp2_feat_fwd_bf16_masked', 'mmft_update_rows_diff']


# ------------------------------------------------------------------------------------------------ the reference cone
@pytest.mark.parametrize('fanin', ['regular', 'irregular'])
def test_the_numpy_cone_is_a_closure(fanin):
    from mmft.synth import synth_design
    d = synth_design(N=2048, L=12, tile=32, seed=700, end_frac=0.25, fanin=fanin)
    rng = np.random.default_rng(1)
    a, b = rng.permutation(d.N)[:20], rng.permutation(d.N)[:20]
    ca, cb, cab = C.design_cone(d, a), C.design_cone(d, b), C.design_cone(d, np.concatenate([a, b]))
    assert ca.dtype == np.uint8 and ca[a].all() and cb[b].all()
    assert np.array_equal(cab, ca | cb)                                        # cone(A u B) = cone(A) | cone(B)
    assert np.array_equal(C.design_cone(d, ca), ca)                            # cone(cone(A)) = cone(A)
    assert np.array_equal(C.design_cone(d, np.flatnonzero(ca)), ca)
    assert not C.design_cone(d, np.zeros(0, dtype=np.int64)).any()
    last = d.levels[d.L - 1][:3]
    for v in last:                                                             # a last-level seed gives exactly itself
        assert np.flatnonzero(C.design_cone(d, [v])).tolist() == [int(v)]
    # it is closed under the edges, and no smaller set holding the seeds is: every marked non-seed has a marked in-neighbour
    for src, dst in C.design_edges(d):
        assert (ca[dst][ca[src] != 0] != 0).all()
    fed = np.zeros(d.N, dtype=bool)
    for src, dst in C.design_edges(d):
        fed[dst[ca[src] != 0]] = True
    seeds = np.zeros(d.N, dtype=bool); seeds[a] = True
    assert ((ca != 0) <= (fed | seeds)).all()
    # a level-0 seed reaches beyond its level; `within` cuts the walk
    lv0 = int(d.levels[0][0])
    c0 = C.design_cone(d, [lv0])
    assert c0.sum() > 1
    within = (C.level_of(d) <= 4).astype(np.uint8)
    cw = C.design_cone(d, [lv0], within)
    assert np.array_equal(cw, c0 & within) and cw.sum() < c0.sum()
    # the fan-in cone is the same closure over the reversed edges
    ends = d.path2endpoint[:5]
    fi = C.fanin_cone(d.N, C.design_edges(d), ends)
    assert fi[ends].all() and all((fi[src][fi[dst] != 0] != 0).all() for src, dst in C.design_edges(d))


def test_the_predictor_case_picks_seeds_that_reach_endpoints_and_stay_small():
    d = C.predictor_designs()[0]
    seeds = C.pick_seeds(d, d.path2endpoint)
    assert C.level_of(d)[seeds].tolist() == [1, 6, 11] and len(set(seeds.tolist())) == 3
    cone = C.design_cone(d, seeds)
    assert 0 < cone.sum() <= d.N // 4
    is_end = np.zeros(d.N, dtype=bool); is_end[d.path2endpoint] = True
    assert (cone.astype(bool) & is_end).any()
    e = C.edited(d, seeds, seed=3)
    assert np.flatnonzero((e.cell_feat != d.cell_feat).any(axis=1)).tolist() == sorted(seeds.tolist()) and e.net_feat is d.net_feat


def test_mask_and_diff_cases_hold_what_they_claim():
    for n in (1, 63, 64, 65, 200):
        m = C.mlp_masks(n)
        assert not m['none'].any() and m['all'].all() and all(v.shape == (n,) and v.dtype == np.uint8 for v in m.values())
        nt = (n + 63) // 64
        assert m['one_per_tile'].sum() == nt and all(m['one_per_tile'][t * 64:(t + 1) * 64].sum() == 1 for t in range(nt))
        assert m['last_tile'][(nt - 1) * 64:].all() and not m['last_tile'][:(nt - 1) * 64].any()
    g = C.mlp_masks(200)['gap']
    assert g[:64].all() and not g[64:128].any() and g[128:].all()
    old = np.random.default_rng(0).standard_normal((65, 36)).astype(np.float32)
    for kind in C.DIFF_KINDS:
        o, nw, ch = C.diff_case(kind, old, seed=4)
        assert ch.sum() == (kind in ('one_element', 'zero_sign'))
        if kind == 'zero_sign':
            assert np.array_equal(o, nw) and not np.array_equal(o.view(np.uint32), nw.view(np.uint32))      # equal as floats, not as bits
        if kind == 'same_nan':
            assert np.isnan(o).sum() == 1 and not np.array_equal(o, nw) and np.array_equal(o.view(np.uint32), nw.view(np.uint32))


# ------------------------------------------------------------------------------------------------ the header's ledger
def test_incr_header_parses_is_exported_and_leaves_the_other_headers_alone():
    inc, plc, ext, ref = (_declared(h) for h in ('mmft_incr.h', 'mmft_place.h', 'mmft_report.h', 'mmft.h'))
    decls = lib.incr_decls()
    assert sorted(inc) == NAMES == sorted(decls)
    assert not set(inc) & (set(plc) | set(ext) | set(ref))
    assert lib.header_symbols() == sorted(ref) and sorted(lib.place_decls()) == sorted(plc) and sorted(lib.ext_decls()) == sorted(ext)
    assert {n: len(decls[n][1]) for n in NAMES} == inc == {'mmft_fanout_cone_step': 11, 'mmft_mlp2_feat_fwd_bf16_masked': 15,
                                                           'mmft_update_rows_diff': 11}
    import ctypes
    for n in NAMES:
        res, args = decls[n]
        assert res is ctypes.c_int and args[-2:] == [ctypes.c_int, ctypes.c_void_p]
    # the masked entry point is the unmasked one plus the flags, in front of (device, stream)
    base = lib.header_decls()['mmft_mlp2_feat_fwd_bf16'][1]
    assert decls['mmft_mlp2_feat_fwd_bf16_masked'][1] == base[:-2] + [ctypes.c_void_p] + base[-2:]
    with pytest.raises(RuntimeError, match='not declared'):
        lib.incr('mmft_version')


def test_the_built_library_exports_the_three_symbols_and_refuses_bad_arguments_on_the_host():
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip('needs the built library')
    L = lib.load()
    assert not [n for n in NAMES if not hasattr(L, n)]
    assert L.mmft_version() >= 204
    with pytest.raises(RuntimeError, match=r'mmft_update_rows_diff failed \(-1\)'):
        lib.incr('mmft_update_rows_diff', None, 36, None, 0, 4, 65, None, 36, None, 0, None)            # width above 64
    with pytest.raises(RuntimeError, match=r'mmft_update_rows_diff failed \(-1\)'):
        lib.incr('mmft_update_rows_diff', None, 36, None, 0, 4, 36, None, 36, None, 0, None)            # null pointers
    with pytest.raises(RuntimeError, match=r'mmft_fanout_cone_step failed \(-1\)'):
        lib.incr('mmft_fanout_cone_step', None, 0, 5, None, None, None, None, None, None, 0, None)
    with pytest.raises(RuntimeError, match=r'mmft_mlp2_feat_fwd_bf16_masked failed \(-1\)'):
        lib.incr('mmft_mlp2_feat_fwd_bf16_masked', None, 36, 0, 4, 36, None, None, None, None, None, 128, 0, None, 0, None)
    # n == 0 launches nothing and needs nothing
    assert lib.incr('mmft_fanout_cone_step', None, 0, 0, None, None, None, None, None, None, 0, None) == 0
    assert lib.incr('mmft_update_rows_diff', None, 36, None, 0, 0, 36, None, 36, None, 0, None) == 0


def test_every_incr_call_site_matches_the_header_and_the_kernel_test_names_the_entry_points():
    protos = _declared('mmft_incr.h')
    checked, bad, seen = 0, [], set()
    for name, n, f, lineno in call_sites('incr'):
        if n is None or name == 'mmft_version':                        # (the refusal test above)
            continue
        checked += 1
        seen.add(name)
        if protos.get(name) != n:
            bad.append((name, protos.get(name, 'not declared'), n, f, lineno))
    assert checked >= 6 and seen == set(NAMES) and not bad, bad
    src = open(os.path.join(HERE, 'test_incr_gpu.py')).read()
    assert 'pytestmark = pytest.mark.gpu' in src
    code = _code_only(src)
    for n in ('fanout_cone_mask', 'update_rows_diff', 'mlp2_feat_fwd_bf16'):
        assert re.search(r'(?<![A-Za-z0-9_])' + n + r'(?![A-Za-z0-9_])', code), n


# ------------------------------------------------------------------------------------------------ update(rows=) on the host
def test_check_rows_refuses_duplicates_range_dtype_and_length():
    good = np.array([5, 0, 9], dtype=np.int64)
    out = check_rows(good, 10, {'cell_feat': 3})
    assert out.dtype == np.int64 and out.tolist() == [5, 0, 9]
    assert check_rows(torch.tensor([3, 1]), 4).tolist() == [3, 1]
    assert check_rows(np.zeros(0, dtype=np.int64), 4, {'cell_feat': 0}).size == 0
    assert check_rows(good[::-1], 10).flags['C_CONTIGUOUS']
    with pytest.raises(ValueError, match='distinct'):
        check_rows(np.array([1, 2, 1], dtype=np.int64), 10)
    for bad in (np.array([0, 10], dtype=np.int64), np.array([-1, 3], dtype=np.int64)):
        with pytest.raises(IndexError):
            check_rows(bad, 10)
    for bad in (good.astype(np.int32), good.astype(np.float32), [5, 0, 9], torch.tensor([1, 2], dtype=torch.int32), None):
        with pytest.raises(TypeError):
            check_rows(bad, 10)
    with pytest.raises(ValueError, match='1-D'):
        check_rows(good.reshape(1, 3), 10)
    with pytest.raises(ValueError, match='net_feat has 2 rows for 3'):
        check_rows(good, 10, {'cell_feat': 3, 'net_feat': 2})


def test_update_design_validates_everything_before_it_writes_anything():
    """On a CPU batch: a sparse update whose second array is wrong leaves the first table as it was."""
    from mmft.infer import update_design, design_permutations
    from mmft.train import DesignBatch
    designs = C.predictor_designs((512, 8))
    b = DesignBatch(designs, 'cpu')
    perm = [torch.from_numpy(p) for p in design_permutations(b.old_of_new, b.node_off)]
    cf, nf = b.graph.ndata['cell_feat'], b.graph.ndata['net_feat']
    before = cf.clone(), nf.clone()
    rows = np.array([7, 3, 100], dtype=np.int64)
    new_c = np.full((3, cf.shape[1]), 2.0, dtype=np.float32)
    for kw, exc in ((dict(cell_feat=new_c, net_feat=np.zeros((2, nf.shape[1]), np.float32), rows=rows), ValueError),
                    (dict(cell_feat=new_c, net_feat=np.zeros((3, nf.shape[1]), np.float64), rows=rows), TypeError),
                    (dict(cell_feat=new_c, rows=np.array([7, 7, 1], dtype=np.int64)), ValueError),
                    (dict(cell_feat=new_c, rows=np.array([7, 3, 512], dtype=np.int64)), IndexError),
                    (dict(cell_feat=new_c, rows=rows.astype(np.int32)), TypeError),
                    (dict(cell_feat=new_c[:2], rows=rows), ValueError),
                    (dict(rows=rows), ValueError),
                    (dict(cell_feat=new_c, image=np.zeros((1, 2, 2), np.float32), rows=rows), ValueError)):
        with pytest.raises(exc):
            update_design(b, perm[1], 1, **kw)
        assert torch.equal(cf, before[0]) and torch.equal(nf, before[1])
    # the plain sparse form (incremental=False): index_copy_ of those rows of design 1, nothing else
    update_design(b, perm[1], 1, cell_feat=new_c, rows=rows)
    want = before[0].clone()
    want[perm[1][torch.from_numpy(rows)]] = 2.0
    assert torch.equal(cf, want) and torch.equal(nf, before[1]) and not torch.equal(cf, before[0])
