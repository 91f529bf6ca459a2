"""Sensitivity without a GPU: the ledger of include/mmft_sens.h (the rules test_head_mlp_cpu.py applies to
include/mmft_head.h), the host-side refusals of its entry point - every one of them comes before the device is looked at -
the reference gradient of tests/sens_oracle.py against central differences, its exactly-zero rows, and the refusals of
mmft.sensitivity that need no device."""
import ctypes

import numpy as np
import pytest
import torch

from abi_ledger import call_sites, declared as _declared, others
from mmft import lib
from sens_oracle import level_parity_rows, oracle_sensitivity

NAMES = ['mmft_mlp2_feat_dx_bf16']
NARGS = {'mmft_mlp2_feat_dx_bf16': 14}
# the other headers' ledgers, as their own tests pin them
PINNED = {'mmft_report.h': ['mmft_timing_report', 'mmft_timing_report_workspace_bytes'],
          'mmft_head.h': ['mmft_head_mlp_bwd', 'mmft_head_mlp_fwd', 'mmft_head_mlp_supported', 'mmft_head_mlp_workspace_bytes'],
          'mmft_crit_sums.h': ['mmft_criticality_sums', 'mmft_criticality_sums_workspace_bytes']}


def test_sens_header_declares_exactly_the_new_name_and_overlaps_no_other_header():
    hd = _declared('mmft_sens.h')
    decls = lib.sens_decls()
    assert sorted(hd) == NAMES == sorted(decls)
    assert {n: len(decls[n][1]) for n in NAMES} == hd == NARGS
    assert not set(hd) & set(_declared('mmft.h')) and 'mmft_mlp2_feat_bwd_bf16' in _declared('mmft.h')
    assert set(PINNED) < set(others('mmft_sens.h'))
    for other in others('mmft_sens.h'):
        theirs = _declared(other)
        assert not set(hd) & set(theirs), other
        assert other not in PINNED or sorted(theirs) == PINNED[other], other
    res, args = decls['mmft_mlp2_feat_dx_bf16']
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    assert res is I and args == [P, LL, P, LL, I, I, I, P, P, P, P, LL, I, P]
    with pytest.raises(RuntimeError, match='not declared'):
        lib.sens('mmft_version')
    with pytest.raises(RuntimeError, match='not declared'):
        lib.sens('mmft_mlp2_feat_bwd_bf16')
    # the accessor's name is its own: the ledgers match call sites by attribute name
    assert lib.sens not in (lib.call, lib.query, lib.ext, lib.place, lib.incr, lib.crit, lib.head, lib.csum)


def test_every_sens_call_site_matches_the_header():
    protos = _declared('mmft_sens.h')
    checked, bad, seen = 0, [], set()
    for name, n, f, lineno in call_sites('sens'):
        if n is None or name in ('mmft_version', 'mmft_mlp2_feat_bwd_bf16'):         # (a list built elsewhere; the refusal test above)
            continue
        checked += 1
        seen.add(name)
        if protos.get(name) != n:
            bad.append((name, protos.get(name, 'not declared'), n, f, lineno))
    assert checked >= 1 and seen == set(NAMES) and not bad, bad


def _dx(**change):
    """A full argument list of mmft_mlp2_feat_dx_bf16 made of host integers: nothing can be launched on it, and nothing is."""
    a = dict(g=64, ldg=128, x=64, ldx=36, row0=3, n=5, fin=36, w1=64, b1=64, w2=64, dx=64, lddx=36, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def test_the_built_library_exports_the_name_and_refuses_bad_arguments_on_the_host():
    L = lib.load()
    assert not [n for n in NAMES if not hasattr(L, n)]
    assert L.mmft_version() >= 208
    assert len(_dx()) == NARGS['mmft_mlp2_feat_dx_bf16']
    refused = dict(null_g=dict(g=None), null_x=dict(x=None), null_w1=dict(w1=None), null_b1=dict(b1=None), null_w2=dict(w2=None),
                   null_dx=dict(dx=None), n_neg=dict(n=-1), row0_neg=dict(row0=-1), rows_beyond_int=dict(row0=(1 << 31) - 3),
                   fin0=dict(fin=0, ldx=0, lddx=0), fin65=dict(fin=65, ldx=65, lddx=65), short_x_pitch=dict(ldx=35),
                   short_dx_pitch=dict(lddx=35), short_g_pitch=dict(ldg=124), odd_g_pitch=dict(ldg=130), odd_g=dict(g=68),
                   odd_b1=dict(b1=72))
    for what, change in refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_mlp2_feat_dx_bf16 failed \(-1\): mlp2_feat_dx_bf16'):
            lib.sens('mmft_mlp2_feat_dx_bf16', *_dx(**change))
    # n == 0 returns 0 and needs nothing - but its sizes are still judged
    assert lib.sens('mmft_mlp2_feat_dx_bf16', *_dx(n=0)) == 0
    assert lib.sens('mmft_mlp2_feat_dx_bf16', *_dx(n=0, g=None, x=None, w1=None, b1=None, w2=None, dx=None)) == 0
    with pytest.raises(RuntimeError, match='bad sizes'):
        lib.sens('mmft_mlp2_feat_dx_bf16', *_dx(n=0, fin=65, ldx=65, lddx=65))


# ------------------------------------------------------------------------------------------------ the reference gradient
SEED = 9294


@pytest.fixture(scope='module')
def case():
    """The two designs of tests/test_sens_gpu.py, host weights of a freshly initialised model, a seeded feature map and
    seeded normal weights over all 56 paths; the plain fp64 reference of each design, computed once."""
    from mmft.synth import synth_design
    from mmft.train import build_models
    designs = {f: synth_design(N=2048, L=16, tile=32, seed=SEED, fanin=f) for f in ('regular', 'irregular')}
    pmodel, _ = build_models(map_size=designs['regular'].map_size, device='cpu', seed=SEED, unet=False)
    state = {k: v.detach().clone() for k, v in pmodel.state_dict().items()}
    out = {}
    for f, d in designs.items():
        fm = torch.rand(d.map_size ** 2, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
        w = torch.randn(d.num_paths, generator=torch.Generator().manual_seed(12), dtype=torch.float64)
        ids = list(range(d.num_paths))
        out[f] = dict(d=d, fm=fm, w=w, ids=ids, ref=oracle_sensitivity(d, ids, state, fm, w))
    out['state'] = state
    return out


def test_reference_gradient_agrees_with_central_differences(case):
    """Plain fp64, step 1e-6, the regular design: for four non-zero rows each of the cell and the net gradient, the row's
    largest entry agrees with the central difference of J to 1e-6 of the gradient's max norm (measured where the issue was
    written: 6e-9 and 3e-9; the bar leaves two orders of margin for another platform's libm)."""
    c, state = case['regular'], case['state']
    d, ref, eps = c['d'], c['ref'], 1e-6
    assert ref['pred'].numel() == d.num_paths == 56

    def J(**feat):
        o = oracle_sensitivity(d, c['ids'], state, c['fm'], c['w'], **feat)
        return float((o['pred'] * c['w']).sum())

    for key, base, name in (('cell', d.cell_feat, 'cell_feat'), ('net', d.net_feat, 'net_feat')):
        g = ref[key]
        scale = float(g.abs().max())
        nz = torch.nonzero(g.abs().amax(1) > 0).reshape(-1)
        assert scale > 0 and nz.numel() >= 4
        worst = 0.0
        for r in nz[torch.linspace(0, nz.numel() - 1, 4).long()].tolist():
            k = int(g[r].abs().argmax())
            up, dn = np.array(base, dtype=np.float64), np.array(base, dtype=np.float64)
            up[r, k] += eps
            dn[r, k] -= eps
            fd = (J(**{name: up}) - J(**{name: dn})) / (2 * eps)
            worst = max(worst, abs(fd - float(g[r, k])) / scale)
        print(f'{key}: central difference vs gradient, worst of four rows {worst:.2e}')
        assert worst < 1e-6, (key, worst)


@pytest.mark.parametrize('fanin', ['regular', 'irregular'])
def test_reference_gradient_is_exactly_zero_on_rows_of_the_other_parity(case, fanin):
    """cell_feat is read by the even levels only and net_feat by the odd ones: the other rows are exactly 0."""
    c = case[fanin]
    even, odd = level_parity_rows(c['d'])
    assert even.size and odd.size and even.size + odd.size == c['d'].N
    ref = c['ref']
    assert float(ref['cell'][odd].abs().max()) == 0.0 and float(ref['net'][even].abs().max()) == 0.0
    assert float(ref['cell'][even].abs().max()) > 0.0 and float(ref['net'][odd].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ host-side refusals
def test_sensitivity_refuses_on_the_host_what_it_cannot_differentiate():
    """mmft.sensitivity's checks are functions that touch no device, as infer.check_rows is: Sensitivity.__init__ and run()
    call them before anything is launched."""
    import model as M
    from mmft import gradsink, sensitivity as S
    from mmft.train import build_models
    pm, _ = build_models(map_size=16, device='cpu', seed=SEED, unet=False)
    S.check_model(pm)
    with pytest.raises(ValueError, match='no netlist branch'):
        S.check_model(M.PathModel(None, None, pm.fcn, None, None, pm.mlp_fuse))
    attn = M.PathConv(out_feat_dim=128, hidden_feat_dim=128, cell_feat_dim=36, net_feat_dim=2, flag_attn=True, num_heads=1)
    with pytest.raises(ValueError, match='flag_attn'):
        S.check_model(M.PathModel(attn, None, pm.fcn, None, None, pm.mlp_fuse))
    with pytest.raises(ValueError, match='nlabels = 1'):
        S.check_model(M.PathModel(pm.gnn, None, pm.fcn, None, None, M.MLP(288, 576, 2)))
    p = pm.mlp_fuse.layers[0].weight
    gradsink.attach(p, torch.zeros_like(p))
    try:
        with pytest.raises(RuntimeError, match='gradient sinks'):
            S.check_model(pm)
        with pytest.raises(RuntimeError, match='gradient sinks'):
            S.Sensitivity(pm, None, [], 'cpu')                       # the first thing the constructor does
    finally:
        gradsink.detach(p)
    S.check_model(pm)
    # weights and objective
    assert S.check_weights(None, 5) is None
    w = S.check_weights(np.ones(5, dtype=np.float32), 5)
    assert torch.is_tensor(w) and w.dtype == torch.float32 and w.shape == (5,)
    assert S.check_weights(torch.ones(5), 5).shape == (5,)
    for bad in (np.ones(5), torch.ones(5, dtype=torch.float64), torch.ones(5, dtype=torch.int32)):
        with pytest.raises(TypeError, match='float32'):
            S.check_weights(bad, 5)
    with pytest.raises(TypeError, match='numpy array or a tensor'):
        S.check_weights([1.0] * 5, 5)
    for bad in (torch.ones(4), torch.ones(6), torch.ones(5, 1), torch.ones(())):
        with pytest.raises(ValueError, match='one weight per predicted path'):
            S.check_weights(bad, 5)
    assert S.check_objective('tns') == 'tns' and S.check_objective('sum') == 'sum'
    for bad in ('wns', None, 'TNS'):
        with pytest.raises(ValueError, match='unknown objective'):
            S.check_objective(bad)
