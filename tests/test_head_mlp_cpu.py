"""The fused fusion-head MLP without a GPU: the ledger of include/mmft_head.h (the rules test_crit_cpu.py applies to
include/mmft_crit.h), the host-side refusals of its two launching entry points - every one of them comes before the device is
looked at - and the gate that decides which shapes take the fused path."""
import ctypes

import pytest
import torch

from abi_ledger import call_sites, declared as _declared, others
from mmft import lib

NAMES = ['mmft_head_mlp_bwd', 'mmft_head_mlp_fwd', 'mmft_head_mlp_supported', 'mmft_head_mlp_workspace_bytes']
NARGS = {'mmft_head_mlp_bwd': 21, 'mmft_head_mlp_fwd': 14, 'mmft_head_mlp_supported': 3, 'mmft_head_mlp_workspace_bytes': 1}
OTHERS = others('mmft_head.h')


def test_head_header_declares_exactly_the_new_names_and_overlaps_no_other_header():
    hd = _declared('mmft_head.h')
    decls = lib.head_decls()
    assert sorted(hd) == NAMES == sorted(decls)
    assert {n: len(decls[n][1]) for n in NAMES} == hd == NARGS
    for other in OTHERS:
        assert not set(hd) & set(_declared(other)), other
    for n in ('mmft_head_mlp_fwd', 'mmft_head_mlp_bwd'):
        res, args = decls[n]
        assert res is ctypes.c_int and args[-2:] == [ctypes.c_int, ctypes.c_void_p]
    assert decls['mmft_head_mlp_workspace_bytes'] == (ctypes.c_longlong, [ctypes.c_longlong])
    assert decls['mmft_head_mlp_supported'] == (ctypes.c_longlong, [ctypes.c_int] * 3)
    with pytest.raises(RuntimeError, match='not declared'):
        lib.head('mmft_version')
    # the accessor's name is its own: the ledgers match call sites by attribute name
    assert lib.head not in (lib.call, lib.query, lib.ext, lib.place, lib.incr, lib.crit)


def test_every_head_call_site_matches_the_header():
    protos = _declared('mmft_head.h')
    checked, bad, seen = 0, [], set()
    for name, n, f, lineno in call_sites('head'):
        if n is None or name == 'mmft_version':                        # (a list built elsewhere; the refusal test above)
            continue
        checked += 1
        seen.add(name)
        if protos.get(name) != n:
            bad.append((name, protos.get(name, 'not declared'), n, f, lineno))
    assert checked >= 6 and seen == set(NAMES) and not bad, bad


def _fwd(**change):
    """A full argument list of mmft_head_mlp_fwd made of host integers: nothing can be launched on it, and nothing is."""
    a = dict(x=64, ldx=288, w1=64, b1=64, w2=64, b2=64, hid=64, pred=64, T=5, inn=288, hidden=576, out=1, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def _bwd(**change):
    a = dict(dpred=64, hid=64, x=64, ldx=288, w1=64, w2=64, dx=64, lddx=288, dw1=64, db1=64, dw2=64, db2=64, T=5, inn=288, hidden=576,
             out=1, accumulate=0, workspace=64, workspace_bytes=1 << 30, device=0, stream=None)
    assert not set(change) - set(a)
    a.update(change)
    return list(a.values())


def test_the_built_library_exports_the_names_and_refuses_bad_arguments_on_the_host():
    L = lib.load()
    assert not [n for n in NAMES if not hasattr(L, n)]
    assert L.mmft_version() >= 206
    assert len(_fwd()) == NARGS['mmft_head_mlp_fwd'] and len(_bwd()) == NARGS['mmft_head_mlp_bwd']
    need = lib.head('mmft_head_mlp_workspace_bytes', 5)
    fwd_refused = dict(null_x=dict(x=None), null_w1=dict(w1=None), null_b2=dict(b2=None), null_pred=dict(pred=None),
                       T0=dict(T=0), T_neg=dict(T=-3), T_above=dict(T=(1 << 24) + 1),
                       wrong_in=dict(inn=256), wrong_hidden=dict(hidden=512), two_labels=dict(out=2),
                       odd_x=dict(x=68), odd_pitch=dict(ldx=290), short_pitch=dict(ldx=284), odd_w1=dict(w1=72), odd_hid=dict(hid=66))
    for what, change in fwd_refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_head_mlp_fwd failed \(-1\): head_mlp_fwd'):
            lib.head('mmft_head_mlp_fwd', *_fwd(**change))
    bwd_refused = dict(null_dpred=dict(dpred=None), null_hid=dict(hid=None), null_x=dict(x=None), null_dw1=dict(dw1=None),
                       null_db2=dict(db2=None), T0=dict(T=0), T_neg=dict(T=-1),
                       wrong_in=dict(inn=128), wrong_hidden=dict(hidden=256), two_labels=dict(out=2),
                       odd_x=dict(x=68), odd_pitch=dict(ldx=289), odd_dx=dict(dx=72), odd_dx_pitch=dict(lddx=290), short_dx_pitch=dict(lddx=280),
                       odd_hid=dict(hid=72), odd_dw1=dict(dw1=68),
                       null_workspace=dict(workspace=None), odd_workspace=dict(workspace=72), short_workspace=dict(workspace_bytes=need - 1))
    for what, change in bwd_refused.items():
        with pytest.raises(RuntimeError, match=r'mmft_head_mlp_bwd failed \(-1\): head_mlp_bwd'):
            lib.head('mmft_head_mlp_bwd', *_bwd(**change))


def test_workspace_query_and_the_shape_gate():
    # [W1^T bf16 pack | 1156 floats per 64-row tile | one 576 x 288 slab per row share]
    pack, part, slab = 288 * 576 * 2, 4 * (2 * 576 + 4), 4 * 576 * 288
    assert lib.head('mmft_head_mlp_workspace_bytes', 1) == pack + part + slab
    assert lib.head('mmft_head_mlp_workspace_bytes', 64) == pack + part + slab
    assert lib.head('mmft_head_mlp_workspace_bytes', 65) == pack + 2 * part + slab
    assert lib.head('mmft_head_mlp_workspace_bytes', 257) == pack + 5 * part + 2 * slab          # 9 chunks of 32 rows: shares of 5 and 4
    assert lib.head('mmft_head_mlp_workspace_bytes', 10800) == pack + 169 * part + 26 * slab     # 338 chunks in shares of 13
    for bad in (0, -5, (1 << 24) + 1):
        with pytest.raises(RuntimeError, match='head_mlp_workspace_bytes'):
            lib.head('mmft_head_mlp_workspace_bytes', bad)
    assert lib.head('mmft_head_mlp_supported', 288, 576, 1) == 1
    for shape in ((288, 576, 2), (288, 512, 1), (256, 576, 1), (576, 288, 1), (1, 64, 32), (128, 256, 128), (0, 0, 0)):
        assert lib.head('mmft_head_mlp_supported', *shape) == 0, shape


def test_the_gate_keeps_every_other_case_on_the_layer_path():
    """head_mlp_usable is what model.MLP.forward asks.  Without a GPU only its first answer can be seen: CPU tensors keep the
    generic layers, whose refusal stays what it was.  f32 mode, LeakyReLU, other shapes and the switch are in
    tests/test_head_mlp_gpu.py (test_only_the_bf16_relu_288_576_1_case_takes_the_fused_kernels)."""
    import model
    from mmft import functional as MF
    lib.load()
    m = model.MLP(288, 576, 1)
    l0, l2 = m.layers[0], m.layers[2]
    x = torch.zeros(4, 288)
    with lib.math_mode('bf16'):
        assert not MF.head_mlp_usable(x, l0.weight, l0.bias, l2.weight, l2.bias, 0)            # CPU tensors
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            m(x)
    assert MF.FUSED_HEAD_MLP is True
