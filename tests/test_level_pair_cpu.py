"""The hand-built level pair of tests/level_pair_oracle.py, checked where no GPU is needed: the graph passes the host's
schedule and table builders and holds every edge case it was built for, the closed form agrees with the autograd reference,
the bounds of the GPU tests are known (and printed) before a kernel runs, and every mistake a reverse level kernel could
make moves some class of rows by more than ten times that class's bound.

Bounds (max |G - ref| / max |ref| per class of rows): max(5e-5, 4 e_32).  Measured e_32 here, the largest class per regime
(relu on / off): unit 1.5e-7 / 2.6e-7, wide 2.8e-6 / 2.8e-6 - the floor of 5e-5 is the bound of every class in both regimes.
Rounding LSE to bf16 moves the classes with consumers by 33 .. 94 bounds in `unit` and by 1100 .. 2000 in `wide` (39 for the
one sink with 17 consumers, whose rows stay in the unit range): it has teeth in both."""
import numpy as np
import pytest
import torch

import level_pair_oracle as O
from mmft import ops
from mmft.pingraph import PinGraph

REGIMES = ('unit', 'wide')


@pytest.fixture(scope='module')
def cases():
    return {r: O.build_case(r) for r in REGIMES}


@pytest.mark.parametrize('regime', REGIMES)
def test_hand_built_pair_holds_every_edge_case(cases, regime):
    c = cases[regime]
    assert c.graph.level_set_is_complete(c.levels)
    rep = O.edge_report(c)
    assert len(rep) >= 40 and all(rep.values()), [k for k, v in rep.items() if not v]
    # the heavy lists of the two pulls: every row above the threshold and none at it
    deg = np.diff(c.graph.csr_host('out', 'net')[0]) + np.diff(c.graph.csr_host('out', 'cell')[0])
    for rows in (c.drv, c.snk):
        hv = O.heavy_rows(c, rows).numpy()
        assert hv.size and (deg[hv] > ops.PAIR_HEAVY_OUT).all() and (deg[np.setdiff1d(rows, hv)] <= ops.PAIR_HEAVY_OUT).all()
        meta = c.graph.level_meta(0 if rows is c.drv else 1, rows.tolist())
        assert meta['heavy_out'].tolist() == hv.tolist() and meta['range'] == (int(rows[0]), rows.size)


def test_whole_tiles_switch_leaves_no_parts(cases):
    """The switch test 5 of the GPU file uses: with the sink budget raised no driver is cut into parts."""
    c = cases['unit']
    sinks0 = PinGraph.BWD_PAIR_TILE_SINKS
    try:
        PinGraph.BWD_PAIR_TILE_SINKS = 1 << 30
        tiles = c.graph.level_bwd_pairs([list(l) for l in c.levels])[1][0]['tiles'].numpy()
    finally:
        PinGraph.BWD_PAIR_TILE_SINKS = sinks0
    assert (tiles[:, 3] == 0).all() and int(tiles[:, 1].sum()) == c.drv.size
    # the 17-driver tile is still there, and a tile now walks its sinks in several rounds of the kernel's 32-row LDS buffer
    assert any(t[1] == O.PAIR_GROUPS + 1 for t in tiles) and int((tiles[:, 7] - tiles[:, 6]).max()) > 2 * PinGraph.BWD_PAIR_PART + 1
    assert int((tiles[:, 7] - tiles[:, 6]).sum()) == c.snk.size


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('regime', REGIMES)
def test_closed_form_agrees_with_autograd_and_bounds_are_known(cases, regime, relu):
    """The closed form the kernels evaluate, in fp64 from fp32 A / LSE, sits inside every class's bound of the autograd
    reference (so handing the kernels fp32 A / LSE costs nothing that matters), also under the cone mask and at D = 16."""
    c = cases[regime]
    for active, width in ((None, O.D), (c.active, O.D), (None, 16)):
        ref, classes, e32, bound = O.g_bounds(c, relu, active, width)
        err = O.class_errors(O.formula(c, relu, active, width=width), ref, classes)
        for k in classes:
            print(f'{regime} relu={relu} active={active is not None} D={width} {k}: rows {classes[k].size} e_32 {e32[k]:.1e} '
                  f'bound {bound[k]:.1e} closed form {err[k]:.1e}')
            assert err[k] < bound[k] / 10 and e32[k] < 1e-5, k
        assert {'sink_c0', 'sink_c1', 'sink_c4', 'sink_c5', 'sink_c9', 'drv_0', 'drv_whole', 'drv_heavy'} <= set(classes)
        if active is not None:
            off = ~active.bool()
            assert float(ref[off].abs().max()) == 0.0


@pytest.mark.parametrize('defect', O.DEFECTS)
def test_reference_has_teeth(cases, defect):
    """One mistake at a time in the closed form: some class moves by more than 10 bounds in at least one regime (the bf16 LSE
    must do so in `wide`; whether it also does in `unit` is printed)."""
    hit = {}
    for regime in REGIMES:
        c = cases[regime]
        active = c.active if defect == 'inactive_counted' else None
        ref, classes, _, bound = O.g_bounds(c, True, active)
        err = O.class_errors(O.formula(c, True, active, defect=defect), ref, classes)
        hit[regime] = {k: err[k] / bound[k] for k in classes if err[k] > 10 * bound[k]}
        print(defect, regime, {k: f'{v:.0f}' for k, v in hit[regime].items()})
    assert hit['wide'] if defect == 'lse_bf16' else (hit['unit'] or hit['wide'])
    where = {'drop_tail': 'sink_c5', 'drop_last_part': 'drv_heavy', 'own_ignored': 'drv_0'}.get(defect)
    if where:
        assert where in hit['unit'] and where in hit['wide']
    if defect == 'drop_last_part':
        assert set(hit['unit']) == {'drv_heavy'}                   # nothing else may move


@pytest.mark.parametrize('regime', REGIMES)
def test_reference_activation_is_relu_where_relu_is_defined(cases, regime):
    """The reference keeps the value of an entry h <= 0 and stops its gradient (the kernels are handed h and use its sign).  On
    inputs a real forward could have produced - h >= 0 - that is torch.relu: the two references agree bit for bit."""
    import copy
    c = copy.copy(cases[regime])
    c.h = cases[regime].h.clamp_min(0.0)
    assert float((c.h == 0).float().mean()) > 0.2
    for active in (None, c.active):
        assert torch.equal(O.reference(c, True, active), O.reference(c, True, active, plain_relu=True))


def test_mlp_reference_is_the_masked_two_layer_product(cases):
    c = cases['unit']
    Gd = O.reference(c)[c.drv].float()
    dhn, da = O.mlp_reference(c, Gd, torch.zeros(c.drv.size, O.HID))
    assert dhn.shape == (c.drv.size, O.HID) and float(da.abs().max()) == 0.0
    assert float(dhn[c.HN[c.drv] <= 0].abs().max()) == 0.0 and float(dhn.abs().max()) > 0
    # bf16-representable weights: rounding them again is the identity
    assert torch.equal(O.B.r(c.W1g), c.W1g) and torch.equal(O.B.r(c.W2g), c.W2g) and torch.equal(O.B.r(c.HN), c.HN)
