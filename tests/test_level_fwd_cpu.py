"""The hand-built forward level pair of tests/level_fwd_oracle.py, checked where no GPU is needed: the graph passes the host's
schedule and table builders and holds every edge case it was built for, in every size; the reference is the restatement
(R.pathconv_level) on these levels; the closed form passes every link of `judge` with a tenth of each bound to spare, so the
bounds of the GPU tests are known (and printed) before a kernel runs; and every mistake a forward level kernel could make moves
some link of some class of rows by more than ten times its bound.

Bounds (per class of rows, relative to the class's scale): A / LSE max(2e-5, 4 e_32); hid 2e-6 (fp32 storage) or one bf16
rounding per element; h 2e-6; net rows bit for bit.  Measured e_32 here (the largest class over A and LSE): unit 6.4e-7 (the
heavy rows), wide 1.9e-7 - the floor of 2e-5 is the bound of every class in both regimes.

Which regime shows which defect (WHERE below): every defect but one shows in `unit`; the max that is not subtracted is
mathematically the same softmax and only shows in `wide`, where exp(90) overflows fp32 and the row is NaN."""
import numpy as np
import pytest
import torch

import level_fwd_oracle as O
from mmft import ops
from oracle import restatement as R

# defect -> (regime in which it must show, (link, class) that must move by more than ten bounds there)
WHERE = {
    'drop_tail': ('unit', ('A', 'f5_H')),
    'pre_on_older': ('unit', ('A', 'older')),
    'net_relu_dropped': ('unit', ('net', 'net')),
    'multi_edge_once': ('unit', ('A', 'f2_4')),
    'no_max': ('wide', ('A', 'f2_4')),
    'lse_no_max': ('unit', ('LSE', 'f1')),
    'fanin0_nan': ('unit', ('A', 'f0')),
    'mean': ('unit', ('A', 'f2_4')),
    'A_unrounded': ('unit', ('hid', 'f2_4')),
    'hid_unrounded': ('unit', ('h', 'f2_4')),
    'no_residual': ('unit', ('h', 'f0')),
    'no_final_act': ('unit', ('h', 'f1')),
    'inactive_written': ('unit', ('kept', 'h')),
}


@pytest.fixture(scope='module')
def cases():
    return {(r, s): O.build_case(r, s) for r in O.REGIMES for s in O.SIZES}


@pytest.mark.parametrize('size', O.SIZES)
@pytest.mark.parametrize('regime', O.REGIMES)
def test_hand_built_levels_hold_every_edge_case(cases, regime, size):
    c = cases[(regime, size)]
    rep = O.edge_report(c)
    assert len(rep) >= (54 if size == 'small' else 40) and all(rep.values()), [k for k, v in rep.items() if not v]
    if size == 'small':
        fans = O.cell_fan_in(c)[c.L[4]]
        assert sorted(set(fans[fans > O.SLOT_W].tolist())) == sorted(O.wide_fanins())
    # the three forms read one graph: the slot rows are a sub-range, the wider rows follow, the heavy list is the fold schedule's
    tb = O.tables(c)
    assert tb['max_in'][4] == (max(O.wide_fanins()) if size == 'small' else O.SLOT_W)
    assert c.slot_range[1] + (len(O.wide_fanins()) if size == 'small' else 0) == c.cell_range[1]


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('size', O.SIZES)
@pytest.mark.parametrize('regime', O.REGIMES)
def test_reference_is_the_restatement_on_these_levels(cases, regime, size, relu):
    """R.pathconv_level over level 3 (fc_net_self = identity on net_feat = PRE) and level 4 (fc_cell_self = identity on zero
    features, fc_cell_neigh = identity, no activation: the row is A itself) in fp64: the reference's net rows and A to 1e-12;
    LSE against torch.logsumexp row by row."""
    c = cases[(regime, size)]
    L3, L4 = c.L[3], c.L[4]
    eye = torch.eye(O.D, dtype=torch.float64)
    zero = torch.zeros(O.D, dtype=torch.float64)
    p = {f'{m}layers.0.{w}': t for m in ('fc_net_self.', 'fc_cell_self.', 'fc_cell_neigh.') for w, t in (('weight', eye), ('bias', zero))}
    csr = {'net': c.graph.csr_host('in', 'net'), 'cell': c.graph.csr_host('in', 'cell')}
    h = c.h.double()
    feat0 = torch.zeros((c.N, O.D), dtype=torch.float64)
    h, _ = R.pathconv_level(p, '', csr, h, feat0, c.PRE.double(), c.levels[3], [], 3, activation=relu)
    assert not bool(torch.isnan(h[L3]).any())
    hA, _ = R.pathconv_level(p, '', csr, h.index_fill(0, torch.from_numpy(L4), 0.0), feat0, feat0, c.levels[4], [], 4, activation=False)
    ref = O.reference(c, relu)
    assert O.rel_err(ref['net'], h[L3]) <= 1e-12 and O.rel_err(ref['A'], hA[L4]) <= 1e-12
    ip, ix = csr['cell']
    for v in (L4 if size == 'small' else L4[:200]):
        src = ix[ip[v]:ip[v + 1]]
        want = torch.logsumexp(h[src], 0) if src.size else torch.zeros(O.D, dtype=torch.float64)
        assert float((ref['LSE'][v - L4[0]] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
        if src.size == 0:
            assert float(ref['A'][v - L4[0]].abs().max()) == 0.0
    # under the cone mask nothing inside the mask changes, and nothing inside it is NaN
    refa = O.reference(c, relu, c.active)
    on = c.active.bool().numpy()[L4]
    assert torch.equal(refa['A'][on], ref['A'][on]) and torch.equal(refa['LSE'][on], ref['LSE'][on])


@pytest.mark.parametrize('hid16', [True, False])
@pytest.mark.parametrize('masked', [True, False])
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('regime', O.REGIMES)
def test_closed_form_passes_every_link_and_bounds_are_known(cases, regime, relu, masked, hid16):
    """The closed form, written as a launch, sits inside a tenth of every bound (bf16-stored hid: inside the bound, its
    rounding IS the bound), every class is there, and e_32 leaves the floor TOL in charge in `unit`."""
    c = cases[(regime, 'small')]
    active = c.active if masked else None
    before, after = O.formula(c, relu, active, hid16=hid16)
    ratios = O.judge(c, before, after, relu, active, c.net_range, c.L[4], tag=f'closed form {regime} relu={int(relu)} cone={int(masked)}')
    assert {'f0', 'f1', 'f2_4', 'f5_H', 'heavy', 'older'} == {k[1] for k in ratios if k[0] == 'A'}
    for k, v in ratios.items():
        assert v <= (1.0 if (hid16 and k[0] == 'hid') else 0.1), (k, v)
    ref, ref32 = O.references(c, relu, active)
    for name in ('A', 'LSE'):
        for k, rows in O.row_classes(c, c.L[4], active).items():
            e32 = O.rel_err(ref32[name][rows - c.L[4][0]], ref[name][rows - c.L[4][0]])
            print(f'{regime} relu={relu} cone={masked} {name} {k}: rows {rows.size} e_32 {e32:.1e}')
            assert e32 < 1e-5
            if regime == 'unit':
                assert e32 < O.TOL / O.E32_MARGIN
    if masked:
        off = c.L[3][~c.active.bool().numpy()[c.L[3]]]
        assert off.size and bool(torch.isnan(after['h'][off]).all())
    else:
        assert not bool(torch.isnan(after['h']).any())


def test_closed_form_on_sub_ranges_and_the_slot_rows(cases):
    """What the GPU file launches the slot form over: the slot rows, and their first 1, 15, 16, 17 and 33."""
    c = cases[('unit', 'small')]
    s0, ns = c.slot_range
    for n in O.SUB_COUNTS + (ns,):
        rows = np.arange(s0, s0 + n)
        for active in (c.active, None):
            before, after = O.formula(c, True, active, cell_rows=rows)
            assert not O.failures(O.judge(c, before, after, True, active, c.net_range, rows))
        # ... and judged against another row set the launch is caught: a row too many was written, or one too few
        assert O.failures(O.judge(c, before, after, True, None, c.net_range, rows[:-1]))
        if n < ns:
            assert O.failures(O.judge(c, before, after, True, None, c.net_range, np.arange(s0, s0 + n + 1)))


@pytest.mark.parametrize('defect', O.DEFECTS)
def test_checks_have_teeth(cases, defect):
    """One mistake at a time in the closed form: some link of some class moves by more than 10 bounds, in the regime and at
    the link WHERE records (hid in fp32 storage: the bf16 form's bound is a whole rounding).  Without the defect nothing
    moves (the test above)."""
    assert set(WHERE) == set(O.DEFECTS)
    hit = {}
    for regime in O.REGIMES:
        c = cases[(regime, 'small')]
        active = c.active if defect == 'inactive_written' else None
        before, after = O.formula(c, True, active, defect=defect)
        ratios = O.judge(c, before, after, True, active, c.net_range, c.L[4])
        hit[regime] = {k: v for k, v in ratios.items() if v > 10}
        print(defect, regime, {f'{k[0]} {k[1]}': f'{v:.3g}' for k, v in hit[regime].items()})
    regime, key = WHERE[defect]
    assert key in hit[regime], (defect, hit)
    if defect == 'no_max':
        assert not hit['unit']                                   # the same softmax on paper: only an overflow shows it


def test_wide_fan_ins_are_written_in_the_kernels_terms():
    H = ops.PAIR_HEAVY_IN
    fans = O.wide_fanins()
    assert fans == sorted(fans) and fans[0] == O.SLOT_W + 1 and H in fans and H + 1 in fans and fans[-1] == 200
    assert sum(f > H for f in fans) == 4 and sum(f <= H for f in fans) == 4
