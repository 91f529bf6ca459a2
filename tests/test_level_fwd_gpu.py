"""The forward level kernels - level_fwd_slots_kernel<RB, KEEP> (the kernel bench.py times), level_fwd_bf16_kernel<KEEP>
(csrc/mlp2_bf16.hip), pair_fwd_gather_kernel<FAST> with its whole-workgroup heavy path (csrc/graph.hip) followed by
mlp2_rows_bf16_kernel, and csrc/fold_gather.h under all of them - against the fp64 reference of ONE hand-built level pair
(tests/level_fwd_oracle.py: what the graph holds, how the reference is formed, what `judge` checks;
tests/test_level_fwd_cpu.py: that `judge` notices a kernel's mistakes).  The kernels are called through their ops wrappers.

Every launch is judged link by link (O.judge): the net rows bit for bit; A and LSE per class of rows (fan-in 0, 1, 2-4,
5-HEAVY_IN, heavy; rows with an older-level edge) at max(2e-5, 4 e_32) of the class's scale; hid given the kernel's own A at
2e-6 (fp32 storage) or one bf16 rounding per element; h given the kernel's own hid at 2e-6; every row outside the launch keeps
its bits (h, PRE, A, LSE, hid; the sentinel fills and the NaN rows of h are plain inputs) and no net row inside the mask stays
NaN.  No bound comes from a kernel's output.

MMFT_FWD_RB is read once per process by the launcher: the tests assert it unset and leave it so; two row blocks per workgroup
are reached through the sizes (6144 rows in either level).

Measured on an MI355X (e_hip, the largest class and case of a kind; the per-class table is in DESIGN 3.4b):
  link   bound        slots              fused (index)      gather + MLP (the larger of the two math modes)
  A      2e-5         2.4e-7 / 1.6e-7    7.7e-7 / 2.5e-7    2.5e-7 / 2.5e-7         (unit / wide; e_32 at most 6.4e-7)
  LSE    2e-5         8.9e-8 / 7.5e-8    1.9e-7 / 9.0e-8    1.3e-7 / 9.1e-8
  hid    2e-6 (fp32)  1.6e-7 / 1.2e-7    1.3e-7 / 8.8e-8    1.3e-7 / 8.3e-8
  h      2e-6         1.2e-7 / 1.3e-7    9.8e-8 / 1.4e-7    9.8e-8 / 1.4e-7
hid stored as bf16 sits inside one rounding per element in every case (3.3e-3 of the class scale at most).  The fused
kernel's 7.7e-7 is the row of 200 in-edges walked by one thread group; the gather's heavy path is at 2e-7 there.  The branch
of fold_gather_edges without the per-edge driver table shows the same figures but not the same bits as the batched one (last
bits of A on rows of two and more edges), so the two are judged separately and not held to each other.
The 86 cases take 3.5 s together with the module fixture; no case takes more than 0.1 s.
"""
import os

import numpy as np
import pytest
import torch

import level_fwd_oracle as O
from mmft import lib, ops

pytestmark = pytest.mark.gpu
KEPT = ('h', 'A', 'LSE', 'hid')


@pytest.fixture(scope='module')
def cases(dev):
    """Every (regime, size) on the device with its tables; every edge case asserted present from those tables."""
    assert 'MMFT_FWD_RB' not in os.environ
    out = {}
    for regime in O.REGIMES:
        for size in O.SIZES:
            c = O.build_case(regime, size)
            c.g = c.graph.to(dev)
            rep = O.edge_report(c, c.g)
            assert len(rep) >= (54 if size == 'small' else 40) and all(rep.values()), [k for k, v in rep.items() if not v]
            c.tb = O.tables(c, c.g)
            c.w = (ops.pack_bf16(c.W1.to(dev)), c.b1.to(dev), ops.pack_bf16(c.W2.to(dev)), c.b2.to(dev))
            assert torch.equal(c.w[0].float().cpu(), c.W1) and torch.equal(c.w[2].float().cpu(), c.W2)
            c.active_d = c.active.to(dev)
            out[(regime, size)] = c
    return out


def fresh(c, dev, hid16):
    return {k: v.to(dev) for k, v in O.inputs(c, hid16).items()}


def host(t):
    return {k: v.cpu() for k, v in t.items()}


def check(c, t, relu, masked, net_range, cell_rows, tag, links=('net', 'A', 'LSE', 'hid', 'h')):
    hid16 = t['hid'].dtype == torch.bfloat16
    ratios = O.judge(c, O.inputs(c, hid16), host(t), relu, c.active if masked else None, net_range, cell_rows, links=links, tag=tag)
    assert not O.failures(ratios), (tag, O.failures(ratios))


def bitwise(x, y, names=KEPT, rows=None, tag=''):
    for k in names:
        a, b = x[k].cpu(), y[k].cpu()
        assert O.same_bits(a, b) if rows is None else O.same_bits(a[rows], b[rows]), (tag, k)


def run_slots(c, t, relu, masked, cell_range, infer=False):
    a = c.active_d if masked else None
    with lib.math_mode('bf16'):
        if infer:
            ops.level_fwd_slots_infer(t['h'], t['PRE'], c.tb['slots'], c.tb['net_drv'], c.net_range, cell_range, *c.w, relu=relu, active=a)
        else:
            ops.level_fwd_slots(t['h'], t['PRE'], c.tb['slots'], c.tb['net_drv'], c.net_range, cell_range, t['A'], t['LSE'], *c.w,
                                t['hid'], relu=relu, active=a)
        torch.cuda.synchronize()


def run_index(c, t, relu, masked, cell_rows, drv=True, infer=False):
    a = c.active_d if masked else None
    d = c.tb['drv'] if drv else None
    with lib.math_mode('bf16'):
        if infer:
            ops.level_fwd_bf16_infer(t['h'], t['PRE'], c.tb['in_net'], c.tb['in_cell'], c.net_range, cell_rows, *c.w, relu=relu,
                                     active=a, in_cell_driver=d)
        else:
            ops.level_fwd_bf16(t['h'], t['PRE'], c.tb['in_net'], c.tb['in_cell'], c.net_range, cell_rows, t['A'], t['LSE'], *c.w,
                               t['hid'], relu=relu, active=a, in_cell_driver=d)
        torch.cuda.synchronize()


def run_two_kernels(c, t, relu, masked, cell_range, mode, heavy=True, drv=True, mlp=True):
    """mmft_pair_fwd_gather in the given math mode (f32: expf / logf; bf16: the hardware's exp2 / log2), then mmft_mlp2_rows_bf16."""
    a = c.active_d if masked else None
    rows = torch.arange(cell_range[0], cell_range[0] + cell_range[1], dtype=torch.int32, device=t['h'].device)
    with lib.math_mode(mode):
        ops.pair_fwd_gather(t['h'], t['PRE'], c.tb['in_net'], c.tb['in_cell'], c.net_range, cell_range, t['A'], t['LSE'], relu=relu,
                            heavy=c.tb['heavy'] if heavy else None, active=a, in_cell_driver=c.tb['drv'] if drv else None)
        if mlp:
            ops.mlp2_rows_bf16(t['A'], rows, *c.w, t['h'], hid_out=t['hid'], add_act=True, relu_out=relu, active=a)
        torch.cuda.synchronize()


def cell_ids(rng):
    return np.arange(rng[0], rng[0] + rng[1])


SLOT_CASES = [('small', rg, r, m, h16) for rg in O.REGIMES for r in (True, False) for m in (False, True) for h16 in (True, False)] + \
             [(s, rg, r, m, h16) for s in ('rb2_nets', 'rb2_cells') for rg in O.REGIMES
              for r, m, h16 in ((True, False, True), (False, True, False), (True, True, False), (False, False, True))]


@pytest.mark.parametrize('size,regime,relu,masked,hid16', SLOT_CASES)
def test_level_fwd_slots_matches_fp64_reference(cases, dev, size, regime, relu, masked, hid16):
    """The slot form over the rows of fan-in <= 4 and the whole net level: one row block per workgroup (`small`: the cell
    rows outnumber the net rows) and two (`rb2_nets`: 6161 nets over 75 cells - a partial first block, a dead second one, 190
    workgroups without a cell tile; `rb2_cells`: 6177 cells over 40 nets).  Under the mask a whole tile of cell rows is
    inactive while its workgroup's net rows are not.  The forward-only twin gives the same h, a second launch on restored
    inputs the same bits."""
    c = cases[(regime, size)]
    t = fresh(c, dev, hid16)
    run_slots(c, t, relu, masked, c.slot_range)
    check(c, t, relu, masked, c.net_range, cell_ids(c.slot_range), f'slots {size} {regime} relu={int(relu)} cone={int(masked)} hid16={int(hid16)}')
    t2 = fresh(c, dev, hid16)
    run_slots(c, t2, relu, masked, c.slot_range)
    bitwise(t, t2)
    ti = fresh(c, dev, hid16)
    run_slots(c, ti, relu, masked, c.slot_range, infer=True)
    bitwise(t, ti, names=('h',))
    bitwise(ti, O.inputs(c, hid16), names=('A', 'LSE', 'hid', 'PRE'))


@pytest.mark.parametrize('hid16', [True, False])
@pytest.mark.parametrize('n_cell', O.SUB_COUNTS)
def test_level_fwd_slots_on_sub_ranges(cases, dev, n_cell, hid16):
    """1, 15, 16, 17 and 33 cell rows under the whole net level, which is then the longer one and sets the grid; the rows past
    the sub-range keep their bits."""
    c = cases[('unit', 'small')]
    masked = n_cell % 2 == 1
    rng = (c.slot_range[0], n_cell)
    t = fresh(c, dev, hid16)
    run_slots(c, t, True, masked, rng)
    check(c, t, True, masked, c.net_range, cell_ids(rng), f'slots sub-range {n_cell} cone={int(masked)} hid16={int(hid16)}')
    ti = fresh(c, dev, hid16)
    run_slots(c, ti, True, masked, rng, infer=True)
    bitwise(t, ti, names=('h',))


@pytest.mark.parametrize('hid16', [True, False])
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('regime', O.REGIMES)
def test_level_fwd_bf16_matches_fp64_reference(cases, dev, regime, relu, masked, hid16):
    """The index form over every L4 row - the rows past the slot width walked in batches of four requests, a missing edge
    of the last batch repeating an edge of the row, the heavy ones serially - as a range, as the same rows in an index tensor
    (in reverse order: other tiles, the same rows; bitwise the range form) and without the per-edge driver table (the serial
    branch of fold_gather_edges: judged on its own - its A differs from the batched branch's in the last bits, see
    fold_gather.h); the forward-only twin gives the same h as the training form of the same branch."""
    c = cases[(regime, 'small')]
    rows = cell_ids(c.cell_range)
    tag = f'{regime} relu={int(relu)} cone={int(masked)} hid16={int(hid16)}'
    t = fresh(c, dev, hid16)
    run_index(c, t, relu, masked, c.cell_range)
    check(c, t, relu, masked, c.net_range, rows, 'index ' + tag)
    rev = torch.from_numpy(rows[::-1].astype(np.int32).copy()).to(dev)
    for spec, drv in ((rev, True), (c.cell_range, False)):
        t2 = fresh(c, dev, hid16)
        run_index(c, t2, relu, masked, spec, drv=drv)
        if drv:
            bitwise(t, t2, tag='rows reversed')
        else:
            check(c, t2, relu, masked, c.net_range, rows, 'index-serial ' + tag)
        ti = fresh(c, dev, hid16)
        run_index(c, ti, relu, masked, spec, drv=drv, infer=True)
        bitwise(t2, ti, names=('h',))
        bitwise(ti, O.inputs(c, hid16), names=('A', 'LSE', 'hid', 'PRE'))


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('regime', O.REGIMES)
def test_pair_fwd_gather_and_mlp_match_fp64_reference(cases, dev, regime, relu, masked, mode):
    """The two-kernel form over every L4 row, the heavy ones (17, 24, 25 and 200 in-edges) on the whole-workgroup path - eight
    thread groups striding, their (max, sum, weighted sum) merged in a fixed order - in the accurate and in the fast math mode,
    with and without the per-edge driver table (each judged on its own)."""
    c = cases[(regime, 'small')]
    hid16 = relu
    assert c.tb['heavy'] is not None and c.tb['heavy'].numel() == 4
    tag = f'{mode} {regime} relu={int(relu)} cone={int(masked)}'
    t2 = fresh(c, dev, hid16)
    run_two_kernels(c, t2, relu, masked, c.cell_range, mode, drv=False)
    check(c, t2, relu, masked, c.net_range, cell_ids(c.cell_range), 'gather-serial+mlp ' + tag)
    t = fresh(c, dev, hid16)
    run_two_kernels(c, t, relu, masked, c.cell_range, mode)
    check(c, t, relu, masked, c.net_range, cell_ids(c.cell_range), 'gather+mlp ' + tag)
    # the gather alone leaves h's cell rows and hid as they were
    t3 = fresh(c, dev, hid16)
    run_two_kernels(c, t3, relu, masked, c.cell_range, mode, mlp=False)
    bitwise(t, t3, names=('A', 'LSE'))
    bitwise(t3, O.inputs(c, hid16), names=('hid', 'PRE'))
    bitwise(t3, O.inputs(c, hid16), names=('h',), rows=torch.from_numpy(c.L[4]))


@pytest.mark.parametrize('relu,masked', [(True, False), (False, True)])
@pytest.mark.parametrize('regime', O.REGIMES)
@pytest.mark.parametrize('size', O.SIZES)
def test_three_forms_agree_bitwise(cases, dev, size, regime, relu, masked):
    """On the slot rows the slot form and the index form write the same bits (every size); on every row the index form and
    the two kernels without the heavy path do, and with the heavy path on every row it does not take."""
    c = cases[(regime, size)]
    ts, tx = fresh(c, dev, True), fresh(c, dev, True)
    run_slots(c, ts, relu, masked, c.slot_range)
    run_index(c, tx, relu, masked, c.slot_range)
    bitwise(ts, tx)
    if size != 'small':
        return
    tx, tk, th = fresh(c, dev, True), fresh(c, dev, True), fresh(c, dev, True)
    run_index(c, tx, relu, masked, c.cell_range)
    run_two_kernels(c, tk, relu, masked, c.cell_range, 'bf16', heavy=False)
    bitwise(tx, tk)
    run_two_kernels(c, th, relu, masked, c.cell_range, 'bf16', heavy=True)
    light = np.ones(c.N, bool)
    light[c.tb['heavy'].cpu().numpy()] = False
    bitwise(tx, th, rows=torch.from_numpy(np.nonzero(light)[0]))
    bitwise(ts, tx, rows=torch.from_numpy(cell_ids(c.slot_range)))
