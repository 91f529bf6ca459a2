"""The fused level kernels called through their ops wrappers on one small folded graph (200 nodes, 6 levels): what the
wrappers refuse, and that a recorded launch (ops.recorded / ops.relaunch) repeats the checked one bit for bit at the sizes
where the grid rule or a shifted argument would show."""
import pytest
import torch

from mmft import lib, ops
from mmft.detrand import det_uniform

pytestmark = pytest.mark.gpu
N, L, D, HD = 200, 6, 128, 256
SENT = 777.0


def T_(shape, seed, dev, lo=-1.0, hi=1.0):
    return torch.from_numpy(det_uniform(shape, seed, lo, hi)).to(dev)


class Level:
    """Static tables of the graph and the operands of one (net level 1, cell level 2) pair; nothing here is written by a test."""
    def __init__(self, dev):
        from mmft.synth import synth_design
        from mmft.train import DesignBatch
        b = DesignBatch([synth_design(N=N, L=L, tile=32, seed=5, end_frac=0.2)], dev)
        g = self.g = b.graph
        assert b.N == N
        self.fold = g.fold_schedule(b.level_nodes)
        self.slots, self.net_drv, max_in = g.level_slots(b.level_nodes)
        assert max(max_in) <= 4 and all(f['range'] is not None for f in self.fold)
        self.cslots, self.pairs, self.scratch, self.counters = g.level_bwd_pairs(b.level_nodes)
        self.in_net, self.in_cell, self.drv = g.csr('in', 'net'), g.csr('in', 'cell'), g.cell_edge_drivers()
        self.out_net, self.out_cell = g.csr('out', 'net'), g.csr('out', 'cell')
        self.net, self.cell = self.fold[1]['range'], self.fold[2]['range']
        self.h0, self.pre = T_((N, D), 1, dev), T_((N, D), 2, dev)
        self.w1p, self.w2p = ops.pack_bf16(T_((HD, D), 3, dev, -0.1, 0.1)), ops.pack_bf16(T_((D, HD), 4, dev, -0.1, 0.1))
        self.b1, self.b2 = T_((HD,), 5, dev, -0.1, 0.1), T_((D,), 6, dev, -0.1, 0.1)
        self.dev = dev

    def kept(self, hid_dtype=torch.bfloat16):
        """Fresh A, LSE, hid_out filled with a sentinel."""
        full = lambda w, dt: torch.full((N, w), SENT, dtype=dt, device=self.dev)
        return full(D, torch.float32), full(D, torch.float32), full(HD, hid_dtype)


@pytest.fixture(scope='module')
def lv(dev):
    return Level(dev)


# ------------------------------------------------------------------------------------------------ refusals
def _call(lv, name, h, pre, w1p, net, cell):
    """One wrapper on the level's operands, with the operand under test replaced."""
    A, LSE, hid = lv.kept()
    w = (w1p, lv.b1, lv.w2p, lv.b2)
    if name == 'level_fwd_bf16':
        return ops.level_fwd_bf16(h, pre, lv.in_net, lv.in_cell, net, cell, A, LSE, *w, hid, in_cell_driver=lv.drv)
    if name == 'level_fwd_bf16_infer':
        return ops.level_fwd_bf16_infer(h, pre, lv.in_net, lv.in_cell, net, cell, *w, in_cell_driver=lv.drv)
    if name == 'level_fwd_slots':
        return ops.level_fwd_slots(h, pre, lv.slots, lv.net_drv, net, cell, A, LSE, *w, hid)
    if name == 'level_fwd_slots_infer':
        return ops.level_fwd_slots_infer(h, pre, lv.slots, lv.net_drv, net, cell, *w)
    # level_bwd_pair has no `pre` and no row range: its operand with the layout of h is A (passed as `pre` here), and its
    # range is the tile table's (`cell` = (0, ntiles))
    pr = lv.pairs[1]
    G, DA, DHN = T_((N, D), 7, lv.dev), torch.zeros((N, D), device=lv.dev), torch.zeros_like(hid)
    return ops.level_bwd_pair(G, h, pre, LSE, DA, None, pr['tiles'], cell[1], lv.out_net[0], pr['sink_shift'], lv.cslots, lv.out_cell,
                              lv.scratch, lv.counters, w1p, lv.w2p, hid, DHN)


@pytest.mark.parametrize('fault', ['pack_shape', 'pitch', 'range'])
@pytest.mark.parametrize('name', ['level_fwd_bf16', 'level_fwd_bf16_infer', 'level_fwd_slots', 'level_fwd_slots_infer', 'level_bwd_pair'])
def test_level_wrappers_refuse_bad_operands(lv, name, fault):
    """A weight pack of shape (128, 128), a `pre` whose row pitch is not h's, a row range reaching past N: ValueError from
    every wrapper (the type each of them has always raised), and nothing is launched - h keeps its contents.  Only shapes and
    pitches are wrong, every tensor is a live device tensor."""
    h = lv.h0.clone()
    bwd = name == 'level_bwd_pair'
    pre = lv.kept()[0] if bwd else lv.pre
    w1p, net = lv.w1p, lv.net
    cell = (0, lv.pairs[1]['ntiles']) if bwd else lv.cell
    if fault == 'pack_shape':
        w1p = torch.zeros((128, 128), dtype=torch.bfloat16, device=lv.dev)
    elif fault == 'pitch':
        pre = torch.zeros((N, D + 4), device=lv.dev)[:, :D]
        assert pre.shape == h.shape and pre.stride(0) != h.stride(0)
    else:
        cell = (cell[0], cell[1] + 1) if bwd else (N - 3, 4)
    with pytest.raises(ValueError):
        _call(lv, name, h, pre, w1p, net, cell)
    torch.cuda.synchronize()
    assert torch.equal(h, lv.h0)


# ------------------------------------------------------------------------------------------------ record and relaunch
# cell rows of the pair, next to the whole net level below them (39 rows = 3 workgroups; the index form recomputes a net from
# its driver only inside the net range it is given, so the two forms agree on whole net levels, as the sweep passes them):
# one row and a partial second 16-row block - the net level is the longer one and sets the grid -, and the whole cell level
SIZES = [1, 17, 39]


@pytest.mark.parametrize('hid_dtype', [torch.bfloat16, torch.float32], ids=['hid_bf16', 'hid_fp32'])
@pytest.mark.parametrize('n_cell', SIZES)
def test_recorded_slot_launches_repeat_the_checked_launch(lv, n_cell, hid_dtype):
    """level_fwd_slots returns its recorded launch; re-issued through ops.relaunch on restored inputs and zeroed outputs it
    reproduces h, A, LSE and hid_out bitwise, and so does level_fwd_slots_infer for h.  What the launch itself must write is
    pinned too: the net rows are relu(pre + h[driver]) exactly, the index form (level_fwd_bf16, equal bit for bit by
    tests/test_bf16_gpu.py) agrees on every buffer, and no row outside the two ranges is touched."""
    assert lv.net[1] == 39 and lv.cell[1] == 39
    net, n_net, cell = lv.net, lv.net[1], (lv.cell[0], n_cell)
    w = (lv.w1p, lv.b1, lv.w2p, lv.b2)
    dv, st = lib.stream_args(lv.h0)
    # training form, checked launch
    h, (A, LSE, hid) = lv.h0.clone(), lv.kept(hid_dtype)
    rec = ops.level_fwd_slots(h, lv.pre, lv.slots, lv.net_drv, net, cell, A, LSE, *w, hid)
    first = [t.clone() for t in (h, A, LSE, hid)]
    # ... what it wrote
    nrows = torch.arange(net[0], net[0] + n_net, device=lv.dev)
    crows = torch.arange(cell[0], cell[0] + n_cell, device=lv.dev)
    assert bool((lv.net_drv[nrows] >= 0).all())
    assert torch.equal(h[nrows], torch.relu(lv.pre[nrows] + lv.h0[lv.net_drv[nrows].long()]))
    outside = torch.ones(N, dtype=torch.bool, device=lv.dev)
    outside[nrows] = False
    outside[crows] = False
    assert torch.equal(h[outside], lv.h0[outside]) and not torch.equal(h[crows], lv.h0[crows])
    outside[nrows] = True                                   # A, LSE, hid_out: the cell rows alone
    for t in (A, LSE, hid):
        assert bool((t[outside] == SENT).all()) and not bool((t[crows] == SENT).any())
    h2, (A2, LSE2, hid2) = lv.h0.clone(), lv.kept(hid_dtype)
    ops.level_fwd_bf16(h2, lv.pre, lv.in_net, lv.in_cell, net, cell, A2, LSE2, *w, hid2, in_cell_driver=lv.drv)
    for x, y in zip(first, (h2, A2, LSE2, hid2)):
        assert torch.equal(x, y)
    # ... re-issued from the record
    h.copy_(lv.h0)
    for t in (A, LSE, hid):
        t.zero_()
    ops.relaunch('mmft_level_fwd_slots', rec, dv, st)
    assert torch.equal(h, first[0])
    for x, y in zip(first[1:], (A, LSE, hid)):
        assert torch.equal(x[crows], y[crows]) and not bool(y[outside].any())
    # forward-only form: the same h, checked and re-issued
    hi = lv.h0.clone()
    rec_i = ops.level_fwd_slots_infer(hi, lv.pre, lv.slots, lv.net_drv, net, cell, *w)
    assert torch.equal(hi, first[0])
    hi.copy_(lv.h0)
    ops.relaunch('mmft_level_fwd_slots_infer', rec_i, dv, st)
    assert torch.equal(hi, first[0])
    assert len(rec) == len(rec_i) + 5 and all(not torch.is_tensor(a) for a in rec + rec_i)
