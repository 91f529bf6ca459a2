"""mmft_mlp2_feat_bwd_bf16 at the edges of its tile loop: the kernel requests the next 32-row tile with unconditional loads
from clamped addresses and turns what lies past the end of the row range, or past fin, into zeros only where the registers
are deposited into LDS; the first-layer gradient keeps ceil(fin / 16) column blocks.  So: partial first tiles and tile edges,
a range on which some workgroups run a second (and partial) tile, every fin at which the K step count or the column block
count changes, and NaN in every element the kernel may load but must not use.

The reference is the fp64 math of test_bf16_gpu.test_feature_mlp_without_hidden_tensor, which rounds where the kernel
rounds (operands, the hidden tile and the hidden gradient through bf16), with that test's tolerances."""
import pytest
import torch

from conftest import rel_err
from mmft import lib, ops

pytestmark = pytest.mark.gpu
TOL = 2e-2
LDG = 132
NS = [(1, 0), (31, 0), (32, 0), (33, 0), (95, 0), (6177, 7)]      # 6177 = 192 x 32 + 33: second tiles, the last one partial
FINS = [1, 2, 16, 17, 32, 33, 36, 48, 49, 64]


def bf(t):
    return t.bfloat16().float()


def rnd(*shape, seed=0, representable=False):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g)
    return bf(t) if representable else t


@pytest.fixture(autouse=True)
def _bf16_mode():
    with lib.math_mode('bf16'):
        yield
    assert lib.get_math_mode() == 'f32'


def _case(fin, n, row0, representable):
    """Host operands; x with row pitch fin + 3 and g with row pitch 132, NaN in their padding columns and in every row
    outside [row0, row0 + n)."""
    N = row0 + n + 5
    xbuf = torch.full((N, fin + 3), float('nan'))
    gbuf = torch.full((N, LDG), float('nan'))
    sl = slice(row0, row0 + n)
    xbuf[sl, :fin] = rnd(N, fin, seed=1, representable=representable)[sl]
    gbuf[sl, :128] = rnd(N, 128, seed=6, representable=representable)[sl]
    w1 = rnd(256, fin, seed=2, representable=representable) * 0.25
    b1 = rnd(256, seed=3, representable=representable) * 0.25
    w2 = rnd(128, 256, seed=4, representable=representable) * 0.125
    if representable:
        w1, b1, w2 = bf(w1), bf(b1), bf(w2)
    return xbuf, gbuf, w1, b1, w2, sl


def _reference(xbuf, gbuf, w1, b1, w2, sl, fin):
    x, g = xbuf[sl, :fin], gbuf[sl, :128]
    xb, w1b, w2b, gb = bf(x).double(), bf(w1).double(), bf(w2).double(), bf(g).double()
    pre = xb @ w1b.T + b1.double()
    H = bf(torch.relu(pre).float()).double()                      # the hidden tile is stored as bf16 in LDS
    dpre = (gb @ w2b) * (pre > 0)
    dH = bf(dpre.float()).double()                                # ... and so is the hidden gradient
    return dH.T @ xb, dpre.sum(0), gb.T @ H, g.double().sum(0)


def _run(dev, xbuf, gbuf, w1, b1, w2, sl, fin):
    xd, gd = xbuf.to(dev), gbuf.to(dev)
    x, g = xd[:, :fin], gd[:, :128]
    assert x.stride(0) == fin + 3 and g.stride(0) == LDG
    return ops.mlp2_feat_bwd_bf16(g, x, (sl.start, sl.stop - sl.start), w1.to(dev), b1.to(dev), w2.to(dev))


def _check(got, ref, tol):
    for t in got:
        assert bool(torch.isfinite(t).all())
    dw1, db1, dw2, db2 = got
    assert rel_err(dw2, ref[2]) < tol
    assert rel_err(db2, ref[3]) < 1e-5             # from the fp32 staging registers: exact in both cases
    assert rel_err(dw1, ref[0]) < tol
    assert rel_err(db1, ref[1]) < tol


@pytest.mark.parametrize('fin', FINS)
@pytest.mark.parametrize('n,row0', NS)
def test_feat_bwd_clamped_loads_ignore_what_lies_outside(dev, fin, n, row0):
    """NaN in the padding columns of x and in all rows outside the range: every gradient is finite and within tolerance of
    the reference.  A select lost at the deposit, or a clamp off by one, shows up as NaN."""
    for representable in (True, False):
        case = _case(fin, n, row0, representable)
        got = _run(dev, *case, fin)
        _check(got, _reference(*case, fin), 1e-3 if representable else TOL)


@pytest.mark.parametrize('fin,n,row0', [(36, 6177, 7), (2, 6177, 7), (64, 95, 0), (17, 33, 0)])
def test_feat_bwd_is_deterministic(dev, fin, n, row0):
    """Two calls on the same inputs: bitwise equal dw1, db1, dw2, db2 (one slab per workgroup, summed in a fixed order)."""
    case = _case(fin, n, row0, False)
    a = [t.clone() for t in _run(dev, *case, fin)]
    b = _run(dev, *case, fin)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize('fin', [f for f in FINS if f > 32])
@pytest.mark.parametrize('n,row0', NS)
def test_feat_fwd_two_workgroups_per_cu(dev, fin, n, row0):
    """mmft_mlp2_feat_fwd_bf16 with fin > 32: the unmasked instantiation that is held to 128 registers (two workgroups per CU)
    on the same row ranges, against the same reference; rows outside the range keep their sentinel."""
    for representable in (True, False):
        xbuf, gbuf, w1, b1, w2, sl = _case(fin, n, row0, representable)
        b2 = rnd(128, seed=5, representable=representable)
        xb, w1b, w2b = bf(xbuf[sl, :fin]).double(), bf(w1).double(), bf(w2).double()
        H = bf(torch.relu(xb @ w1b.T + b1.double()).float()).double()
        ref = H @ w2b.T + b2.double()
        out = torch.full((xbuf.shape[0], 128), 7.0, device=dev)
        ops.mlp2_feat_fwd_bf16(xbuf.to(dev)[:, :fin], (row0, n), w1.to(dev), b1.to(dev), w2.to(dev), b2.to(dev), out)
        assert rel_err(out[sl], ref) < (1e-3 if representable else TOL)
        assert float((out[:row0] - 7.0).abs().max()) == 0.0 if row0 else True      # rows outside the range are not touched
        assert float((out[row0 + n:] - 7.0).abs().max()) == 0.0
