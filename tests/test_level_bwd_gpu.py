"""The reverse level kernels - mmft_level_bwd_pair (csrc/mlp2_bf16.hip) and its unfused counterpart mmft_level_bwd_pull
(csrc/graph.hip) - against the fp64 autograd reference of ONE hand-built level pair (tests/level_pair_oracle.py: what the graph
holds and how the reference is formed; tests/test_level_pair_cpu.py: that the reference notices a kernel's mistakes).  No forward
kernel runs here: A, LSE, DA and HN are inputs.

Metric: max |got - ref| / max |ref| PER CLASS of rows (sinks by consumer count, drivers by {no sinks, whole, heavy}, DHN, DA).
Bounds: G max(5e-5, 4 e_32) with e_32 the same reference evaluated in torch fp32 on the CPU; DHN 2e-6 (fp32 storage) or one
bf16 rounding per element (|d| <= 2^-8 |ref| + 1e-6 scale), DA 1e-5 given the kernel's own DHN (test_mlp2_rows_prepacked's
bounds for the same tile).  No bound comes from a kernel's output.

Measured on an MI355X: e_hip per class, the largest over the cases of a kind (pair: bf16 mode, every relu / hid16 / poisoned /
whole-tile case; pull: every rows / heavy / own / cone case of that math mode), beside the largest e_32.  4 e_32 stays under the
floor, so the bound of every class is 5e-5 in both regimes.

               ------------- unit -------------    ------------- wide -------------
  class        e_32     pair     pull f32 pull bf16  e_32     pair     pull f32 pull bf16
  sink_c0      0        0        0        0          0        0        0        0
  sink_c1      6.6e-08  9.2e-08  9.2e-08  9.2e-08    2.6e-06  1.8e-06  1.8e-06  1.8e-06
  sink_c2      8.9e-08  1.2e-07  1.1e-07  1.2e-07    2.8e-06  1.2e-06  1.2e-06  1.2e-06
  sink_c3      9.1e-08  1.5e-07  1.5e-07  1.5e-07    9.4e-07  1.1e-06  1.3e-06  1.3e-06
  sink_c4      1.1e-07  1.3e-07  1.5e-07  1.5e-07    2.2e-06  1.7e-06  1.8e-06  1.8e-06
  sink_c5      9.1e-08  1.5e-07  1.6e-07  1.5e-07    2.5e-06  1.7e-06  1.7e-06  1.7e-06
  sink_c9      1.0e-07  1.5e-07  1.7e-07  1.7e-07    2.1e-06  1.3e-06  1.6e-06  1.6e-06
  sink_c17     1.3e-07  1.3e-07  1.3e-07  1.3e-07    6.3e-08  1.2e-07  1.2e-07  1.2e-07
  drv_0        0        0        0        0          0        0        0        0
  drv_whole    1.6e-07  1.8e-07  1.6e-07  1.6e-07    1.1e-06  7.6e-07  7.7e-07  7.7e-07
  drv_heavy    3.1e-07  1.4e-07  2.5e-07  1.5e-07    9.3e-07  6.5e-07  7.5e-07  7.5e-07
  DHN fp32     pair: unit 8.9e-08, wide 9.0e-08   (bound 2e-6)
  DHN bf16     pair: unit 2.3e-03, wide 2.5e-03   (bound 2^-8 per element)
  DA           pair: unit 1.1e-07, wide 1.1e-07   (bound 1e-5)
The 61 cases take 3.6 s together with the module fixture; no case takes more than 0.3 s.
"""
import numpy as np
import pytest
import torch

import level_pair_oracle as O
from mmft import lib, ops
from mmft.pingraph import PinGraph

pytestmark = pytest.mark.gpu
REGIMES = ('unit', 'wide')
NAN = float('nan')
JUNK = 7.0                  # finite filler of rows a kernel must not use, where a test does not poison them


@pytest.fixture(scope='module')
def cases(dev):
    """Both value regimes on the device, each with its tables; every edge case asserted present from those tables."""
    out = {}
    for r in REGIMES:
        c = O.build_case(r)
        c.g = c.graph.to(dev)
        rep = O.edge_report(c, c.g)
        assert len(rep) >= 40 and all(rep.values()), [k for k, v in rep.items() if not v]
        c.tables = c.g.level_bwd_pairs(c.levels)
        c.w1p = ops.pack_bf16(c.W2g.to(dev), transpose=True)            # W2g^T: hidden gradient = G . W2g
        c.w2p = ops.pack_bf16(c.W1g.to(dev), transpose=True)            # W1g^T
        assert torch.equal(c.w1p.float().cpu(), c.W2g.T.contiguous()) and torch.equal(c.w2p.float().cpu(), c.W1g.T.contiguous())
        out[r] = c
    return out


_refs = {}


def bounds(c, relu, active=False, width=O.D):
    """The fp64 reference, its row classes, e_32 and the bounds: computed once per (regime, relu, mask, width), never changed."""
    key = (c.regime, relu, active, width)
    if key not in _refs:
        _refs[key] = O.g_bounds(c, relu, c.active if active else None, width)
    return _refs[key]


def same_bits(a, b):
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    iv = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return a.dtype == b.dtype and torch.equal(a.view(iv), b.view(iv))


def others(c, rows):
    m = np.ones(c.N, bool)
    m[np.asarray(rows, dtype=np.int64)] = False
    return torch.from_numpy(np.nonzero(m)[0])


def check_G(c, G, relu, tag, active=False, width=O.D):
    ref, classes, e32, bound = bounds(c, relu, active, width)
    G = G.cpu()
    assert bool(torch.isfinite(G[np.concatenate(list(classes.values()))]).all()), tag
    err = O.class_errors(G, ref, classes)
    for k in classes:
        print(f'MEAS {tag} {k}: e_hip {err[k]:.1e} e_32 {e32[k]:.1e} bound {bound[k]:.1e}')
    bad = {k: (err[k], bound[k]) for k in classes if not err[k] <= bound[k]}
    assert not bad, (tag, bad)


def check_mlp(c, G, DA, DHN, hid16, tag):
    drv = torch.from_numpy(c.drv)
    G, DA, DHN = G.cpu(), DA.cpu(), DHN.cpu()
    got_dhn, got_da = DHN[drv].float().cpu().double(), DA[drv].cpu().double()
    assert bool(torch.isfinite(got_dhn).all() and torch.isfinite(got_da).all()), tag
    dhn, da = O.mlp_reference(c, G[drv], DHN[drv].float())
    scale = float(dhn.abs().max())
    e_dhn, e_da = O.rel_err(got_dhn, dhn), O.rel_err(got_da, da)
    print(f'MEAS {tag} DHN: e_hip {e_dhn:.1e} (hid16 {hid16})  DA: e_hip {e_da:.1e}')
    if hid16:
        assert bool(((got_dhn - dhn).abs() <= 2.0 ** -8 * dhn.abs() + 1e-6 * scale).all()), tag
    else:
        assert e_dhn < O.EXACT, (tag, e_dhn)
    assert e_da < 1e-5, (tag, e_da)
    assert float(got_dhn[c.HN[c.drv] <= 0].abs().max()) == 0.0                      # relu'(HN) at HN = 0 and below


def pair_inputs(c, dev, hid16, poison):
    """Device inputs of one pair launch.  poison: everything the kernel must ignore is NaN - G rows without an own flag, A / LSE /
    DA rows of every node that is no consumer, HN rows outside the drivers, all of DHN, the whole heavy-part scratch."""
    fill = NAN if poison else JUNK
    own = c.own.bool()
    G = c.G0.clone()
    G[~own] = fill
    G[c.cons] = fill
    t = {'G': G}
    for name, src in (('A', c.A), ('LSE', c.LSE), ('DA', c.DA0)):
        x = torch.full_like(src, fill)
        x[c.cons] = src[c.cons]
        t[name] = x
    hn = torch.full_like(c.HN, fill)
    hn[c.drv] = c.HN[c.drv]
    hd = torch.bfloat16 if hid16 else torch.float32
    t['HN'], t['DHN'] = hn.to(hd), torch.full((c.N, O.HID), fill, dtype=hd)
    t = {k: v.to(dev) for k, v in t.items()}
    t['h'], t['own'] = c.h.to(dev), c.own.to(dev)
    return t


def launch_pair(c, t, relu, has_mlp, tables=None, graph=None, scratch_fill=None):
    g = graph or c.g
    cslots, plist, scratch, counters = tables or c.tables
    pr = plist[0]
    assert pr['n_cell'] == c.drv.size and pr['n_net'] == c.snk.size and pr['sink_shift'] == int(c.snk[0])
    if scratch_fill is not None:
        scratch.fill_(scratch_fill)
    with lib.math_mode('bf16'):
        ops.level_bwd_pair(t['G'], t['h'], t['A'], t['LSE'], t['DA'], t['own'], pr['tiles'], pr['ntiles'], g.csr('out', 'net')[0],
                           pr['sink_shift'], cslots, g.csr('out', 'cell'), scratch, counters, c.w1p, c.w2p, t['HN'], t['DHN'],
                           relu=relu, has_mlp=has_mlp)
        torch.cuda.synchronize()
    assert int(counters.abs().sum()) == 0                                           # the part counters are back at zero
    return scratch


def on_host(t):
    return {k: v.cpu() for k, v in t.items() if v is not None}


def check_pair(c, t, before, relu, hid16, has_mlp, tag):
    t, before = on_host(t), on_host(before)
    check_G(c, t['G'], relu, tag)
    rows = np.concatenate([c.drv, c.snk])
    assert same_bits(t['G'][others(c, rows)], before['G'][others(c, rows)]), tag     # NaN-aware: bit patterns
    if has_mlp:
        check_mlp(c, t['G'], t['DA'], t['DHN'], hid16, tag)
    keep = others(c, c.drv if has_mlp else [])
    assert same_bits(t['DA'][keep], before['DA'][keep]) and same_bits(t['DHN'][keep], before['DHN'][keep]), tag
    for k in ('h', 'A', 'LSE', 'HN', 'own'):
        assert same_bits(t[k], before[k]) if t[k].dtype != torch.uint8 else torch.equal(t[k], before[k]), (tag, k)


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('hid16', [True, False])
@pytest.mark.parametrize('regime', REGIMES)
def test_level_bwd_pair_matches_fp64_reference(cases, dev, regime, hid16, relu):
    """Test 1: the paired kernel in bf16 math mode (hardware exponential), drivers cut into parts as shipped: G on sinks and
    drivers against the fp64 autograd reference, DHN / DA against the decoupled MLP reference."""
    c = cases[regime]
    t = pair_inputs(c, dev, hid16, poison=False)
    before = {k: v.clone() for k, v in t.items()}
    launch_pair(c, t, relu, True, scratch_fill=0.0)
    check_pair(c, t, before, relu, hid16, True, f'pair {regime} relu={int(relu)} hid16={int(hid16)}')


def test_level_bwd_pair_without_mlp(cases, dev):
    """has_mlp=False (the pair of cell level 0): G as before, DA / DHN not written at all."""
    c = cases['wide']
    t = pair_inputs(c, dev, False, poison=False)
    t['HN'] = t['DHN'] = None
    before = {k: v.clone() for k, v in t.items() if v is not None}
    launch_pair(c, t, True, False, scratch_fill=0.0)
    check_G(c, t['G'], True, 'pair wide no-mlp')
    cons = torch.from_numpy(c.cons)
    assert same_bits(t['DA'], before['DA']) and same_bits(t['G'].cpu()[cons], before['G'].cpu()[cons])


@pytest.mark.parametrize('hid16,has_mlp', [(True, True), (False, True), (False, False)])
@pytest.mark.parametrize('regime', REGIMES)
def test_level_bwd_pair_ignores_what_it_must(cases, dev, regime, hid16, has_mlp):
    """Test 3: the rows the kernel must not use are torch.empty memory in production - here NaN, and so is the scratch of the
    heavy drivers' parts.  Every row the kernel owns comes out finite and right, every other row keeps its bits."""
    c = cases[regime]
    t = pair_inputs(c, dev, hid16, poison=True)
    before = {k: v.clone() for k, v in t.items()}
    scratch = launch_pair(c, t, True, has_mlp, scratch_fill=NAN)
    check_pair(c, t, before, True, hid16, has_mlp, f'pair-poisoned {regime} hid16={int(hid16)} mlp={int(has_mlp)}')
    nparts = int(c.tables[1][0]['tiles'][:, 3].gt(0).sum())
    assert bool(torch.isfinite(scratch[:nparts]).all())                              # every part published its partial sum


@pytest.mark.parametrize('regime', REGIMES)
def test_level_bwd_pair_reuses_scratch_bit_for_bit(cases, dev, regime):
    """Test 4: a second launch on restored inputs, the scratch left as the first launch wrote it (stale partial sums of the
    same rows), reproduces the first bit for bit - whichever workgroup arrives last adds the parts in part order."""
    c = cases[regime]
    assert int(c.tables[1][0]['tiles'][:, 3].gt(0).sum()) >= 7                       # parts enabled: 2 + 2 + 3
    res = []
    for i in range(2):
        t = pair_inputs(c, dev, True, poison=False)
        launch_pair(c, t, True, True, scratch_fill=0.0 if i == 0 else None)
        res.append(t)
    for k in ('G', 'DA', 'DHN'):
        assert same_bits(res[0][k], res[1][k]), k


def pull_inputs(c, dev, width, own_given, active, poison):
    fill = NAN if poison else JUNK
    own = c.own.bool()
    G = c.G0[:, :width].clone()
    G[~own] = fill if own_given else 0.0                                            # own=None: the caller zero-fills G
    G[c.cons] = fill
    if active:
        G[~c.active.bool()] = 0.0                                                   # rows outside the cone keep the caller's zero
    t = {'G': G}
    for name, src in (('A', c.A), ('LSE', c.LSE), ('DA', c.DA0)):
        x = torch.full((c.N, width), fill)
        x[c.cons] = src[c.cons, :width]
        if active:
            off = c.cons[~c.active.bool().numpy()[c.cons]]
            x[off] = fill                                                           # consumers outside the cone: stale rows
        t[name] = x
    t['h'] = c.h[:, :width].contiguous()
    return {k: v.to(dev) for k, v in t.items()}


def launch_pulls(c, dev, t, mode, rows_form, heavy, own_given, relu, active):
    """mmft_level_bwd_pull twice, the sinks first and then their drivers."""
    g = c.g
    with lib.math_mode(mode):
        for rows in (c.snk, c.drv):
            spec = (int(rows[0]), rows.size) if rows_form == 'range' else torch.from_numpy(rows[::-1].astype(np.int32).copy()).to(dev)
            hv = O.heavy_rows(c, rows).to(dev) if heavy else None
            assert hv is None or hv.numel() > 0
            ops.level_bwd_pull(t['G'], t['h'], spec, g.csr('out', 'net'), g.out_net_weight(), g.csr('out', 'cell'), t['A'], t['LSE'],
                               t['DA'], relu=relu, own=c.own.to(dev) if own_given else None, heavy=hv,
                               active=c.active.to(dev) if active else None)
        torch.cuda.synchronize()


def check_pulls(c, t, before, relu, tag, active=False, width=O.D):
    t, before = on_host(t), on_host(before)
    check_G(c, t['G'], relu, tag, active, width)
    _, classes, _, _ = bounds(c, relu, active, width)
    keep = others(c, np.concatenate(list(classes.values())))                         # consumers and rows outside the cone
    assert same_bits(t['G'][keep], before['G'][keep]), tag
    for k in ('h', 'A', 'LSE', 'DA'):
        assert same_bits(t[k], before[k]), (tag, k)


@pytest.mark.parametrize('own_given', [True, False])
@pytest.mark.parametrize('heavy', [True, False])
@pytest.mark.parametrize('rows_form', ['range', 'index'])
@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('regime', REGIMES)
def test_level_bwd_pull_matches_fp64_reference(cases, dev, regime, mode, rows_form, heavy, own_given):
    """Test 2: the unfused pull, sinks then drivers, in both math modes (f32: expf; bf16: the hardware exponential), rows as a
    range and as an index tensor, with and without the workgroup-per-heavy-row path, with own flags and with a zero-filled G."""
    c = cases[regime]
    t = pull_inputs(c, dev, O.D, own_given, False, poison=False)
    before = {k: v.clone() for k, v in t.items()}
    launch_pulls(c, dev, t, mode, rows_form, heavy, own_given, True, False)
    check_pulls(c, t, before, True, f'pull {regime} {mode} {rows_form} heavy={int(heavy)} own={int(own_given)}')


@pytest.mark.parametrize('heavy', [True, False])
def test_level_bwd_pull_narrow_rows(cases, dev, heavy):
    """D = 16 in fp32 mode, without the ReLU: four lanes per row, 64 rows per workgroup, eight of them on a heavy row."""
    c = cases['unit']
    t = pull_inputs(c, dev, 16, True, False, poison=False)
    before = {k: v.clone() for k, v in t.items()}
    launch_pulls(c, dev, t, 'f32', 'range', heavy, True, False, False)
    check_pulls(c, t, before, False, f'pull unit f32 D=16 heavy={int(heavy)}', width=16)


@pytest.mark.parametrize('heavy', [True, False])
@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('regime', REGIMES)
def test_level_bwd_pull_cone_mask_and_ignored_rows(cases, dev, regime, mode, heavy):
    """Tests 2 and 3 for the pull: under a cone mask the consumers outside it are dropped (the reference drops exactly those) and
    the rows outside it keep the caller's zero; the G rows without an own flag and the A / LSE / DA rows of every node that is
    no consumer inside the cone are NaN."""
    c = cases[regime]
    t = pull_inputs(c, dev, O.D, True, True, poison=True)
    before = {k: v.clone() for k, v in t.items()}
    launch_pulls(c, dev, t, mode, 'range', heavy, True, True, True)
    check_pulls(c, t, before, True, f'pull-poisoned-cone {regime} {mode} heavy={int(heavy)}', active=True)
    off = torch.from_numpy(np.concatenate([c.drv, c.snk])[~c.active.bool().numpy()[:c.cons[0]]])
    assert off.numel() and float(t['G'].cpu()[off].abs().max()) == 0.0


@pytest.mark.parametrize('regime', REGIMES)
def test_pair_with_whole_tiles_equals_two_pulls_bitwise(cases, dev, regime):
    """Test 5: with the host kept from cutting drivers into parts, the pair kernel adds what two pulls (without their heavy-row
    path) add, in the same order: bitwise equal G - here on the driver without sinks, the pin with five consumers (the first
    CSR-tail case) and a tile of 17 drivers, which a random design only meets by luck."""
    c = cases[regime]
    g2 = c.graph.to(dev)
    sinks0 = PinGraph.BWD_PAIR_TILE_SINKS
    try:
        PinGraph.BWD_PAIR_TILE_SINKS = 1 << 30
        tables = g2.level_bwd_pairs([list(l) for l in c.levels])
    finally:
        PinGraph.BWD_PAIR_TILE_SINKS = sinks0
    tiles = tables[1][0]['tiles'].cpu().numpy()
    assert (tiles[:, 3] == 0).all() and any(t[1] == O.PAIR_GROUPS + 1 for t in tiles) and int(tiles[:, 1].sum()) == c.drv.size
    tp = pair_inputs(c, dev, True, poison=False)
    launch_pair(c, tp, True, True, tables=tables, graph=g2)
    check_G(c, tp['G'], True, f'pair-whole {regime}')
    tq = pull_inputs(c, dev, O.D, True, False, poison=False)
    launch_pulls(c, dev, tq, 'bf16', 'range', False, True, True, False)
    rows = torch.from_numpy(np.concatenate([c.drv, c.snk]))
    assert same_bits(tp['G'].cpu()[rows], tq['G'].cpu()[rows])
