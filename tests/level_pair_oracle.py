"""One hand-built (cell level, net level, cell level) triple and its fp64 reference  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The reverse level kernels (mmft_level_bwd_pair, mmft_level_bwd_pull) are held to this module by tests/test_level_bwd_gpu.py;
tests/test_level_pair_cpu.py checks on the CPU that the graph holds every edge case it is built for and that the reference
notices the mistakes a kernel could make.  Plain numpy / torch on the CPU.

Graph: level 0 = the DRIVERS (cell rows), level 1 = the SINKS (net rows, one driver each, numbered by driver), level 2 = the
CONSUMERS (cell rows whose A / LSE / DA the sinks read).  Fan-out per driver and consumers per sink are written down below in
terms of the host's thresholds (PinGraph.BWD_PAIR_*, ops.PAIR_HEAVY_OUT), not drawn; every kernel table comes from
PinGraph.level_bwd_pairs / csr / out_net_weight.

Reference (`reference`): torch autograd over the restated forward of these three levels,
    h_v = act(z_v),  h_w = act(pre_w + h_v),  a_c = R.seg_softmax_sum(h, in-cell edges of c),
    loss = sum_c a_c . DA_c + sum_{own rows} h . g
with the leaves z at the drivers' and sinks' rows; G is the gradient at the leaves.  The kernels take h as GIVEN and use
only its sign for relu' (G = [h > 0] ...), so `act` keeps the value of a non-positive entry and stops its gradient: for
every entry the kernels can tell apart that is relu, it lets a test hand them h <= 0 rows (as
test_level_bwd_pull_matches_autograd does) and lets the wide regime reach h - LSE = -80 with the ReLU on.
pre_w is the constant h_w - h_v.  With relu=False act is the identity.

`formula` is the closed form the kernels are documented to evaluate (csrc/mlp2_bf16.hip, csrc/graph.hip), in fp64 from the
fp32-rounded A / LSE they are given.  It exists to be BROKEN: each entry of DEFECTS switches one mistake on, and the CPU test
demands that the mistake moves some row class by more than ten times that class's bound against `reference`.
"""
import numpy as np
import torch

from mmft import ops
from mmft.detrand import det_uniform
from mmft.pingraph import PinGraph
from oracle import bf16 as B
from oracle import restatement as R

D = 128
HID = 256
# the two constants below belong to the kernels, not to the host: level_bwd_pair_kernel runs 512 threads = 16 thread groups of
# 32 lanes and one or two 16-row MFMA blocks (nrb = nd > 16); level_bwd_pull_kernel's heavy path strides 8 thread groups
PAIR_GROUPS = 16
PULL_HEAVY_GROUPS = 8
G_FLOOR = 5e-5            # the bound tests/test_kernels_gpu.py already holds level_bwd_pull to
E32_MARGIN = 4            # over the reference's own fp32 spread: summation order
EXACT = 2e-6              # fp32 accumulation of exact bf16 products (tests/test_bf16_gpu.py)
DEFECTS = ('drop_tail', 'own_ignored', 'drop_last_part', 'no_one', 'mask_from_grad', 'inactive_counted', 'lse_bf16')


def driver_fanouts():
    """Sinks per driver, in driver order, from the host's thresholds.  Heavy drivers (more than TILE_SINKS sinks) are kept
    apart by tiles of whole drivers."""
    TD, TS, PART, HO = PinGraph.BWD_PAIR_TILE_DRIVERS, PinGraph.BWD_PAIR_TILE_SINKS, PinGraph.BWD_PAIR_PART, ops.PAIR_HEAVY_OUT
    half = TD // 2
    fans = [0, 1] * (TD // 2)                        # TILE_DRIVERS drivers, few sinks: closed by the driver count
    fans += [TS + 1]                                 # heavy: two parts, the last one holds one sink
    fans += [HO] + [1] * (half - 1)                  # exactly one MFMA block of drivers; a fan-out AT the pulls' heavy threshold
    fans += [2 * PART]                               # heavy: two full parts
    fans += [HO + 1] + [1] * (half - 1) + [0]        # one driver more than a block; a fan-out one ABOVE the threshold
    fans += [2 * PART + 1]                           # heavy: three parts
    fans += [TS]                                     # exactly the sink budget: still whole, alone in its tile ...
    fans += [3, 5, 2, 1, 0, 2, 1, 1, 0, 4, 1, 2]     # ... which the next driver closes by the sink budget
    # (2 TILE_DRIVERS + TILE_DRIVERS / 2 + 1 drivers in all: with the sink budget lifted the last tile holds one block + 1)
    return fans


CONSUMERS_PER_SINK = (1, 0, 4, 5, 2, 9, 3, 1, 4, 0, 5, 2)      # cycled over the sinks; 5 is the first CSR-tail case
MANY_CONSUMERS_SINK = 40                                      # this sink gets PAIR_HEAVY_OUT + 1 consumers (the pulls' heavy path)
CONSUMER_FAN_IN = (1, 2, 3, 1, 4, 2, 6, 1, 3, 2)               # cycled over the consumers


class Case:
    pass


def build_case(regime):
    """The graph, its level lists and every input tensor (fp32 on the CPU; h, A, LSE, DA, G0 are [N, 128])."""
    assert regime in ('unit', 'wide')
    c = Case()
    c.regime = regime
    fans = driver_fanouts()
    nD, nS = len(fans), int(sum(fans))
    c.drv = np.arange(nD)
    c.snk = np.arange(nD, nD + nS)
    c.sink_driver = np.repeat(np.arange(nD), fans)                         # driver of every sink, in sink order
    ncons = [CONSUMERS_PER_SINK[i % len(CONSUMERS_PER_SINK)] for i in range(nS)]
    ncons[MANY_CONSUMERS_SINK] = ops.PAIR_HEAVY_OUT + 1
    # deal the sinks' out-edges to the consumers round by round (first every sink's first edge, then the second ones, ...):
    # a consumer takes the next CONSUMER_FAN_IN stubs and closes early rather than take one sink twice
    stubs = [w for k in range(max(ncons)) for w in range(nS) if ncons[w] > k]
    cons_in, i, k = [], 0, 0
    while i < len(stubs):
        want, mine = CONSUMER_FAN_IN[k % len(CONSUMER_FAN_IN)], []
        while i < len(stubs) and len(mine) < want and stubs[i] not in mine:
            mine.append(stubs[i]); i += 1
        cons_in.append(mine); k += 1
    nC = len(cons_in)
    c.cons = np.arange(nD + nS, nD + nS + nC)
    c.N = N = nD + nS + nC
    net_src, net_dst = c.sink_driver, c.snk
    cell_src = np.array([c.snk[w] for mine in cons_in for w in mine])
    cell_dst = np.array([c.cons[j] for j, mine in enumerate(cons_in) for _ in mine])
    c.graph = PinGraph(N, {'net': (net_src, net_dst), 'cell': (cell_src, cell_dst)})
    c.levels = [c.drv.tolist(), c.snk.tolist(), c.cons.tolist()]
    c.fans = np.array(fans)

    # ---- values
    lo, hi = -1.0, 2.0                                                     # a third of the entries <= 0
    h = det_uniform((N, D), 11, lo, hi)
    if regime == 'wide':
        taken = set()
        for j, mine in enumerate(cons_in):
            if len(mine) < 2 or j % 2 == 0 or j % 10 == 9 or mine[0] in taken or mine[1] in taken \
                    or MANY_CONSUMERS_SINK in mine[:2]:
                continue
            a, b = c.snk[mine[0]], c.snk[mine[1]]
            # j % 4 == 1: in-neighbours near +40 and -40 (h - LSE ~ -80);  j % 4 == 3: near +40 and +38 (|LSE| ~ 40, h - LSE ~ -2)
            h[a] = 40.0 + det_uniform((D,), 1000 + j, -2, 2)
            h[b] = (-40.0 if j % 4 == 1 else 38.0) + det_uniform((D,), 2000 + j, -2, 2)
            taken.update(mine[:2])
    for r in range(0, nD + nS, 5):                                         # a few exact zeros on driver and sink rows
        h[r, (7 * r + 3) % D] = 0.0
    eq = next(j for j, mine in enumerate(cons_in) if len(mine) == 2 and j % 10 == 9)
    h[c.snk[cons_in[eq][1]]] = h[c.snk[cons_in[eq][0]]]                    # a fan-in-2 consumer with equal in-neighbours
    c.equal_consumer = int(c.cons[eq])
    c.h = torch.from_numpy(h)
    c.G0 = torch.from_numpy(det_uniform((N, D), 12))                       # own-row gradients (used where `own` is set)
    c.DA0 = torch.from_numpy(det_uniform((N, D), 13))
    own = (det_uniform((N,), 14) > 0).astype(np.uint8)
    c.own = torch.from_numpy(own)
    hn = det_uniform((N, HID), 15)
    hn[np.abs(hn) < 0.05] = 0.0                                            # mixed signs and some exact zeros
    c.HN = B.r(torch.from_numpy(hn))
    c.W1g = B.r(torch.from_numpy(det_uniform((HID, D), 16, -0.1, 0.1)))    # fc_cell_neigh: Linear(128, 256)
    c.W2g = B.r(torch.from_numpy(det_uniform((D, HID), 17, -0.1, 0.1)))    # ... Linear(256, 128)

    # ---- the cone mask of the `active` case, consistent the way a fan-in cone is: an active consumer has active
    # in-neighbours, an active sink an active driver
    act = np.ones(N, dtype=np.uint8)
    whole = c.fans <= PinGraph.BWD_PAIR_TILE_SINKS
    off_drv = np.array([v for v in range(nD) if v % 5 == 2 and whole[v]] + [int(np.nonzero(~whole)[0][0])])
    act[off_drv] = 0
    act[c.snk[np.isin(c.sink_driver, off_drv)]] = 0
    for j, mine in enumerate(cons_in):
        if j % 3 == 0 or any(act[c.snk[w]] == 0 for w in mine):
            act[c.cons[j]] = 0
    c.active = torch.from_numpy(act)

    # ---- A, LSE of the consumers from the fp64 forward, rounded to fp32 (what the kernels are given)
    ip, ix = c.graph.csr_host('in', 'cell')
    h64 = c.h.double()
    A = torch.zeros((N, D), dtype=torch.float64)
    LSE = torch.zeros((N, D), dtype=torch.float64)
    A[c.cons] = R.seg_softmax_sum(h64, ip, ix, c.cons)
    for v in c.cons:
        LSE[v] = torch.logsumexp(h64[ix[ip[v]:ip[v + 1]]], 0)
    c.A, c.LSE = A.float(), LSE.float()
    return c


# ---------------------------------------------------------------------------------------------------------------- row classes
def row_classes(c, active=None):
    """Row ids per class: sinks by consumer count, drivers by {0 sinks, whole, heavy}; with `active`, the rows inside the mask."""
    cdeg = np.diff(c.graph.csr_host('out', 'cell')[0])
    keep = np.ones(c.N, bool) if active is None else active.numpy().astype(bool)
    out = {}
    for k in sorted(set(cdeg[c.snk].tolist())):
        out[f'sink_c{k}'] = c.snk[(cdeg[c.snk] == k) & keep[c.snk]]
    TS = PinGraph.BWD_PAIR_TILE_SINKS
    out['drv_0'] = c.drv[(c.fans == 0) & keep[c.drv]]
    out['drv_whole'] = c.drv[(c.fans > 0) & (c.fans <= TS) & keep[c.drv]]
    out['drv_heavy'] = c.drv[(c.fans > TS) & keep[c.drv]]
    return {k: v for k, v in out.items() if v.size}


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def class_errors(got, ref, classes):
    """max |got - ref| / max |ref| PER CLASS of rows: one number over the whole tensor hides a small-magnitude class (a sink
    without consumers) behind a large one (a driver of 65 sinks)."""
    return {k: rel_err(got[rows], ref[rows]) for k, rows in classes.items()}


# ------------------------------------------------------------------------------------------------------------------ reference
def reference(c, relu=True, active=None, dtype=torch.float64, width=D, plain_relu=False):
    """[N, width] tensor whose driver and sink rows hold G: autograd of the restated forward in `dtype` (fp64: the reference;
    fp32: its own rounding spread e_32).  active: uint8 [N] cone mask - consumers outside it are dropped, rows outside it are 0.
    plain_relu: torch.relu itself as the activation - the same thing wherever h >= 0 (the CPU test holds the two together)."""
    h = c.h[:, :width].to(dtype)
    keep = torch.ones(c.N, dtype=torch.bool) if active is None else active.bool()
    act = (lambda z: torch.where(z > 0, z, z.detach())) if relu else (lambda z: z)
    if plain_relu:
        assert relu
        act = torch.relu
    zv = h[c.drv].clone().requires_grad_(True)
    zw = h[c.snk].clone().requires_grad_(True)
    hv = act(zv)
    carry = hv[c.sink_driver]
    hw = act(zw + (carry - carry.detach()))                   # pre_w + h_v with pre_w = h_w - h_v: the value is h_w
    ip, ix = c.graph.csr_host('in', 'cell')
    mail = hw[torch.from_numpy(ix - c.snk[0])]                # one row per cell in-edge, in in-CSR order
    cons = c.cons[keep[c.cons].numpy()]
    a = R.seg_softmax_sum(mail, ip, np.arange(ix.shape[0]), cons)
    own = (c.own.bool() & keep).to(dtype)[:, None]
    g = c.G0[:, :width].to(dtype)
    loss = (a * c.DA0[cons, :width].to(dtype)).sum() + (hw * (g * own)[c.snk]).sum() + (hv * (g * own)[c.drv]).sum()
    loss.backward()
    out = torch.zeros((c.N, width), dtype=dtype)
    out[c.drv], out[c.snk] = zv.grad, zw.grad
    return out


def formula(c, relu=True, active=None, defect=None, width=D):
    """The kernels' closed form in fp64 from the fp32 A / LSE they are given; `defect` switches one mistake on."""
    assert defect is None or defect in DEFECTS
    TS, PART = PinGraph.BWD_PAIR_TILE_SINKS, PinGraph.BWD_PAIR_PART
    h, g = c.h[:, :width].double(), c.G0[:, :width].double()
    A, LSE, DA = c.A[:, :width].double(), c.LSE[:, :width].double(), c.DA0[:, :width].double()
    keep = torch.ones(c.N, dtype=torch.bool) if active is None else active.bool()
    cptr, cidx = c.graph.csr_host('out', 'cell')
    src = np.repeat(np.arange(c.N), np.diff(cptr))
    k = np.arange(cidx.shape[0]) - cptr[src]                               # position of the edge among its sink's consumers
    use = torch.ones(cidx.shape[0], dtype=torch.bool) if defect == 'inactive_counted' else keep[cidx]
    if defect == 'drop_tail':
        use = use & torch.from_numpy(k < 4)
    lse = B.r(LSE[cidx]) if defect == 'lse_bf16' else LSE[cidx]
    one = 0.0 if defect == 'no_one' else 1.0
    term = DA[cidx] * torch.exp(h[src] - lse) * (one + h[src] - A[cidx])
    S = torch.zeros_like(h).index_add_(0, torch.from_numpy(src), term * use[:, None])
    own = torch.ones(c.N, 1, dtype=torch.float64) if defect == 'own_ignored' else c.own.double()[:, None]
    out = torch.zeros_like(h)
    gw = (own * g + S)[c.snk]
    mask = lambda x, hrows: x * ((x > 0) if defect == 'mask_from_grad' else (hrows > 0)) if relu else x
    out[c.snk] = mask(gw, h[c.snk]) * keep[c.snk][:, None]
    contrib = out[c.snk].clone()
    if defect == 'drop_last_part':
        start = np.concatenate([[0], np.cumsum(c.fans)])[c.sink_driver]
        pos = np.arange(c.snk.size) - start
        f = c.fans[c.sink_driver]
        last = (f > TS) & (pos >= (-(-f // PART) - 1) * PART)
        contrib[torch.from_numpy(last)] = 0.0
    T = torch.zeros((c.drv.size, width), dtype=torch.float64).index_add_(0, torch.from_numpy(c.sink_driver), contrib)
    out[c.drv] = mask((own * g)[c.drv] + T, h[c.drv]) * keep[c.drv][:, None]
    return out


def g_bounds(c, relu=True, active=None, width=D):
    """(fp64 reference, classes, e_32 per class, bound per class): bound = max(G_FLOOR, E32_MARGIN e_32), e_32 the same autograd
    reference evaluated in fp32 - an fp32 LSE near 40 carries 4e-6 into an exponent whatever a kernel does."""
    ref = reference(c, relu, active, torch.float64, width)
    classes = row_classes(c, active)
    e32 = class_errors(reference(c, relu, active, torch.float32, width), ref, classes)
    return ref, classes, e32, {k: max(G_FLOOR, E32_MARGIN * e) for k, e in e32.items()}


def mlp_reference(c, G_drivers, DHN_kernel):
    """The MLP phase judged decoupled: from the kernel's own G rows of the drivers, DHN = (bf16(G) W2g) * (HN > 0); from the
    kernel's own DHN, DA = bf16(DHN) W1g.  fp64 arithmetic on bf16-rounded operands (the weights are bf16-representable)."""
    dhn = (B.r(G_drivers.double().cpu()) @ c.W2g.double()) * (c.HN[c.drv] > 0)
    da = B.r(DHN_kernel.double().cpu()) @ c.W1g.double()
    return dhn, da


# --------------------------------------------------------------------------------------------------------------- edge presence
def edge_report(c, graph=None):
    """{edge case: present?} read from the tables the kernels get: tile rows by (count, parts, sink range), slot rows by
    cslots[:, 3], fan-outs from the CSRs.  graph: c.graph or a copy of it on a device."""
    g = c.graph if graph is None else graph
    TD, TS, PART, HO = PinGraph.BWD_PAIR_TILE_DRIVERS, PinGraph.BWD_PAIR_TILE_SINKS, PinGraph.BWD_PAIR_PART, ops.PAIR_HEAVY_OUT
    rep = {'fold_schedule': g.fold_schedule(c.levels) is not None}
    pairs = g.level_bwd_pairs(c.levels)
    rep['level_bwd_pairs'] = pairs is not None and pairs[1][0] is not None
    if not rep['level_bwd_pairs']:
        return rep
    cslots, tiles = pairs[0].cpu().numpy(), pairs[1][0]['tiles'].cpu().numpy()
    optr = g.csr_host('out', 'net')[0]
    cptr = g.csr_host('out', 'cell')[0]
    iptr, iidx = g.csr_host('in', 'cell')
    fan = np.diff(optr)[c.drv]
    rep['tiles_cover_drivers_once'] = sorted(np.concatenate([np.arange(t[0], t[0] + t[1]) for t in tiles if t[2] == 0]).tolist()) \
        == c.drv.tolist()
    for name, f in (('driver_0_sinks', 0), ('driver_1_sink', 1), ('driver_TILE_SINKS_whole', TS), ('driver_TILE_SINKS+1', TS + 1),
                    ('driver_2PART', 2 * PART), ('driver_2PART+1', 2 * PART + 1), ('fanout_HEAVY_OUT', HO), ('fanout_HEAVY_OUT+1', HO + 1)):
        rep[name] = bool((fan == f).any())
    rep['fanout_above_3x8'] = bool((fan > 3 * PULL_HEAVY_GROUPS).any())

    def parts_of(f):
        return sorted((int(t[2]), int(t[3]), int(t[7] - t[6])) for t in tiles if t[3] > 0 and fan[t[0] - c.drv[0]] == f)
    rep['whole_at_TILE_SINKS'] = any(t[3] == 0 and t[1] == 1 and t[7] - t[6] == TS for t in tiles)
    rep['parts_of_TILE_SINKS+1'] = parts_of(TS + 1) == [(0, 2, PART), (1, 2, TS + 1 - PART)] and TS + 1 - PART == 1
    rep['parts_of_2PART'] = parts_of(2 * PART) == [(0, 2, PART), (1, 2, PART)]
    rep['parts_of_2PART+1'] = parts_of(2 * PART + 1) == [(0, 3, PART), (1, 3, PART), (2, 3, 1)]
    heavy = sorted({int(t[0]) for t in tiles if t[3] > 0})
    whole_v0 = [int(t[0]) for t in tiles if t[3] == 0]
    rep['heavy_drivers_apart'] = len(heavy) >= 3 and all(any(a < v < b for v in whole_v0) for a, b in zip(heavy, heavy[1:]))
    whole = [t for t in tiles if t[3] == 0]
    rep['tile_closed_by_TILE_DRIVERS'] = any(t[1] == TD for t in whole)
    rep['tile_closed_by_sink_budget'] = any(
        t[1] < TD and t[0] + t[1] <= c.drv[-1] and fan[t[0] + t[1] - c.drv[0]] <= TS and (t[7] - t[6]) + fan[t[0] + t[1] - c.drv[0]] > TS
        for t in whole)
    rep['tile_of_16_drivers'] = any(t[1] == PAIR_GROUPS for t in whole)
    rep['tile_of_17_drivers'] = any(t[1] == PAIR_GROUPS + 1 for t in whole)
    rep['tile_with_partial_round'] = any((t[7] - t[6]) % PAIR_GROUPS for t in whole)
    rep['no_tile_above_its_limits'] = all(t[1] <= TD and t[7] - t[6] <= max(TS, PART) for t in tiles)
    cdeg = np.diff(cptr)
    for k in (0, 1, 4, 5, 9):
        rep[f'sink_with_{k}_consumers'] = bool((cdeg[c.snk] == k).any())
    rep['sink_above_HEAVY_OUT_consumers'] = bool((cdeg[c.snk] > HO).any())
    many = c.snk[cdeg[c.snk] > 4]
    rep['csr_tail_slots'] = bool((cslots[many, 3] == -2 - (cptr[many] + 3)).all() and (cslots[many, 3] <= -2).all()
                                 and (cslots[c.snk[cdeg[c.snk] <= 4], 3] >= -1).all())
    rep['slots_count_consumers'] = all(int((cslots[w] >= 0).sum()) == min(int(cdeg[w]), 4) - (cdeg[w] > 4) for w in c.snk)
    ideg = np.diff(iptr)[c.cons]
    rep['consumer_fan_in_1'] = bool((ideg == 1).any())
    rep['consumer_fan_in_3_or_more'] = bool((ideg >= 3).any())
    e = iidx[iptr[c.equal_consumer]:iptr[c.equal_consumer + 1]]
    rep['consumer_fan_in_2_equal_values'] = e.size == 2 and e[0] != e[1] and bool(torch.equal(c.h[e[0]], c.h[e[1]]))
    # values
    rows = np.concatenate([c.drv, c.snk])
    share = float((c.h[rows] <= 0).float().mean())
    rep['a_third_non_positive'] = 0.25 < share < 0.45
    rep['a_few_exact_zeros'] = 0 < int((c.h[rows] == 0).sum()) < rows.size
    for name, r in (('drivers', c.drv), ('sinks', c.snk)):
        rep[f'own_on_half_of_the_{name}'] = 0.3 < float(c.own[r].float().mean()) < 0.7
    src = np.repeat(np.arange(c.N), cdeg)
    x = c.h[src].double() - c.LSE[g.csr_host('out', 'cell')[1]].double()
    if c.regime == 'wide':
        rep['wide_h_minus_LSE_near_-80'] = float(x.min()) < -75
        rep['wide_LSE_near_40'] = float(c.LSE[c.cons].abs().max()) > 38
        rep['wide_large_LSE_that_matters'] = bool(((c.LSE[g.csr_host('out', 'cell')[1]] > 35) & (x.float() > -3) & (x.float() < -1)).any())
    else:
        rep['unit_h_within_2'] = float(c.h.abs().max()) <= 2
    hn = c.HN[c.drv]
    rep['HN_mixed_signs_and_zeros'] = bool((hn > 0).any() and (hn < 0).any() and (hn == 0).any())
    a = c.active.numpy().astype(bool)
    rep['active_is_a_cone'] = all(a[iidx[iptr[v]:iptr[v + 1]]].all() for v in c.cons if a[v]) and \
        bool(a[c.drv[c.sink_driver]][a[c.snk]].all())
    rep['active_drops_rows_and_consumers'] = bool((~a[c.drv]).any() and (~a[c.snk]).any() and (~a[c.cons]).any()) and \
        any(a[w] and (~a[g.csr_host('out', 'cell')[1][cptr[w]:cptr[w + 1]]]).any() for w in c.snk)
    return rep


def heavy_rows(c, rows):
    """The rows of one level above the pulls' heavy threshold (what PinGraph.level_meta hands the sweep), as an int32 tensor."""
    optr, cptr = c.graph.csr_host('out', 'net')[0], c.graph.csr_host('out', 'cell')[0]
    deg = np.diff(optr)[rows] + np.diff(cptr)[rows]
    return torch.from_numpy(rows[deg > ops.PAIR_HEAVY_OUT].astype(np.int32))
