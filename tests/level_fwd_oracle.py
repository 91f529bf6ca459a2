"""One hand-built (net level, cell level) pair of the FORWARD level chain and its fp64 reference  --  TEST INFRASTRUCTURE, NOT
PRODUCT CODE.

The forward level kernels (mmft_level_fwd_slots, mmft_level_fwd_bf16, their *_infer twins, mmft_pair_fwd_gather +
mmft_mlp2_rows_bf16, all through csrc/fold_gather.h) are held to this module by tests/test_level_fwd_gpu.py;
tests/test_level_fwd_cpu.py checks on the CPU that the graph holds every edge case it is built for and that the checks notice
the mistakes a kernel could make.  Plain numpy / torch on the CPU.

Graph, five levels of contiguous ids: L0 cells, L1 nets (the OLDER net level, one driver each in L0), L2 cells, L3 nets (the
FOLDED level: one driver each in L2; its rows of h are written by the launch and NaN before it), L4 cells (the level under
test).  The L4 rows of fan-in <= 4 come first (the slot form's sub-range), the wider ones after them.  Which nets a row reads
is written down below (patterns cycled over the rows and a few rows given by hand), not drawn; every kernel table comes from
PinGraph (csr, cell_edge_drivers, fold_schedule, level_slots).

`reference`: net rows act(PRE + h[driver]); x_e that value for an L3 source and h[u] for an L1 source; A = sum softmax(x) x
through R.seg_softmax_sum and LSE = logsumexp(x), both 0 at fan-in 0.  The MLP is judged link by link from the kernel's OWN
previous output (`judge`): hid against relu(r(A_kernel) W1^T + b1), h against act(h0 + r(hid_kernel) W2^T + b2), r = the bf16
rounding of oracle/bf16.py - a flip of bf16(A) at a rounding boundary then cannot blur the check.

`formula` is the closed form the kernels are documented to evaluate, written as a launch (it takes the input buffers and
returns them as a kernel would leave them).  It exists to be BROKEN: each entry of DEFECTS switches one mistake on, and the CPU
test demands that `judge` sees it at more than ten times a bound.
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
# constants of the kernels, not of the host: a slot row holds four edges (LevelSlotsCommon), fold_gather_edges requests four
# edges together, a tile is 16 rows (one MFMA block; the slot form takes two per workgroup from RB2_ROWS rows on, see
# level_slots_rb), the gather's heavy path strides eight thread groups over a row's edges
SLOT_W = 4
BATCH = 4
TILE = 16
HEAVY_GROUPS = 8
RB2_ROWS = 32 * 192
TOL = 2e-5                # what tests/test_kernels_gpu.py holds seg_softmax_sum to
E32_MARGIN = 4            # over the reference's own fp32 spread, as tests/level_pair_oracle.py
EXACT = 2e-6              # fp32 accumulation of exact bf16 products (tests/test_bf16_gpu.py)
SENT = 777.0              # finite filler of everything a launch must not touch (and of PRE outside L3)
NAN = float('nan')
SIZES = ('small', 'rb2_nets', 'rb2_cells')
REGIMES = ('unit', 'wide')
SUB_COUNTS = (1, 15, 16, 17, 33)           # cell counts passed as sub-ranges of the slot rows (small)
DEFECTS = ('drop_tail', 'pre_on_older', 'net_relu_dropped', 'multi_edge_once', 'no_max', 'lse_no_max', 'fanin0_nan', 'mean',
           'A_unrounded', 'hid_unrounded', 'no_residual', 'no_final_act', 'inactive_written')

N0, N1, N2 = 24, 40, 24
# L3 nets with a role (all of them driven by L2's first cell, as every fourth net is)
NET_EQ = (0, 4)           # equal PRE, same driver: a tie in the running max of the row that reads both
NET_NEG = 8               # PRE + h[driver] < 0 in every channel
NET_P40, NET_M40, NET_P38 = 12, 16, 20      # `wide`: near +40, -40, +38
OLD_P40, OLD_M40, OLD_P90, OLD_M20 = 1, 2, 3, 5   # `wide`, L1 nets: near +40, -40 and the pair 110 apart
# slot rows given by hand: ('f', k) = net k of L3 (folded), ('o', k) = net k of L1 (older)
SPECIAL_ROWS = {
    1: [('f', NET_NEG)],
    2: [('f', NET_EQ[0]), ('f', NET_EQ[1])],
    3: [('f', 5), ('f', 5)],
    16: [('o', OLD_P40), ('o', OLD_M40)],
    17: [('f', NET_P40), ('f', NET_M40)],
    18: [('f', NET_P40), ('f', NET_P38)],
    19: [('o', OLD_P90), ('o', OLD_M20)],
    20: [('f', NET_P40), ('o', OLD_M40), ('f', NET_P38), ('o', OLD_P40)],
}


class Case:
    pass


def _readable(n3):
    """The L3 nets that L4 rows may read; every tenth net is read by nobody."""
    return [k for k in range(n3) if k % 10 != 9]


def slot_row_sources(i, n3):
    """Sources of the i-th row of fan-in <= 4, in edge order."""
    if i in SPECIAL_ROWS:
        return SPECIAL_ROWS[i]
    rd = _readable(n3)
    f = lambda j: ('f', rd[(83 * j) % len(rd)])
    o = lambda j: ('o', (7 * j + 3) % N1)
    return [[],
            [f(i)],
            [f(i), f(i + 1)],
            [f(i), f(i)],                               # a multi-edge
            [f(i), f(i + 1), f(i + 2)],
            [f(i), f(i + 1), f(i + 2), f(i + 3)],       # slots full
            [o(i), f(i), f(i + 1)],                     # an older-level edge in slot 0
            [f(i), o(i), f(i + 1), f(i + 2)],           # ... in the middle
            [f(i), f(i + 1), f(i + 2), o(i)],           # ... last
            [o(i), o(i + 1)],                           # every edge from the older level
            [f(i), f(i + 1), f(i), o(i)],               # a multi-edge in a full row
            [o(i)]][i % 12]


def wide_fanins():
    """Fan-ins of the rows past the slot width, in row order: the index form's batches (a missing edge of the last batch
    repeats an edge of the row) up to the heavy threshold, then the gather's heavy path (8 thread groups striding)."""
    H = ops.PAIR_HEAVY_IN
    return [SLOT_W + 1, 2 * BATCH, 2 * BATCH + 1, H, H + 1, H + HEAVY_GROUPS, H + HEAVY_GROUPS + 1, 200]


def wide_row_sources(w, fan, n3):
    rd = _readable(n3)
    return [('o', (3 * j + w) % N1) if j % 4 == 2 else ('f', rd[(j + 13 * w) % len(rd)]) for j in range(fan)]


def build_case(regime, size):
    """The graph, its level lists and every input tensor (fp32 on the CPU; h, PRE are [N, 128])."""
    assert regime in REGIMES and size in SIZES
    c = Case()
    c.regime, c.size = regime, size
    n3 = {'small': 90, 'rb2_nets': RB2_ROWS + 17, 'rb2_cells': 40}[size]
    n_slot = {'small': 6 * TILE + 8, 'rb2_nets': 75, 'rb2_cells': RB2_ROWS + 33}[size]
    fans = wide_fanins() if size == 'small' else []
    rows = [slot_row_sources(i, n3) for i in range(n_slot)] + [wide_row_sources(w, f, n3) for w, f in enumerate(fans)]
    n4 = len(rows)
    starts = np.cumsum([0, N0, N1, N2, n3, n4])
    c.N = N = int(starts[-1])
    c.L = [np.arange(starts[i], starts[i + 1]) for i in range(5)]
    L0, L1, L2, L3, L4 = c.L
    c.levels = [l.tolist() for l in c.L]
    drv1 = L0[np.arange(N1) % N0]
    drv3 = np.where(np.arange(n3) % 4 == 0, L2[0], L2[1 + np.arange(n3) % (N2 - 1)])
    net_src, net_dst = np.concatenate([drv1, drv3]), np.concatenate([L1, L3])
    node = {'f': L3, 'o': L1}
    cell_src = np.array([L1[j % N1] for j in range(N2)] + [node[t][k] for r in rows for t, k in r])
    cell_dst = np.array(L2.tolist() + [L4[i] for i, r in enumerate(rows) for _ in r])
    c.graph = PinGraph(N, {'net': (net_src, net_dst), 'cell': (cell_src, cell_dst)})
    c.net_range = (int(L3[0]), n3)
    c.slot_range = (int(L4[0]), n_slot)
    c.cell_range = (int(L4[0]), n4)
    c.drv3 = drv3

    # ---- values: a third of the net values <= 0
    h = det_uniform((N, D), 21, -1.0, 2.0)
    pre = np.full((N, D), SENT, dtype=np.float32)
    pre[L3] = det_uniform((n3, D), 22, -1.5, 1.5)
    for k in range(0, n3, 7):                                              # a few exact zeros among the net values
        ch = (5 * k + 1) % D
        pre[L3[k], ch] = -h[drv3[k], ch]
    for k in range(0, N1, 6):                                              # ... and among the older rows
        h[L1[k], (3 * k + 2) % D] = 0.0
    pre[L3[NET_EQ[1]]] = pre[L3[NET_EQ[0]]]
    pre[L3[NET_NEG]] = -3.0 - np.abs(h[drv3[NET_NEG]])
    if regime == 'wide':
        u = lambda seed, a: det_uniform((D,), seed, -a, a)
        h[L1[OLD_P40]], h[L1[OLD_M40]] = 40.0 + u(31, 2), -40.0 + u(32, 2)
        h[L1[OLD_P90]], h[L1[OLD_M20]] = 90.0 + u(33, 1), -20.0 + u(34, 1)
        for k, (t, a, seed) in {NET_P40: (40.0, 2, 35), NET_M40: (-40.0, 2, 36), NET_P38: (38.0, 1, 37)}.items():
            pre[L3[k]] = (t + u(seed, a)) - h[drv3[k]]
    h[L3] = NAN                                                            # written by the launch; never to be read
    c.h, c.PRE = torch.from_numpy(h), torch.from_numpy(pre)
    c.W1 = B.r(torch.from_numpy(det_uniform((HID, D), 23, -0.1, 0.1)))     # fc_cell_neigh: Linear(128, 256)
    c.W2 = B.r(torch.from_numpy(det_uniform((D, HID), 24, -0.1, 0.1)))     # ... Linear(256, 128)
    c.b1 = torch.from_numpy(det_uniform((HID,), 25, -0.1, 0.1))
    c.b2 = torch.from_numpy(det_uniform((D,), 26, -0.1, 0.1))

    # ---- the cone mask: an active cell has active in-neighbours, an active net an active driver.  Two whole 16-row tiles
    # (one 32-row tile) of slot rows are outside it, every seventh slot row, one light and one heavy wide row, and every
    # second net that nobody reads
    act = np.ones(N, dtype=np.uint8)
    i = np.arange(n_slot)
    act[L4[:n_slot][((i >= 2 * TILE) & (i < 4 * TILE)) | (i % 7 == 5)]] = 0
    if fans:
        act[L4[n_slot + 1]] = 0
        act[L4[n_slot + 6]] = 0
    act[L3[np.arange(n3) % 20 == 19]] = 0
    c.active = torch.from_numpy(act)
    return c


# ------------------------------------------------------------------------------------------------------------- tables, classes
def tables(c, graph=None):
    """What the kernels get from PinGraph, on the graph's device."""
    g = c.graph if graph is None else graph
    fold = g.fold_schedule(c.levels)
    slots, net_drv, max_in = g.level_slots(c.levels)
    return dict(fold=fold, slots=slots, net_drv=net_drv, max_in=max_in, in_net=g.csr('in', 'net'), in_cell=g.csr('in', 'cell'),
                drv=g.cell_edge_drivers(), heavy=fold[4]['heavy_in'])


def cell_fan_in(c):
    return np.diff(c.graph.csr_host('in', 'cell')[0])


def row_classes(c, cell_rows, active=None):
    """Row ids per class among `cell_rows`: by fan-in {0, 1, 2-4, 5-HEAVY_IN, heavy}, and the rows with an older-level edge
    (a class across the others); with `active`, the rows inside the mask."""
    ip, ix = c.graph.csr_host('in', 'cell')
    rows = np.asarray(cell_rows, dtype=np.int64)
    if active is not None:
        rows = rows[active.numpy().astype(bool)[rows]]
    deg = np.diff(ip)[rows]
    H = ops.PAIR_HEAVY_IN
    out = {'f0': rows[deg == 0], 'f1': rows[deg == 1], 'f2_4': rows[(deg >= 2) & (deg <= SLOT_W)],
           'f5_H': rows[(deg > SLOT_W) & (deg <= H)], 'heavy': rows[deg > H]}
    L3 = c.L[3]
    dst = np.repeat(np.arange(c.N), np.diff(ip))
    n_old = np.bincount(dst[(ix < L3[0]) | (ix > L3[-1])], minlength=c.N)
    out['older'] = rows[n_old[rows] > 0]
    return {k: v for k, v in out.items() if v.size}


def rel_err(got, ref):
    """max |got - ref| / max |ref|; inf when `got` is not finite where `ref` is."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    e = float((got - ref).abs().max() / (ref.abs().max() + 1e-30)) if ref.numel() else 0.0
    return e if np.isfinite(e) else float('inf')


def same_bits(a, b):
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    iv = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(iv), b.view(iv))


# ------------------------------------------------------------------------------------------------------------------ reference
def _act(relu):
    return torch.relu if relu else (lambda z: z)


def seg_lse(h, indptr, indices, nodes):
    """logsumexp over the in-edges per channel, 0 at fan-in 0; degree buckets as R.seg_softmax_sum."""
    start, deg = R._in_edges(indptr, indices, nodes)
    out = h.new_zeros((len(nodes), h.shape[1]))
    for d in np.unique(deg):
        if d == 0:
            continue
        sel = np.nonzero(deg == d)[0]
        eid = start[sel][:, None] + np.arange(d)[None, :]
        out = out.index_copy(0, torch.from_numpy(sel), torch.logsumexp(h[torch.from_numpy(indices[eid])], dim=1))
    return out


def reference(c, relu=True, active=None, dtype=torch.float64):
    """{'net': [n3, 128], 'A', 'LSE': [n4, 128]} in `dtype` (fp64: the reference; fp32: its own rounding spread e_32).
    active: the net rows outside the mask are NOT written - they stay NaN, and a cell row inside the mask that reads one is
    NaN too (the mask must be a cone)."""
    L3, L4 = c.L[3], c.L[4]
    h = c.h.to(dtype).clone()
    net = _act(relu)(c.PRE[L3].to(dtype) + h[c.drv3])
    h[L3] = net
    if active is not None:
        h[L3[~active.numpy().astype(bool)[L3]]] = NAN
    ip, ix = c.graph.csr_host('in', 'cell')
    return {'net': net, 'A': R.seg_softmax_sum(h, ip, ix, L4), 'LSE': seg_lse(h, ip, ix, L4)}


_cache = {}


def references(c, relu, active):
    """(fp64 reference, fp32 reference) of a case: computed once per (case, relu, mask), never changed."""
    key = (c.regime, c.size, relu, active is not None)
    if key not in _cache:
        _cache[key] = (reference(c, relu, active), reference(c, relu, active, torch.float32))
    return _cache[key]


def mlp_links(c, A_kernel, hid_kernel, h0, relu):
    """(hid_ref, h_ref) in fp64 for rows whose A / hid came out of the kernel and whose h was h0 before the launch."""
    hid = torch.relu(B.r(A_kernel.double()) @ c.W1.double().T + c.b1.double())
    h = _act(relu)(h0.double() + B.r(hid_kernel.double()) @ c.W2.double().T + c.b2.double())
    return hid, h


# --------------------------------------------------------------------------------------------------------- a launch, and judging it
def inputs(c, hid16=False):
    """The buffers of one launch: h (NaN at the L3 rows), PRE, and A / LSE / hid filled with the sentinel."""
    full = lambda w, dt: torch.full((c.N, w), SENT, dtype=dt)
    return {'h': c.h.clone(), 'PRE': c.PRE.clone(), 'A': full(D, torch.float32), 'LSE': full(D, torch.float32),
            'hid': full(HID, torch.bfloat16 if hid16 else torch.float32)}


def judge(c, before, after, relu, active, net_range, cell_rows, links=('net', 'A', 'LSE', 'hid', 'h'), tag=None):
    """{(link, class): error / bound} of one launch - `before` / `after` are the buffers of `inputs` around it, net_range the
    net rows it was given (or None) and cell_rows the cell rows.  Every link of DESIGN 3.4b's forward net:
      net    the net rows, bit for bit fp32 act(PRE + h[driver]);
      A, LSE per class of rows, relative to the class's scale, against max(TOL, E32_MARGIN e_32);
      hid    against relu(r(A_kernel) W1^T + b1): EXACT of the class scale (fp32 storage), 2^-8 |ref| + EXACT scale per element (bf16);
      h      against act(h0 + r(hid_kernel) W2^T + b2): EXACT of the class scale;
      kept   (always) every row outside the launch's rows keeps its bits in h, PRE, A, LSE, hid; with a net range no row of it
             inside the mask is left NaN.
    A ratio above 1 is a failure; inf stands for a NaN or a touched row.  With `tag` every figure is printed."""
    cell_rows = np.asarray(cell_rows, dtype=np.int64)
    keep = np.ones(c.N, bool) if active is None else active.numpy().astype(bool)
    ref, ref32 = references(c, relu, active)
    L3, L4 = c.L[3], c.L[4]
    classes = row_classes(c, cell_rows, active)
    out, fig = {}, {}
    nrows = np.arange(net_range[0], net_range[0] + net_range[1]) if net_range is not None else np.zeros(0, np.int64)
    nrows = nrows[keep[nrows]]
    if 'net' in links and nrows.size:
        want = _act(relu)(c.PRE[nrows] + before['h'][c.drv3[nrows - L3[0]]])                  # fp32: one add and a select
        out[('net', 'net')] = 0.0 if torch.equal(after['h'][nrows], want) else float('inf')
    for name in ('A', 'LSE'):
        if name in links:
            for k, rows in classes.items():
                e32 = rel_err(ref32[name][rows - L4[0]], ref[name][rows - L4[0]])
                bound = max(TOL, E32_MARGIN * e32)
                err = rel_err(after[name][rows], ref[name][rows - L4[0]])
                out[(name, k)], fig[(name, k)] = err / bound, (err, e32, bound)
    if 'hid' in links or 'h' in links:
        for k, rows in classes.items():
            hid_ref, h_ref = mlp_links(c, after['A'][rows], after['hid'][rows].float(), before['h'][rows], relu)
            if 'hid' in links:
                got, scale = after['hid'][rows].double(), float(hid_ref.abs().max())
                if after['hid'].dtype == torch.bfloat16:
                    r_ = ((got - hid_ref).abs() / (2.0 ** -8 * hid_ref.abs() + EXACT * scale + 1e-300)).max()
                    out[('hid', k)] = float(r_) if bool(torch.isfinite(r_)) else float('inf')
                    fig[('hid', k)] = (rel_err(got, hid_ref), 0.0, 2.0 ** -8)
                else:
                    err = rel_err(got, hid_ref)
                    out[('hid', k)], fig[('hid', k)] = err / EXACT, (err, 0.0, EXACT)
            if 'h' in links:
                err = rel_err(after['h'][rows], h_ref)
                out[('h', k)], fig[('h', k)] = err / EXACT, (err, 0.0, EXACT)
    # what the launch must leave alone
    mine = np.zeros(c.N, bool)
    mine[cell_rows[keep[cell_rows]]] = True
    others = torch.from_numpy(np.nonzero(~mine)[0])
    for name in ('A', 'LSE', 'hid'):
        out[('kept', name)] = 0.0 if same_bits(after[name][others], before[name][others]) else float('inf')
    mine[nrows] = True
    others = torch.from_numpy(np.nonzero(~mine)[0])
    out[('kept', 'h')] = 0.0 if same_bits(after['h'][others], before['h'][others]) else float('inf')
    out[('kept', 'PRE')] = 0.0 if same_bits(after['PRE'], before['PRE']) else float('inf')
    if nrows.size:
        out[('kept', 'net rows all written')] = float('inf') if bool(torch.isnan(after['h'][nrows]).any()) else 0.0
    if tag:
        for k, (err, e32, bound) in fig.items():
            print(f'MEAS {tag} {k[0]} {k[1]}: e_hip {err:.1e} e_32 {e32:.1e} bound {bound:.1e}')
    return out


def failures(ratios):
    return {k: v for k, v in ratios.items() if not v <= 1.0}


def formula(c, relu=True, active=None, defect=None, hid16=False, cell_rows=None):
    """The closed form of one launch over the whole net level and `cell_rows` (default: all of L4), in fp64 from fp32 inputs;
    returns (before, after) as `inputs` gives them.  `defect` switches one mistake on."""
    assert defect is None or defect in DEFECTS
    L3, L4 = c.L[3], c.L[4]
    t = inputs(c, hid16)
    before = {k: v.clone() for k, v in t.items()}
    keep = np.ones(c.N, bool) if active is None or defect == 'inactive_written' else active.numpy().astype(bool)
    cell_rows = L4 if cell_rows is None else np.asarray(cell_rows, dtype=np.int64)
    act = _act(relu)
    z = c.PRE[L3] + c.h[c.drv3]                                                 # fp32, as the kernels: one add ...
    net = z if defect == 'net_relu_dropped' else act(z)                          # ... and a select
    val = c.h.double().clone()
    val[L3] = net.double()
    if defect == 'pre_on_older':
        L1 = c.L[1]
        val[L1] = act(c.PRE[L1] + c.h[L1]).double()
    t['h'][L3[keep[L3]]] = net[keep[L3]]
    ip, ix = c.graph.csr_host('in', 'cell')
    rows = cell_rows[keep[cell_rows]]
    A = torch.zeros((rows.size, D), dtype=torch.float64)
    LSE = torch.zeros((rows.size, D), dtype=torch.float64)
    for i, v in enumerate(rows):
        src = ix[ip[v]:ip[v + 1]]
        if defect == 'drop_tail':
            src = src[:SLOT_W]
        if defect == 'multi_edge_once':
            src = src[np.sort(np.unique(src, return_index=True)[1])]
        if src.size == 0:
            if defect == 'fanin0_nan':
                A[i] = LSE[i] = NAN                                              # 0 / 0 and log 0 + (-inf)
            continue
        x = val[torch.from_numpy(src)]
        if defect == 'no_max':                                                   # in fp32, as a kernel would: exp overflows
            x32 = x.float()
            w = torch.exp(x32)
            A[i], LSE[i] = ((w * x32).sum(0) / w.sum(0)).double(), torch.log(w.sum(0)).double()
            continue
        m = x.max(0).values
        w = torch.exp(x - m)
        s = w.sum(0)
        A[i] = x.mean(0) if defect == 'mean' else (w * x).sum(0) / s
        LSE[i] = torch.log(s) if defect == 'lse_no_max' else m + torch.log(s)
    A32 = A.float()
    hid = torch.relu((A32 if defect == 'A_unrounded' else B.r(A32)).double() @ c.W1.double().T + c.b1.double())
    hid_in = hid if defect == 'hid_unrounded' else B.r(hid)
    o = hid_in @ c.W2.double().T + c.b2.double()
    if defect != 'no_residual':
        o = o + c.h[rows].double()
    rows_t = torch.from_numpy(rows)
    t['A'][rows_t], t['LSE'][rows_t] = A32, LSE.float()
    t['hid'][rows_t] = hid.to(t['hid'].dtype)
    t['h'][rows_t] = (o if defect == 'no_final_act' else act(o)).float()
    return before, t


# --------------------------------------------------------------------------------------------------------------- edge presence
def edge_report(c, graph=None):
    """{edge case: present?} read from the tables the kernels get (CSRs, slot table, driver tables, fold schedule), the level
    lists, the row ranges handed to the wrappers and the value tensors.  graph: c.graph or a copy of it on a device."""
    g = c.graph if graph is None else graph
    H = ops.PAIR_HEAVY_IN
    rep = {'schedule_complete': g.level_set_is_complete(c.levels), 'fold_schedule': g.fold_schedule(c.levels) is not None}
    if not rep['fold_schedule']:
        return rep
    tb = tables(c, g)
    fold, slots, net_drv = tb['fold'], tb['slots'].cpu().numpy(), tb['net_drv'].cpu().numpy()
    ip, ix = g.csr_host('in', 'cell')
    deg = np.diff(ip)
    L1, L2, L3, L4 = (np.asarray(c.levels[i]) for i in (1, 2, 3, 4))
    s0, ns = c.slot_range
    srows = np.arange(s0, s0 + ns)
    wrows = np.arange(s0 + ns, c.cell_range[0] + c.cell_range[1])
    rep['levels_are_the_ranges'] = fold[3]['range'] == c.net_range and fold[4]['range'] == c.cell_range and s0 == c.cell_range[0]
    rep['every_folded_net_has_one_driver_in_L2'] = bool(np.isin(net_drv[L3], L2).all()) and \
        bool((np.diff(g.csr_host('in', 'net')[0])[L3] == 1).all())
    rep['driver_table_matches'] = bool((tb['drv'].cpu().numpy() == net_drv[ix]).all())
    # the slot rows and the wider ones
    rep['slot_rows_fan_in_at_most_4'] = bool((deg[srows] <= SLOT_W).all()) and bool((slots[srows, 0] != -2).all())
    rep['wider_rows_marked'] = bool((slots[wrows, 0] == -2).all()) and bool((deg[wrows] > SLOT_W).all())
    hrow, prow = slots[srows, :4], slots[srows, 4:]
    sdeg = deg[srows]
    rep['slots_count_edges'] = bool(((hrow >= 0).sum(1) == sdeg).all())
    for f in range(SLOT_W + 1):
        rep[f'fan_in_{f}'] = bool((sdeg == f).any())
    older = (hrow >= 0) & (prow < 0)
    rep['older_edges_come_from_L1'] = bool(np.isin(hrow[older], L1).all()) and older.any()
    rep['folded_slots_read_driver_and_PRE'] = bool((hrow[prow >= 0] == net_drv[prow[prow >= 0]]).all()) and \
        bool(np.isin(prow[prow >= 0], L3).all())
    k = np.arange(SLOT_W)[None, :]
    rep['older_edge_in_slot_0'] = bool((older[:, 0] & (sdeg >= 2) & ~older[:, 1:].any(1)).any())
    rep['older_edge_in_the_middle'] = bool((older & (k > 0) & (k < sdeg[:, None] - 1)).any())
    rep['older_edge_last'] = bool((older & (k == sdeg[:, None] - 1) & (sdeg[:, None] >= 3) & ~older[:, :1]).any())
    rep['row_with_every_edge_older'] = bool(((older.sum(1) == sdeg) & (sdeg >= 2)).any())
    two = srows[sdeg == 2]
    pair = np.stack([ix[ip[two]], ix[ip[two] + 1]], 1)
    rep['fan_in_2_multi_edge'] = bool((pair[:, 0] == pair[:, 1]).any())
    rep['multi_edge_in_a_full_row'] = any(len(set(ix[ip[v]:ip[v + 1]])) < SLOT_W for v in srows[sdeg == SLOT_W])
    # net values (fp32, both activations) and what reads them
    z = c.PRE[L3] + c.h[net_drv[L3]]
    both = np.isin(pair, L3).all(1) & (pair[:, 0] != pair[:, 1])
    rep['fan_in_2_equal_values'] = any(bool(torch.equal(z[a - L3[0]], z[b - L3[0]])) for a, b in pair[both])
    negs = L3[(z < 0).all(1).numpy()]
    rep['net_negative_everywhere_and_read'] = negs.size > 0 and bool(np.isin(negs, ix[ip[L4[0]]:]).any())
    rep['a_third_of_net_values_non_positive'] = 0.2 < float((z <= 0).float().mean()) < 0.5
    rep['a_few_exact_zero_net_values'] = 0 < int((z == 0).sum()) < L3.size
    rep['a_few_exact_zeros_in_older_rows'] = 0 < int((c.h[L1] == 0).sum()) < L1.size
    rep['driver_shared_by_many_nets'] = int(np.bincount(net_drv[L3]).max()) > max(SLOT_W, L3.size // 8)
    unread = np.setdiff1d(L3, ix[ip[L4[0]]:])
    rep['nets_nobody_reads'] = unread.size > 0
    rep['net_rows_NaN_before_the_launch'] = bool(torch.isnan(c.h[L3]).all()) and not bool(torch.isnan(c.h[:L3[0]]).any()) \
        and not bool(torch.isnan(c.h[L4]).any())
    rep['PRE_is_a_sentinel_outside_L3'] = bool((c.PRE[:L3[0]] == SENT).all()) and bool((c.PRE[L4] == SENT).all())
    rep['weights_are_bf16_representable'] = bool(torch.equal(B.r(c.W1), c.W1) and torch.equal(B.r(c.W2), c.W2))
    # the cone mask
    a = c.active.numpy().astype(bool)
    rep['active_is_a_cone'] = all(a[ix[ip[v]:ip[v + 1]]].all() for v in L4 if a[v]) and bool(a[net_drv[L3[a[L3]]]].all())
    tiles16 = [b for b in range(ns // TILE) if not a[s0 + TILE * b:s0 + TILE * (b + 1)].any()]
    rep['inactive_16_row_tile_with_active_net_rows'] = any(a[L3[TILE * b:TILE * (b + 1)]].any() for b in tiles16)
    rep['inactive_32_row_tile_with_active_net_rows'] = any(
        not a[s0 + 2 * TILE * b:s0 + 2 * TILE * (b + 1)].any() and a[L3[2 * TILE * b:2 * TILE * (b + 1)]].any() for b in range(ns // (2 * TILE)))
    rep['tile_partly_inactive'] = any(0 < a[s0 + TILE * b:s0 + TILE * (b + 1)].sum() < TILE for b in range(ns // TILE))
    rep['inactive_nets_nobody_reads'] = bool((~a[unread]).any()) and bool(a[unread].any())
    # values per regime: the in-neighbours of the rows of fan-in 2, per channel, with and without the ReLU
    val = {relu: c.h.double().clone() for relu in (True, False)}
    val[True][L3], val[False][L3] = torch.relu(z).double(), z.double()
    distinct = two[pair[:, 0] != pair[:, 1]]
    x = {relu: torch.stack([val[relu][ix[ip[distinct]]], val[relu][ix[ip[distinct] + 1]]]) for relu in (True, False)}
    spread = {relu: (x[relu][0] - x[relu][1]).abs().min(1).values.numpy() for relu in (True, False)}      # the row's smallest gap
    all_old = np.isin(ix[ip[distinct]], L1) & np.isin(ix[ip[distinct] + 1], L1)
    all_fold = np.isin(ix[ip[distinct]], L3) & np.isin(ix[ip[distinct] + 1], L3)
    if c.regime == 'wide':
        rep['wide_older_pair_+40_-40'] = bool(((spread[True] > 70) & all_old).any())
        rep['wide_folded_pair_+40_-40_without_relu'] = bool(((spread[False] > 70) & all_fold).any())
        lo = torch.minimum(x[True][0], x[True][1]).min(1).values.numpy()
        gap = (x[True][0] - x[True][1]).abs().max(1).values.numpy()
        rep['wide_folded_pair_+40_+38'] = bool(((lo > 30) & (gap < 8) & all_fold).any())
        rep['wide_pair_above_104_underflows_fp32'] = bool((spread[True] > 104).any()) and \
            float(torch.exp(torch.tensor(-float(spread[True].max()), dtype=torch.float32))) == 0.0
    else:
        rep['unit_h_in_-1_2'] = float(c.h[~torch.isnan(c.h)].min()) >= -1 and float(c.h[~torch.isnan(c.h)].max()) <= 2
        rep['unit_net_values_within_5'] = float(z.abs().max()) <= 5
    # sizes
    cdiv = lambda n, m: -(-n // m)
    if c.size == 'small':
        rep['one_row_block_per_workgroup'] = max(L3.size, L4.size) < RB2_ROWS
        wdeg = deg[wrows].tolist()
        for f in (SLOT_W + 1, 2 * BATCH, 2 * BATCH + 1, H, H + 1, H + HEAVY_GROUPS, H + HEAVY_GROUPS + 1):
            rep[f'fan_in_{f}'] = f in wdeg
        rep['fan_in_far_above_the_heavy_groups'] = max(wdeg) >= 25 * HEAVY_GROUPS
        rep['last_batch_with_a_missing_edge'] = any(f % BATCH for f in wdeg if f <= H)
        heavy = tb['heavy'].cpu().numpy() if tb['heavy'] is not None else np.zeros(0)
        rep['heavy_list_is_the_rows_above_HEAVY_IN'] = heavy.tolist() == L4[deg[L4] > H].tolist() and heavy.size >= 4
        rep['older_edges_in_the_wider_rows'] = all(np.isin(ix[ip[v]:ip[v + 1]], L1).any() for v in wrows)
        rep['inactive_light_and_heavy_wide_rows'] = bool((~a[wrows[deg[wrows] <= H]]).any() and (~a[wrows[deg[wrows] > H]]).any()
                                                         and a[wrows[deg[wrows] <= H]].any() and a[wrows[deg[wrows] > H]].any())
        rep['slot_rows_longer_than_the_net_level'] = cdiv(ns, TILE) > cdiv(L3.size, TILE)
        rep['net_level_longer_than_the_sub_ranges'] = all(n <= ns and cdiv(n, TILE) < cdiv(L3.size, TILE) for n in SUB_COUNTS)
        rep['partial_last_tile'] = ns % TILE != 0 and L3.size % TILE != 0
    elif c.size == 'rb2_nets':
        rep['two_row_blocks_by_the_net_level'] = L3.size >= RB2_ROWS > L4.size
        rep['partial_first_block_dead_second_block'] = 0 < ns % (2 * TILE) < TILE
        rep['partial_last_net_tile'] = L3.size % (2 * TILE) != 0
        rep['190_workgroups_without_a_cell_tile'] = cdiv(L3.size, 2 * TILE) - cdiv(ns, 2 * TILE) == 190
        rep['no_wider_rows'] = wrows.size == 0
    else:
        rep['two_row_blocks_by_the_cell_level'] = L4.size >= RB2_ROWS > L3.size
        rep['cells_6144_+_33'] = ns == RB2_ROWS + 33 and L3.size == 40
        rep['no_wider_rows'] = wrows.size == 0
    return rep
