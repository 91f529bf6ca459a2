"""Kernel-level parity of the second half of csrc/graph.hip (segment sums, row flags, fan-in cone, attention branch): every
entry point called by name through the C ABI, against fp64 references on the same inputs, at the widths and segment lengths
where the kernels change code path."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from mmft import lib, ops
from mmft.detrand import det_uniform, det_ints
from oracle import restatement as R

pytestmark = pytest.mark.gpu
TOL = 2e-5          # as tests/test_kernels_gpu.py
BAD_ARG = -1        # MMFT_ERR_BAD_ARG
SENT = 777.0


def T_(shape, seed, dev, lo=-1.0, hi=1.0):
    return torch.from_numpy(det_uniform(shape, seed, lo, hi)).to(dev)


def I32(a, dev):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev)


# --------------------------------------------------------------------------------------------- segment sums
# empty, 1, the thread-group counts 32 and 64 crossed from both sides, one long segment, empty segments in the middle and last
SEG_LENS = [0, 1, 31, 32, 33, 65, 0, 3000, 2, 0]
NSRC = 3300


def _segments():
    ip = np.concatenate([[0], np.cumsum(SEG_LENS)]).astype(np.int64)
    ix = det_ints((int(ip[-1]),), 3, 0, NSRC)
    return ip, ix


def _seg_ref(src64, ip, ix, rows):
    out = torch.zeros((len(rows), src64.shape[1]), dtype=torch.float64)
    for i, v in enumerate(rows):
        out[i] = src64[ix[ip[v]:ip[v + 1]]].sum(0)
    return out


@pytest.mark.parametrize('permuted', [False, True])
@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('D', [4, 16, 20, 128, 256])
def test_seg_sum_fwd_and_rows_wg(dev, D, accumulate, permuted):
    """mmft_seg_sum_fwd (one thread group per row) and mmft_seg_sum_rows_wg (one workgroup per row) against fp64 sums.
    D = 16 / 20 straddle the narrow and wide LDS layouts of the workgroup kernel; D = 20 (5 channel groups, no divisor of 256)
    is computed by seg_sum_fwd but is unreachable in the workgroup form through the ABI: the entry point rejects it, which is
    asserted instead.  The workgroup form promises a fixed order: two calls agree bitwise."""
    ip, ix = _segments()
    n = len(SEG_LENS)
    assert {0, 1, 31, 32, 33, 65, 3000} <= set(SEG_LENS)
    rows_h = np.array([7, 0, 3, 9, 5, 2, 4, 1]) if permuted else np.arange(n)
    rows = I32(rows_h, dev) if permuted else None
    nr = len(rows_h)
    src_w = T_((NSRC, D + 4), 1, dev)
    src = src_w[:, :D]                                           # row stride larger than the width
    ref = _seg_ref(src.double().cpu(), ip, ix, rows_h)
    old = T_((n, D + 4), 2, dev)
    ipd, ixd = I32(ip, dev), I32(ix, dev)
    d, st = lib.stream_args(src)
    # seg_sum_fwd: accumulate = 0 writes out[i], accumulate = 1 adds into out[rows[i]]
    out = old.clone()
    lib.call('mmft_seg_sum_fwd', src, src.stride(0), ipd, ixd, rows, nr, D, out, out.stride(0), accumulate, d, st)
    exp = old.double().cpu().clone()
    if accumulate:
        exp[rows_h, :D] += ref
    else:
        exp[:nr, :D] = ref
    assert rel_err(out, exp) < TOL and torch.equal(out[:, D:], old[:, D:])
    # seg_sum_rows_wg: out[rows[i]] (+)=
    out = old.clone()
    args = (src, src.stride(0), ipd, ixd, rows, nr, D, out, out.stride(0), accumulate, d, st)
    if D == 20:
        assert lib.query('mmft_seg_sum_rows_wg', *args) == BAD_ARG and b'seg_sum_rows_wg' in lib.load().mmft_last_error()
        torch.cuda.synchronize()
        assert torch.equal(out, old)
        return
    lib.call('mmft_seg_sum_rows_wg', *args)
    exp = old.double().cpu().clone()
    exp[rows_h, :D] = ref + (exp[rows_h, :D] if accumulate else 0.0)
    assert rel_err(out, exp) < TOL and torch.equal(out[:, D:], old[:, D:])
    out2 = old.clone()
    lib.call('mmft_seg_sum_rows_wg', src, src.stride(0), ipd, ixd, rows, nr, D, out2, out2.stride(0), accumulate, d, st)
    assert torch.equal(out, out2)


@pytest.mark.parametrize('keys', ['skipping', 'all_equal'])
@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('D', [4, 16, 20, 128, 256])
def test_seg_sum_sorted(dev, D, accumulate, keys):
    """mmft_seg_sum_sorted against fp64 index_add: keys that skip values (empty segments in the middle), all keys equal, R
    larger than the largest key; two calls agree bitwise.  D = 20 is rejected by the entry point (as in the workgroup form)."""
    R_ = 12
    if keys == 'skipping':
        k = np.repeat([0, 1, 4, 5, 9], [1, 33, 3000, 64, 31])    # keys 2, 3, 6, 7, 8, 10, 11 never occur
    else:
        k = np.full(700, 5)
    assert k.max() < R_ - 1 and (np.diff(k) >= 0).all()
    nsrc = len(k)
    src = T_((nsrc, D + 4), 1, dev)[:, :D]
    old = T_((R_, D + 4), 2, dev)
    out = old.clone()
    d, st = lib.stream_args(src)
    args = lambda o: (src, src.stride(0), I32(k, dev), nsrc, R_, D, o, o.stride(0), accumulate, d, st)
    if D == 20:
        assert lib.query('mmft_seg_sum_sorted', *args(out)) == BAD_ARG
        torch.cuda.synchronize()
        assert torch.equal(out, old)
        return
    lib.call('mmft_seg_sum_sorted', *args(out))
    exp = old.double().cpu().clone()
    if not accumulate:
        exp[:, :D] = 0
    exp[:, :D].index_add_(0, torch.from_numpy(k).long(), src.double().cpu())
    assert rel_err(out, exp) < TOL and torch.equal(out[:, D:], old[:, D:])
    out2 = old.clone()
    lib.call('mmft_seg_sum_sorted', *args(out2))
    assert torch.equal(out, out2)


@pytest.mark.parametrize('scatter', [0, 1])
@pytest.mark.parametrize('permuted', [False, True])
@pytest.mark.parametrize('D', [1, 2, 3, 4, 16, 20, 128, 256])
def test_seg_mean_rows_any(dev, D, permuted, scatter):
    """mmft_seg_mean_rows_any ("any D"; the model uses 2) against fp64 means; zero for an empty segment; scatter by row id on
    and off; rows = NULL and a permuted row list."""
    ip, ix = _segments()
    n = len(SEG_LENS)
    rows_h = np.array([7, 0, 3, 9, 5, 2, 4, 1]) if permuted else np.arange(n)
    rows = I32(rows_h, dev) if permuted else None
    nr = len(rows_h)
    src = T_((NSRC, D + 3), 1, dev)[:, :D]
    lens = np.maximum(np.diff(ip)[rows_h], 1)
    ref = _seg_ref(src.double().cpu(), ip, ix, rows_h) / torch.from_numpy(lens).double()[:, None]
    out = torch.full((n, D + 5), SENT, device=dev)
    d, st = lib.stream_args(src)
    lib.call('mmft_seg_mean_rows_any', src, src.stride(0), I32(ip, dev), I32(ix, dev), rows, nr, D, out, out.stride(0), scatter, d, st)
    exp = torch.full((n, D + 5), SENT, dtype=torch.float64)
    exp[rows_h if scatter else np.arange(nr), :D] = ref
    got = out.double().cpu()
    assert float((got[:, :D] - exp[:, :D]).abs().max()) <= TOL * float(ref.abs().max())
    assert torch.equal(got[:, D:], exp[:, D:]) and torch.equal(got[:, :D] == SENT, exp[:, :D] == SENT)


@pytest.mark.parametrize('D', [4, 16, 128])
def test_scatter_add_rows_sorted(dev, D):
    """mmft_scatter_add_rows_sorted against fp64 index_add: heavily duplicated destinations (one taken 65 times), rows added in
    batch order without atomics - two calls agree bitwise - and destinations that are not named keep their value."""
    R_, n = 40, 333
    idx_h = det_ints((n,), 1, 0, R_ - 3)                          # rows R_ - 3 .. R_ - 1 are never named
    idx_h[:65] = 7
    order_h = np.argsort(idx_h, kind='stable')
    src = T_((n, D + 4), 2, dev)[:, :D]
    old = T_((R_, D + 4), 3, dev)
    d, st = lib.stream_args(src)
    outs = []
    for _ in range(2):
        dst = old.clone()
        lib.call('mmft_scatter_add_rows_sorted', dst, dst.stride(0), I32(idx_h, dev), I32(order_h, dev), n, D, src, src.stride(0), d, st)
        outs.append(dst)
    exp = old.double().cpu().clone()
    exp[:, :D].index_add_(0, torch.from_numpy(idx_h).long(), src.double().cpu())
    assert rel_err(outs[0], exp) < TOL and torch.equal(outs[0][:, D:], old[:, D:]) and torch.equal(outs[0][R_ - 3:], old[R_ - 3:])
    assert torch.equal(outs[0], outs[1])


# --------------------------------------------------------------------------------------------- row flags
@pytest.mark.parametrize('D', [16, 128])
def test_target_rows_and_mark_rows(dev, D):
    """mmft_target_rows_begin / _end and mmft_mark_rows: duplicate indices, n = 0; only the named rows of G are zeroed, the
    flags are set and cleared for exactly those rows."""
    N = 200
    idx_h = np.array([5, 199, 0, 5, 77, 5, 199, 42])              # duplicates
    idx = I32(idx_h, dev)
    G0 = T_((N, D + 4), 1, dev)
    G = G0.clone()
    flags = torch.zeros(N, dtype=torch.uint8, device=dev)
    flags[3] = 1                                                 # a flag of somebody else's stays
    d, st = lib.stream_args(G)
    lib.call('mmft_target_rows_begin', G, G.stride(0), idx, 0, D, flags, d, st)          # n = 0: nothing happens
    assert torch.equal(G, G0) and int(flags.sum()) == 1
    lib.call('mmft_target_rows_begin', G, G.stride(0), idx, len(idx_h), D, flags, d, st)
    exp = G0.clone()
    exp[np.unique(idx_h), :D] = 0
    ef = np.zeros(N, dtype=np.uint8)
    ef[idx_h] = 1
    ef[3] = 1
    assert torch.equal(G, exp) and np.array_equal(flags.cpu().numpy(), ef)
    lib.call('mmft_target_rows_end', idx, 0, flags, d, st)
    assert np.array_equal(flags.cpu().numpy(), ef)
    lib.call('mmft_target_rows_end', idx, len(idx_h), flags, d, st)
    ef[idx_h] = 0
    assert np.array_equal(flags.cpu().numpy(), ef) and torch.equal(G, exp)
    lib.call('mmft_mark_rows', idx, len(idx_h), flags, 1, d, st)
    ef[idx_h] = 1
    assert np.array_equal(flags.cpu().numpy(), ef)
    lib.call('mmft_mark_rows', idx, 0, flags, 0, d, st)
    assert np.array_equal(flags.cpu().numpy(), ef)
    lib.call('mmft_mark_rows', idx[:3], 3, flags, 0, d, st)
    ef[idx_h[:3]] = 0
    assert np.array_equal(flags.cpu().numpy(), ef)


def _csr_in(N, src, dst):
    order = np.argsort(dst, kind='stable')
    ip = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=N), out=ip[1:])
    return ip, src[order]


@pytest.mark.parametrize('form', ['two_csr_rows', 'one_csr_row0'])
def test_fanin_cone_step_matches_bfs(dev, form):
    """mmft_fanin_cone_step called level by level (L - 1 .. 1) on a 5-level DAG of 300 nodes against a host BFS over the
    in-edges: two CSRs with a row list, and one CSR (the second NULL) with the row0 form.  A node whose mark is clear must not
    mark its in-neighbours - the DAG holds such a node with an in-neighbour that nothing else reaches."""
    N, L, per = 300, 5, 60
    level = np.arange(N) // per

    def edges(m, seed):
        d_ = det_ints((m,), seed, per, N)
        s_ = det_ints((m,), seed + 1, 0, 1 << 30) % ((d_ // per) * per)          # any node of a lower level
        return s_, d_
    s0, d0 = edges(260, 71)
    s1, d1 = edges(200, 73)
    two = form == 'two_csr_rows'
    ip0, ix0 = _csr_in(N, s0, d0)
    ip1, ix1 = _csr_in(N, s1, d1)
    seeds = np.array([299, 250, 250, 181, 130, 61])              # endpoints on several levels, one duplicate
    mark = np.zeros(N, dtype=np.uint8)
    mark[seeds] = 1
    stack = list(seeds)
    while stack:
        v = stack.pop()
        nb = list(ix0[ip0[v]:ip0[v + 1]]) + (list(ix1[ip1[v]:ip1[v + 1]]) if two else [])
        for u in nb:
            if not mark[u]:
                mark[u] = 1
                stack.append(u)
    assert 0 < mark.sum() < N
    clear = [v for v in range(per, N) if not mark[v] and any(not mark[u] for u in ix0[ip0[v]:ip0[v + 1]])]
    assert clear                                                  # a clear node whose in-neighbour stays clear
    flags = torch.zeros(N, dtype=torch.uint8, device=dev)
    d, st = lib.stream_args(flags)
    lib.call('mmft_mark_rows', I32(seeds, dev), len(seeds), flags, 1, d, st)
    t0, t1 = (I32(ip0, dev), I32(ix0, dev)), (I32(ip1, dev), I32(ix1, dev))
    for l in range(L - 1, 0, -1):
        if two:
            rows = I32(l * per + np.argsort(det_ints((per,), 80 + l, 0, 1 << 30), kind='stable'), dev)
            lib.call('mmft_fanin_cone_step', rows, 0, per, t0[0], t0[1], t1[0], t1[1], flags, d, st)
        else:
            lib.call('mmft_fanin_cone_step', None, l * per, per, t0[0], t0[1], None, None, flags, d, st)
    lib.call('mmft_fanin_cone_step', None, 0, 0, t0[0], t0[1], None, None, flags, d, st)          # n = 0
    assert np.array_equal(flags.cpu().numpy(), mark)


# --------------------------------------------------------------------------------------------- attention branch
NSRC_A, NA = 150, 300           # sources 0..149, net sinks 150..224, cell sinks 225..299
W_KEY = [[1.0], [0.5]]          # fc_key.weight (dk = 2, 1)
W_ATTN = [[0.75, 0.5, -0.5, 0.25]]     # fc_attn.weight (1, 2 dk): c1 = 0.75 + 0.25 = 1, c2 = -0.5 + 0.125 = -0.375, exact in fp32


def _attn_graph():
    from mmft.pingraph import PinGraph
    ns, nd = det_ints((400,), 31, 0, NSRC_A), det_ints((400,), 32, 150, 225)
    degs = det_ints((NA,), 33, 1, 9)
    cs, cd = [], []
    for v in range(225, NA):
        deg = {225: 0, 226: 1, 227: 200}.get(v, int(degs[v]))
        cs += list(det_ints((deg,), 40 + v, 0, NSRC_A))
        cd += [v] * deg
    cs += [17, 17]                                               # two parallel edges from the same source
    cd += [228, 228]
    g = PinGraph(NA, {'net': (ns, nd), 'cell': (np.array(cs), np.array(cd))})
    ip, ix = g.csr_host('in', 'cell')
    deg = np.diff(ip)
    assert deg[225] == 0 and deg[226] == 1 and deg[227] == 200
    seg = ix[ip[228]:ip[229]]
    assert (seg == 17).sum() >= 2
    return g


@pytest.mark.parametrize('scale', [1.0, 25.0])
@pytest.mark.parametrize('D', [4, 16, 128])
def test_attention_branch_matches_autograd(dev, D, scale):
    """mmft_seg_attn_fwd, mmft_level_bwd_pull_attn and mmft_seg_attn_bwd_scores against fp64 autograd of
    oracle.restatement.seg_attn_sum (c1, c2 formed from w_key / w_attn in fp64; the weights are dyadic so that the fp32 pair
    handed to the kernels is the same number).  Cell rows of degree 0, 1 and 200, two parallel edges; keys in [-2, 2] (both
    signs of the leaky-ReLU argument); scale = 25 puts the scores around +-60 (the max subtraction).  D = 4, 16, 128 are 1, 4
    and 32 lanes per node in the shuffle reduction of the score gradient.  5e-5 relative, as the existing reverse-pull test."""
    g = _attn_graph().to(dev)
    ip, ix = g.csr_host('in', 'cell')
    cell_rows, net_rows = np.arange(225, NA), np.arange(150, 225)
    key_h = det_uniform((NA,), 9, -2, 2)
    w_key = torch.tensor(W_KEY, dtype=torch.float64)
    w_attn = (torch.tensor(W_ATTN, dtype=torch.float64) * scale).requires_grad_(True)
    c1 = float((w_attn[0, :2] * w_key[:, 0]).sum())
    c2 = float((w_attn[0, 2:] * w_key[:, 0]).sum())
    assert (c1, c2) == (scale, -0.375 * scale) and np.float32(c1) == c1 and np.float32(c2) == c2
    dst = np.repeat(np.arange(NA), np.diff(ip))
    pre = c1 * key_h[ix].astype(np.float64) + c2 * key_h[dst].astype(np.float64)
    assert (pre > 0).any() and (pre < 0).any()
    if scale > 1:
        assert pre.max() > 55 and pre.min() < -55
    h64 = torch.from_numpy(det_uniform((NA, D), 1, -2, 2)).double().requires_grad_(True)
    key64 = torch.from_numpy(key_h).double()[:, None]
    a_cell = R.seg_attn_sum(h64, key64, ip, ix, cell_rows, w_key, w_attn)
    a_net = R.seg_mean(h64, *g.csr_host('in', 'net'), net_rows)
    gn = torch.from_numpy(det_uniform((75, D), 2)).double()
    gc = torch.from_numpy(det_uniform((75, D), 3)).double()
    gt = torch.from_numpy(det_uniform((NA, D), 4)).double()
    own_h = (np.arange(NA) % 2 == 0).astype(np.uint8)
    ((a_net * gn).sum() + (a_cell * gc).sum()).backward()
    pulled = h64.grad[:NSRC_A].clone()                            # what the sinks send back, without the rows' own gradient
    dc = torch.stack([w_attn.grad[0, 0], w_attn.grad[0, 2]])       # w_key[0] = 1: d loss / d c1 = d loss / d w_attn[0, 0], c2 alike
    assert torch.allclose(w_attn.grad[0, 1], 0.5 * w_attn.grad[0, 0]) and torch.allclose(w_attn.grad[0, 3], 0.5 * w_attn.grad[0, 2])

    h = h64.detach().float().to(dev)
    key = torch.from_numpy(key_h).to(dev)
    c12 = torch.tensor([c1, c2], dtype=torch.float32, device=dev)
    csr_in = g.csr('in', 'cell')
    E = int(ip[-1])
    # forward on the odd rows first, the rest after: alpha slots of rows that are not named stay untouched
    A = torch.full((NA, D), SENT, device=dev)
    alpha = torch.full((E,), SENT, device=dev)
    part = cell_rows[1::2]
    ops.seg_attn_fwd(h, key, c12, csr_in, I32(part, dev), A, alpha)
    ah = alpha.cpu().numpy()
    named = np.zeros(E, dtype=bool)
    for v in part:
        named[ip[v]:ip[v + 1]] = True
    assert (ah[~named] == SENT).all() and (ah[named] != SENT).all()
    assert bool((A[:225] == SENT).all()) and bool((A[torch.from_numpy(cell_rows[0::2]).to(dev)] == SENT).all())
    ops.seg_attn_fwd(h, key, c12, csr_in, (225, 75), A, alpha)                    # row0 form, all cell rows
    assert bool((A[:225] == SENT).all())
    assert rel_err(A[225:], a_cell) < 5e-5
    assert bool((A[225] == 0).all())                                              # degree 0: A = 0
    ah = alpha.cpu().numpy()
    assert ah[ip[226]] == 1.0                                                     # degree 1: alpha = 1
    sums = np.array([ah[ip[v]:ip[v + 1]].astype(np.float64).sum() for v in cell_rows if ip[v + 1] > ip[v]])
    assert np.abs(sums - 1.0).max() < 1e-6
    # score gradient
    DA = torch.zeros((NA, D), device=dev)
    DA[225:] = gc.float().to(dev)
    dcp = torch.zeros((NA, 2), device=dev)
    ops.seg_attn_bwd_scores(DA, h, A, alpha, key, c12, csr_in, (225, 75), dcp)
    dcp_rows = torch.zeros((NA, 2), device=dev)
    ops.seg_attn_bwd_scores(DA, h, A, alpha, key, c12, csr_in, I32(cell_rows[::-1].copy(), dev), dcp_rows)
    assert torch.equal(dcp, dcp_rows)
    assert bool((dcp[225] == 0).all()) and bool((dcp[226] == 0).all())            # degree 0; degree 1: exactly zero
    got = ops.colsum(dcp)
    e_dc = rel_err(got, dc)
    print(f'attention D={D} scale={scale}: A err {rel_err(A[225:], a_cell):.3e}, d(c1, c2) err {e_dc:.3e}, ref {dc.tolist()}')
    assert e_dc < 5e-5
    # reverse pull: own_mask NULL / given, relu 0 / 1, rows / row0 forms, an odd n (the last wave partial at D = 16)
    onw, o2i = g.out_net_weight(), g.out2in('cell')
    for relu in (0, 1):
        for own in (None, torch.from_numpy(own_h).to(dev)):
            for rows, n in ((None, 149), (I32(np.arange(NSRC_A)[::-1].copy(), dev), 150)):
                G = gt.float().to(dev).clone()
                G[150:225] = gn.float().to(dev)
                G0 = G.clone()
                d, st = lib.stream_args(G)
                lib.call('mmft_level_bwd_pull_attn', G, h, h.stride(0), rows, 0, n, D, *g.csr('out', 'net'), onw, *g.csr('out', 'cell'),
                         o2i, alpha, DA, relu, own, d, st)
                ref = pulled + (gt[:NSRC_A] if own is None else gt[:NSRC_A] * torch.from_numpy(own_h[:NSRC_A]).double()[:, None])
                if relu:
                    ref = torch.where(h64.detach()[:NSRC_A] > 0, ref, torch.zeros_like(ref))
                assert rel_err(G[:n], ref[:n]) < 5e-5
                assert torch.equal(G[n:], G0[n:])                                 # rows past n and the sinks are left alone
