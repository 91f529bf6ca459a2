"""The run-form backward of the masked projection resolves a block's boundary list once per workgroup (csrc/fusion.hip,
masked_fc_bwd_runs_kernel); the MSE kernel's summation order is pinned bit for bit.  Both through the C ABI by name.

1. the backward's two paths (list resolved in LDS / list too long: direct walk) give the same bits: one live case, with 0 to
   64 000 entries of never-sampled paths appended per block - the LDS capacity is crossed from both sides;
2. the resolved path at its edges (round remainders, `next` chains, an unsampled entry between sampled ones, empty cells and an
   empty block) against the fp64 dense reference, within the run-form bound of tests/test_head_kernels_gpu.py;
3. the MSE kernel's loss and gradient, bit for bit a serial fp64 loop in the kernel's element order."""
import numpy as np
import pytest
import torch

from mmft import lib
from mmft.detrand import det_uniform, det_ints
from mmft.fusion import PathMasks, batch_links
from test_head_kernels_gpu import S, TOL, EPS24, T_, I32, close, dense_reference

pytestmark = pytest.mark.gpu


def csr(per):
    ip, cols = [0], []
    for q in per:
        assert list(q) == sorted(set(q))
        cols += list(q)
        ip.append(len(cols))
    return np.array(ip, dtype=np.int64), np.array(cols, dtype=np.int64)


def masks_of(per_design, P, dev):
    ms = [PathMasks(*csr(per), P, dev) for per in per_design]
    return ms[0] if len(ms) == 1 else PathMasks.batch(ms)


def backward(pmk, first, nxt, gout, f, wT, Dout, P, B, dev):
    dwT = torch.full((P, Dout), 7.0, device=dev)
    df = torch.full((B * P,), 7.0, device=dev)
    need = lib.query('mmft_masked_fc_bwd_runs_workspace_bytes', B, P, Dout)
    assert need == (B * P * Dout * 4 if B > 1 else 0)
    ws = torch.empty(max(need // 4, 4), device=dev)
    d, st = lib.stream_args(f)
    lib.call('mmft_masked_fc_bwd_runs', pmk.bnd_ptr, pmk.bnd_code, first, nxt, gout, gout.stride(0), f, wT, dwT, df, B, P, Dout, S,
             ws, ws.numel() * 4, d, st)
    return dwT, df.reshape(B, P)


def cell_lists(pmk):
    """Per cell (design-major) the boundary entries in list order as (path id, sign)."""
    bp, bc = pmk.bnd_ptr.cpu().numpy(), pmk.bnd_code.cpu().numpy()
    path = np.where(bc >= 0, bc, -bc - 1)
    return bp, path, np.where(bc >= 0, 1, -1)


# ------------------------------------------------------------------------------ 1. both paths of the kernel, the same bits
P1, B1, NLIVE = 128, 2, 24
DEAD = (0, 1000, 4000, 16000, 64000)           # entries of never-sampled paths appended per block; 64 000 > any LDS list


def live_paths(b):
    """NLIVE masks of design b: one to three runs each, some starting at a block's first cell, some ending at its last."""
    per = []
    for q in range(NLIVE):
        r = det_ints((6,), 100 * b + q, 0, P1)
        cells = set()
        for k in range(1 + q % 3):
            a, n = int(r[2 * k]), 1 + int(r[2 * k + 1]) % 23
            cells |= set(range(a, min(a + n, P1)))
        if q % 5 == 0:
            cells |= set(range(S * (q % 2), S * (q % 2) + 9))          # a run from a block's first cell
        if q % 7 == 0:
            cells |= set(range(S * (1 + q % 2) - 6, S * (1 + q % 2)))  # a run to a block's last cell
        per.append(sorted(cells))
    return per


def dead_paths(n_per_block):
    """Single-cell masks off the block starts: each adds a plus entry at its cell and a minus entry at the cell before."""
    per = []
    for blk in range(P1 // S):
        per += [[blk * S + 1 + k % (S - 1)] for k in range(n_per_block // 2)]
    return per


@pytest.fixture(scope='module')
def variants(dev):
    """The live case with each amount of dead entries: (masks, batch paths, first, next), built once for all widths; the host
    checks that the appended paths are never sampled and leave the order of the live entries in every cell's list alone."""
    per_live = [live_paths(b) for b in range(B1)]
    loc = [q for q in range(NLIVE) if q % 6 != 4]                      # 20 sampled paths per design, rows interleaved
    rows = [(b, loc[q]) for q in range(20) for b in range(B1)] + [(0, loc[3]), (1, loc[5]), (0, loc[3])]   # one path 3x, one 2x
    out, order0 = [], None
    for nd in DEAD:
        dead = dead_paths(nd)
        pmk = masks_of([per_live[b] + dead for b in range(B1)], P1, dev)
        npd = NLIVE + len(dead)                                         # paths per design: the live ones first
        paths = np.array([b * npd + q for b, q in rows], dtype=np.int64)
        first_h, nxt_h = batch_links(paths, pmk.num_paths)
        bp, path, sign = cell_lists(pmk)
        per_block = bp[S::S] - bp[:-1:S]
        print(f'dead={nd}: boundary entries per block {per_block.tolist()}')
        assert (per_block >= nd).all() and (nd > 0 or per_block.max() < 1000)
        live = (path % npd) < NLIVE
        assert (first_h[path[~live]] == -1).all()
        order = [[(int(q) // npd, int(q) % npd, int(sg)) for q, sg, lv in zip(path[bp[c]:bp[c + 1]], sign[bp[c]:bp[c + 1]],
                                                                             live[bp[c]:bp[c + 1]]) if lv]
                 for c in range(B1 * P1)]
        order0 = order0 or order
        assert order == order0
        chains = np.bincount(paths, minlength=pmk.num_paths)
        assert chains.max() == 3 and (chains == 2).any() and (chains > 0).sum() == 40
        out.append((pmk, paths, I32(first_h, dev), I32(nxt_h, dev)))
    return out


@pytest.mark.parametrize('Dout', [128, 256, 32])
def test_resolved_list_and_direct_walk_give_the_same_bits(dev, variants, Dout):
    Tn = len(variants[0][1])
    f = T_((B1, P1), 1, dev).reshape(-1).contiguous()
    wT = T_((P1, Dout), 2, dev, -0.05, 0.05)
    gout = T_((Tn, Dout), 4, dev)
    results = [backward(pmk, first, nxt, gout, f, wT, Dout, P1, B1, dev) for pmk, _, first, nxt in variants]
    pmk, paths = variants[0][:2]
    ref, dwT_ref, df_ref, ncells = dense_reference(pmk, paths, f, wT.t().contiguous(), None, gout, P1, B1)
    m = float(f.abs().max() * wT.abs().max())
    ok1, e1 = close(results[0][0], dwT_ref, TOL * np.abs(dwT_ref).max() + ncells * S * m * EPS24)
    ok2, e2 = close(results[0][1], df_ref, TOL * np.abs(df_ref).max() + ncells * S * m * EPS24)
    print(f'Dout={Dout}: dwT err {e1:.3e}, df err {e2:.3e}')
    assert ok1 and ok2
    for nd, (dwT, df) in zip(DEAD[1:], results[1:]):
        assert torch.equal(dwT, results[0][0]) and torch.equal(df, results[0][1]), f'{nd} dead entries per block'


# ------------------------------------------------------------------------------ 2. round remainders and chains
LIVE_COUNTS = (1, 7, 8, 9, 17, 70)             # live entries of one cell: multiples of the in-flight depth and one either side
COUNT_CELL = (5, 10, 15, 20, 25, 40)           # ... at these cells of a block


def edge_masks(P):
    """One design.  Block 0: for each n of LIVE_COUNTS, n paths whose only run goes from the block's first cell to one cell
    (plus entries only); three paths ending at cell 30, the middle one never sampled; runs that start inside the block (minus
    entries) and one that ends at the block's last cell.  P = 256: block 1 holds inner runs only, block 2 nothing at all,
    block 3 the counted cells again, shifted by three."""
    per, never = [], []
    for blk, shift in ((0, 0), (3, 3)):
        if blk * S >= P:
            continue
        c0 = blk * S
        for n, c in zip(LIVE_COUNTS, COUNT_CELL):
            per += [list(range(c0, c0 + c + shift + 1)) for _ in range(n)]
        never.append(len(per) + 1)
        per += [list(range(c0, c0 + 31 + shift)) for _ in range(3)]
        per.append(list(range(c0 + 33, c0 + 48)))                      # a run inside the block: one plus and one minus entry
        per.append(list(range(c0 + 60, c0 + S)))                       # ... ending at the block's last cell
        per.append(list(range(c0 + 50, c0 + 52)) + list(range(c0 + 54, c0 + 58)))
    if P > S:
        per += [list(range(S + 3 + k, S + 20 + 2 * k)) for k in range(5)]
    return per, never


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('P', [64, 256])
@pytest.mark.parametrize('Dout', [32, 128, 256])
def test_resolved_backward_at_its_edges(dev, Dout, P, B):
    per, never = edge_masks(P)
    npd = len(per)
    pmk = masks_of([per] * B, P, dev)
    designs = [0] if B == 1 else [0, 2]                                # B = 3: design 1 has no sampled path
    sampled = [q for q in range(npd) if q not in never]
    local = sampled + [sampled[2], sampled[-1], sampled[2]]            # one path three times, one twice
    paths = np.array([b * npd + q for q in local for b in designs], dtype=np.int64)
    Tn = len(paths)
    first_h, nxt_h = batch_links(paths, pmk.num_paths)
    # the edges are in the input
    bp, path, sign = cell_lists(pmk)
    livecnt = np.array([(first_h[path[bp[c]:bp[c + 1]]] >= 0).sum() for c in range(B * P)])
    for b in designs:
        for n, c in zip(LIVE_COUNTS, COUNT_CELL):
            assert livecnt[b * P + c] == n
        assert livecnt[b * P + 50] == 0 and bp[b * P + 51] == bp[b * P + 50]          # a cell without an entry
        mid = first_h[path[bp[b * P + 30]:bp[b * P + 31]]]
        assert len(mid) == 3 and mid[0] >= 0 and mid[1] == -1 and mid[2] >= 0        # unsampled between two sampled entries
        assert (sign[bp[b * P + 32]:bp[b * P + 33]] == -1).all() and bp[b * P + 33] > bp[b * P + 32]   # a minus entry
        assert bp[b * P + S] > bp[b * P + S - 1]                                      # a run ending at the block's last cell
        assert sign[bp[b * P]:bp[b * P + S]].sum() > 0                                # runs from the block's first cell: no minus
    chains = np.bincount(paths, minlength=pmk.num_paths)
    assert chains.max() == 3 and (chains == 2).any() and (chains[[b * npd + never[0] for b in range(B)]] == 0).all()
    if P == 256:
        for b in range(B):
            assert bp[b * P + 3 * S] == bp[b * P + 2 * S]                             # a block with no entry at all
    if B == 3:
        assert livecnt[P:2 * P].sum() == 0 and bp[2 * P] > bp[P]                      # a design whose entries are all unsampled
    f = T_((B, P), 1, dev).reshape(-1).contiguous()
    w = T_((Dout, P), 2, dev, -0.05, 0.05)
    wT = w.t().contiguous()
    gwide = T_((Tn, Dout + 8), 4, dev)
    gout = gwide[:, 4:4 + Dout]                                        # a column slice of a wider tensor: ldg > Dout
    assert gout.stride(0) == Dout + 8 and gout.data_ptr() % 16 == 0
    ref, dwT_ref, df_ref, ncells = dense_reference(pmk, paths, f, w, None, gout, P, B)
    m = float(f.abs().max() * w.abs().max())
    first, nxt = I32(first_h, dev), I32(nxt_h, dev)
    dwT, df = backward(pmk, first, nxt, gout, f, wT, Dout, P, B, dev)
    extra = ncells * S * m * EPS24
    ok1, e1 = close(dwT, dwT_ref, TOL * np.abs(dwT_ref).max() + extra)
    ok2, e2 = close(df, df_ref, TOL * np.abs(df_ref).max() + extra)
    print(f'Dout={Dout} P={P} B={B}: dwT err {e1:.3e} (max {np.abs(dwT_ref).max():.3e}), df err {e2:.3e} '
          f'(max {np.abs(df_ref).max():.3e}), bound term {extra:.3e}')
    assert ok1 and ok2
    dwT2, df2 = backward(pmk, first, nxt, gout, f, wT, Dout, P, B, dev)
    assert torch.equal(dwT, dwT2) and torch.equal(df, df2)


# ------------------------------------------------------------------------------ 3. MSE
def mse_serial(p, t, n):
    """The kernel's arithmetic on the host: thread i of 1024 adds fl32(p - t)^2 of the elements i, i + 1024, ... in fp64, the
    1024 sums are folded in halves, loss = fl32(sum / n); grad = fl32(fl32(p - t) fl32(2 / n))."""
    d = (p - t).astype(np.float32)
    sq = np.zeros(-(-n // 1024) * 1024, dtype=np.float64)
    sq[:n] = d.astype(np.float64) ** 2
    s = np.zeros(1024, dtype=np.float64)
    for row in sq.reshape(-1, 1024):
        s = s + row
    o = 512
    while o:
        s[:o] = s[:o] + s[o:2 * o]
        o >>= 1
    inv = np.float32(2.0) / np.float32(n)
    return np.float32(s[0] / np.float64(n)), (d * inv).astype(np.float32)


@pytest.mark.parametrize('n', [1, 1023, 1024, 1025, 10800, 16385, 40000])
def test_mse_bits(dev, n):
    p_h, t_h = det_uniform((n,), 1, -2, 2), det_uniform((n,), 2, -2, 2)
    p, t = torch.from_numpy(p_h).to(dev), torch.from_numpy(t_h).to(dev)
    d, st = lib.stream_args(p)
    loss_ref, grad_ref = mse_serial(p_h, t_h, n)
    loss, grad = torch.zeros(1, device=dev), torch.full((n + 8,), 5.0, device=dev)
    lib.call('mmft_mse_fwd_bwd', p, t, n, loss, grad, d, st)
    assert np.array_equal(loss.cpu().numpy(), np.array([loss_ref])), (float(loss), float(loss_ref))
    assert np.array_equal(grad[:n].cpu().numpy(), grad_ref) and bool((grad[n:] == 5.0).all())
    loss2 = torch.zeros(1, device=dev)
    lib.call('mmft_mse_fwd_bwd', p, t, n, loss2, None, d, st)                 # grad = NULL
    assert torch.equal(loss2, loss)
    for ld in (2, 3):
        rows = max(n // 3, 1)                                                 # fewer table rows than batch rows: indices repeat
        table_h = det_uniform((rows, ld), 3, -2, 2)
        idx_h = det_ints((n,), 4, 0, rows)
        assert n < 3 or len(np.unique(idx_h)) < n
        table, idx = torch.from_numpy(table_h).to(dev), I32(idx_h, dev)
        loss_ref, grad_ref = mse_serial(p_h, table_h[idx_h, 0], n)
        loss, grad = torch.zeros(1, device=dev), torch.full((n + 8,), 5.0, device=dev)
        lib.call('mmft_mse_gather_fwd_bwd', p, table, ld, idx, n, loss, grad, d, st)
        assert np.array_equal(loss.cpu().numpy(), np.array([loss_ref])), (ld, float(loss), float(loss_ref))
        assert np.array_equal(grad[:n].cpu().numpy(), grad_ref) and bool((grad[n:] == 5.0).all())
        loss2 = torch.zeros(1, device=dev)
        lib.call('mmft_mse_gather_fwd_bwd', p, table, ld, idx, n, loss2, None, d, st)
        assert torch.equal(loss2, loss)
