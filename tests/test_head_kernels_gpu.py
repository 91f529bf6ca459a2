"""Kernel-level parity of the fusion head and the step glue (csrc/fusion.hip): every entry point called by name through the
C ABI, against plain fp64 math on the same inputs, at the shapes where the kernels change code path.  The test picks the
kernel (per-cell form, run form, host-scalar / device-scalar / counted Adam); no Python dispatcher does."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from mmft import lib
from mmft.detrand import det_uniform, det_ints
from mmft.fusion import PathMasks, batch_links

pytestmark = pytest.mark.gpu
TOL = 2e-5          # as tests/test_kernels_gpu.py: fp32 fmaf chains vs the fp64 reference, relative to the largest magnitude
EPS24 = 2.0 ** -24  # half an ulp of 1.0 in fp32
S = 64              # cells per prefix block of the run form (mmft.fusion.RUN_BLOCK)
BAD_ARG = -1        # MMFT_ERR_BAD_ARG


def T_(shape, seed, dev, lo=-1.0, hi=1.0):
    return torch.from_numpy(det_uniform(shape, seed, lo, hi)).to(dev)


def I32(a, dev):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev)


def close(got, ref, atol):
    """max |got - ref| <= atol, both printed so that a failure names the figure."""
    err = float((got.detach().double().cpu() - torch.as_tensor(ref).double().cpu()).abs().max())
    return err <= atol, err


# --------------------------------------------------------------------------------------------- masked projection
def hand_masks(P):
    """Cell lists of one design's paths, built by hand so that every edge of the run form occurs (asserted in `_edges`)."""
    last = P - 1
    paths = [
        [],                                                  # 0: empty mask row
        [0],                                                 # 1: cell 0; a run starting at cell 0 of a block
        [last],                                              # 2: cell P - 1; a run ending at a block's last cell (P % 64 == 0)
        list(range(0, min(S, P))),                           # 3: one whole block
        list(range(S, 4 * S)) if P >= 4 * S else list(range(40, min(90, P))),   # 4: three consecutive blocks end to end
        list(range(3, 9)),                                   # 5: never sampled (first = -1)
        list(range(5, 21)) + list(range(30, 41)),            # 6: sampled three times (the `next` chain)
    ]
    paths += [list(range(10 + i, 21)) for i in range(6)]     # 7..12: six runs ending at cell 20 -> a boundary list of > 4 entries
    paths.append(list(range(33, 48)) + ([c for c in range(70, 76) if c < P]))   # 13: runs that start inside a block
    paths.append(list(range(1, P, 2)))                       # 14: a comb, P / 2 single-cell runs (two runs per trip of fwd_runs)
    return paths


NP_ = 15                                                     # paths per design in hand_masks
SAMPLED = [1, 2, 3, 6, 4, 7, 8, 6, 9, 10, 11, 12, 13, 14, 0, 6]     # batch rows of one design: 5 never, 6 three times


def build_case(P, B, dev):
    per = hand_masks(P)
    assert len(per) == NP_
    ip, cols = [0], []
    for q in per:
        assert q == sorted(set(q)) and (not q or (q[0] >= 0 and q[-1] < P))
        cols += q
        ip.append(len(cols))
    ms = [PathMasks(np.array(ip), np.array(cols, dtype=np.int64), P, dev) for _ in range(B)]
    pmk = ms[0] if B == 1 else PathMasks.batch(ms)
    designs = [0] if B == 1 else [0, 2]                      # B = 3: design 1 has no sampled path
    paths = np.array([b * NP_ + q for b in designs for q in SAMPLED], dtype=np.int64)
    if B > 1:                                                # interleave the designs' rows
        paths = paths.reshape(len(designs), -1).T.reshape(-1).copy()
    return per, pmk, paths


def _edges(per, pmk, paths, P, B):
    """Every hand-built edge is present in this case's input (those a P of one block or of no block cannot hold are skipped
    there and asserted at P = 256)."""
    first, nxt = batch_links(paths, pmk.num_paths)
    ip, cc = pmk.host_indptr, pmk.host_cols
    lens = np.diff(ip)
    covered = np.unique(cc)
    assert covered[0] == 0 and covered[-1] == P - 1                               # cell 0 and cell P - 1
    assert (lens == 0).any()                                                      # an empty mask row
    sampled = set(paths.tolist())
    assert (first[[q for q in range(pmk.num_paths) if q not in sampled]] == -1).all() and len(sampled) < pmk.num_paths
    chains = []
    for q in sampled:
        n, t = 0, first[q]
        while t >= 0:
            n, t = n + 1, nxt[t]
        chains.append(n)
    assert max(chains) == 3                                                       # one path sampled three times
    assert int(np.diff(pmk.csc_indptr.cpu().numpy()).max()) > 4                   # per-cell backward: 4 in flight + tail
    if B == 3:
        assert set(pmk.row_design[paths].tolist()) == {0, 2}                      # one design without a sampled path
    if P % S:
        assert pmk.run_block == 0                                                 # no run form: per-cell kernels both ways
        return first, nxt
    assert pmk.run_block == S
    rs, rl = pmk.run_start.cpu().numpy(), pmk.run_len.cpu().numpy()
    assert ((rs % S) == 0).any()                                                  # a run starting at cell 0 of a block
    assert (((rs + rl) % S) == 0).any()                                           # a run ending at a block's last cell
    assert any(len(q) == S and q[0] % S == 0 and q[-1] == q[0] + S - 1 for q in per)          # one mask = a whole block
    if P >= 4 * S:
        assert any(len(q) == 3 * S and q[0] % S == 0 and q[-1] == q[0] + 3 * S - 1 for q in per)   # three blocks end to end
    assert int(np.diff(pmk.bnd_ptr.cpu().numpy()).max()) > 4                      # a boundary list of more than four entries
    assert int(np.diff(pmk.run_ptr.cpu().numpy()).max()) >= P // 2                # the comb: more runs than fwd_runs' lanes
    return first, nxt


def dense_reference(pmk, paths, f, w, bias, gout, P, B):
    """fp64: out = (mask_rows * f[design]) @ w.T + bias and its gradients dwT [P, Dout], df [B, P]."""
    Tn = len(paths)
    M = np.zeros((Tn, P))
    des = pmk.row_design[paths]
    for t, q in enumerate(paths):
        M[t, pmk.host_cols[pmk.host_indptr[q]:pmk.host_indptr[q + 1]]] = 1.0
    f64, w64, g64 = f.double().cpu().numpy().reshape(B, P), w.double().cpu().numpy(), gout.double().cpu().numpy()
    X = M * f64[des]
    out = X @ w64.T + (bias.double().cpu().numpy() if bias is not None else 0.0)
    dwT = (g64.T @ X).T
    dX = (g64 @ w64) * M
    df = np.zeros((B, P))
    np.add.at(df, des, dX)
    ncells = int(M.sum(1).max())
    return out, dwT, df, ncells


def run_forward(kind, pmk, paths_d, foff, f, wT, bias, Dout, P, B, dev):
    Tn = paths_d.numel()
    out = torch.full((Tn, Dout), 7.0, device=dev)
    d, st = lib.stream_args(f)
    if kind == 'cells':
        lib.call('mmft_masked_fc_fwd', pmk.indptr, pmk.cols, paths_d, foff, Tn, f, wT, bias, out, P, Dout, d, st)
    else:
        GP = torch.empty((B * P, Dout), device=dev)
        lib.call('mmft_masked_fc_prefix', f, wT, GP, B, P, Dout, S, d, st)
        lib.call('mmft_masked_fc_fwd_runs', pmk.run_ptr, pmk.run_start, pmk.run_len, paths_d, foff, Tn, GP, bias, out, Dout, S, d, st)
    return out


def run_backward(kind, pmk, first, nxt, gout, f, wT, Dout, P, B, dev):
    dwT = torch.full((P, Dout), 7.0, device=dev)
    df = torch.full((B * P,), 7.0, device=dev)
    need = B * P * Dout * 4 if B > 1 else 0
    assert lib.query('mmft_masked_fc_bwd_runs_workspace_bytes', B, P, Dout) == need
    ws = torch.empty(max(need // 4, 4), device=dev)
    d, st = lib.stream_args(f)
    if kind == 'cells':
        lib.call('mmft_masked_fc_bwd', pmk.csc_indptr, pmk.csc_paths, first, nxt, gout, gout.stride(0), f, wT, dwT, df, B, P, Dout,
                 ws, ws.numel() * 4, d, st)
    else:
        lib.call('mmft_masked_fc_bwd_runs', pmk.bnd_ptr, pmk.bnd_code, first, nxt, gout, gout.stride(0), f, wT, dwT, df, B, P,
                 Dout, S, ws, ws.numel() * 4, d, st)
    return dwT, df.reshape(B, P)


RUN_BWD_DOUT = (32, 64, 128, 256)      # 1, 2, 4, 8 cells per entry lane of the run-form backward; 256 fills 64 KB of LDS


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('P', [64, 256, 100])
@pytest.mark.parametrize('Dout', [4, 12, 32, 64, 128, 256])
def test_masked_fc_kernels(dev, Dout, P, B):
    """mmft_transpose, mmft_masked_fc_fwd, mmft_masked_fc_prefix + mmft_masked_fc_fwd_runs, mmft_masked_fc_bwd and
    mmft_masked_fc_bwd_runs against the dense fp64 product and its gradients, on hand-built masks.

    Tolerances.  Per-cell forms: TOL * max|ref|.  Run form, forward: every add inside a block's prefix is rounded at a
    magnitude of at most S m, m = max|f| max|w|, so TOL max|ref| + ncells S m 2^-24 (ncells = the largest mask).  dwT and df are
    compared the same way: TOL max|ref| for the per-cell backward, the same bound with the same m for the run-form backward."""
    per, pmk, paths = build_case(P, B, dev)
    first_h, nxt_h = _edges(per, pmk, paths, P, B)
    Tn = len(paths)
    f = T_((B, P), 1, dev).reshape(-1).contiguous()
    w = T_((Dout, P), 2, dev, -0.05, 0.05)
    bias = T_((Dout,), 3, dev)
    gwide = T_((Tn, Dout + 8), 4, dev)
    gout = gwide[:, 4:4 + Dout]                                   # a column slice of a wider tensor: ldg > Dout
    assert gout.stride(0) == Dout + 8 and gout.data_ptr() % 16 == 0
    d, st = lib.stream_args(f)
    wT = torch.empty((P, Dout), device=dev)
    lib.call('mmft_transpose', w, wT, Dout, P, d, st)
    assert torch.equal(wT, w.t().contiguous())
    paths_d = I32(paths, dev)
    foff = I32(pmk.row_design[paths] * P, dev) if B > 1 else None
    first, nxt = I32(first_h, dev), I32(nxt_h, dev)
    ref, dwT_ref, df_ref, ncells = dense_reference(pmk, paths, f, w, bias, gout, P, B)
    m = float(f.abs().max() * w.abs().max())
    kinds = ('cells', 'runs') if pmk.run_block else ('cells',)
    for kind in kinds:
        extra = ncells * S * m * EPS24 if kind == 'runs' else 0.0
        out = run_forward(kind, pmk, paths_d, foff, f, wT, bias, Dout, P, B, dev)
        ok, err = close(out, ref, TOL * np.abs(ref).max() + extra)
        print(f'{kind} fwd Dout={Dout} P={P} B={B}: max abs err {err:.3e}, max|ref| {np.abs(ref).max():.3e}')
        assert ok
        # bias = None: the same sums without the bias row
        out0 = run_forward(kind, pmk, paths_d, foff, f, wT, None, Dout, P, B, dev)
        ok, err = close(out0, ref - bias.double().cpu().numpy(), TOL * np.abs(ref).max() + extra)
        assert ok, err
        if B == 1:                                               # f_off given (all zero) and not given: the same launch result
            z = torch.zeros(Tn, dtype=torch.int32, device=dev)
            assert torch.equal(run_forward(kind, pmk, paths_d, z, f, wT, bias, Dout, P, B, dev), out)
    for kind in kinds:
        if kind == 'runs' and Dout not in RUN_BWD_DOUT:
            # Dout / 4 = 1 leaves S short of the 512 entry lanes, Dout / 4 = 3 is no power of two: an error, not a launch
            dwT = torch.full((P, Dout), 7.0, device=dev)
            df = torch.full((B * P,), 7.0, device=dev)
            ws = torch.empty(B * P * Dout, device=dev)
            rc = lib.query('mmft_masked_fc_bwd_runs', pmk.bnd_ptr, pmk.bnd_code, first, nxt, gout, gout.stride(0), f, wT, dwT, df, B, P,
                           Dout, S, ws, ws.numel() * 4, d, st)
            assert rc == BAD_ARG and b'masked_fc_bwd_runs' in lib.load().mmft_last_error()
            torch.cuda.synchronize()
            assert bool((dwT == 7.0).all()) and bool((df == 7.0).all())
            continue
        dwT, df = run_backward(kind, pmk, first, nxt, gout, f, wT, Dout, P, B, dev)
        extra = ncells * S * m * EPS24 if kind == 'runs' else 0.0
        ok1, e1 = close(dwT, dwT_ref, TOL * np.abs(dwT_ref).max() + extra)
        ok2, e2 = close(df, df_ref, TOL * np.abs(df_ref).max() + extra)
        print(f'{kind} bwd Dout={Dout} P={P} B={B}: dwT err {e1:.3e} (max {np.abs(dwT_ref).max():.3e}), '
              f'df err {e2:.3e} (max {np.abs(df_ref).max():.3e})')
        assert ok1 and ok2
        dwT2, df2 = run_backward(kind, pmk, first, nxt, gout, f, wT, Dout, P, B, dev)
        assert torch.equal(dwT, dwT2) and torch.equal(df, df2)     # fixed slab / gather order: bitwise reproducible


def test_masked_fc_same_sign_prefix_cancellation(dev):
    """f and w in [0.5, 1], every mask a single cell at position 63 of its block: the run form computes GP[63] - GP[62] with
    both prefixes near 64 m, so its error is set by the block prefix (S m 2^-24 per cell), not by the row's sum - the term the
    run-form bound carries.  The per-cell form on the same input stays within plain TOL."""
    P, Dout, B = 256, 128, 1
    nblk = P // S
    cols = np.array([b * S + S - 1 for b in range(nblk)], dtype=np.int64)
    pmk = PathMasks(np.arange(nblk + 1), cols, P, dev)
    rs, rl = pmk.run_start.cpu().numpy(), pmk.run_len.cpu().numpy()
    assert pmk.run_block == S and (rs % S == S - 1).all() and (rl == 1).all()
    paths = np.arange(nblk)
    f = T_((P,), 1, dev, 0.5, 1.0)
    w = T_((Dout, P), 2, dev, 0.5, 1.0)
    gout = T_((nblk, Dout), 3, dev)
    d, st = lib.stream_args(f)
    wT = torch.empty((P, Dout), device=dev)
    lib.call('mmft_transpose', w, wT, Dout, P, d, st)
    ref, dwT_ref, df_ref, ncells = dense_reference(pmk, paths, f, w, None, gout, P, B)
    assert ncells == 1
    m = float(f.abs().max() * w.abs().max())
    paths_d = I32(paths, dev)
    out_c = run_forward('cells', pmk, paths_d, None, f, wT, None, Dout, P, B, dev)
    out_r = run_forward('runs', pmk, paths_d, None, f, wT, None, Dout, P, B, dev)
    okc, ec = close(out_c, ref, TOL * np.abs(ref).max())
    okr, er = close(out_r, ref, TOL * np.abs(ref).max() + ncells * S * m * EPS24)
    print(f'same sign: per-cell err {ec:.3e}, run form err {er:.3e}, max|ref| {np.abs(ref).max():.3e}, S m 2^-24 = {S * m * EPS24:.3e}')
    assert okc and okr
    fh, nh = batch_links(paths, nblk)
    first, nxt = I32(fh, dev), I32(nh, dev)
    for kind in ('cells', 'runs'):
        dwT, df = run_backward(kind, pmk, first, nxt, gout, f, wT, Dout, P, B, dev)
        assert rel_err(dwT, torch.from_numpy(dwT_ref)) < TOL and rel_err(df, torch.from_numpy(df_ref)) < TOL


# --------------------------------------------------------------------------------------------- one-call level head
@pytest.mark.parametrize('nout', [1, 4])
@pytest.mark.parametrize('Dc', [32, 128])
@pytest.mark.parametrize('T', [1, 37, 300])
def test_head_level_fwd(dev, T, Dc, nout):
    """mmft_head_level_fwd against the fp64 composition gather | dense masked projection | level embedding -> Linear - ReLU -
    Linear, within TOL of the largest reference magnitude.  Sentinels behind the stated workspace
    and output sizes must survive; T = 0 returns OK and writes nothing."""
    Dh, Da, H1, P, N = 128, 4, 64, 256, 500
    Dz = Dh + Dc + Da
    per = [sorted({(7 * q + 3 * k) % P for k in range(1 + q % 9)} | ({q % P, (q + 1) % P} if q % 2 else set())) for q in range(40)]
    ip, cols = [0], []
    for q in per:
        cols += q
        ip.append(len(cols))
    pmk = PathMasks(np.array(ip), np.array(cols, dtype=np.int64), P, dev)
    assert pmk.run_block == S
    paths = det_ints((max(T, 1),), 5, 0, 40)[:T]
    targets = det_ints((max(T, 1),), 6, 0, N)[:T]
    hwide = T_((N, Dh + 4), 1, dev)
    h = hwide[:, :Dh]                                            # row stride larger than the width
    f = T_((P,), 2, dev)
    wf = T_((Dc, P), 3, dev, -0.02, 0.02)
    bf = T_((Dc,), 4, dev)
    alpha_row = T_((Da,), 5, dev)
    w1, b1 = T_((H1, Dz), 6, dev, -Dz ** -0.5, Dz ** -0.5), T_((H1,), 7, dev)
    w2, b2 = T_((nout, H1), 8, dev, -H1 ** -0.5, H1 ** -0.5), T_((nout,), 9, dev)
    d, st = lib.stream_args(f)
    wT = torch.empty((P, Dc), device=dev)
    lib.call('mmft_transpose', wf, wT, Dc, P, d, st)
    GP = torch.empty((P, Dc), device=dev)
    lib.call('mmft_masked_fc_prefix', f, wT, GP, 1, P, Dc, S, d, st)
    need = lib.query('mmft_head_level_workspace_bytes', T, Dh, Dc, Da, H1)
    assert need == T * (Dz + H1) * 4
    SENT = 12345.0
    ws = torch.full((need // 4 + 64,), SENT, device=dev)
    outbuf = torch.full((T * nout + 64,), SENT, device=dev)
    paths_d, targets_d = I32(paths, dev), I32(targets, dev)

    def call(Tn):
        lib.call('mmft_head_level_fwd', h, h.stride(0), targets_d, Tn, Dh, pmk.run_ptr, pmk.run_start, pmk.run_len, paths_d, None,
                 GP, bf, Dc, S, alpha_row, Da, w1, b1, H1, w2, b2, nout, ws, need, outbuf, d, st)
    call(0)
    torch.cuda.synchronize()
    assert bool((ws == SENT).all()) and bool((outbuf == SENT).all())          # T = 0: OK, nothing written
    call(T)
    torch.cuda.synchronize()
    assert bool((ws[need // 4:] == SENT).all()) and bool((outbuf[T * nout:] == SENT).all())
    M = np.zeros((T, P))
    for t, q in enumerate(paths):
        M[t, per[q]] = 1.0
    proj = (M * f.double().cpu().numpy()) @ wf.double().cpu().numpy().T + bf.double().cpu().numpy()
    z = np.concatenate([h.double().cpu().numpy()[targets], proj, np.tile(alpha_row.double().cpu().numpy(), (T, 1))], 1)
    hid = np.maximum(z @ w1.double().cpu().numpy().T + b1.double().cpu().numpy(), 0.0)
    ref = hid @ w2.double().cpu().numpy().T + b2.double().cpu().numpy()
    atol = TOL * np.abs(ref).max()
    ok, err = close(outbuf[:T * nout].reshape(T, nout), ref, atol)
    print(f'head_level T={T} Dc={Dc} nout={nout}: err {err:.3e}, bound {atol:.3e}, max|ref| {np.abs(ref).max():.3e}')
    assert ok


# --------------------------------------------------------------------------------------------- concatenation
@pytest.mark.parametrize('three', [False, True])
def test_concat_cols(dev, three):
    """mmft_concat_cols: two and three blocks of unequal widths (4, 128, 12) read and written with row strides larger than
    the widths; exactly torch.cat, and nothing outside the written columns changes."""
    T, Da, Db, Dc = 77, 4, 128, 12
    a = T_((T, Da + 4), 1, dev)[:, :Da]
    b = T_((T, Db + 8), 2, dev)[:, 4:4 + Db]
    c = T_((T, Dc + 4), 3, dev)[:, :Dc] if three else None
    W = Da + Db + (Dc if three else 0)
    SENT = -9.0
    out = torch.full((T, W + 8), SENT, device=dev)
    d, st = lib.stream_args(a)
    lib.call('mmft_concat_cols', a, a.stride(0), Da, b, b.stride(0), Db, c, c.stride(0) if three else 0, Dc if three else 0, out,
             out.stride(0), T, d, st)
    assert torch.equal(out[:, :W], torch.cat([a, b] + ([c] if three else []), 1))
    assert bool((out[:, W:] == SENT).all())


# --------------------------------------------------------------------------------------------- losses and metrics
N_LOSS = [1, 63, 1024, 1025, 4097, 70001]      # one partial wave, one full block, the four-per-thread request loop and its tails


@pytest.mark.parametrize('n', N_LOSS)
def test_mse_fwd_bwd(dev, n):
    """mmft_mse_fwd_bwd / mmft_mse_gather_fwd_bwd: loss against fp64 (1e-6 relative); the gradient is fl32(d fl32(2 / n)) with
    d = fl32(p - t), recomputed the same way on the host: bit equality.  Gather form: ld in {1, 3}, repeated indices."""
    p_h, t_h = det_uniform((n,), 1, -2, 2), det_uniform((n,), 2, -2, 2)
    inv = np.float32(2.0) / np.float32(n)
    p, t = torch.from_numpy(p_h).to(dev), torch.from_numpy(t_h).to(dev)
    loss, grad = torch.zeros(1, device=dev), torch.full((n + 8,), 5.0, device=dev)
    d, st = lib.stream_args(p)
    lib.call('mmft_mse_fwd_bwd', p, t, n, loss, grad, d, st)
    ref = float(((p_h.astype(np.float64) - t_h.astype(np.float64)) ** 2).mean())
    assert abs(float(loss) - ref) <= 1e-6 * abs(ref)
    gref = ((p_h - t_h).astype(np.float32) * inv).astype(np.float32)
    assert np.array_equal(grad[:n].cpu().numpy(), gref) and bool((grad[n:] == 5.0).all())
    loss2 = torch.zeros(1, device=dev)
    lib.call('mmft_mse_fwd_bwd', p, t, n, loss2, None, d, st)                 # grad = NULL: the loss alone
    assert torch.equal(loss2, loss)
    for ld in (1, 3):
        rows = max(n // 3, 1)                                                 # fewer table rows than batch rows: indices repeat
        table_h = det_uniform((rows, ld), 3, -2, 2)
        idx_h = det_ints((n,), 4, 0, rows)
        assert n < 3 or len(np.unique(idx_h)) < n
        table, idx = torch.from_numpy(table_h).to(dev), I32(idx_h, dev)
        loss, grad = torch.zeros(1, device=dev), torch.full((n + 8,), 5.0, device=dev)
        lib.call('mmft_mse_gather_fwd_bwd', p, table, ld, idx, n, loss, grad, d, st)
        tg = table_h[idx_h, 0]
        ref = float(((p_h.astype(np.float64) - tg.astype(np.float64)) ** 2).mean())
        assert abs(float(loss) - ref) <= 1e-6 * abs(ref)
        gref = ((p_h - tg).astype(np.float32) * inv).astype(np.float32)
        assert np.array_equal(grad[:n].cpu().numpy(), gref) and bool((grad[n:] == 5.0).all())


def _ce_inputs(n, C, wide):
    z = det_uniform((n, C), 11, -90, 90) if wide else det_uniform((n, C), 11, -4, 4)
    y = det_ints((n,), 12, 0, C)
    y[0] = 0
    y[-1] = C - 1 if n > 1 else y[-1]
    if n == 1:
        y[0] = C - 1
    # tied maxima: every third row holds its maximum twice, once in class 0 on every sixth (predicted class = the FIRST maximum)
    for i in range(0, n, 3):
        j = int(np.argmax(z[i]))
        k = 0 if i % 6 == 0 else (j + 1 + i) % C
        z[i, k] = z[i, j]
    return z, y


# every n of N_LOSS with C = 2 and 5; C = 1024 with every n but 70001 (a 287 MB logit tensor, and no path of the kernel depends on
# both sizes at once: it strides rows by 1024 threads and loops over C inside a row)
CE_CASES = [(n, C) for C in (2, 5) for n in N_LOSS] + [(n, 1024) for n in N_LOSS if n != 70001]


@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('n,C', CE_CASES)
def test_cross_entropy_fwd_bwd(dev, n, C, wide):
    """mmft_cross_entropy_fwd_bwd against torch.nn.functional.cross_entropy in fp64 within TOL (loss relative to itself, the
    gradient relative to its largest entry); logits in [-90, 90] where a plain exp overflows; rows with tied maxima counted
    through eval_out's tp / fp / tn / fn against torch.argmax (first maximum); labels hitting class 0 and C - 1; grad = NULL;
    loss = NULL with eval_out."""
    z_h, y_h = _ce_inputs(n, C, wide)
    assert y_h.min() == 0 or n == 1
    assert y_h.max() == C - 1
    am = torch.from_numpy(z_h).argmax(1).numpy()
    assert n < 3 or ((z_h == z_h.max(1, keepdims=True)).sum(1) > 1).any()
    z, y = torch.from_numpy(z_h).to(dev), torch.from_numpy(y_h).to(dev)
    z64 = torch.from_numpy(z_h).double().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(z64, torch.from_numpy(y_h))
    ref.backward()
    loss, grad = torch.zeros(1, device=dev), torch.empty((n, C), device=dev)
    ev = torch.zeros(6, dtype=torch.float64, device=dev)
    d, st = lib.stream_args(z)
    lib.call('mmft_cross_entropy_fwd_bwd', z, y, n, C, loss, grad, ev, d, st)
    el = abs(float(loss) - float(ref)) / abs(float(ref))
    eg = rel_err(grad, z64.grad)
    print(f'cross entropy n={n} C={C} wide={wide}: loss rel err {el:.3e}, grad rel err {eg:.3e}')
    assert el < TOL and eg < TOL
    pp, ap = am != 0, y_h != 0
    counts = [n, None, int((pp & ap).sum()), int((pp & ~ap).sum()), int((~pp & ~ap).sum()), int((~pp & ap).sum())]
    evh = ev.cpu().numpy()
    assert [int(evh[k]) for k in (0, 2, 3, 4, 5)] == [counts[k] for k in (0, 2, 3, 4, 5)]
    assert abs(evh[1] / n - float(ref)) < TOL * abs(float(ref))
    loss2 = torch.zeros(1, device=dev)
    lib.call('mmft_cross_entropy_fwd_bwd', z, y, n, C, loss2, None, None, d, st)          # grad = NULL
    assert torch.equal(loss2, loss)
    ev2 = torch.zeros(6, dtype=torch.float64, device=dev)
    lib.call('mmft_cross_entropy_fwd_bwd', z, y, n, C, None, None, ev2, d, st)            # loss = NULL, eval_out given
    assert torch.equal(ev2, ev)


def _eval_inputs(n):
    pred, arr = det_uniform((n,), 21, 0, 4), det_uniform((n,), 22, 0, 4)
    req = det_uniform((n,), 23, 0, 4)
    label = (det_ints((n,), 24, 0, 2)).astype(np.float32)
    arr[::5] = 0.0                                          # targets that are exactly 0: skipped in the MAPE numerator
    req[1::7] = pred[1::7]                                  # required == pred exactly: not critical
    if n >= 8:                                              # every tp / fp / tn / fn quadrant at least once
        req[:4] = pred[:4] + np.float32([-1, -1, 1, 1])
        label[:4] = [1, 0, 0, 1]
    return pred, arr, req, label


def _eval_ref(pred, arr, req, label):
    p, t, r = pred.astype(np.float64), arr.astype(np.float64), req.astype(np.float64)
    dd = p - t
    nz = t != 0
    pc, ac = (r - p) < 0, label != 0
    return np.array([len(p), t.sum(), (t * t).sum(), (dd * dd).sum(), np.abs(dd).sum(), (np.abs(dd[nz]) / np.abs(t[nz])).sum(),
                     (pc & ac).sum(), (pc & ~ac).sum(), (~pc & ~ac).sum(), (~pc & ac).sum()], dtype=np.float64)


@pytest.mark.parametrize('n', N_LOSS)
def test_eval_sums(dev, n):
    """mmft_eval_sums and mmft_eval_sums_by_level against fp64 numpy: the kernel accumulates in fp64 and only the order
    differs, so 1e-12 relative on the real sums and exact counts.  By level: 7 levels, two of them empty (rows of zeros), one
    holding a single element; the rows add up to the whole batch's sums."""
    pred, arr, req, label = _eval_inputs(n)
    assert (arr == 0).any() and (n < 2 or (req == pred).any())
    ref = _eval_ref(pred, arr, req, label)
    if n >= 8:
        assert (ref[6:] > 0).all()
    dt = [torch.from_numpy(a).to(dev) for a in (pred, arr, req, label)]
    out = torch.full((12,), -1.0, dtype=torch.float64, device=dev)
    d, st = lib.stream_args(dt[0])
    lib.call('mmft_eval_sums', *dt, n, out, d, st)
    got = out.cpu().numpy()
    assert np.all(np.abs(got[:6] - ref[:6]) <= 1e-12 * np.abs(ref[:6])) and np.array_equal(got[6:10], ref[6:]) and \
        (got[10:] == -1.0).all()
    L = 7
    lev = np.array([0, 1, 3, 6])[det_ints((n,), 25, 0, 4)]             # levels 2 and 4 stay empty
    if n > 1:
        lev[lev == 5] = 0
        lev[n // 2] = 5                                                # level 5: a single element
    lo = torch.full((L * 10 + 2,), -1.0, dtype=torch.float64, device=dev)
    lib.call('mmft_eval_sums_by_level', *dt, I32(lev, dev), n, L, lo, d, st)
    got_l = lo.cpu().numpy()
    assert (got_l[L * 10:] == -1.0).all()
    got_l = got_l[:L * 10].reshape(L, 10)
    assert (got_l[[2, 4]] == 0).all()
    if n > 1:
        assert got_l[5, 0] == 1
    for l in range(L):
        sel = lev == l
        rl = _eval_ref(pred[sel], arr[sel], req[sel], label[sel])
        assert np.all(np.abs(got_l[l, :6] - rl[:6]) <= 1e-12 * np.abs(rl[:6])) and np.array_equal(got_l[l, 6:], rl[6:])
    tot = got_l.sum(0)
    assert np.all(np.abs(tot - got[:10]) <= 1e-12 * np.abs(got[:10]))


# --------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('n', [1, 255, 256, 100003])
def test_adam_three_forms(dev, n, wd):
    """Five steps of mmft_adam_step, mmft_adam_step_dev and mmft_adam_step_counted (gscale = 0.5) against torch.optim.Adam in
    fp64 on the same gradients (1e-6 relative, the bound of test_flat_adam_matches_torch); the three forms agree bitwise;
    the counted form with zero_grad = 1 leaves g all zero and advances state[0] by one per launch."""
    lr, b1, b2, eps, gscale, steps = 1e-3, 0.9, 0.999, 1e-8, 0.5, 5
    p0 = det_uniform((n,), 1, -1, 1)
    grads = [det_uniform((n,), 10 + k, -1, 1) for k in range(steps)]
    pr = torch.from_numpy(p0).double().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    forms = {}
    for name in ('host', 'dev', 'counted'):
        forms[name] = dict(p=torch.from_numpy(p0).to(dev), m=torch.zeros(n, device=dev), v=torch.zeros(n, device=dev))
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    d, st = lib.stream_args(forms['host']['p'])
    for k in range(steps):
        t = k + 1
        pr.grad = torch.from_numpy(grads[k]).double() * gscale
        opt.step()
        # the same inputs for all three: the fp32 values of lr and the betas that cross the ABI, bias corrections in fp64
        bc1, bc2 = 1.0 - float(np.float32(b1)) ** t, 1.0 - float(np.float32(b2)) ** t
        g = torch.from_numpy(grads[k]).to(dev)
        s = forms['host']
        lib.call('mmft_adam_step', s['p'], g, s['m'], s['v'], n, lr, b1, b2, eps, wd, bc1, bc2, gscale, d, st)
        s = forms['dev']
        scal = torch.tensor([float(np.float32(lr)) / bc1, bc2 ** 0.5], dtype=torch.float64).float().to(dev)
        lib.call('mmft_adam_step_dev', s['p'], g, s['m'], s['v'], n, scal, b1, b2, eps, wd, gscale, d, st)
        s = forms['counted']
        gz = g.clone()
        lib.call('mmft_adam_step_counted', s['p'], gz, s['m'], s['v'], n, state, lr, b1, b2, eps, wd, gscale, 1, d, st)
        assert not bool(gz.any())                                         # zero_grad = 1
        assert state.cpu().tolist() == [t, 0]
        for name in ('host', 'dev', 'counted'):
            e = rel_err(forms[name]['p'], pr)
            assert e < 1e-6, (name, t, e)
        for key in ('p', 'm', 'v'):
            assert torch.equal(forms['host'][key], forms['dev'][key]), (key, t, 'host vs dev')
            assert torch.equal(forms['dev'][key], forms['counted'][key]), (key, t, 'dev vs counted')
    gk = torch.from_numpy(grads[0]).to(dev)
    s = forms['counted']
    lib.call('mmft_adam_step_counted', s['p'], gk, s['m'], s['v'], n, state, lr, b1, b2, eps, wd, gscale, 0, d, st)
    assert torch.equal(gk, torch.from_numpy(grads[0]).to(dev)) and state.cpu().tolist() == [steps + 1, 0]     # zero_grad = 0
