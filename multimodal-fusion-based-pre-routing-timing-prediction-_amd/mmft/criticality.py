"""Timing criticality per pin and per map cell, on the device: for every pin the worst slack of any predicted path through it,
the batch row of that path, the number of violating paths through it and a criticality in [0, 1]; for every cell of every
design's map the worst slack and the number of violating paths whose mask covers it - what a timing-driven placer turns into
net weights and into regions to spread.  One entry point (mmft_criticality, include/mmft_crit.h: three small launches) on
the tables a `placement.PlacedPaths` already holds, and one device->host copy, instead of a copy of the predictions, a walk
over the path nodes and a re-rasterisation of the masks on the host.

The rules (the header states them, `reference_criticality` restates them in numpy):
  slack = required - pred, one fp32 subtraction, -0.0 canonicalised to +0.0 (report.reference_slack: the rule of the timing
  report); a row is valid unless its slack is NaN and violates when slack < 0; minima are taken over valid rows, the smaller
  batch row first on equal slack; node_crit = node_slack / (worst slack of the design), one fp32 division, 1 when they are
  equal, 0 without a violation; the mask of a row is the mask rule of include/mmft_place.h (placement.rasterize_host).

The second half of the module (mmft_criticality_sums, include/mmft_crit_sums.h) adds the sums of negative slack per pin, per
cell and per design as exact integer sums of quanta, and each pin's and cell's share of its design's TNS.
"""
import functools

import numpy as np
import torch

from . import lib
from .placement import MAX_CELLS, batch_tables, rasterize_host
from .report import AfterHead, reference_slack

FIELDS = ('node_slack', 'node_row', 'node_viol', 'node_crit', 'cell_slack', 'cell_viol', 'counts')
SUM_FIELDS = ('node_nsum', 'cell_nsum', 'design_nsum', 'saturated', 'node_share', 'cell_share')
_KINDS = dict(f4=torch.float32, i4=torch.int32, i8=torch.int64)


def workspace_bytes(N, B, P):
    """Bytes of the keyed words; P = 0 without the cell outputs."""
    return lib.crit('mmft_criticality_workspace_bytes', int(N), int(B), int(P))


class _Buffers:
    """The static output buffers of one launch, carved out of ONE buffer of 4-byte words so that `host()` is one device->host
    copy.  A subclass states `fields`, the order in which `tensors()` and `host()` give them (and `count`, their number in
    words), and `layout`, the order in which they lie in the buffer: (name, f4 | i4 | i8, shape) with the shape one of N, B,
    B2 = [B, 2] and BP = [B, P].  The cell_ fields exist only with cells."""

    def __init__(self, N, B, P, device, cells=True):
        self.N, self.B, self.cells = int(N), int(B), bool(cells)
        self.P = int(P) if self.cells else 0
        if self.N < 1 or self.B < 1 or (self.cells and (self.P < 64 or self.P % 64 or self.P > MAX_CELLS)):
            raise ValueError(f'{type(self).__name__}: need N >= 1, B >= 1 and, with cells, a map of a multiple of 64 cells up to {MAX_CELLS} '
                             f'(N {N}, B {B}, P {P})')
        self._layout = self.shapes(self.N, self.B, self.P, self.cells)
        self.raw = torch.empty(sum(self._words(dt, s) for _, dt, s in self._layout), dtype=torch.int32, device=device)

    @classmethod
    def shapes(cls, N, B, P, cells):
        """`layout` with the shapes as tuples, without the cell_ fields unless `cells`."""
        shape = dict(N=(N,), B=(B,), B2=(B, 2), BP=(B, P))
        return tuple((name, dt, shape[s]) for name, dt, s in cls.layout if cells or not name.startswith('cell_'))

    @staticmethod
    def _words(dt, shape):
        return int(np.prod(shape)) * int(dt[1]) // 4

    def _carve(self, raw, view):
        out, pos = dict.fromkeys(self.fields), 0
        for name, dt, shape in self._layout:
            n = self._words(dt, shape)
            out[name] = view(raw[pos:pos + n], dt, shape)
            pos += n
        return tuple(out[k] for k in self.fields)

    def tensors(self):
        """`fields` as views of the one buffer; the cell_ tensors are None without cells."""
        return self._carve(self.raw, lambda t, dt, shape: t.view(_KINDS[dt]).view(shape))

    def host(self):
        """One device->host copy -> `fields` as numpy arrays (`decode` / `decode_sums` take them)."""
        return self._carve(self.raw.cpu().numpy(), lambda a, dt, shape: a.view(dt).reshape(shape))


class CritBuffers(_Buffers):
    """The seven outputs of mmft_criticality: node_slack fp32, node_row, node_viol int32, node_crit fp32 [N]; counts int32
    [B, 2]; with cells cell_slack fp32 and cell_viol int32 [B, P]."""
    fields, count = FIELDS, 'seven'
    layout = (('node_slack', 'f4', 'N'), ('node_row', 'i4', 'N'), ('node_viol', 'i4', 'N'), ('node_crit', 'f4', 'N'), ('counts', 'i4', 'B2'),
              ('cell_slack', 'f4', 'BP'), ('cell_viol', 'i4', 'BP'))


def _vec(fn, t, name, dtype, n=None):
    if not torch.is_tensor(t):
        raise TypeError(f'{fn}: {name} must be a tensor')
    if t.dtype != dtype:
        raise TypeError(f'{fn}: {name} must be {dtype}, got {t.dtype}')
    if t.dim() != 1 or not t.is_contiguous():
        raise ValueError(f'{fn}: {name} must be a contiguous 1-D tensor, got shape {tuple(t.shape)} with strides {t.stride()}')
    if n is not None and t.numel() != n:
        raise ValueError(f'{fn}: {name} holds {t.numel()} entries, {n} expected')
    return t


# The host-side validation that criticality() and criticality_sums() share, in the order in which both run it: _rows, _sizes,
# _buffers.  criticality_sums() has a check of its own after each of the first two, and the order of the refusals is part of
# the contract, so the three stay three.
def _rows(fn, pred, required, paths, row_design):
    """dtype, shape and contiguity of the per-row vectors -> T."""
    _vec(fn, pred, 'pred', torch.float32)
    T = pred.numel()
    _vec(fn, required, 'required', torch.float32, T)
    _vec(fn, paths, 'paths', torch.int32, T)
    if row_design is not None:
        _vec(fn, row_design, 'row_design', torch.int32, T)
    return T


def _sizes(fn, T, placed, B, cells):
    """The limits of T, B and N -> (N, B, P, cells), P = 0 without cells."""
    B, cells = int(B), bool(cells)
    N = int(placed.loc_x.numel())
    P = int(placed.P) if cells else 0
    if T < 1 or T > 1 << 24 or B < 1 or N < 1:
        raise ValueError(f'{fn}: need 1 <= T <= 2^24, B >= 1, N >= 1 (T {T}, B {B}, N {N})')
    return N, B, P, cells


def _buffers(fn, cls, need_bytes, rows, placed, N, B, P, cells, out, workspace):
    """The map's size, `out` (allocated from `cls` when None) field by field, one device for everything, cuda only, the
    workspace (from lib.workspace when None) and its size -> ({field: tensor, the cell_ fields None without cells}, workspace).
    `rows` are the tensors _rows looked at."""
    if cells and (P % 64 or P > MAX_CELLS or P < 64):
        raise ValueError(f'{fn}: cells=True needs a map of a multiple of 64 cells, at most {MAX_CELLS}; it has {P}')
    pred = rows[0]
    if out is None:
        out = cls(N, B, P, pred.device, cells=cells).tensors()
    if len(out) != len(cls.fields):
        raise ValueError(f'{fn}: out must be the {cls.count} tensors of {cls.__name__}.tensors()')
    shapes = {name: (_KINDS[dt], shape) for name, dt, shape in cls.shapes(N, B, P, cells)}
    given = [(name, t) for name, t in zip(cls.fields, out) if name in shapes]
    for name, t in given:
        dt, shape = shapes[name]
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f'{fn}: {name} must be a contiguous {dt} tensor of shape {shape}')
    dev = placed.nodes.device
    every = [t for t in rows if t is not None] + [placed.lens, placed.loc_x, placed.loc_y] + [t for _, t in given]
    if any(t.device != dev for t in every):
        raise ValueError(f'{fn}: every tensor must live on the device of the placement tables ({dev})')
    if dev.type != 'cuda':
        raise RuntimeError(f'{fn}: the mmft hot path runs on the GPU only (got {dev} tensors); there is no CPU fallback')
    need = need_bytes(N, B, P)
    if workspace is None:
        workspace = lib.workspace(dev, need)
    elif not (torch.is_tensor(workspace) and workspace.device == dev and workspace.is_contiguous()):
        raise ValueError(f'{fn}: workspace must be a contiguous tensor on {dev}')
    if workspace.numel() * workspace.element_size() < need:
        raise ValueError(f'{fn}: workspace of {need} bytes needed, got {workspace.numel() * workspace.element_size()}')
    return {**dict.fromkeys(cls.fields), **dict(given)}, workspace


def criticality(pred, required, placed, paths, row_design, B, cells=True, out=None, workspace=None):
    """Launch mmft_criticality on the current stream -> (node_slack, node_row, node_viol, node_crit, cell_slack, cell_viol,
    counts) on the device (the two cell tensors None with cells=False); `decode` turns their host copies into per-design dicts.

    pred, required     fp32, contiguous 1-D, T rows each
    placed             placement.PlacedPaths: path nodes and lengths, the pins' current coordinates, the map
    paths              int32 [T]: the row of placed.nodes that each batch row predicts
    row_design         int32 [T], the design of each batch row in [0, B), or None: every row belongs to design 0
    B                  designs; pins are numbered as placed.nodes numbers them (N = placed.loc_x.numel())
    out, workspace     buffers the caller owns (CritBuffers.tensors(); a tensor of workspace_bytes bytes on the same device):
                       a captured launch needs static ones.  Without `workspace` the scratch comes from lib.workspace, which
                       never grows during a capture.

    Everything is validated on the host, dtypes, shapes and contiguity first, before anything is launched."""
    fn = 'criticality'
    T = _rows(fn, pred, required, paths, row_design)
    N, B, P, cells = _sizes(fn, T, placed, B, cells)
    o, workspace = _buffers(fn, CritBuffers, workspace_bytes, (pred, required, paths, row_design), placed, N, B, P, cells, out, workspace)
    lib.crit('mmft_criticality', pred, required, placed.nodes, placed.lens, placed.maxlen,
             placed.loc_x if cells else None, placed.loc_y if cells else None, placed.map_x if cells else 0, placed.map_y if cells else 0,
             paths, row_design, T, N, B, o['node_slack'], o['node_row'], o['node_viol'], o['node_crit'], o['cell_slack'], o['cell_viol'],
             o['counts'], workspace, workspace.numel() * workspace.element_size(), *lib.stream_args(pred))
    return tuple(o[k] for k in FIELDS)


def reference_criticality(pred, required, path_nodes, path_lens, pin_x, pin_y, map_x, map_y, paths, row_design, N, B,
                          cells=True, masks=None):
    """The contract of include/mmft_crit.h in plain numpy from host arrays -> the seven arrays in the layout of the device
    buffers (cell_slack / cell_viol None with cells=False).  The masks come from placement.rasterize_host - the mask rule
    lives there - or from `masks` = (indptr, cols) of the rows of path_nodes, rasterised by somebody else from the same pins."""
    nodes, lens = np.asarray(path_nodes).astype(np.int64), np.asarray(path_lens).astype(np.int64)
    paths = np.asarray(paths).astype(np.int64)
    T, maxlen = paths.shape[0], nodes.shape[1]
    design = np.zeros(T, dtype=np.int64) if row_design is None else np.asarray(row_design).astype(np.int64)
    slack = reference_slack(pred, required)
    P = int(map_x) * int(map_y) if cells else 0
    inf = np.float32(np.inf)
    node_slack, node_row = np.full(N, inf, dtype=np.float32), np.full(N, -1, dtype=np.int32)
    node_viol, node_crit = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.float32)
    cell_slack = np.full((B, P), inf, dtype=np.float32) if cells else None
    cell_viol = np.zeros((B, P), dtype=np.int32) if cells else None
    counts = np.zeros((B, 2), dtype=np.int32)
    worst = np.full(B, inf, dtype=np.float32)                      # per design, over every valid row
    if cells:
        indptr, cols = masks if masks is not None else rasterize_host(nodes, lens, pin_x, pin_y, map_x, map_y)
    for t in range(T):                                             # ascending rows: a strict `<` keeps the smaller row on a tie
        s, b, q = slack[t], int(design[t]), int(paths[t])
        if np.isnan(s):
            counts[b, 1] += 1
            continue
        counts[b, 0] += 1
        worst[b] = min(worst[b], s)
        for n in nodes[q, :min(int(lens[q]), maxlen)]:
            if node_row[n] < 0 or s < node_slack[n]:
                node_slack[n], node_row[n] = s, t
            if s < 0:
                node_viol[n] += 1
        if cells:
            c = np.asarray(cols[indptr[q]:indptr[q + 1]]).astype(np.int64)
            cell_slack[b, c] = np.minimum(cell_slack[b, c], s)
            if s < 0:
                cell_viol[b, c] += 1
    for n in np.flatnonzero((node_row >= 0) & (node_slack < 0)):
        w = worst[design[node_row[n]]]
        with np.errstate(invalid='ignore'):
            node_crit[n] = np.float32(1.0) if node_slack[n] == w else np.float32(node_slack[n]) / np.float32(w)
    return node_slack, node_row, node_viol, node_crit, cell_slack, cell_viol, counts


def decode(node_slack, node_row, node_viol, node_crit, cell_slack, cell_viol, counts, node_off, map_x=None, map_y=None):
    """Host copies of the seven buffers -> one dict per design: node_slack, node_row, node_viol, node_crit as arrays in the
    design's own node order (node_off [B + 1]: the designs' offsets in the numbering of the path nodes; node_row stays a row
    of the batch), cell_slack, cell_viol as [map_x, map_y] arrays or None, n (valid rows) and n_nan."""
    node_off, counts = np.asarray(node_off).astype(np.int64), np.asarray(counts)
    out = []
    for b in range(counts.shape[0]):
        lo, hi = int(node_off[b]), int(node_off[b + 1])
        d = dict(node_slack=np.asarray(node_slack)[lo:hi], node_row=np.asarray(node_row)[lo:hi], node_viol=np.asarray(node_viol)[lo:hi],
                 node_crit=np.asarray(node_crit)[lo:hi], cell_slack=None, cell_viol=None, n=int(counts[b, 0]), n_nan=int(counts[b, 1]))
        if cell_slack is not None:
            d['cell_slack'] = np.asarray(cell_slack)[b].reshape(int(map_x), int(map_y))
            d['cell_viol'] = np.asarray(cell_viol)[b].reshape(int(map_x), int(map_y))
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------ negative-slack sums and shares
# include/mmft_crit_sums.h (mmft_criticality_sums, bound by lib.csum): the seven outputs above, bitwise, and next to them how
# much negative slack flows through every pin and every cell.  A violating row contributes q = rint(min(-slack, 2^(32 - L)) *
# 2^L) quanta of 2^-L (L = scale_log2), an integer, so the sums are integer sums: exact, the same in every order.
MAX_ROW_PINS = 1 << 30                             # T * maxlen: every sum is then at most 2^62


def sums_workspace_bytes(N, B, P):
    """Bytes of the keyed words (the sums accumulate in their outputs); P = 0 without the cell outputs."""
    return lib.csum('mmft_criticality_sums_workspace_bytes', int(N), int(B), int(P))


class CritSumsBuffers(_Buffers):
    """The thirteen outputs of mmft_criticality_sums: the seven of CritBuffers, then node_nsum, cell_nsum, design_nsum,
    saturated, node_share, cell_share.  In the buffer the int64 fields come first - node_nsum [N], design_nsum [B], with cells
    cell_nsum [B, P] - so that they are 8-byte aligned; then the fields of CritBuffers, saturated int32 [B], node_share fp32
    [N] and, with cells, cell_share fp32 [B, P]."""
    fields, count = FIELDS + SUM_FIELDS, 'thirteen'
    layout = (('node_nsum', 'i8', 'N'), ('design_nsum', 'i8', 'B'), ('cell_nsum', 'i8', 'BP'),
              ('node_slack', 'f4', 'N'), ('node_row', 'i4', 'N'), ('node_viol', 'i4', 'N'), ('node_crit', 'f4', 'N'), ('counts', 'i4', 'B2'),
              ('saturated', 'i4', 'B'), ('node_share', 'f4', 'N'), ('cell_slack', 'f4', 'BP'), ('cell_viol', 'i4', 'BP'), ('cell_share', 'f4', 'BP'))


def criticality_sums(pred, required, placed, paths, row_design, B, scale_log2=20, cells=True, out=None, workspace=None):
    """Launch mmft_criticality_sums on the current stream -> the seven tensors of `criticality` (bitwise the same) followed by
    node_nsum, cell_nsum, design_nsum, saturated, node_share, cell_share on the device (the four cell tensors None with
    cells=False); `decode_sums` turns their host copies into per-design dicts.

    The arguments are those of `criticality`; scale_log2 in [0, 30] is the binary logarithm of the quanta per unit of slack,
    T * maxlen may be at most 2^30, `out` is CritSumsBuffers.tensors() and `workspace` holds sums_workspace_bytes bytes.

    Everything is validated on the host, dtypes, shapes and contiguity first, before anything is launched."""
    fn = 'criticality_sums'
    T = _rows(fn, pred, required, paths, row_design)
    if isinstance(scale_log2, bool) or not isinstance(scale_log2, (int, np.integer)) or not 0 <= scale_log2 <= 30:
        raise ValueError(f'{fn}: scale_log2 must be an integer in [0, 30], got {scale_log2!r}')
    N, B, P, cells = _sizes(fn, T, placed, B, cells)
    if T * int(placed.maxlen) > MAX_ROW_PINS:
        raise ValueError(f'{fn}: T * maxlen must be at most 2^30 for the sums to fit int64 (T {T}, maxlen {placed.maxlen})')
    o, workspace = _buffers(fn, CritSumsBuffers, sums_workspace_bytes, (pred, required, paths, row_design), placed, N, B, P, cells, out,
                            workspace)
    lib.csum('mmft_criticality_sums', pred, required, placed.nodes, placed.lens, placed.maxlen,
             placed.loc_x if cells else None, placed.loc_y if cells else None, placed.map_x if cells else 0, placed.map_y if cells else 0,
             paths, row_design, T, N, B, o['node_slack'], o['node_row'], o['node_viol'], o['node_crit'], o['cell_slack'], o['cell_viol'],
             o['counts'], int(scale_log2), o['node_nsum'], o['cell_nsum'], o['design_nsum'], o['saturated'], o['node_share'], o['cell_share'],
             workspace, workspace.numel() * workspace.element_size(), *lib.stream_args(pred))
    return tuple(o[k] for k in FIELDS + SUM_FIELDS)


def reference_quanta(slack, scale_log2):
    """(q int64 [T], saturated bool [T]) of fp32 slacks: q = rint(min(-slack, 2^(32 - scale_log2)) * 2^scale_log2) for a row
    that violates (slack < 0, -inf included), 0 for every other row, NaN rows among them.  In fp64, where the scaling of an
    fp32 value by a power of two is exact; np.rint rounds to nearest, ties to even."""
    s = np.asarray(slack, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid='ignore'):
        viol = s < 0
    cap = 2.0 ** (32 - int(scale_log2))
    m = np.where(viol, -s, 0.0)
    return np.rint(np.minimum(m, cap) * 2.0 ** int(scale_log2)).astype(np.int64), viol & (m >= cap)


def reference_share(nsum, total):
    """fp32 shares of int64 sums: 0 where total == 0, else float32(float64(nsum) / float64(total)), every step rounded to nearest."""
    nsum, total = np.asarray(nsum, dtype=np.int64), np.asarray(total, dtype=np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(total == 0, np.float64(0), nsum.astype(np.float64) / total.astype(np.float64)).astype(np.float32)


def reference_criticality_sums(pred, required, path_nodes, path_lens, pin_x, pin_y, map_x, map_y, paths, row_design, N, B,
                               scale_log2=20, cells=True, masks=None):
    """The contract of include/mmft_crit_sums.h in plain numpy from host arrays -> the thirteen arrays in the layout of the
    device buffers: the seven of `reference_criticality`, then node_nsum, cell_nsum, design_nsum, saturated, node_share,
    cell_share (the four cell arrays None with cells=False).  `masks` as in `reference_criticality`."""
    nodes, lens = np.asarray(path_nodes).astype(np.int64), np.asarray(path_lens).astype(np.int64)
    paths = np.asarray(paths).astype(np.int64)
    T, maxlen = paths.shape[0], nodes.shape[1]
    if cells and masks is None:
        masks = rasterize_host(nodes, lens, pin_x, pin_y, map_x, map_y)
    old = reference_criticality(pred, required, nodes, lens, pin_x, pin_y, map_x, map_y, paths, row_design, N, B, cells=cells, masks=masks)
    design = np.zeros(T, dtype=np.int64) if row_design is None else np.asarray(row_design).astype(np.int64)
    slack = reference_slack(pred, required)
    q, sat = reference_quanta(slack, scale_log2)
    P = int(map_x) * int(map_y) if cells else 0
    node_nsum, design_nsum = np.zeros(N, dtype=np.int64), np.zeros(B, dtype=np.int64)
    cell_nsum = np.zeros((B, P), dtype=np.int64) if cells else None
    saturated = np.zeros(B, dtype=np.int32)
    with np.errstate(invalid='ignore'):
        violating = np.flatnonzero(slack < 0)                      # the violating valid rows (a NaN is not below zero)
    for t in violating:
        b, p = int(design[t]), int(paths[t])
        design_nsum[b] += q[t]                                     # every such row, whatever its path holds
        saturated[b] += sat[t]
        np.add.at(node_nsum, nodes[p, :min(int(lens[p]), maxlen)], q[t])        # once per live position
        if cells:
            c = np.asarray(masks[1][masks[0][p]:masks[0][p + 1]]).astype(np.int64)
            cell_nsum[b, c] += q[t]                                # a mask is a set: once per row
    node_row = old[1]
    total = np.where(node_row >= 0, design_nsum[design[np.maximum(node_row, 0)]], 0)
    node_share = reference_share(node_nsum, total)
    cell_share = reference_share(cell_nsum, design_nsum[:, None]) if cells else None
    return tuple(old) + (node_nsum, cell_nsum, design_nsum, saturated, node_share, cell_share)


def decode_sums(node_slack, node_row, node_viol, node_crit, cell_slack, cell_viol, counts, node_nsum, cell_nsum, design_nsum,
                saturated, node_share, cell_share, node_off, scale_log2, map_x=None, map_y=None):
    """Host copies of the thirteen buffers -> one dict per design: what `decode` gives, and node_tns (fp64, the design's own
    node order) and cell_tns (fp64 [map_x, map_y] or None) = -nsum / 2^scale_log2, so <= 0 like the report's tns; tns, the
    design's own; node_share, cell_share (fp32) and saturated, the number of rows that hit the cap."""
    out = decode(node_slack, node_row, node_viol, node_crit, cell_slack, cell_viol, counts, node_off, map_x=map_x, map_y=map_y)
    node_off, unit = np.asarray(node_off).astype(np.int64), 2.0 ** int(scale_log2)
    for b, d in enumerate(out):
        lo, hi = int(node_off[b]), int(node_off[b + 1])
        d['node_tns'] = 0.0 - np.asarray(node_nsum)[lo:hi].astype(np.float64) / unit
        d['node_share'] = np.asarray(node_share)[lo:hi]
        d['cell_tns'] = d['cell_share'] = None
        if cell_nsum is not None:
            d['cell_tns'] = 0.0 - np.asarray(cell_nsum)[b].astype(np.float64).reshape(int(map_x), int(map_y)) / unit
            d['cell_share'] = np.asarray(cell_share)[b].reshape(int(map_x), int(map_y))
        d['tns'] = 0.0 - float(np.asarray(design_nsum)[b]) / unit
        d['saturated'] = int(np.asarray(saturated)[b])
    return out


# ------------------------------------------------------------------------------------------------ the Predictor's side
class PredictorCriticality(AfterHead):
    """Predictor(criticality=True or dict(cells=..., sums=..., scale_log2=...)): the criticality launches on every predict()'s
    output.  Holds the placement tables (those of placement=True, which follow update(); or tables of its own, whose pins never
    move), the rows' slack inputs (predictor.slack), static output buffers and the keyed-word workspace - static addresses, kept
    alive with the replay.  Plain or sums is decided ONCE, here: the buffer class, the workspace size, the launch and the decoder."""

    @staticmethod
    def spec(spec):
        """criticality= as a dict, or None when the option is off; refuses anything else - host only, before a device is touched."""
        if spec is None or spec is False:
            return None
        spec = {} if spec is True else spec
        if not isinstance(spec, dict):
            raise ValueError(f'Predictor: criticality= takes None, True or dict(cells=...), got {spec!r}')
        unknown = set(spec) - {'cells', 'sums', 'scale_log2'}
        if unknown:
            raise ValueError(f'Predictor: criticality= takes cells, sums and scale_log2, got {sorted(unknown)}')
        if 'scale_log2' in spec:
            L = spec['scale_log2']
            if not spec.get('sums'):
                raise ValueError(f'Predictor: criticality= takes scale_log2 only with sums=True, got {spec!r}')
            if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or not 0 <= L <= 30:
                raise ValueError(f'Predictor: criticality= takes an integer scale_log2 in [0, 30], got {L!r}')
        return spec

    def __init__(self, predictor, spec):
        b, dev = predictor.batch, predictor.device
        self.cells, self.sums, self.scale_log2 = bool(spec.get('cells', True)), bool(spec.get('sums', False)), int(spec.get('scale_log2', 20))
        s = self.slack = predictor.slack
        s.require_regression(predictor.pmodel, 'Predictor: criticality=')
        if self.cells and (b.P % 64 or b.P > MAX_CELLS):
            raise ValueError(f'Predictor: criticality=dict(cells=True) needs a map of a multiple of 64 cells, at most {MAX_CELLS}; '
                             f'it has {b.P}')
        # tables of its own feed no projection: the paths' nodes are all it reads, so neither the run form nor masks that
        # match the stored ones are asked for
        self.placed = predictor._placed if predictor._placed is not None else \
            batch_tables(b.designs, b, dev, 'Predictor(criticality=)', projection=False)
        if self.sums and s.T * int(self.placed.maxlen) > MAX_ROW_PINS:
            raise ValueError(f'Predictor: criticality=dict(sums=True) needs rows * maxlen <= 2^30 for the sums to fit int64; '
                             f'it has {s.T} * {self.placed.maxlen}')
        if self.sums:                                            # one launch group: the sums' kernels write the other outputs too
            buffers, need = CritSumsBuffers, sums_workspace_bytes
            self._launch = functools.partial(criticality_sums, scale_log2=self.scale_log2)
            self._decode = functools.partial(decode_sums, scale_log2=self.scale_log2)
        else:
            buffers, need, self._launch, self._decode = CritBuffers, workspace_bytes, criticality, decode
        N = int(b.node_off[-1])
        self.required, self.row_design, self.paths, self.node_off = s.required, s.row_design, predictor._sel.paths, b.node_off
        self.bufs = buffers(N, s.B, self.placed.P, dev, cells=self.cells)
        self.scratch = torch.empty((need(N, s.B, self.placed.P if self.cells else 0) + 7) // 8, dtype=torch.int64, device=dev)

    def launch(self, pred):
        self._launch(pred.contiguous().reshape(-1), self.required, self.placed, self.paths, self.row_design, self.slack.B, cells=self.cells,
                     out=self.bufs.tensors(), workspace=self.scratch)
        self.ready = True

    def result(self, i=None):
        out = self._decode(*self.bufs.host(), node_off=self.node_off, map_x=self.placed.map_x, map_y=self.placed.map_y)
        return out if i is None else out[i]
