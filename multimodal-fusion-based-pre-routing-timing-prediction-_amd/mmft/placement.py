"""Path masks that follow a moving placement (include/mmft_place.h).

A path mask is the union of the drive -> sink bounding boxes along a path, in map cells
(src/verilog_parser_asap7.py:1302-1369): a pure function of the path's nodes and the pins' coordinates.  A design may carry
that placement data - `path_nodes` [num_paths, maxlen] (-1 padded, the layout prep.trace_critical_paths emits), `path_lens`
[num_paths], `pin_x` / `pin_y` [N] map-cell coordinates - next to its rasterised `mask_indptr` / `mask_cols`:

    rasterize_host / runs_host   the mask rule and its run form in numpy (host side: attach_placement, tests, tools)
    attach_placement             validates the four arrays, sets them on a design and rebuilds its masks from them
    PlacedPaths                  the device tables of a batch of such designs; set_pins() moves a design's pins in place
    batch_tables                 the PlacedPaths of a resident batch, with the refusals every front end makes before it uses them
    placed_fc                    the masked projection computed from those tables by mmft_placed_fc_fwd: bitwise what
                                 fusion.masked_fc gives on masks rasterised from the same pins, with nothing to rebuild
"""
import numpy as np
import torch

from . import fusion, lib

FIELDS = ('path_nodes', 'path_lens', 'pin_x', 'pin_y')
MAX_CELLS = 65536          # the kernel's LDS bitmap (mmft_place.h)


def has_placement(design):
    return all(getattr(design, k, None) is not None for k in FIELDS)


def require_placement(designs, who):
    """ValueError, prefixed with `who`, for the first design that carries no placement data.  Host only."""
    for i, d in enumerate(designs):
        if not has_placement(d):
            raise ValueError(f'{who}: design {i} carries no placement data ({", ".join(FIELDS)}: placement.attach_placement)')


def _bitmaps(path_nodes, path_lens, pin_x, pin_y, map_x, map_y):
    """Per path the bool [map_x, map_y] union of its boxes: the mask rule of include/mmft_place.h."""
    nodes, lens = np.asarray(path_nodes), np.asarray(path_lens)
    px, py = np.asarray(pin_x).astype(np.int64), np.asarray(pin_y).astype(np.int64)
    if nodes.ndim != 2 or lens.shape != (nodes.shape[0],) or px.shape != py.shape or px.ndim != 1:
        raise ValueError('path_nodes [num_paths, maxlen], path_lens [num_paths] and pin_x / pin_y [N] expected')
    maxlen = nodes.shape[1]
    for q in range(nodes.shape[0]):
        bm = np.zeros((map_x, map_y), dtype=bool)
        n = min(int(lens[q]), maxlen)
        for j in range(n - 1):
            a, b = int(nodes[q, j]), int(nodes[q, j + 1])
            x1, x2 = max(min(px[a], px[b]), 0), min(max(px[a], px[b]), map_x - 1)
            y1, y2 = max(min(py[a], py[b]), 0), min(max(py[a], py[b]), map_y - 1)
            if x1 <= x2 and y1 <= y2:
                bm[x1:x2 + 1, y1:y2 + 1] = True
        yield bm


def rasterize_host(path_nodes, path_lens, pin_x, pin_y, map_x, map_y):
    """(indptr int64 [num_paths + 1], cols int64 [nnz], ascending per row) of the path masks; column = x * map_y + y."""
    indptr, cols = [0], []
    for bm in _bitmaps(path_nodes, path_lens, pin_x, pin_y, int(map_x), int(map_y)):
        c = np.flatnonzero(bm.reshape(-1))
        cols.append(c)
        indptr.append(indptr[-1] + c.shape[0])
    return np.asarray(indptr, dtype=np.int64), (np.concatenate(cols) if cols else np.zeros(0)).astype(np.int64)


def runs_host(path_nodes, path_lens, pin_x, pin_y, map_x, map_y):
    """(run_ptr [num_paths + 1], run_start [R], run_len [R]) int64 with S = fusion.RUN_BLOCK: per path the groups of
    consecutive ones of each S-bit block of its bitmap, ascending - the runs the kernel numbers, and those
    fusion._runs_from_csr derives from the CSR."""
    S, P = fusion.RUN_BLOCK, int(map_x) * int(map_y)
    if not S or P % S:
        raise ValueError(f'runs_host: the map holds {P} cells, no multiple of the prefix block of {S}')
    ptr, starts, lens = [0], [], []
    for bm in _bitmaps(path_nodes, path_lens, pin_x, pin_y, int(map_x), int(map_y)):
        v = bm.reshape(P // S, S)
        prev = np.zeros_like(v); prev[:, 1:] = v[:, :-1]          # v << 1: the cell below, inside the block
        nxt = np.zeros_like(v); nxt[:, :-1] = v[:, 1:]
        s, e = np.flatnonzero((v & ~prev).reshape(-1)), np.flatnonzero((v & ~nxt).reshape(-1))
        starts.append(s)
        lens.append(e - s + 1)
        ptr.append(ptr[-1] + s.shape[0])
    cat = lambda xs: (np.concatenate(xs) if xs else np.zeros(0)).astype(np.int64)
    return np.asarray(ptr, dtype=np.int64), cat(starts), cat(lens)


def _int_array(x, name, ndim):
    a = np.asarray(x)
    if a.dtype.kind not in 'iu' or a.ndim != ndim:
        raise ValueError(f'attach_placement: {name} must be an integer array with {ndim} dimension(s), got {a.dtype} {a.shape}')
    a = a.astype(np.int64)
    if a.size and (a.max() >= 2 ** 31 or a.min() < -2 ** 31):
        raise ValueError(f'attach_placement: {name} does not fit 32-bit integers')
    return a


def attach_placement(design, path_nodes, path_lens, pin_x, pin_y):
    """Give `design` its placement data and rebuild `mask_indptr` / `mask_cols` from it (rasterize_host), so that the
    design is self-consistent.  path_nodes holds the design's own node ids, in [0, N) for j < min(len, maxlen) and -1
    elsewhere; a length above maxlen marks a truncated row (prep.trace_critical_paths) and is clipped.  Coordinates may
    be any 32-bit int: boxes are clamped to the map.  Nothing is set unless everything is valid.  Returns the design."""
    nodes, lens = _int_array(path_nodes, 'path_nodes', 2), _int_array(path_lens, 'path_lens', 1)
    px, py = _int_array(pin_x, 'pin_x', 1), _int_array(pin_y, 'pin_y', 1)
    num_paths, N = int(design.num_paths), int(design.N)
    if nodes.shape[0] != num_paths or nodes.shape[1] < 1 or lens.shape != (num_paths,):
        raise ValueError(f'attach_placement: the design has {num_paths} paths, path_nodes is {nodes.shape} and path_lens {lens.shape}')
    if px.shape != (N,) or py.shape != (N,):
        raise ValueError(f'attach_placement: the design has {N} nodes, pin_x is {px.shape} and pin_y {py.shape}')
    if lens.size and lens.min() < 0:
        raise ValueError('attach_placement: negative path length')
    live = np.arange(nodes.shape[1])[None, :] < np.minimum(lens, nodes.shape[1])[:, None]
    if (live & ((nodes < 0) | (nodes >= N))).any():
        raise ValueError(f'attach_placement: a path node id outside [0, {N})')
    if (~live & (nodes != -1)).any():
        raise ValueError('attach_placement: entries beyond a path\'s length must be -1')
    m = int(design.map_size)
    indptr, cols = rasterize_host(nodes, lens, px, py, m, m)
    design.path_nodes, design.path_lens, design.pin_x, design.pin_y = nodes, lens, px, py
    design.mask_indptr, design.mask_cols = indptr, cols
    return design


def _pins(x, name, n):
    """Tensor (host or device) of one design's coordinates, or an error; nothing is copied to a device here.  The tables
    hold 32-bit coordinates, as attach_placement requires: int64 values are range-checked (a device tensor is read back for
    that, which synchronises - pass int32 to avoid it)."""
    t = torch.from_numpy(x) if isinstance(x, np.ndarray) else x
    if not torch.is_tensor(t):
        raise TypeError(f'{name} must be a numpy array or a tensor')
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f'{name} must be int32 or int64, got {t.dtype}')
    if tuple(t.shape) != (n,):
        raise ValueError(f'{name} has shape {tuple(t.shape)}, the design has {n} pins')
    if t.dtype == torch.int64 and n and (int(t.max()) >= 2 ** 31 or int(t.min()) < -2 ** 31):
        raise ValueError(f'{name} does not fit 32-bit integers')
    return t


class PlacedPaths:
    """Device tables of a batch of designs that carry placement data, at static addresses.

    nodes [total paths, maxlen] int32   path nodes, shifted by the design's offset in `node_off` (the caller's numbering:
                                        the location tables are their own and do not follow DesignBatch's renumbering),
                                        -1 padded to the largest maxlen of the designs
    lens [total paths], loc_x / loc_y [total nodes] int32
    Rows follow the designs' paths one after another, as PathMasks.batch numbers them."""

    def __init__(self, designs, node_off, device):
        require_placement(designs, 'PlacedPaths')
        self.node_off = np.asarray(node_off, dtype=np.int64)
        if self.node_off.shape != (len(designs) + 1,) or any(int(self.node_off[i + 1] - self.node_off[i]) != int(d.N) for i, d in enumerate(designs)):
            raise ValueError('PlacedPaths: node_off must hold the designs\' node offsets')
        sizes = {int(d.map_size) for d in designs}
        if len(sizes) != 1:
            raise ValueError(f'PlacedPaths: one map size expected, got {sorted(sizes)}')
        self.map_x = self.map_y = sizes.pop()
        self.P = self.map_x * self.map_y
        self.B = len(designs)
        self.maxlen = max(int(np.asarray(d.path_nodes).shape[1]) for d in designs)
        self.path_off = np.concatenate([[0], np.cumsum([d.num_paths for d in designs])]).astype(np.int64)
        nodes = np.full((int(self.path_off[-1]), self.maxlen), -1, dtype=np.int64)
        lens = np.zeros(int(self.path_off[-1]), dtype=np.int64)
        for i, d in enumerate(designs):
            pn, pl = np.asarray(d.path_nodes, dtype=np.int64), np.asarray(d.path_lens, dtype=np.int64)
            if pn.ndim != 2 or pn.shape[0] != d.num_paths or pl.shape != (d.num_paths,) or \
                    np.asarray(d.pin_x).shape != (d.N,) or np.asarray(d.pin_y).shape != (d.N,):
                raise ValueError(f'PlacedPaths: design {i}: placement data does not fit the design')
            # a length above the design's own maxlen marks a truncated row: clipped HERE, to the design's row width - the
            # device clips to the batch's common maxlen only, and would read the -1 padding of a narrower design as nodes
            pl = np.minimum(pl, pn.shape[1])
            live = np.arange(pn.shape[1])[None, :] < pl[:, None]
            if (pl < 0).any() or (live & ((pn < 0) | (pn >= d.N))).any():
                raise ValueError(f'PlacedPaths: design {i}: a path node id outside [0, {d.N}) inside its row\'s length')
            nodes[self.path_off[i]:self.path_off[i + 1], :pn.shape[1]] = np.where(live, pn + self.node_off[i], -1)
            lens[self.path_off[i]:self.path_off[i + 1]] = pl
        self.device = torch.device(device)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64).astype(np.int32)).to(self.device)
        self.nodes = i32(nodes)
        self.lens = i32(lens)
        self.loc_x = i32(np.concatenate([np.asarray(d.pin_x) for d in designs]))
        self.loc_y = i32(np.concatenate([np.asarray(d.pin_y) for d in designs]))

    def check_pins(self, i, pin_x, pin_y):
        """(x, y) as validated tensors for set_pins; raises without writing anything."""
        if not 0 <= i < self.B:
            raise IndexError(f'design {i} of {self.B}')
        n = int(self.node_off[i + 1] - self.node_off[i])
        return _pins(pin_x, 'pin_x', n), _pins(pin_y, 'pin_y', n)

    def set_pins(self, i, pin_x, pin_y):
        """New map-cell coordinates of design i's pins (int32 / int64 [N_i], numpy or tensor), copied into the design's
        slice of loc_x / loc_y on the current stream: addresses stay.  Validated before anything is written."""
        x, y = self.check_pins(i, pin_x, pin_y)
        a, b = int(self.node_off[i]), int(self.node_off[i + 1])
        self.loc_x[a:b].copy_(x.to(torch.int32), non_blocking=True)
        self.loc_y[a:b].copy_(y.to(torch.int32), non_blocking=True)

    def csr(self):
        """(indptr int32 [paths + 1], cols int32 [nnz]) on the device: the masks of the pins as they are now, rasterised by
        prep.rasterize_path_masks (inspection, saving; synchronises)."""
        from . import prep
        return prep.rasterize_path_masks(self.nodes, self.lens, self.loc_x, self.loc_y, self.map_x, self.map_y)


def batch_tables(designs, batch, device, who, projection=True):
    """The PlacedPaths of a resident batch (train.DesignBatch), or a ValueError prefixed with `who`: a design without
    placement data; and, with projection=True - the tables then stand in for the stored masks in the masked projection
    (placed_fc) - a map the run form does not take, and stored masks that are not the masks of the pins (the results would
    change before a pin has moved).  projection=False: for a caller that walks the paths' nodes only (criticality)."""
    require_placement(designs, who)
    if projection and (not batch.masks.run_block or batch.P > MAX_CELLS):
        raise ValueError(f'{who} needs a map of a multiple of 64 cells, at most {MAX_CELLS}; it has {batch.P}')
    placed = PlacedPaths(designs, batch.node_off, device)
    if projection:
        ip, cols = (t.cpu().numpy().astype(np.int64) for t in placed.csr())
        m = batch.masks
        for i in range(batch.B):
            q0, q1 = int(batch.path_off[i]), int(batch.path_off[i + 1])
            if not (np.array_equal(ip[q0:q1 + 1], m.host_indptr[q0:q1 + 1]) and
                    np.array_equal(cols[ip[q0]:ip[q1]], m.host_cols[ip[q0]:ip[q1]])):
                raise ValueError(f'{who}: the stored masks of design {i} are not the masks of its pins '
                                 '(placement.attach_placement rebuilds them)')
    return placed


def placed_fc(placed, paths, f_off, feat_map, w, b, masks, stats=None, keep=None):
    """fcn(mask rows * feat_map) with the mask of every batch row taken from `placed`'s current pins.

    paths int32 [T] (rows of placed.nodes), f_off int32 [T] or None (one design), feat_map [B, P], w [Dout, P], b [Dout] or
    None; `masks` is the batch's PathMasks and only says how the prefix table is laid out (B, P, run_block): the table comes
    from fusion.masked_fc_prefix - same cache, same launches as fusion.masked_fc.  stats: optional int32 [T, 2], filled with
    (cells, runs) of each row's mask.  keep: a dict that receives the prefix table this call projected through as keep['GP']
    (mmft.trial projects trial rows through the same table); absent, nothing else happens.  Forward only."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (feat_map, w, b)):
        raise RuntimeError('placed_fc is forward only: call it under torch.no_grad() (moving masks have no backward)')
    if masks.P != placed.P or masks.B != placed.B:
        raise ValueError(f'placed_fc: masks are {masks.B} x {masks.P}, the placement tables {placed.B} x {placed.P}')
    if w.dim() != 2 or w.shape[1] != masks.P or w.shape[0] % 4:
        raise ValueError(f'placed_fc: fcn weight {tuple(w.shape)} does not fit {masks.P} map cells / a multiple of 4 outputs')
    if placed.P > MAX_CELLS:
        raise ValueError(f'placed_fc: maps above {MAX_CELLS} cells are not supported')
    if paths.dtype != torch.int32 or not paths.is_contiguous() or paths.device != placed.nodes.device or \
            (f_off is not None and (f_off.dtype != torch.int32 or not f_off.is_contiguous() or f_off.numel() != paths.numel())):
        raise ValueError('placed_fc: paths / f_off must be contiguous int32 tensors of one length on the tables\' device')
    GP = fusion.masked_fc_prefix(feat_map, w, masks)
    if GP is None:
        raise ValueError('placed_fc: the masks have no run form (the map must hold a multiple of fusion.RUN_BLOCK cells, '
                         'fusion.USE_RUNS on, contiguous feat_map and weight)')
    if keep is not None:
        keep['GP'] = GP
    T, Dout = paths.numel(), w.shape[0]
    if stats is not None and (stats.dtype != torch.int32 or tuple(stats.shape) != (T, 2) or not stats.is_contiguous()):
        raise ValueError('placed_fc: stats must be a contiguous int32 [T, 2] tensor')
    out = torch.empty((T, Dout), dtype=torch.float32, device=GP.device)
    lib.place('mmft_placed_fc_fwd', placed.nodes, placed.lens, placed.maxlen, placed.loc_x, placed.loc_y, placed.map_x,
              placed.map_y, paths, f_off, T, GP, b, out, Dout, Dout, masks.run_block, stats, *lib.stream_args(GP))
    return out


# ------------------------------------------------------------------------------------------------ one-cell moves of a pin
def pin_incidence_host(path_nodes, path_lens, paths, n_nodes):
    """(inc_ptr int64 [n_nodes + 1], inc_slot int64 [nnz]): per pin the slots t * maxlen + j of the batch rows t (path paths[t])
    and live positions j < min(len, maxlen) at which the pin occurs FIRST in its row, ascending - the incidence CSR of
    include/mmft_sens_pins.h.  The selection and the paths' nodes are static: built once, whatever the pins do."""
    nodes, lens = np.asarray(path_nodes, dtype=np.int64), np.asarray(path_lens, dtype=np.int64)
    paths = np.asarray(paths, dtype=np.int64).reshape(-1)
    maxlen = nodes.shape[1]
    R = nodes[paths].reshape(paths.shape[0], maxlen)
    live = np.arange(maxlen)[None, :] < np.minimum(lens[paths], maxlen)[:, None]
    if (live & ((R < 0) | (R >= n_nodes))).any():
        raise ValueError(f'pin_incidence: a path node id outside [0, {n_nodes}) inside its row\'s length')
    # a later occurrence follows its equal in a stable sort of the row (entries beyond the length sit behind the live ones)
    order = np.argsort(R, axis=1, kind='stable')
    Rs = np.take_along_axis(R, order, 1)
    again = np.zeros(R.shape, dtype=bool)
    again[:, 1:] = Rs[:, 1:] == Rs[:, :-1]
    dup = np.zeros(R.shape, dtype=bool)
    np.put_along_axis(dup, order, again, 1)
    t, j = np.nonzero(live & ~dup)                                      # ascending (t, j)
    pins, slots = R[t, j], t * maxlen + j
    by_pin = np.argsort(pins, kind='stable')
    ptr = np.zeros(n_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(pins, minlength=n_nodes), out=ptr[1:])
    return ptr, slots[by_pin].astype(np.int64)


def pin_incidence(placed, paths):
    """The incidence CSR of a selection `paths` (rows of placed.nodes; host array or tensor) over `placed`'s pins as int32
    device tensors (inc_ptr [N + 1], inc_slot [nnz]) for ops.pin_move_sum.  One device -> host copy of the node table."""
    p = paths.detach().cpu().numpy() if torch.is_tensor(paths) else np.asarray(paths)
    if p.ndim != 1 or p.dtype.kind not in 'iu' or (p.size and (p.min() < 0 or p.max() >= placed.nodes.shape[0])):
        raise ValueError(f'pin_incidence: paths must be a 1-D integer array of rows of the {placed.nodes.shape[0]} placed paths')
    if p.size * placed.maxlen >= 2 ** 29:
        raise ValueError(f'pin_incidence: rows * maxlen must stay below 2^29, got {p.size} * {placed.maxlen}')
    ptr, slot = pin_incidence_host(placed.nodes.cpu().numpy(), placed.lens.cpu().numpy(), p, int(placed.loc_x.numel()))
    i32 = lambda a: torch.from_numpy(a.astype(np.int32)).to(placed.device)
    return i32(ptr), i32(slot)


def _axis_range(u, v, lim):
    """[lo, hi] of the mask rule along one axis of `lim` cells for pins at u and v (arrays); empty where lo > hi."""
    return np.maximum(np.minimum(u, v), 0), np.minimum(np.maximum(u, v), lim - 1)


def _holds(boxes, v, pf):
    """[len(pf)] bool: is the cell (v, pf[i]) - moving axis, fixed axis - inside one of `boxes` [n, 4] = (lo, hi, f1, f2)?"""
    on_line = (boxes[:, 0] <= v) & (v <= boxes[:, 1])
    b = boxes[on_line]
    return ((b[None, :, 2] <= pf[:, None]) & (pf[:, None] <= b[None, :, 3])).any(1)


def pin_move_host(path_nodes, path_lens, pin_x, pin_y, map_x, map_y, paths, f_off, feat, w, g):
    """(row_move fp64 [T, maxlen, 4], pin_move fp64 [N, 4]) of include/mmft_sens_pins.h on the host: per batch row t (path
    paths[t], feature-map offset f_off[t], or 0 without f_off) and first-occurrence position the change of g[t] . h_cnn[t] when
    that pin alone moves one map cell - directions x + 1, x - 1, y + 1, y - 1 - and the sums per pin.  feat [B * P], w = fcn.weight
    [Dout, P], g [T, Dout].

    EXACT IN THE MASK: the cells are the set differences of the masks under the rule of include/mmft_place.h, the pin displaced
    at all of its occurrences in the row before clamping.  LINEAR IN THE HEAD: the change of h_cnn is contracted with g - a
    first-order estimate of the change of J, not a prediction of the moved design (that is update() followed by predict()).

    Written in the segment form of the kernel, as rasterize_host restates the masks: the boxes next to an occurrence of the pin
    each gain and lose at most two lines; a cell of such a line counts once, at the first box that proposes it, unless
    another box of the row holds it."""
    nodes, lens = np.asarray(path_nodes, dtype=np.int64), np.asarray(path_lens, dtype=np.int64)
    px, py = np.asarray(pin_x).astype(np.int64), np.asarray(pin_y).astype(np.int64)
    paths = np.asarray(paths, dtype=np.int64).reshape(-1)
    map_x, map_y = int(map_x), int(map_y)
    P, T, maxlen = map_x * map_y, paths.shape[0], nodes.shape[1]
    feat = np.asarray(feat, dtype=np.float64).reshape(-1)
    w, g = np.asarray(w, dtype=np.float64), np.asarray(g, dtype=np.float64)
    if w.ndim != 2 or w.shape[1] != P or g.shape != (T, w.shape[0]) or feat.size % P:
        raise ValueError(f'pin_move_host: feat [B * {P}], w [Dout, {P}] and g [{T}, Dout] expected')
    off = np.zeros(T, dtype=np.int64) if f_off is None else np.asarray(f_off, dtype=np.int64).reshape(-1)
    row_move = np.zeros((T, maxlen, 4), dtype=np.float64)
    pin_move = np.zeros((px.shape[0], 4), dtype=np.float64)
    for t in range(T):
        q = int(paths[t])
        ids = nodes[q, :max(min(int(lens[q]), maxlen), 0)]
        if ids.shape[0] == 0:
            continue
        score = feat[off[t]:off[t] + P] * (g[t] @ w)                   # s_t(c) for every cell of the map
        x, y = px[ids], py[ids]
        seen = set()
        for j, n in enumerate(ids.tolist()):
            if n in seen:
                continue
            seen.add(n)
            at = ids == n
            touched = np.flatnonzero(at[:-1] | at[1:])                 # the boxes next to an occurrence, ascending
            for d in range(4):
                cm, cf, lim_m, lim_f = (x, y, map_x, map_y) if d < 2 else (y, x, map_y, map_x)
                mv = cm + np.where(at, -1 if d & 1 else 1, 0)          # displaced before the rule clamps (int64: no overflow)
                now = np.stack(_axis_range(cm[:-1], cm[1:], lim_m) + _axis_range(cf[:-1], cf[1:], lim_f), 1)
                then = now.copy()
                then[:, 0], then[:, 1] = _axis_range(mv[:-1], mv[1:], lim_m)
                live = now[:, 2] <= now[:, 3]                          # an empty fixed-axis range: no box before or after
                now_boxes, then_boxes = now[live & (now[:, 0] <= now[:, 1])], then[live & (then[:, 0] <= then[:, 1])]
                total = 0.0
                for k in touched.tolist():
                    a1, a2, f1, f2 = now[k].tolist()
                    b1, b2 = then[k, :2].tolist()
                    if f1 > f2:
                        continue
                    pf = np.arange(f1, f2 + 1)
                    gained = [v for v in dict.fromkeys((b1, b2)) if b1 <= b2 and not (a1 <= a2 and a1 <= v <= a2)]
                    lost = [v for v in dict.fromkeys((a1, a2)) if a1 <= a2 and not (b1 <= b2 and b1 <= v <= b2)]
                    earlier = touched[touched < k]
                    for sign, lines, held_by, proposed_by in ((1.0, gained, now_boxes, then), (-1.0, lost, then_boxes, now)):
                        first = proposed_by[earlier]
                        first = first[(first[:, 0] <= first[:, 1]) & (first[:, 2] <= first[:, 3])]
                        for v in lines:
                            counts = ~(_holds(held_by, v, pf) | _holds(first, v, pf))
                            cells = v * map_y + pf[counts] if d < 2 else pf[counts] * map_y + v
                            total += sign * float(score[cells].sum())
                row_move[t, j, d] = total
            pin_move[n] += row_move[t, j]
    return row_move, pin_move
