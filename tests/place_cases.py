"""Shared inputs of test_place_cpu.py / test_place_gpu.py (and tools/bench_placement.py): designs with placement data, moved
pins, hand-built kernel cases that hold every edge of the mask rule of include/mmft_place.h, and a literal second
restatement of that rule whose flags each break one clause."""
import numpy as np

from mmft.placement import attach_placement

S = 64          # cells per prefix block (mmft.fusion.RUN_BLOCK)


# ------------------------------------------------------------------------------------------------ designs
def placed(design, seed, maxlen=12):
    """Seeded placement data for a synth_design, attached with attach_placement (which rebuilds the design's masks).

    Pins sit on a jittered sqrt(N) x sqrt(N) grid scaled to the map, all inside [0, map); a path is its endpoint (first, the
    layout prep.trace_critical_paths emits) followed by nodes from the endpoint's grid neighbourhood, 0 .. maxlen nodes in all
    (0: not even the endpoint), so that the boxes stay local as those of routed nets do."""
    rng = np.random.default_rng(seed)
    N, m, npaths = int(design.N), int(design.map_size), int(design.num_paths)
    g = int(np.ceil(np.sqrt(N)))
    ids = np.arange(N)
    jit = max(m // 32, 1)
    pin_x = np.clip((ids // g) * m // g + rng.integers(-jit, jit + 1, N), 0, m - 1).astype(np.int64)
    pin_y = np.clip((ids % g) * m // g + rng.integers(-jit, jit + 1, N), 0, m - 1).astype(np.int64)
    r = max(g // 16, 1)
    lens = rng.integers(0, maxlen + 1, npaths).astype(np.int64)
    lens[:min(3, npaths)] = [0, 1, maxlen][:min(3, npaths)]             # the short rows and a full one, whatever the seed
    nodes = np.full((npaths, maxlen), -1, dtype=np.int64)
    ends = np.asarray(design.path2endpoint, dtype=np.int64)
    for q in range(npaths):
        n = int(lens[q])
        if n == 0:
            continue
        hop = rng.integers(-r, r + 1, (n, 2))
        nodes[q, :n] = np.clip(ends[q] + hop[:, 0] * g + hop[:, 1], 0, N - 1)
        nodes[q, 0] = ends[q]
    return attach_placement(design, nodes, lens, pin_x, pin_y)


def move(design, seed, frac):
    """(pin_x, pin_y): a fraction `frac` of the design's pins displaced by up to map / 8 cells each way, kept inside the map."""
    rng = np.random.default_rng(seed)
    m, N = int(design.map_size), int(design.N)
    step = max(m // 8, 1)
    who = rng.random(N) < frac
    x = np.where(who, np.clip(design.pin_x + rng.integers(-step, step + 1, N), 0, m - 1), design.pin_x).astype(np.int64)
    y = np.where(who, np.clip(design.pin_y + rng.integers(-step, step + 1, N), 0, m - 1), design.pin_y).astype(np.int64)
    assert (x != design.pin_x).any() or (y != design.pin_y).any()
    return x, y


# ------------------------------------------------------------------------------------------------ hand-built kernel cases
class Case:
    """One kernel input: map, pin table, path rows.  in_range: no clamping, no clipping, no garbage - the reference's own
    rule (oracle.prep_restatement.path_mask_rows) applies as it stands."""

    def __init__(self, name, map_x, map_y, maxlen):
        self.name, self.map_x, self.map_y, self.maxlen = name, map_x, map_y, maxlen
        self.px, self.py, self.rows, self.lens, self.tags = [], [], [], [], []
        self.in_range = True

    def path(self, tag, pts, length=None, tail=()):
        """A path through the points `pts` (new pins each); `length`: the stored length when it is not len(pts); `tail`: points
        stored after the path's end where padding belongs (garbage that must be ignored)."""
        ids = []
        for x, y in list(pts) + list(tail):
            ids.append(len(self.px))
            self.px.append(x)
            self.py.append(y)
            if not (0 <= x < self.map_x and 0 <= y < self.map_y):
                self.in_range = False
        n = len(pts) if length is None else length
        assert len(ids) <= self.maxlen
        if tail or n > self.maxlen or n != len(pts):
            self.in_range = False
        self.rows.append(ids + [-1] * (self.maxlen - len(ids)))
        self.lens.append(n)
        self.tags.append(tag)
        return self

    @property
    def P(self):
        return self.map_x * self.map_y

    def arrays(self):
        """(path_nodes [np, maxlen], path_lens [np], pin_x [N], pin_y [N]) int64."""
        return (np.array(self.rows, dtype=np.int64).reshape(len(self.rows), self.maxlen), np.array(self.lens, dtype=np.int64),
                np.array(self.px, dtype=np.int64), np.array(self.py, dtype=np.int64))

    def point_lists(self):
        """For path_mask_rows: the paths as node lists, and loc[node] = (x, y)."""
        return [[i for i in row[:n]] for row, n in zip(self.rows, self.lens)], list(zip(self.px, self.py))


def _general():
    c = Case('edges_16x16', 16, 16, 4)
    c.path('len0', [])
    c.path('len1', [(5, 5)])
    c.path('len2', [(2, 3), (4, 9)])
    c.path('one_cell', [(3, 3), (3, 3)])
    c.path('overlap', [(1, 1), (5, 5), (3, 3), (8, 9)])
    c.path('whole_map', [(0, 0), (15, 15)])
    c.path('rows_across_a_block_boundary', [(3, 0), (4, 15)])          # cells 48 .. 79: one stretch, split at 64
    c.path('starts_a_block', [(4, 0), (4, 5)])                         # cells 64 .. 69
    c.path('ends_a_block', [(3, 10), (3, 15)])                         # cells 58 .. 63
    c.path('comb', [(0, 1), (15, 1), (15, 3), (0, 3)])                 # columns 1 and 3 (and row 15 between them)
    return c


def _clamped():
    c = Case('clamped_16x16', 16, 16, 4)
    c.path('below_and_above', [(-3, -2), (4, 20)])
    c.path('outside_high', [(20, 20), (25, 30)])                       # empty after clamping: skipped
    c.path('outside_low', [(-5, -5), (-1, -1)])
    c.path('outside_then_inside', [(17, 2), (30, 4), (6, 6)])
    c.path('garbage_after_len', [(2, 2), (3, 6)], tail=[(9, 9), (12, 1)])
    c.path('garbage_after_len1', [(7, 7)], tail=[(1, 1), (14, 14)])
    return c


def _clipped():
    c = Case('clipped_16x16', 16, 16, 3)
    c.path('len_above_maxlen', [(1, 1), (2, 5), (6, 2)], length=5)     # the row behind it is full: reading on would show
    c.path('full_row', [(10, 10), (12, 14), (9, 15)])
    return c


def _single_block():
    c = Case('single_block_8x8', 8, 8, 3)
    c.path('box', [(1, 1), (2, 6)])
    c.path('whole_map', [(0, 0), (7, 7)])
    c.path('corner', [(7, 7), (7, 7)])
    c.path('len0', [])
    return c


def _odd_rows():
    c = Case('rows_of_24', 24, 24, 3)                                  # map_y no multiple of 32: rows straddle words and blocks
    c.path('row_across_64', [(2, 0), (2, 23)])                         # cells 48 .. 71
    c.path('box', [(1, 20), (9, 23), (5, 2)])
    c.path('last_cell', [(23, 23), (23, 22)])
    c.path('whole_map', [(0, 0), (23, 23)])
    return c


def _wide():
    c = Case('wide_32x64', 32, 64, 3)                                  # map_x != map_y: a row is a block
    c.path('box', [(3, 60), (30, 63)])
    c.path('row', [(31, 0), (31, 63)])
    c.path('mixed', [(0, 0), (2, 40), (1, 63)])
    return c


def _serpentine(m=32):
    """(0,0) -> (m-1,0) -> (m-1,2) -> (0,2) -> ... on m x m: full-height columns 0, 2, 4, ... - a row of the map holds m / 2
    one-cell runs.  m = 32: more than 256 runs in the mask, every entry lane makes several trips even at Dout = 4 (256 lanes).
    m = 64: more than 1024, past the kernel's run list - such masks are searched in the bitmap, run by run."""
    c = Case(f'serpentine_{m}x{m}', m, m, m + 1)
    pts, x = [], 0
    for k in range(m + 1):
        y = min(2 * (k // 2), m - 1)
        if k % 2 == 1:
            x = m - 1 - x
        pts.append((x, y))
    c.path('serpentine', pts)
    c.path('len1', [(4, 4)])
    return c


def _long():
    """More nodes than the kernel stages at once (256): a walk of 300 steps, and a row that ends exactly on a stage."""
    c = Case('long_walk_16x16', 16, 16, 300)
    rng = np.random.default_rng(3)
    walk = np.clip(np.cumsum(rng.integers(-3, 4, (300, 2)), 0) + 8, 0, 15)
    c.path('walk_300', [(int(x), int(y)) for x, y in walk])
    c.path('walk_256', [(int(x), int(15 - y)) for x, y in walk[:256]])
    c.path('walk_257', [(int(15 - x), int(y)) for x, y in walk[:257]])
    c.path('len2', [(0, 15), (1, 14)])
    return c


def seeded(name, m, npaths, seed, maxlen=9):
    """npaths random paths of 0 .. maxlen pins on an m x m map, a few pins outside it."""
    rng = np.random.default_rng(seed)
    c = Case(name, m, m, maxlen)
    side = max(m // 6, 2)
    for q in range(npaths):
        n = int(rng.integers(0, maxlen + 1))
        x0, y0 = rng.integers(-2, m + 2 - side, 2)
        c.path(f'p{q}', [(int(x0 + rng.integers(0, side)), int(y0 + rng.integers(0, side))) for _ in range(n)])
    return c


HAND = [_general(), _clamped(), _clipped(), _single_block(), _odd_rows(), _wide(), _serpentine(), _serpentine(64), _long()]
SEEDED = [seeded('seeded_16x16', 16, 40, 11), seeded('seeded_128x128', 128, 40, 12)]
CASES = {c.name: c for c in HAND + SEEDED}


# ------------------------------------------------------------------------------------------------ the rule, literally
def literal(case, exclusive_upper=False, no_block_split=False, no_clamp=False, len_unclipped=False, padding_counts=False):
    """(rows, runs): per path the sorted column list and the list of (start, length) runs, from the words of
    include/mmft_place.h, cell by cell.  Each flag breaks one clause."""
    nodes, lens, px, py = case.arrays()
    mx, my, maxlen = case.map_x, case.map_y, case.maxlen
    flat = np.concatenate([nodes.reshape(-1), np.full(64, -1)])         # reading past a row: what a missing clip would do
    rows, runs = [], []
    for q in range(nodes.shape[0]):
        n = int(lens[q]) if len_unclipped else min(int(lens[q]), maxlen)
        if padding_counts:
            n = int((nodes[q] != -1).sum())
        cells = set()
        for j in range(n - 1):
            a, b = int(flat[q * maxlen + j]), int(flat[q * maxlen + j + 1])
            if a < 0 or b < 0:
                continue
            x1, x2 = min(px[a], px[b]), max(px[a], px[b])
            y1, y2 = min(py[a], py[b]), max(py[a], py[b])
            if not no_clamp:
                x1, y1, x2, y2 = max(x1, 0), max(y1, 0), min(x2, mx - 1), min(y2, my - 1)
            for x in range(x1, x2 + (0 if exclusive_upper else 1)):
                for y in range(y1, y2 + (0 if exclusive_upper else 1)):
                    cells.add(int(x * my + y))
        cols = sorted(cells)
        rr = []
        for c in cols:
            if rr and c == rr[-1][0] + rr[-1][1] and (no_block_split or c % S != 0):
                rr[-1][1] += 1
            else:
                rr.append([c, 1])
        rows.append(cols)
        runs.append([tuple(r) for r in rr])
    return rows, runs


def csr_rows(indptr, cols):
    return [np.asarray(cols[indptr[q]:indptr[q + 1]]).tolist() for q in range(len(indptr) - 1)]


def run_rows(run_ptr, run_start, run_len):
    return [list(zip(np.asarray(run_start[run_ptr[q]:run_ptr[q + 1]]).tolist(), np.asarray(run_len[run_ptr[q]:run_ptr[q + 1]]).tolist()))
            for q in range(len(run_ptr) - 1)]
