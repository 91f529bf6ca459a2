"""Shared inputs of test_pin_move_cpu.py / test_pin_move_gpu.py: the kernel cases of place_cases.py, unchanged, as one-design
selections, and hand-built rows with REPEATED pins (place_cases.Case.path makes new pins per point, so none of its rows has
one), pins on and beyond the map's edge, int32 extremes and a batch of two designs (f_off != 0) - every clause of
include/mmft_sens_pins.h."""
import numpy as np

from place_cases import CASES as PLACE_CASES

DOUTS = (4, 12, 128)
DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1))                  # 0: x + 1, 1: x - 1, 2: y + 1, 3: y - 1
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


class PinCase:
    """One input of mmft_pin_move_rows / _sum: map, pin table, path rows given as NODE IDS, the selected batch rows and their
    feature-map offsets (None: one design)."""

    def __init__(self, name, map_x, map_y, maxlen, B=1):
        self.name, self.map_x, self.map_y, self.maxlen, self.B = name, map_x, map_y, maxlen, B
        self.px, self.py, self.rows, self.lens, self.tags = [], [], [], [], []
        self.paths = self.f_off = None

    def pin(self, x, y):
        self.px.append(x)
        self.py.append(y)
        return len(self.px) - 1

    def row(self, tag, ids, length=None):
        assert len(ids) <= self.maxlen and all(0 <= i < len(self.px) for i in ids)
        self.rows.append(list(ids) + [-1] * (self.maxlen - len(ids)))
        self.lens.append(len(ids) if length is None else length)
        self.tags.append(tag)
        return self

    @property
    def P(self):
        return self.map_x * self.map_y

    def arrays(self):
        """(path_nodes [np, maxlen], path_lens [np], pin_x [N], pin_y [N]) int64."""
        return (np.array(self.rows, dtype=np.int64).reshape(len(self.rows), self.maxlen), np.array(self.lens, dtype=np.int64),
                np.array(self.px, dtype=np.int64), np.array(self.py, dtype=np.int64))

    def selection(self):
        """(paths int64 [T], f_off int64 [T] or None)."""
        paths = np.arange(len(self.rows), dtype=np.int64) if self.paths is None else np.asarray(self.paths, dtype=np.int64)
        return paths, (None if self.f_off is None else np.asarray(self.f_off, dtype=np.int64))


def _from_place(c):
    p = PinCase(c.name, c.map_x, c.map_y, c.maxlen)
    p.px, p.py, p.rows, p.lens, p.tags = list(c.px), list(c.py), [list(r) for r in c.rows], list(c.lens), list(c.tags)
    return p


def _repeats():
    c = PinCase('repeats_16x16', 16, 16, 5)
    A, B_, C = c.pin(3, 3), c.pin(6, 8), c.pin(9, 2)
    c.row('A_B_A', [A, B_, A])
    c.row('A_A', [A, A])                                               # an (n, n) box: its single cell moves
    c.row('A_B_A_B', [A, B_, A, B_])
    c.row('A_B_C_A_B', [A, B_, C, A, B_])
    c.row('B_B_B', [B_, B_, B_])
    # a pin that is the max-x (and, for its first box, max-y) corner of both its boxes: x + 1 proposes (11, 10) twice
    D, E, F = c.pin(7, 8), c.pin(10, 10), c.pin(8, 12)
    c.row('shared_corner', [D, E, F])
    # G is the min corner of the box (G, H): x + 1 takes the line x = 2, y in [2, 5] away from it - but the boxes (H, J) and
    # (J, K), which G does not touch, keep (2, 4) and (2, 5)
    G, H, J, K = c.pin(2, 2), c.pin(5, 5), c.pin(1, 4), c.pin(3, 6)
    c.row('kept_alive', [G, H, J, K])
    c.row('kept_alive_by_a_far_box', [G, H, c.pin(9, 9), J, K])
    return c


def _edges():
    c = PinCase('edges_of_the_map_16x16', 16, 16, 4)
    a, b = c.pin(15, 4), c.pin(12, 6)
    c.row('on_the_edge_moving_out', [a, b])                            # x + 1: clamped back, nothing changes
    a, b = c.pin(0, 0), c.pin(0, 3)
    c.row('on_the_low_edge', [a, b])
    z = c.pin(0, 0)
    c.row('single_cell_vanishes', [z, z])                              # (z, z) at the corner: x - 1 / y - 1 empties the mask
    z = c.pin(15, 15)
    c.row('single_cell_vanishes_high', [z, z])
    a, b = c.pin(-1, 5), c.pin(3, 7)
    c.row('outside_moving_in_nothing_new', [a, b])                     # the lower corner was clamped to 0 already
    a, b = c.pin(-1, 5), c.pin(-1, 7)
    c.row('outside_moving_in_box_appears', [a, b])                     # empty -> the line x = 0
    a, b = c.pin(4, 16), c.pin(9, 17)
    c.row('outside_high_moving_in', [a, b])
    a, b = c.pin(17, 3), c.pin(11, 5)
    c.row('outside_by_two_moving_in', [a, b])                          # 17 -> 16: still clamped to 15
    a, b = c.pin(-3, 5), c.pin(2, 2)
    c.row('outside_moving_further_out', [a, b])
    a, b, d = c.pin(I32_MAX, 5), c.pin(13, I32_MIN), c.pin(I32_MIN, I32_MAX)
    c.row('int32_extremes', [a, b, d, a])
    c.row('len_above_maxlen', [c.pin(1, 1), c.pin(2, 5), c.pin(6, 2), c.pin(4, 4)], length=7)
    c.row('len0', [])
    c.row('len1', [c.pin(8, 8)])
    return c


def _two_designs():
    """Two designs of 12 pins each on a 16 x 16 map, rows of both in one selection that is not in path order and takes one path
    twice: f_off != 0, and pins with several first-occurrence slots."""
    rng = np.random.default_rng(21)
    c = PinCase('two_designs_16x16', 16, 16, 6, B=2)
    per = 12
    for _ in range(2 * per):
        c.pin(int(rng.integers(-1, 17)), int(rng.integers(-1, 17)))
    design = []
    for q in range(10):
        b = q // 5
        n = int(rng.integers(2, 7))
        c.row(f'd{b}_p{q}', (rng.integers(0, per, n) + b * per).tolist())      # drawn with replacement: repeats happen
        design.append(b)
    c.paths = [7, 0, 3, 9, 0, 5, 2, 8, 1, 6, 4]
    c.f_off = [design[q] * c.P for q in c.paths]
    return c


HAND = [_repeats(), _edges(), _two_designs()]
CASES = {c.name: c for c in [_from_place(c) for c in PLACE_CASES.values()] + HAND}
assert len(CASES) == len(PLACE_CASES) + len(HAND)


def operands(case, Dout, seed=5):
    """Seeded fp32 (feat [B * P], w [Dout, P], g [T, Dout]) of a case; feat and g carry both signs."""
    rng = np.random.default_rng([seed, Dout, len(case.name)])
    T = case.selection()[0].shape[0]
    return (rng.standard_normal(case.B * case.P).astype(np.float32), (rng.standard_normal((Dout, case.P)) / np.sqrt(Dout)).astype(np.float32),
            rng.standard_normal((T, Dout)).astype(np.float32))
