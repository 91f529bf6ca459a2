"""The literal definition of include/mmft_sens_pins.h: for every (batch row, first-occurrence position, direction) the path is
rasterised again with the pin moved (mmft.placement._bitmaps, the mask rule), the two set differences are taken and the cell
scores summed in fp64.  Next to each value: K, the number of changed cells, and A = sum over them of |feat_c| sum_k |g_k W_kc|,
the magnitudes an fp32 evaluation's error scales with.  Each flag breaks one clause of the definition."""
import numpy as np

from mmft.placement import _bitmaps
from pin_move_cases import DIRS

FLAGS = ('first_only', 'ignore_coverage', 'double_count', 'clamp_first')
_GEOMETRY = {}


def _mask(ids, px, py, mx, my):
    """int [P]: the mask of one row of node ids under the pins (px, py), by placement._bitmaps."""
    n = len(ids)
    nodes = np.asarray(ids, dtype=np.int64).reshape(1, max(n, 1)) if n else np.zeros((1, 1), dtype=np.int64)
    return next(_bitmaps(nodes, np.array([n]), px, py, mx, my)).reshape(-1).astype(np.int64)


def geometry(case, flag=None):
    """[(t, j, d, gained, lost)]: per entry two int [P] arrays counting how often a cell joins / leaves the mask (0 / 1 under the
    true rule).  Independent of feat / w / g, so made once per case and flag."""
    key = (case.name, flag)
    if key in _GEOMETRY:
        return _GEOMETRY[key]
    assert flag is None or flag in FLAGS
    nodes, lens, px, py = case.arrays()
    paths, _ = case.selection()
    mx, my, N = case.map_x, case.map_y, px.shape[0]
    out = []
    for t, q in enumerate(paths.tolist()):
        ids = nodes[q, :max(min(int(lens[q]), case.maxlen), 0)].tolist()
        if not ids:
            continue
        M = _mask(ids, px, py, mx, my)
        for j, n in enumerate(ids):
            if n in ids[:j]:
                continue
            for d, (dx, dy) in enumerate(DIRS):
                x0, y0 = int(px[n]), int(py[n])
                if flag == 'clamp_first':                              # displaced AFTER clamping
                    x0, y0 = min(max(x0, 0), mx - 1), min(max(y0, 0), my - 1)
                x2, y2 = np.append(px, x0 + dx), np.append(py, y0 + dy)                 # the moved pin is pin N
                moved = [N if (m == n and (flag != 'first_only' or i == j)) else m for i, m in enumerate(ids)]
                M2 = _mask(moved, x2, y2, mx, my)
                if flag in ('ignore_coverage', 'double_count'):
                    gained, lost = np.zeros_like(M), np.zeros_like(M)
                    for k in range(len(ids) - 1):
                        if n not in ids[k:k + 2]:
                            continue
                        was, now = _mask(ids[k:k + 2], px, py, mx, my), _mask(moved[k:k + 2], x2, y2, mx, my)
                        g_k, l_k = now & (1 - was), was & (1 - now)
                        if flag == 'double_count':                     # the other boxes are honoured, but every proposal counts
                            gained, lost = gained + g_k * (1 - M), lost + l_k * (1 - M2)
                        else:                                          # whatever the pin's boxes gain or lose, covered or not
                            gained, lost = gained | g_k, lost | l_k
                else:
                    gained, lost = M2 & (1 - M), M & (1 - M2)
                out.append((t, j, d, gained, lost))
    _GEOMETRY[key] = out
    return out


def oracle(case, feat, w, g, flag=None):
    """dict(row_move, K, A [T, maxlen, 4]; pin_move, pin_K, pin_A, pin_slots [N, 4]) in fp64 / int64 from fp32 operands."""
    paths, f_off = case.selection()
    T, P = paths.shape[0], case.P
    feat, w, g = (np.asarray(a, dtype=np.float64) for a in (feat, w, g))
    N = len(case.px)
    row = {k: np.zeros((T, case.maxlen, 4), dtype=np.int64 if k == 'K' else np.float64) for k in ('row_move', 'K', 'A')}
    pin = {k: np.zeros((N, 4), dtype=np.float64 if k in ('pin_move', 'pin_A') else np.int64) for k in ('pin_move', 'pin_K', 'pin_A', 'pin_slots')}
    nodes = case.arrays()[0]
    score = mag = None
    last_t = -1
    for t, j, d, gained, lost in geometry(case, flag):
        if t != last_t:
            f = feat[(0 if f_off is None else int(f_off[t])):][:P]
            score, mag, last_t = f * (g[t] @ w), np.abs(f) * (np.abs(g[t]) @ np.abs(w)), t
        row['row_move'][t, j, d] = float((gained * score).sum() - (lost * score).sum())
        row['K'][t, j, d] = int(gained.sum() + lost.sum())
        row['A'][t, j, d] = float(((gained + lost) * mag).sum())
        n = int(nodes[paths[t], j])
        pin['pin_move'][n, d] += row['row_move'][t, j, d]              # geometry() runs in ascending (t, j)
        pin['pin_K'][n, d] += row['K'][t, j, d]
        pin['pin_A'][n, d] += row['A'][t, j, d]
        pin['pin_slots'][n, d] += 1
    return {**row, **pin}


def bound(Dout, K, A, slots=0):
    """The forward bound of an fp32 chain of Dout + K + 1 (+ slots) operations on the fp64 sum of magnitudes A; the factor 2
    covers fma contraction and the order of the sums."""
    return 2.0 * (Dout + K + 1 + slots) * 2.0 ** -24 * A
