"""Shared by test_incr_cpu.py and test_incr_gpu.py: a numpy fan-out cone (a level-free closure over the out-edges, so that it
shares nothing with the level-by-level pull of mmft_fanout_cone_step), and the builders of the cases both files use."""
import copy

import numpy as np

SENTINEL = np.uint32(0x7FC0BEEF)          # a quiet NaN with a payload: no MLP output has these bits


# ------------------------------------------------------------------------------------------------ the reference closure
def fanout_cone(n, edges, seeds, within=None):
    """uint8[n]: 1 on `seeds` (node ids, or a uint8[n] flag array) and on everything reachable from them along `edges`, a list
    of (src, dst) int arrays.  within (uint8[n]): nodes outside it are neither marked nor walked through."""
    mark = np.zeros(n, dtype=bool)
    seeds = np.asarray(seeds)
    if seeds.dtype == np.uint8 and seeds.shape == (n,):
        mark[:] = seeds != 0
    else:
        mark[seeds.astype(np.int64)] = True
    ok = np.ones(n, dtype=bool) if within is None else np.asarray(within) != 0
    mark &= ok
    src = np.concatenate([np.asarray(s, dtype=np.int64) for s, _ in edges]) if edges else np.zeros(0, np.int64)
    dst = np.concatenate([np.asarray(d, dtype=np.int64) for _, d in edges]) if edges else np.zeros(0, np.int64)
    frontier = mark.copy()
    while frontier.any():
        new = np.zeros(n, dtype=bool)
        new[dst[frontier[src]]] = True
        new &= ok & ~mark
        mark |= new
        frontier = new
    return mark.astype(np.uint8)


def design_edges(d):
    return [(d.net_src, d.net_dst), (d.cell_src, d.cell_dst)]


def design_cone(d, seeds, within=None):
    """The cone inside one design, in the design's own node numbering."""
    return fanout_cone(d.N, design_edges(d), seeds, within)


def csr_edges(indptr, indices):
    """(src, dst) of an in-edge CSR given as host arrays."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    return indices, np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr))


def fanin_cone(n, edges, targets):
    """The backward closure (what prep.cone_mask computes): the fan-out cone of the reversed edges."""
    return fanout_cone(n, [(d, s) for s, d in edges], targets)


# ------------------------------------------------------------------------------------------------ designs
def cone_designs(fanin):
    from mmft.synth import synth_design
    return [synth_design(N=6000, L=12, tile=32, seed=120 + i, end_frac=0.2, fanin=fanin) for i in range(2)]


def predictor_designs(shape=(2048, 12), fanin='regular'):
    from mmft.synth import synth_design
    return [synth_design(N=shape[0], L=shape[1], tile=32, seed=700 + i, end_frac=0.25, fanin=fanin) for i in range(2)]


def level_of(d):
    """int64[N]: the level of every node of a design (-1: in no level)."""
    out = np.full(d.N, -1, dtype=np.int64)
    for l, nodes in enumerate(d.levels):
        out[nodes] = l
    return out


def pick_seeds(d, endpoints, levels=(1, 6, 11)):
    """One node per level by rule: the first node of the level whose cone holds one of `endpoints` (an edit there must move a
    prediction), else the level's first node."""
    reaches = fanin_cone(d.N, design_edges(d), np.asarray(endpoints, dtype=np.int64)) != 0     # v's cone holds an endpoint
    out = []
    for l in levels:
        if l >= d.L or not len(d.levels[l]):
            continue
        nodes = np.asarray(d.levels[l], dtype=np.int64)
        hit = nodes[reaches[nodes]]
        out.append(int(hit[0]) if hit.size else int(nodes[0]))
    return np.array(out, dtype=np.int64)


def edited(d, rows, seed, scale=0.5, net=False):
    """A copy of design d whose cell_feat (and, with net=True, net_feat) rows `rows` moved - every one of them bitwise."""
    rng = np.random.default_rng(seed)
    e = copy.copy(d)
    rows = np.asarray(rows, dtype=np.int64)
    for name in ('cell_feat', 'net_feat') if net else ('cell_feat',):
        t = getattr(d, name).copy()
        t[rows] = t[rows] + (scale * (1.0 + rng.random((rows.size, t.shape[1])))).astype(np.float32)
        assert (t[rows].view(np.uint32) != getattr(d, name)[rows].view(np.uint32)).any(axis=1).all()
        setattr(e, name, t)
    return e


# ------------------------------------------------------------------------------------------------ row masks of the masked MLP
def mlp_masks(n, tile=64):
    """{name: uint8[n]} - the flag patterns a tile-skipping kernel can get wrong, for a launch over n rows."""
    nt = (n + tile - 1) // tile
    one = np.zeros(n, dtype=np.uint8)
    one[[min(t * tile + (7 * t + 3) % tile, n - 1) for t in range(nt)]] = 1
    gap = np.ones(n, dtype=np.uint8)
    if nt >= 3:
        gap[tile:2 * tile] = 0                       # a clear tile between two set ones
    else:
        gap[n // 2:] = 0
    last = np.zeros(n, dtype=np.uint8)
    last[(nt - 1) * tile:] = 1                       # only the last - partial, unless tile divides n - tile
    return {'none': np.zeros(n, dtype=np.uint8), 'all': np.ones(n, dtype=np.uint8), 'one_per_tile': one, 'gap': gap, 'last_tile': last}


# ------------------------------------------------------------------------------------------------ update_rows_diff
DIFF_KINDS = ('same', 'one_element', 'zero_sign', 'same_nan')


def diff_case(kind, old, seed=0):
    """(old', new, changed): old' [n, width] float32 is what the table's rows hold before the call (old, with a zero or a NaN
    planted where the case needs one), new the rows pushed, changed uint8[n] the rows that differ bitwise."""
    rng = np.random.default_rng(seed)
    old = np.array(old, dtype=np.float32, copy=True)
    n, width = old.shape
    r, c = int(rng.integers(n)), int(rng.integers(width))
    changed = np.zeros(n, dtype=np.uint8)
    if kind == 'zero_sign':
        old[r, c] = 0.0
    elif kind == 'same_nan':
        old.view(np.uint32)[r, c] = 0x7FC01234
    new = old.copy()
    if kind == 'one_element':
        new[r, c] = old[r, c] + np.float32(1.0)
        changed[r] = 1
    elif kind == 'zero_sign':
        new[r, c] = -0.0
        changed[r] = 1
    assert np.array_equal((old.view(np.uint32) != new.view(np.uint32)).any(axis=1).astype(np.uint8), changed)
    return old, new, changed
