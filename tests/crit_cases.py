"""Inputs shared by test_crit_cpu.py and test_crit_gpu.py: the kernel cases of place_cases (maps 8 x 8 to 128 x 128, the
300-pin walk, clamped / clipped / garbage rows), every row given a slack through chosen (pred, required) pairs, laid out as
one design and as three designs (row_design not sorted, one design without rows).  Each slack pattern is tagged with the
rules of include/mmft_crit.h that it decides."""
import functools
from types import SimpleNamespace

import numpy as np

import place_cases as PC

NAMES = tuple(sorted(PC.CASES))
LAYOUTS = ('one', 'three')
F = np.float32
NAN, INF = F(np.nan), F(np.inf)
TINY = F(1e-45)                                  # the smallest denormal

# pattern -> the rules it decides
PATTERNS = {
    'ties': {'equal_slack_shared_pin'},                       # both selections of a path carry one slack: the smaller row wins
    'twice': {'same_path_twice_different_slack'},
    'specials': {'nan_pred', 'plus_inf', 'minus_inf', 'required_equals_pred', 'negative_zero', 'tiny_negative'},
    'nonneg_design': {'design_without_violation'},
    'lonely_empty': {'only_valid_row_has_an_empty_path'},
    'worst_unmasked': {'worst_row_has_no_mask'},              # w comes from a row whose path has fewer than two pins
    'random': {'inexact_division'},
}


@functools.lru_cache(maxsize=None)
def tables(name):
    """(path_nodes [np + 1, maxlen], path_lens [np + 1], pin_x [N], pin_y [N]) int64: the case's tables with one more,
    empty, path at the end (every case then holds a row without pins)."""
    nodes, lens, px, py = PC.CASES[name].arrays()
    nodes = np.concatenate([nodes, np.full((1, nodes.shape[1]), -1, dtype=np.int64)])
    return nodes, np.concatenate([lens, [0]]).astype(np.int64), px, py


def selection(name):
    """paths [T]: every path twice, rows t and t + T / 2 select the same one."""
    n = tables(name)[0].shape[0]
    return np.concatenate([np.arange(n), np.arange(n)]).astype(np.int64)


def designs(name, layout):
    """(row_design or None, B).  'three': designs 0 and 2 interleaved without order, design 1 has no rows; the first selection
    of the empty path (row T / 2 - 1) belongs to design 2."""
    T = selection(name).shape[0]
    if layout == 'one':
        return None, 1
    d = np.where(np.random.default_rng(len(name)).random(T) < 0.5, 0, 2).astype(np.int64)
    d[0], d[1], d[T // 2 - 1] = 2, 0, 2
    return d, 3


def _pairs(slack):
    """(pred, required) with required - pred == slack exactly, for slacks of a few bits."""
    slack = np.asarray(slack, dtype=F)
    required = np.ones_like(slack)
    return (required - slack).astype(F), required


SPECIALS = (('nan_pred', NAN, F(1.0)), ('plus_inf', -INF, F(1.0)), ('minus_inf', INF, F(0.0)), ('inf_minus_inf', INF, INF),
            ('required_equals_pred', F(0.75), F(0.75)), ('negative_zero', F(0.0), F(-0.0)), ('tiny_negative', TINY, F(0.0)),
            ('smallest_normal', F(1.1754944e-38), F(0.0)), ('neg', F(1.5), F(1.0)), ('pos', F(0.5), F(1.0)), ('neg2', F(1.25), F(1.0)))


@functools.lru_cache(maxsize=None)
def batch(name, pattern, layout):
    c = PC.CASES[name]
    nodes, lens, px, py = tables(name)
    paths = selection(name)
    T, half = paths.shape[0], paths.shape[0] // 2
    row_design, B = designs(name, layout)
    d = np.zeros(T, dtype=np.int64) if row_design is None else row_design
    live = np.minimum(lens, c.maxlen)[paths]
    t = np.arange(T)
    if pattern == 'ties':
        pred, required = _pairs(np.array([-0.5, -0.25, 0.25, -0.5], dtype=F)[paths % 4])
    elif pattern == 'twice':
        first = (t < half) == (paths % 2 == 0)
        pred, required = _pairs(np.where(first, F(-0.25), F(-0.75)) * np.where(paths % 3 == 2, F(-1.0), F(1.0)))
    elif pattern == 'specials':
        kind = (t + t // half) % len(SPECIALS)                  # the two selections of a path differ in kind
        pred = np.array([SPECIALS[k][1] for k in kind], dtype=F)
        required = np.array([SPECIALS[k][2] for k in kind], dtype=F)
    elif pattern == 'nonneg_design':
        s = np.array([-1.0, 0.5, -0.125, 0.0, -2.0], dtype=F)[t % 5]
        last = d == d.max()                                     # the one design, or design 2 of three: nothing below zero
        s[last] = np.array([0.0, 0.5, np.inf, 2.0], dtype=F)[t[last] % 4]
        pred, required = _pairs(s)
    elif pattern == 'lonely_empty':
        s = np.array([-1.0, 0.5, -0.125, -3.0], dtype=F)[t % 4]
        pred, required = _pairs(s)
        last = d == d.max()
        pred[last] = NAN
        pred[half - 1], required[half - 1] = F(3.0), F(1.0)     # the empty path's first selection: slack -2, the design's only valid row
    elif pattern == 'worst_unmasked':
        s = np.array([-0.5, -1.0, -3.0, 0.25, -0.75], dtype=F)[paths % 5]
        s[live < 2] = F(-4.0)
        pred, required = _pairs(s)
    elif pattern == 'random':
        rng = np.random.default_rng(len(name) + 100)
        required = (1.0 + 0.3 * rng.standard_normal(T)).astype(F)
        pred = (required - rng.standard_normal(T).astype(F) + F(0.2)).astype(F)
    else:
        raise KeyError(pattern)
    return SimpleNamespace(name=name, pattern=pattern, layout=layout, nodes=nodes, lens=lens, px=px, py=py, map_x=c.map_x, map_y=c.map_y,
                           maxlen=c.maxlen, P=c.P, paths=paths, pred=pred, required=required, row_design=row_design, B=B,
                           N=int(px.shape[0]), T=T, tags=PATTERNS[pattern])


def permuted(b, seed):
    """The same batch with its rows (pred, required, paths, row_design together) in another order."""
    p = np.random.default_rng(seed).permutation(b.T)
    q = SimpleNamespace(**vars(b))
    q.pred, q.required, q.paths = b.pred[p], b.required[p], b.paths[p]
    q.row_design = None if b.row_design is None else b.row_design[p]
    return q


def reference(b, cells=True):
    from mmft.criticality import reference_criticality
    return reference_criticality(b.pred, b.required, b.nodes, b.lens, b.px, b.py, b.map_x, b.map_y, b.paths, b.row_design, b.N, b.B,
                                 cells=cells)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def differences(a, b, fields=None):
    """Names of the outputs (mmft.criticality.FIELDS order) that differ BITWISE: floats as int32 views, so +0.0 / -0.0, inf
    and every bit of a quotient count; None == None."""
    from mmft.criticality import FIELDS
    out = []
    for k, x, y in zip(FIELDS, a, b):
        if fields is not None and k not in fields:
            continue
        if (x is None) != (y is None):
            out.append(k)
        elif x is not None:
            x, y = np.asarray(x), np.asarray(y)
            if x.dtype != y.dtype or x.shape != y.shape or not np.array_equal(_bits(x), _bits(y)):
                out.append(k)
    return out
