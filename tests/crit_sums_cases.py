"""Inputs shared by test_crit_sums_cpu.py and test_crit_sums_gpu.py: the batches of crit_cases, each at three scales, and
one hand-built batch for the clauses of include/mmft_crit_sums.h that those cannot decide - their paths visit every pin once
and their slacks are few-bit numbers.  Nothing here touches crit_cases or place_cases; both are imported as they are."""
import functools
from types import SimpleNamespace

import numpy as np

import crit_cases as C

F = np.float32
SCALES = (0, 20, 30)
QUANTUM20 = 2.0 ** -20
NAMES13 = None                                   # mmft.criticality.FIELDS + SUM_FIELDS, filled in on first use


def names13():
    global NAMES13
    if NAMES13 is None:
        from mmft.criticality import FIELDS, SUM_FIELDS
        NAMES13 = FIELDS + SUM_FIELDS
    return NAMES13


@functools.lru_cache(maxsize=None)
def hand():
    """'repeat_8x8': two designs on an 8 x 8 map.  Path 0 holds pin 0 twice and path 4 pin 1 twice (a pin counts per
    position; the two boxes of path 0 are one box, whose cells count once); rows 1, 2, 3 are 1.5, 0.5 and 2.5 quanta of 2^-20
    below zero (ties to even: 2, 0, 2); at scale 20 the cap is 2^12: row 6 lies beyond it and row 9 on it exactly; row 7
    violates on the empty path; design 1 has no violation; row 8 is a NaN."""
    nodes = np.array([[0, 1, 0, -1], [2, 3, -1, -1], [4, -1, -1, -1], [-1, -1, -1, -1], [1, 2, 3, 1]], dtype=np.int64)
    lens = np.array([3, 2, 1, 0, 4], dtype=np.int64)
    px, py = np.array([1, 3, 5, 6, 0, 7], dtype=np.int64), np.array([1, 4, 5, 2, 7, 0], dtype=np.int64)
    paths = np.array([0, 0, 1, 4, 2, 3, 1, 3, 0, 2], dtype=np.int64)
    row_design = np.array([0, 0, 0, 0, 1, 1, 0, 0, 0, 0], dtype=np.int64)
    slack = np.array([-0.75, -1.5 * QUANTUM20, -0.5 * QUANTUM20, -2.5 * QUANTUM20, 1.0, 0.0, -8192.0, -3.0, np.nan, -4096.0], dtype=F)
    required = np.zeros(slack.shape[0], dtype=F)
    pred = (-slack).astype(F)                      # required - pred == slack exactly
    return SimpleNamespace(name='repeat_8x8', pattern='hand', layout='two', nodes=nodes, lens=lens, px=px, py=py, map_x=8, map_y=8,
                           maxlen=4, P=64, paths=paths, pred=pred, required=required, row_design=row_design, B=2, N=6,
                           T=int(paths.shape[0]))


def reference(b, scale_log2, cells=True):
    from mmft.criticality import reference_criticality_sums
    return reference_criticality_sums(b.pred, b.required, b.nodes, b.lens, b.px, b.py, b.map_x, b.map_y, b.paths, b.row_design, b.N, b.B,
                                      scale_log2=scale_log2, cells=cells)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def differences(a, b, fields=None):
    """Names of the thirteen outputs (FIELDS + SUM_FIELDS order) that differ BITWISE - floats as int32 views, dtype and shape
    count; None == None."""
    out = []
    for k, x, y in zip(names13(), a, b):
        if fields is not None and k not in fields:
            continue
        if (x is None) != (y is None):
            out.append(k)
        elif x is not None:
            x, y = np.asarray(x), np.asarray(y)
            if x.dtype != y.dtype or x.shape != y.shape or not np.array_equal(_bits(x), _bits(y)):
                out.append(k)
    return out


def batches():
    """Every (batch, tag): name x pattern x layout of crit_cases, then the hand-built one."""
    for name in C.NAMES:
        for pattern in C.PATTERNS:
            for layout in C.LAYOUTS:
                yield C.batch(name, pattern, layout)
    yield hand()
