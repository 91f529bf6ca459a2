"""Inputs shared by test_report_cpu.py and test_report_gpu.py: one batch of ten designs whose row counts sit on the edges of
the report kernel (mmft_timing_report), the value regimes that decide each of its rules, and a second, literal restatement of
the contract (a Python loop per design) whose rules can be broken one at a time."""
import math

import numpy as np

SIZES = (0, 1, 63, 64, 65, 1023, 1025, 4096, 4097, 20000)       # empty; wave and workgroup edges; one part; two parts, the second with one row; five parts
B = len(SIZES)
T = sum(SIZES)
KS = (1, 7, 64)
NBINS = (0, 1, 64)
HIST_LO, HIST_HI = -1.0, 1.0
REGIMES = ('normal', 'five_values', 'no_violation', 'nan', 'zeros', 'inf')
ALL_NAN_DESIGN = 5


def layout():
    """(design_of_row [T], design_ptr [B + 1], design_rows [T]): the rows of the designs interleaved by a fixed permutation, so
    that design_rows is a real gather."""
    from mmft.report import group_rows
    design_of_row = np.repeat(np.arange(B), SIZES)[np.random.default_rng(20240).permutation(T)]
    ptr, rows = group_rows(design_of_row, B)
    return design_of_row, ptr, rows


def regime(name):
    """(pred, required) fp32 [T]."""
    rng = np.random.default_rng(REGIMES.index(name) + 77)
    design_of_row, ptr, rows = layout()
    z = rng.standard_normal(T).astype(np.float32)
    if name == 'normal':                                    # slack = required - pred is z up to one rounding
        required = (1.0 + 0.3 * rng.standard_normal(T)).astype(np.float32)
        return (required - z).astype(np.float32), required
    if name == 'five_values':                               # every selection is decided by the row tie-break; the values sit
        vals = np.array([-1.0, -0.25, 0.0, 0.5, 1.0], dtype=np.float32)      # on the histogram's edges lo and hi, and on zero
        required = np.ones(T, dtype=np.float32)
        return (required - vals[rng.integers(0, 5, T)]).astype(np.float32), required
    if name == 'no_violation':
        return np.zeros(T, dtype=np.float32), np.abs(z)
    if name == 'nan':                                       # 3 % NaN predictions, one design all NaN, and the lone row of a
        pred, required = z.copy(), np.zeros(T, dtype=np.float32)           # second part NaN (a part without a valid row)
        pred[rng.random(T) < 0.03] = np.nan
        pred[design_of_row == ALL_NAN_DESIGN] = np.nan
        pred[rows[ptr[8] + 4096]] = np.nan
        return pred, required
    if name == 'zeros':                                     # half of the rows have slack zero - the worst value there is - in
        required = np.abs(z) + np.float32(0.5)                             # two spellings: -0.0 - +0.0 = -0.0 and +0.0 - +0.0
        pred = np.zeros(T, dtype=np.float32)
        zero = rng.random(T) < 0.5
        required[zero] = np.where(rng.random(int(zero.sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
        return pred, required
    if name == 'inf':                                       # +-inf are ordinary values, inf - inf is a NaN row; values a hair
        pred, required = z.copy(), np.zeros(T, dtype=np.float32)           # below hi, whose bin index rounds up to nbins
        pick = rng.permutation(T)
        pred[pick[:40]], pred[pick[40:80]] = np.inf, -np.inf
        pred[pick[80:100]], required[pick[80:100]] = np.inf, np.inf
        pred[pick[100:200]] = -np.nextafter(np.float32(HIST_HI), np.float32(0.0))
        return pred, required
    raise KeyError(name)


def literal_report(pred, required, design_ptr, design_rows, k, hist=None, tie_largest_row=False, nan_is_valid=False,
                   zero_violates=False):
    """The contract of include/mmft_report.h row by row in plain Python.  The three flags each break ONE rule (the order of
    rows on equal slack, the exclusion of NaN rows, `<` against `<=` for a violation): the regimes must notice each."""
    nb = len(design_ptr) - 1
    nbins = int(hist[2]) if hist is not None else 0
    summary = np.zeros((nb, 6), dtype=np.float64)
    worst_row = np.full((nb, k), -1, dtype=np.int32)
    worst_slack = np.full((nb, k), np.inf, dtype=np.float32)
    h = np.zeros((nb, nbins + 2), dtype=np.int32) if nbins else None
    if nbins:
        lo, hi = np.float32(hist[0]), np.float32(hist[1])
        w = np.float32((hi - lo) / np.float32(nbins))
    with np.errstate(invalid='ignore'):
        for b in range(nb):
            items, n_nan = [], 0
            for i in range(int(design_ptr[b]), int(design_ptr[b + 1])):
                r = int(design_rows[i])
                s = np.float32(np.float32(required[r]) - np.float32(pred[r]))
                if s == 0:
                    s = np.float32(0.0)                     # -0.0 becomes +0.0
                if math.isnan(s):
                    if not nan_is_valid:
                        n_nan += 1
                        continue
                    s = np.float32(np.inf)
                items.append((float(s), -r if tie_largest_row else r, r))
            items.sort()
            viol = [s for s, _, _ in items if (s <= 0 if zero_violates else s < 0)]
            summary[b] = (len(items), n_nan, len(viol), items[0][0] if items else np.nan, items[0][2] if items else -1, math.fsum(viol))
            for j, (s, _, r) in enumerate(items[:k]):
                worst_row[b, j], worst_slack[b, j] = r, s
            for s, _, _ in items if nbins else ():
                s = np.float32(s)
                if s < lo:
                    h[b, 0] += 1
                elif s >= hi:
                    h[b, nbins + 1] += 1
                else:
                    h[b, 1 + min(nbins - 1, int(math.floor(np.float32(np.float32(s - lo) / w))))] += 1
    return summary, worst_row, worst_slack, h


def same_report(a, b, tns_exact=True):
    """Bitwise equality of two reports in the device layout (NaN == NaN, -0.0 != +0.0); tns (summary column 5) optional."""
    cols = slice(0, 6 if tns_exact else 5)
    bits = lambda x: np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32)
    return bool(np.array_equal(bits(np.asarray(a[0], dtype=np.float64)[:, cols]), bits(np.asarray(b[0], dtype=np.float64)[:, cols])) and
                np.array_equal(a[1], b[1]) and
                np.array_equal(bits(np.asarray(a[2], dtype=np.float32)), bits(np.asarray(b[2], dtype=np.float32))) and
                ((a[3] is None and b[3] is None) or np.array_equal(a[3], b[3])))


def tns_bound(ref_summary, pred, required, design_ptr, design_rows):
    """Per design n_b * 2^-52 * sum |violating slack|: twice the textbook bound (n - 1) u sum |x|, u = 2^-53, of any-order
    fp64 summation against the exact sum (math.fsum rounds it once more: one more u, inside the factor 2)."""
    from mmft.report import reference_slack
    slack = reference_slack(pred, required).astype(np.float64)
    out = np.zeros(len(design_ptr) - 1)
    for b in range(out.shape[0]):
        s = slack[design_rows[design_ptr[b]:design_ptr[b + 1]]]
        s = s[s < 0]                                        # (NaN rows drop out here too)
        out[b] = ref_summary[b, 0] * 2.0 ** -52 * np.abs(s).sum()
    return out
