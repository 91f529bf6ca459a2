"""Timing report on the device: per design the worst negative slack (WNS), the total negative slack (TNS), the number of
violating endpoints, the k most critical endpoints and a slack histogram - what a timing engine prints, from the predictions
and the required times of a batch, in ONE kernel launch (mmft_timing_report, include/mmft_report.h) and one small
device->host copy, instead of a copy of all T predictions and a host sort per design.

The rules (the header states them, `reference_report` restates them in numpy / fp64):
  slack = required - pred, one fp32 subtraction, -0.0 canonicalised to +0.0; a row violates when slack < 0 (the rule of
  evaluate.eval_sums); a row whose slack is NaN is counted in n_nan and takes part in nothing else; the worst rows are in
  ascending (slack, batch row) order - a total order.
"""
import functools
import math

import numpy as np
import torch

from . import lib, ops

K_MAX = 64
BINS_MAX = 64


def group_rows(design_of_row, B):
    """(design_ptr [B + 1], design_rows [T]) as int32 numpy arrays: the batch rows of design b are
    design_rows[design_ptr[b]:design_ptr[b + 1]], in ascending row order (a stable grouping); a design may be empty.
    On the host, once per selection."""
    d = np.asarray(design_of_row).astype(np.int64).reshape(-1)
    if d.size and (d.min() < 0 or d.max() >= B):
        raise ValueError(f'group_rows: design index outside [0, {B})')
    rows = np.argsort(d, kind='stable').astype(np.int32)
    ptr = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(np.bincount(d, minlength=B), out=ptr[1:])
    return ptr, rows


class SlackRows:
    """The slack inputs of a selection's rows, stated once for everything that forms slacks per design (the report, the
    criticality, the trial moves, evaluate.timing_report): SlackRows(selection, batch) has
      required     fp32 [T] on the device, Selection.required_times(batch): one gather, made here
      design       host int64 [T], Selection.design; B, T
      groups       (design_ptr, design_rows) of `group_rows`, int32 on the device
      rows_of(i)   design i's rows, ascending: the slice design_rows[ptr[i]:ptr[i + 1]], a view
      row_design   int32 [T] on the device, None when B == 1 (every row belongs to design 0): what the criticality kernels take
    `groups` and `row_design` are uploaded once, on first use - who launches on them from a captured graph touches them when it
    is built.  `from_rows` builds the same from a design vector and any `required` tensor, a CPU one included."""

    def __init__(self, selection, batch):
        self._fill(selection.design, batch.B, selection.required_times(batch))

    @classmethod
    def from_rows(cls, design, B, required):
        self = cls.__new__(cls)
        self._fill(design, B, required)
        return self

    def _fill(self, design, B, required):
        self.design, self.B, self.T, self.required = design, int(B), int(required.numel()), required

    def _put(self, a):
        return torch.from_numpy(a).to(self.required.device)

    @functools.cached_property
    def _grouped(self):
        ptr, rows = group_rows(self.design, self.B)
        return ptr.tolist(), (self._put(ptr), self._put(rows))

    @property
    def groups(self):
        return self._grouped[1]

    def rows_of(self, i):
        cuts, (_, rows) = self._grouped
        return rows[cuts[i]:cuts[i + 1]]

    @functools.cached_property
    def row_design(self):
        return self._put(np.asarray(self.design).astype(np.int32)) if self.B > 1 else None

    @staticmethod
    def require_regression(pmodel, who):
        """ValueError unless the model's head is the regression head: a slack needs ONE predicted arrival time per row."""
        nlabels = pmodel.mlp_fuse.layers[-1].out_features
        if nlabels != 1:
            raise ValueError(f'{who} needs the regression head (nlabels = 1), the model has {nlabels} labels')


def _hist_args(hist):
    if hist is None:
        return 0.0, 0.0, 0
    lo, hi, nbins = float(hist[0]), float(hist[1]), int(hist[2])
    if nbins == 0:
        return 0.0, 0.0, 0
    if not (math.isfinite(lo) and math.isfinite(hi) and np.float32(lo) < np.float32(hi)) or not 1 <= nbins <= BINS_MAX:
        raise ValueError(f'timing_report: hist = (lo, hi, nbins) needs finite lo < hi and 1 <= nbins <= {BINS_MAX}, got {hist}')
    return lo, hi, nbins


def workspace_bytes(T, B, k, hist=None):
    return lib.ext('mmft_timing_report_workspace_bytes', int(T), int(B), int(k), _hist_args(hist)[2])


class ReportBuffers:
    """The output buffers of `reports` launches with the same (B, k, hist), carved out of ONE byte buffer so that `host()` is
    one device->host copy: per report summary [B, 6] fp64, worst_row [B, k] int32, worst_slack [B, k] fp32 and
    hist [B, nbins + 2] int32 (None without a histogram)."""

    def __init__(self, B, k, hist, device, reports=1):
        nbins = _hist_args(hist)[2]
        self.B, self.k, self.nh, self.reports = int(B), int(k), (nbins + 2 if nbins else 0), int(reports)
        self._fields = (('f8', 6), ('i4', self.k), ('f4', self.k)) + ((('i4', self.nh),) if self.nh else ())
        self.report_bytes = (self.B * (48 + 8 * self.k + 4 * self.nh) + 7) // 8 * 8       # fp64 first: every report 8-byte aligned
        self.raw = torch.empty(self.reports * self.report_bytes, dtype=torch.uint8, device=device)

    def tensors(self, i=0):
        """(summary, worst_row, worst_slack, hist) of report i: views of the one buffer."""
        out, pos = [], i * self.report_bytes
        for dt, cols in self._fields:
            nb = self.B * cols * int(dt[1])
            tdt = {'f8': torch.float64, 'i4': torch.int32, 'f4': torch.float32}[dt]
            out.append(self.raw[pos:pos + nb].view(tdt).view(self.B, cols))
            pos += nb
        return tuple(out) if self.nh else tuple(out) + (None,)

    def host(self):
        """One device->host copy -> per report the four numpy arrays (`decode` takes them)."""
        a = self.raw.cpu().numpy()
        res = []
        for i in range(self.reports):
            out, pos = [], i * self.report_bytes
            for dt, cols in self._fields:
                nb = self.B * cols * int(dt[1])
                out.append(a[pos:pos + nb].view(dt).reshape(self.B, cols))
                pos += nb
            res.append(tuple(out) if self.nh else tuple(out) + (None,))
        return res


def timing_report(pred, required, design_ptr, design_rows, k, hist=None, out=None, workspace=None):
    """Launch the report kernel on the current stream -> (summary, worst_row, worst_slack, hist) on the device (hist None
    without a histogram); `decode` turns their host copies into per-design dicts.

    pred, required             fp32 CUDA, contiguous 1-D, T rows each
    design_ptr, design_rows    int32 CUDA tensors of B + 1 and T entries (group_rows)
    k                          1 .. 64 worst endpoints per design;  hist = (lo, hi, nbins), nbins <= 64, or None
    out, workspace             buffers the caller owns (ReportBuffers.tensors(); a CUDA tensor of workspace_bytes bytes):
                               a captured launch needs static ones.  Without `workspace` the scratch comes from lib.workspace,
                               which never grows during a capture."""
    for t, nm in ((pred, 'pred'), (required, 'required')):
        ops._chk(t, nm)
        if t.dim() != 1 or not t.is_contiguous() or t.numel() != pred.numel():
            raise ValueError(f'timing_report: {nm} must be a contiguous 1-D tensor of the prediction length')
    T = pred.numel()
    ops._idx(design_rows, 'design_rows', T)
    ops._idx(design_ptr, 'design_ptr')
    B = design_ptr.numel() - 1
    k = int(k)
    lo, hi, nbins = _hist_args(hist)
    if not 1 <= k <= K_MAX or B < 1 or T < 1:
        raise ValueError(f'timing_report: need 1 <= k <= {K_MAX}, at least one design and one row (k {k}, B {B}, T {T})')
    if out is None:
        out = ReportBuffers(B, k, hist, pred.device).tensors()
    summary, worst_row, worst_slack, h = out
    for t, nm, dt, shape in ((summary, 'summary', torch.float64, (B, 6)), (worst_row, 'worst_row', torch.int32, (B, k)),
                             (worst_slack, 'worst_slack', torch.float32, (B, k))) + \
            (((h, 'hist', torch.int32, (B, nbins + 2)),) if nbins else ()):
        ops._chk(t, nm, dt)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f'timing_report: {nm} must be a contiguous {dt} tensor of shape {shape}')
    need = lib.ext('mmft_timing_report_workspace_bytes', T, B, k, nbins)
    if workspace is None:
        workspace = lib.workspace(pred.device, need)
    elif not (torch.is_tensor(workspace) and workspace.is_cuda and workspace.is_contiguous()):
        raise ValueError('timing_report: workspace must be a contiguous CUDA tensor')
    dev, st = lib.stream_args(pred)
    lib.ext('mmft_timing_report', pred, required, design_ptr, design_rows, T, B, k, lo, hi, nbins, summary, worst_row,
            worst_slack, h if nbins else None, workspace, workspace.numel() * workspace.element_size(), dev, st)
    return summary, worst_row, worst_slack, (h if nbins else None)


def decode(summary, worst_row, worst_slack, hist, endpoints=None):
    """Host copies of the four buffers -> one dict per design: n, n_nan, violations, wns (None without a valid row), wns_row,
    tns, worst = [(row, slack), ...] without the padding, hist (a list, or None); with `endpoints` (the batch rows' endpoint
    ids in the caller's numbering) also wns_endpoint and worst_endpoints."""
    summary, worst_row, worst_slack = np.asarray(summary), np.asarray(worst_row), np.asarray(worst_slack)
    out = []
    for b in range(summary.shape[0]):
        n, n_nan, viol, wns, wrow, tns = summary[b]
        keep = worst_row[b] >= 0
        d = dict(n=int(n), n_nan=int(n_nan), violations=int(viol), wns=float(wns) if n > 0 else None, wns_row=int(wrow),
                 tns=float(tns), worst=[(int(r), float(s)) for r, s in zip(worst_row[b][keep], worst_slack[b][keep])],
                 hist=[int(c) for c in np.asarray(hist)[b]] if hist is not None else None)
        if endpoints is not None:
            d['wns_endpoint'] = int(endpoints[d['wns_row']]) if d['wns_row'] >= 0 else None
            d['worst_endpoints'] = [int(endpoints[r]) for r, _ in d['worst']]
        out.append(d)
    return out


class AfterHead:
    """What Predictor runs on its predictions after the head, as one object per option: built from the predictor -
    all validation and every static buffer there, nothing launched -, then `launch(pred)` on the current stream inside every
    eager or capturing predict(), which sets `ready`, and `result(...)`, the decode of the last call's buffers in one
    device->host copy.  The Predictor keeps the object alive with its replayed graph."""
    ready = False

    def check_ready(self, what):
        if not self.ready:
            raise RuntimeError(f'{what}: predict() has not run yet')


class PredictorReport(AfterHead):
    """Predictor(report=dict(k=32, hist=(lo, hi, nbins) or None)): the report kernel on every predict()'s output and the rows'
    slack inputs (predictor.slack); the output buffers and the scratch are static, as a replayed launch needs them."""

    def __init__(self, predictor, spec):
        unknown = set(spec) - {'k', 'hist'}
        if unknown:
            raise ValueError(f'Predictor: report= takes k and hist, got {sorted(unknown)}')
        s = self.slack = predictor.slack
        s.require_regression(predictor.pmodel, 'Predictor: report=')
        self.k, self.hist, self.endpoints = int(spec.get('k', 32)), spec.get('hist'), predictor.endpoints
        self.design_ptr, self.design_rows = s.groups
        self.bufs = ReportBuffers(s.B, self.k, self.hist, predictor.device)
        self.scratch = torch.empty((workspace_bytes(s.T, s.B, self.k, self.hist) + 7) // 8, dtype=torch.int64, device=predictor.device)

    def launch(self, pred):
        timing_report(pred.contiguous(), self.slack.required, self.design_ptr, self.design_rows, self.k, self.hist,
                      out=self.bufs.tensors(), workspace=self.scratch)
        self.ready = True

    def result(self):
        return decode(*self.bufs.host()[0], endpoints=self.endpoints)


def reference_slack(pred, required):
    """fp32 slack as the kernel forms it: one fp32 subtraction, + 0.0f (-0.0 -> +0.0)."""
    with np.errstate(invalid='ignore'):
        return (np.asarray(required, dtype=np.float32) - np.asarray(pred, dtype=np.float32)) + np.float32(0.0)


def reference_report(pred, required, design_ptr, design_rows, k, hist=None):
    """The kernel's contract restated in numpy / fp64 from host arrays -> (summary, worst_row, worst_slack, hist) in the
    layout of the device buffers (hist None without a histogram): np.lexsort((row, slack)) for the order, math.fsum for
    TNS, np.floor for the bins."""
    design_ptr, design_rows = np.asarray(design_ptr), np.asarray(design_rows)
    B = design_ptr.shape[0] - 1
    lo, hi, nbins = _hist_args(hist)
    slack = reference_slack(pred, required)
    summary = np.zeros((B, 6), dtype=np.float64)
    worst_row = np.full((B, k), -1, dtype=np.int32)
    worst_slack = np.full((B, k), np.inf, dtype=np.float32)
    h = np.zeros((B, nbins + 2), dtype=np.int32) if nbins else None
    for b in range(B):
        rows = design_rows[design_ptr[b]:design_ptr[b + 1]].astype(np.int64)
        s = slack[rows]
        valid = ~np.isnan(s)
        rows, s = rows[valid], s[valid]
        order = np.lexsort((rows, s))                                  # ascending slack, the smaller row first on a tie
        m = min(k, rows.shape[0])
        worst_row[b, :m], worst_slack[b, :m] = rows[order[:m]], s[order[:m]]
        neg = s < 0
        summary[b] = (rows.shape[0], int((~valid).sum()), int(neg.sum()), s[order[0]] if m else np.nan,
                      rows[order[0]] if m else -1, math.fsum(float(v) for v in s[neg]))
        if nbins:
            lo32, hi32 = np.float32(lo), np.float32(hi)
            w = (hi32 - lo32) / np.float32(nbins)
            mid = s[(s >= lo32) & (s < hi32)]
            bins = 1 + np.minimum(nbins - 1, np.floor((mid - lo32) / w).astype(np.int64))
            h[b] = np.bincount(bins, minlength=nbins + 2)
            h[b, 0], h[b, nbins + 1] = int((s < lo32).sum()), int((s >= hi32).sum())
    return summary, worst_row, worst_slack, h
