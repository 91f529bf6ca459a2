"""On-device evaluation of the hot path: the validate() / test() forward (src/train.py:137-291, src/test.py:124-318)
with every metric the reference prints derived from ONE fp64 sums kernel and one device->host copy, instead of
the reference's seven `.item()` syncs per batch (src/train.py:525-541).

As in the reference, modules stay in train mode by default (BatchNorm uses batch statistics and updates its running
stats: SURVEY D5) and the whole design is evaluated as one batch over all of its paths (src/train.py:188,
src/test.py:176).  `frozen_stats=True` is the inference variant the reference's scripts do not have: the CNN is put in
eval mode for the call, so BatchNorm normalises with its running statistics and the model is left untouched.
`endpoint_slack_mae` = mean |(required - y_hat) - (required - arrival)| = mean |y_hat - arrival| is the accuracy
metric BASELINE.json names.
"""
import contextlib

import numpy as np
import torch
from . import lib, ops


@contextlib.contextmanager
def frozen_statistics(cnn, on=True):
    """with frozen_statistics(cnn): ...  - the CNN in eval mode (BatchNorm from its running statistics, nothing written),
    every module back in the mode it was in afterwards, also when the body raises."""
    if not on or cnn is None:
        yield cnn
        return
    modes = [(m, m.training) for m in cnn.modules()]
    cnn.eval()
    try:
        yield cnn
    finally:
        for m, was in modes:
            m.training = was


def eval_sums(pred, arrival, required, label):
    for t, nm in ((pred, 'pred'), (arrival, 'arrival'), (required, 'required'), (label, 'label')):
        ops._chk(t, nm)
        if t.dim() != 1 or not t.is_contiguous() or t.numel() != pred.numel():
            raise ValueError(f'eval_sums: {nm} must be a contiguous 1-D tensor of the prediction length')
    out = torch.empty(10, dtype=torch.float64, device=pred.device)
    dev, st = lib.stream_args(pred)
    lib.call('mmft_eval_sums', pred, arrival, required, label, pred.numel(), out, dev, st)
    return out


def metrics_from_sums(s):
    """s: the 10 sums of mmft_eval_sums (host floats). Same formulas as src/train.py:230-278 / torchmetrics R2Score."""
    n, sy, syy, sse, sae, sape, tp, fp, tn, fn = [float(v) for v in s]
    ss_tot = syy - sy * sy / n
    recall = tp / (tp + fn) if tp else 0.0
    precision = tp / (tp + fp) if tp else 0.0
    f1 = 2 * recall * precision / (recall + precision) if (precision or recall) else 0.0
    return dict(n=int(n), loss=sse / n, r2=1.0 - sse / ss_tot if ss_tot > 0 else float('nan'),
                endpoint_slack_mae=sae / n, mape=sape / n, acc=(tp + tn) / n, recall=recall, precision=precision,
                f1=f1, tp=int(tp), fp=int(fp), tn=int(tn), fn=int(fn))


def eval_sums_by_level(pred, arrival, required, label, level, num_levels):
    """[num_levels, 10] fp64 sums, one row per topological level (mmft_eval_sums_by_level)."""
    for t, nm in ((pred, 'pred'), (arrival, 'arrival'), (required, 'required'), (label, 'label')):
        ops._chk(t, nm)
        if t.dim() != 1 or not t.is_contiguous() or t.numel() != pred.numel():
            raise ValueError(f'eval_sums_by_level: {nm} must be a contiguous 1-D tensor of the prediction length')
    ops._idx(level, 'level', pred.numel())
    out = torch.empty((num_levels, 10), dtype=torch.float64, device=pred.device)
    dev, st = lib.stream_args(pred)
    lib.call('mmft_eval_sums_by_level', pred, arrival, required, label, level, pred.numel(), int(num_levels), out, dev, st)
    return out


def level_metrics_from_sums(rows):
    """Per-level R2 / MAPE as src/test.py:211-216 prints them (levels with >= 2 predictions), from the [L, 10] sums."""
    out = []
    for l, srow in enumerate(rows):
        n = int(srow[0])
        if n < 2:
            continue
        m = metrics_from_sums(srow)
        out.append(dict(level=l, n=n, r2=m['r2'], mape=m['mape'], mae=m['endpoint_slack_mae']))
    return out


@torch.no_grad()
def validate(train_step, path_ids_per_design=None, per_level=False, frozen_stats=False, per_design=False):
    """Forward over all (or the given) paths of the designs held by `train_step` (a mmft.train.TrainStep) and
    return the metric dict; per_level=True adds 'levels': R2 / MAPE of every topological level (src/test.py:211-216).
    One device->host copy.  frozen_stats=False (default) is the reference's behaviour: the modules stay in train mode
    (SURVEY D5).  frozen_stats=True: the CNN runs in eval mode for this call (running statistics, no buffer written) and is
    returned to the mode it was in.

    per_design=True adds 'designs': one metric dict per design of the batch - what the reference reports per case and
    averages over the cases (src/train.py:280-290, src/test.py:283-313) - from the SAME forward.  Task 'reg': one more
    mmft_eval_sums_by_level launch keyed by each row's design index (with per_level a second one keyed by design and
    level, for each design's 'levels'); the sums ride in the one device->host copy.  Task 'cls' has no keyed sums kernel:
    the pooled call is followed by one call per design with the other designs' path lists empty - correct, but B more
    forwards (and, unless frozen_stats, B more updates of the BatchNorm running statistics)."""
    b = train_step.batch
    if path_ids_per_design is None:
        path_ids_per_design = [np.arange(d.num_paths) for d in b.designs]
    if per_design and getattr(train_step, 'task', 'reg') == 'cls':
        m = validate(train_step, path_ids_per_design, per_level=per_level, frozen_stats=frozen_stats)
        empty = np.zeros(0, dtype=np.int64)
        m['designs'] = [validate(train_step, [ids if j == i else empty for j, ids in enumerate(path_ids_per_design)],
                                 per_level=per_level, frozen_stats=frozen_stats) if len(path_ids_per_design[i]) else dict(n=0)
                        for i in range(b.B)]
        return m
    sel = b.select(path_ids_per_design)
    with frozen_statistics(train_step.cnn, frozen_stats):
        hats, ends_d, _ = train_step.forward(path_ids_per_design, _sel=sel)
    idx = ends_d.long()
    arrival = b.arrival[idx].squeeze(-1).contiguous()
    required = b.required[idx].squeeze(-1).contiguous()
    label = b.graph.ndata['label'][idx].squeeze(-1).to(torch.float32).contiguous()
    hats = hats.contiguous()
    if getattr(train_step, 'task', 'reg') == 'cls':
        # classification task (src/train.py:516-518,536-549): CrossEntropy + argmax prediction, positive = class != 0
        from .fusion import cls_eval_sums
        labels = b.graph.ndata['label'][idx].squeeze(-1).contiguous()
        n, lsum, tp, fp, tn, fn = [float(v) for v in cls_eval_sums(hats, labels).cpu().tolist()]
        recall = tp / (tp + fn) if tp else 0.0
        precision = tp / (tp + fp) if tp else 0.0
        f1 = 2 * recall * precision / (recall + precision) if (precision or recall) else 0.0
        return dict(n=int(n), loss=lsum / n, r2=0.0, acc=(tp + tn) / n, recall=recall, precision=precision, f1=f1,
                    tp=int(tp), fp=int(fp), tn=int(tn), fn=int(fn))
    if per_design:
        return _validate_per_design(b, sel, hats, arrival, required, label, per_level)
    if not per_level:
        return metrics_from_sums(eval_sums(hats, arrival, required, label).cpu().tolist())
    both = torch.cat([eval_sums(hats, arrival, required, label).reshape(1, 10),
                      eval_sums_by_level(hats, arrival, required, label, sel.levels.contiguous(), b.L)], 0).cpu().tolist()
    m = metrics_from_sums(both[0])
    m['levels'] = level_metrics_from_sums(both[1:])
    return m


def _validate_per_design(b, sel, hats, arrival, required, label, per_level):
    """The 'reg' tail of validate(per_design=True): pooled sums [1], per-level sums [L] (per_level), per-design sums [B],
    per-design-and-level sums [B * L] (per_level) - one concatenation, one device->host copy."""
    B, L = b.B, b.L
    design = torch.div(sel.feat_off, b.P, rounding_mode='floor').to(torch.int32).contiguous()      # on the device: no upload
    parts = [eval_sums(hats, arrival, required, label).reshape(1, 10)]
    if per_level:
        parts.append(eval_sums_by_level(hats, arrival, required, label, sel.levels.contiguous(), L))
    parts.append(eval_sums_by_level(hats, arrival, required, label, design, B))
    if per_level:
        parts.append(eval_sums_by_level(hats, arrival, required, label, (design * L + sel.levels).contiguous(), B * L))
    rows = torch.cat(parts, 0).cpu().tolist()
    m = metrics_from_sums(rows[0])
    pos = 1
    if per_level:
        m['levels'] = level_metrics_from_sums(rows[pos:pos + L])
        pos += L
    m['designs'] = [metrics_from_sums(r) if r[0] > 0 else dict(n=0) for r in rows[pos:pos + B]]
    pos += B
    if per_level:
        for i, dm in enumerate(m['designs']):
            if dm['n']:
                dm['levels'] = level_metrics_from_sums(rows[pos + i * L:pos + (i + 1) * L])
    return m


@torch.no_grad()
def timing_report(train_step, path_ids_per_design=None, k=32, hist=None, frozen_stats=False):
    """What a timing engine prints, for the model and for the truth: one forward as validate() runs it, then the report
    kernel (mmft.report) twice over the same rows - on the predictions and on the true arrival times - and ONE device->host
    copy.  Per design a dict with
      predicted, actual   the two reports (mmft.report.decode: n, n_nan, violations, wns, wns_row, tns, worst, hist, ...;
                          rows are rows of the forward's output, endpoints the batch's node ids)
      wns_error, tns_error   predicted - actual (None for a design without a valid row)
      topk_overlap        |worst-k rows predicted & worst-k rows actual| / min(k, valid rows) (None without a valid row)
    Regression task only."""
    from . import report as R
    if getattr(train_step, 'task', 'reg') != 'reg':
        raise ValueError('timing_report: the regression task only')
    b = train_step.batch
    if path_ids_per_design is None:
        path_ids_per_design = [np.arange(d.num_paths) for d in b.designs]
    if not sum(len(p) for p in path_ids_per_design):
        raise ValueError('timing_report: no path selected')
    sel = b.select(path_ids_per_design)
    with frozen_statistics(train_step.cnn, frozen_stats):
        hats, ends_d, _ = train_step.forward(path_ids_per_design, _sel=sel)
    arrival = b.arrival[ends_d.long()].reshape(sel.T).contiguous()
    slack = R.SlackRows(sel, b)
    bufs = R.ReportBuffers(b.B, k, hist, hats.device, reports=2)
    R.timing_report(hats.contiguous(), slack.required, *slack.groups, k, hist, out=bufs.tensors(0))
    R.timing_report(arrival, slack.required, *slack.groups, k, hist, out=bufs.tensors(1))
    predicted, actual = (R.decode(*h, endpoints=np.asarray(sel.endpoints)) for h in bufs.host())
    out = []
    for p, a in zip(predicted, actual):
        m = min(int(k), p['n'], a['n'])
        both = len({r for r, _ in p['worst']} & {r for r, _ in a['worst']})
        out.append(dict(predicted=p, actual=a, wns_error=p['wns'] - a['wns'] if m else None,
                        tns_error=p['tns'] - a['tns'] if m else None, topk_overlap=both / m if m else None))
    return out


def validate_designs(pmodel, cnn, designs, device, per_level=True, mode='sweep', frozen_stats=False):
    """The per-design loop of validate() / test() (src/train.py:137-291, src/test.py:124-318): every design is evaluated
    on its own as ONE batch over all of its paths (modules stay in train mode, SURVEY D5, unless frozen_stats=True puts
    the CNN in eval mode for each call), the reference's per-case line
    (loss, r2, acc, recall, precision, F1 + per-level R2 / MAPE) is returned per design together with the averages over
    the designs that the loops print at the end (src/train.py:280-290)."""
    from .train import TrainStep
    cases = []
    # (TrainStep puts the modules in train mode, as the reference's loops have them; with frozen_stats the CNN is handed
    # back in the mode it came in, also on an exception)
    modes = [(m, m.training) for m in cnn.modules()] if (frozen_stats and cnn is not None) else []
    try:
        for d in designs:
            ts = TrainStep(pmodel, cnn, [d], device, mode=mode, overlap=False, with_optimizer=False)
            cases.append(validate(ts, per_level=per_level, frozen_stats=frozen_stats))
    finally:
        for m, was in modes:
            m.training = was
    keys = ('loss', 'r2', 'acc', 'recall', 'precision', 'f1', 'endpoint_slack_mae', 'mape')
    overall = {k: float(np.mean([c[k] for c in cases])) for k in keys} if cases else {}
    return dict(cases=cases, overall=overall)
