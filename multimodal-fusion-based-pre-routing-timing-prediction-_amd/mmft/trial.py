"""Exact predictions for a batch of trial pin moves (include/mmft_trial.h).

A pin's coordinates feed the path masks and nothing else, so a trial move changes the prediction only on the rows whose path
holds a moved pin, and on those rows only the h_cnn columns of the head's input.  Predictor(placement=True, trials=True) keeps
what its last predict() handed to the head; `trial_moves` re-projects the affected rows under each candidate, runs the head
over them and reduces each candidate's WNS / TNS - without writing the placement, h or anything predict() returns.

    rows_of_pin        the static incidence of a selection: pin -> rows of `pred` (from placement.pin_incidence_host)
    check_moves        host validation of (pins, pin_x, pin_y, cand_ptr)
    expand_candidates  the (row, candidate) pairs of a call: per candidate the union of its pins' rows, vectorised
    reduce_host        mmft_trial_reduce restated in numpy, in the kernel's summation order
    prepare / launch / fetch   the three stages of a call (host expansion and upload, three launches, one copy back);
                       trial_moves runs them one after another, tools/bench_placement.py times them apart

The entry points are bound by `abi`, an accessor of this module: the table of mmft.lib's accessors is pinned by its own ledger
and is not touched here.
"""
import numpy as np
import torch

from . import functional as MF
from . import lib
from . import placement as PL
from .report import AfterHead, reference_slack

abi = lib.Header('mmft_trial.h')         # trial moves: rows under a candidate's overrides, per-candidate WNS / TNS
abi_decls = abi.decls

MAX_MOVES = 64                           # moves of one candidate (the kernel stages them in LDS)
FIELDS = ('n', 'n_nan', 'violations', 'wns', 'wns_row', 'tns')


# ------------------------------------------------------------------------------------------------ host side
def rows_of_pin(path_nodes, path_lens, paths, maxlen, n_nodes):
    """(ptr int64 [n_nodes + 1], rows int64 [nnz]): per pin (the tables' numbering) the rows of `pred` whose path holds it,
    ascending, each once.  placement.pin_incidence_host lists the slots t * maxlen + j of a pin's FIRST occurrence per row, so
    the row is slot // maxlen and no row repeats.  Static: the selection and the paths' nodes do not move."""
    ptr, slot = PL.pin_incidence_host(path_nodes, path_lens, paths, n_nodes)
    return ptr, slot // int(maxlen)


def _host(a, name, kinds, who='trial_moves'):
    """`a` (numpy array or tensor) as a host numpy array of one of the dtypes `kinds`, 1-D; `who` names the caller's method."""
    h = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    if not isinstance(h, np.ndarray) or h.dtype not in kinds:
        raise TypeError(f'{who}: {name} must be a numpy array or tensor of {" or ".join(np.dtype(k).name for k in kinds)}, '
                        f'got {getattr(h, "dtype", type(a).__name__)}')
    if h.ndim != 1:
        raise ValueError(f'{who}: {name} must be 1-D, got shape {h.shape}')
    return h


def check_pin_sets(n_nodes, pins, ptr=None, who='trial_moves', ptr_name='cand_ptr', unit='candidate', item='moves'):
    """(pins int64 [M], ptr int64 [K + 1]) or an exception: the part of `check_moves` that has no coordinates - sets of at most
    MAX_MOVES distinct pins, CSR over `pins`; None: every pin a set of its own.  search.check_groups is this under its own names."""
    pins = _host(pins, 'pins', (np.int64,), who)
    M = pins.shape[0]
    if M and (int(pins.min()) < 0 or int(pins.max()) >= n_nodes):
        raise IndexError(f'{who}: pins outside the design\'s {n_nodes} nodes')
    if ptr is None:
        ptr = np.arange(M + 1, dtype=np.int64)
    else:
        ptr = _host(ptr, ptr_name, (np.int64,), who)
        if ptr.shape[0] < 1 or int(ptr[0]) != 0:
            raise ValueError(f'{who}: {ptr_name} must start at 0')
        if (np.diff(ptr) < 0).any():
            raise ValueError(f'{who}: {ptr_name} must not decrease')
        if int(ptr[-1]) != M:
            raise ValueError(f'{who}: {ptr_name} must end at the number of {item}, {M}, got {int(ptr[-1])}')
        if ptr.shape[0] > 1 and int(np.diff(ptr).max()) > MAX_MOVES:
            raise ValueError(f'{who}: a {unit} holds {int(np.diff(ptr).max())} {item}, at most {MAX_MOVES} are supported')
        cand = np.repeat(np.arange(ptr.shape[0] - 1, dtype=np.int64), np.diff(ptr))
        if np.unique(cand * max(int(n_nodes), 1) + pins).shape[0] != M:
            raise ValueError(f'{who}: the same pin twice in one {unit}')
    return np.ascontiguousarray(pins), np.ascontiguousarray(ptr)


def check_moves(n_nodes, pins, pin_x, pin_y, cand_ptr=None):
    """(pins int64 [M], x int32 [M], y int32 [M], cand_ptr int64 [K + 1]) or an exception; host only, no device is touched.
    TypeError for a wrong type or dtype, IndexError for a pin outside [0, n_nodes), ValueError for everything else: shapes,
    coordinates beyond 32 bits, a cand_ptr that does not start at 0 / decreases / does not end at M, a candidate of more than
    MAX_MOVES moves, a pin twice in one candidate."""
    M = _host(pins, 'pins', (np.int64,)).shape[0]
    xy = []
    for name, a in (('pin_x', pin_x), ('pin_y', pin_y)):
        h = _host(a, name, (np.int32, np.int64))
        if h.shape != (M,):
            raise ValueError(f'trial_moves: {name} has shape {h.shape} for {M} pins')
        if h.dtype == np.int64 and M and (int(h.max()) >= 2 ** 31 or int(h.min()) < -2 ** 31):
            raise ValueError(f'trial_moves: {name} does not fit 32-bit integers')
        xy.append(h.astype(np.int32))
    pins, ptr = check_pin_sets(n_nodes, pins, cand_ptr)
    return pins, xy[0], xy[1], ptr


def expand_candidates(rows_of_pin, node_off, pins, cand_ptr):
    """(pair_ptr int64 [K + 1], pair_row int64 [n_pairs], pair_cand int64 [n_pairs]): per candidate k the union of the rows of
    its pins - pins[cand_ptr[k]:cand_ptr[k + 1]], the design's own node ids, + node_off in the tables' numbering -, ascending,
    each row once; the candidates one after another.  rows_of_pin = (ptr, rows) as `rows_of_pin` returns them.  Vectorised:
    one gather of the pins' row lists, one sort of (candidate, row) keys."""
    ptr, rows = rows_of_pin
    pins, cand_ptr = np.asarray(pins, dtype=np.int64), np.asarray(cand_ptr, dtype=np.int64)
    K = cand_ptr.shape[0] - 1
    g = pins + int(node_off)
    start, count = ptr[g], ptr[g + 1] - ptr[g]
    total = int(count.sum())
    first = np.cumsum(count) - count                                   # where each move's rows start in the flat list
    flat = np.arange(total, dtype=np.int64) - np.repeat(first - start, count)
    cand = np.repeat(np.repeat(np.arange(K, dtype=np.int64), np.diff(cand_ptr)), count)
    span = int(rows.max()) + 1 if rows.size else 1
    key = np.unique(cand * span + rows[flat])                          # sorted: by candidate, then by row; a shared row once
    pair_cand, pair_row = key // span, key % span
    pair_ptr = np.zeros(K + 1, dtype=np.int64)
    np.cumsum(np.bincount(pair_cand, minlength=K), out=pair_ptr[1:])
    return pair_ptr, pair_row, pair_cand


def _tree_sum(terms_by_thread):
    """The fp64 sum of mmft_trial_reduce: [256] per-thread sums -> lanes of a wave combined by s = s + s[lane ^ o] for
    o = 32 .. 1 (every lane ends with the same bits: fp addition commutes), the four waves added in order to 0.0."""
    v = np.asarray(terms_by_thread, dtype=np.float64).reshape(4, 64).copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    total = np.float64(0.0)
    for w in range(4):
        total = total + v[w, 0]
    return total


def reduce_host(pred_base, required, design_rows, pair_ptr, pair_row, pred_trial):
    """summary float64 [K + 1, 6] of mmft_trial_reduce (n_valid, n_nan, n_violating, wns, wns_row, tns; entry K the base) from
    host arrays: the slack rule of mmft_report.h, the smallest row on equal slack, and tns in the kernel's order - thread j of
    256 adds its rows design_rows[j::256] in ascending order, then `_tree_sum`."""
    pred_base, required = np.asarray(pred_base, dtype=np.float32), np.asarray(required, dtype=np.float32)
    design_rows = np.asarray(design_rows, dtype=np.int64)
    pair_ptr, pair_row = np.asarray(pair_ptr, dtype=np.int64), np.asarray(pair_row, dtype=np.int64)
    pred_trial = np.asarray(pred_trial, dtype=np.float32)
    K, n, T = pair_ptr.shape[0] - 1, design_rows.shape[0], pred_base.shape[0]
    inside = (design_rows >= 0) & (design_rows < T)
    safe = np.where(inside, design_rows, 0)
    out = np.zeros((K + 1, 6), dtype=np.float64)
    for k in range(K + 1):
        pred = pred_base.copy()
        if k < K:
            pred[pair_row[pair_ptr[k]:pair_ptr[k + 1]]] = pred_trial[pair_ptr[k]:pair_ptr[k + 1]]
        s = np.where(inside, reference_slack(pred[safe], required[safe]), np.float32(np.nan)).astype(np.float32)
        valid = ~np.isnan(s)
        neg = valid & (s < 0)
        per_thread = np.zeros(256, dtype=np.float64)
        for j in range(min(256, n)):
            acc = np.float64(0.0)
            for v in s[j::256][neg[j::256]]:
                acc = acc + np.float64(v)
            per_thread[j] = acc
        if valid.any():
            order = np.lexsort((design_rows[valid], s[valid]))
            wns, wrow = float(s[valid][order[0]]), float(design_rows[valid][order[0]])
        else:
            wns, wrow = np.nan, -1.0
        out[k] = (int(valid.sum()), int((~valid).sum()), int(neg.sum()), wns, wrow, _tree_sum(per_thread))
    return out


def decode(summary):
    """summary rows [m, 6] -> dict of arrays: n, n_nan, violations, wns_row (int64), wns, tns (float64; wns NaN without a valid
    row)."""
    s = np.asarray(summary, dtype=np.float64).reshape(-1, 6)
    return dict(n=s[:, 0].astype(np.int64), n_nan=s[:, 1].astype(np.int64), violations=s[:, 2].astype(np.int64), wns=s[:, 3].copy(),
                wns_row=s[:, 4].astype(np.int64), tns=s[:, 5].copy())


# ------------------------------------------------------------------------------------------------ the Predictor's side
class TrialState(AfterHead):
    """What Predictor(trials=True) keeps for trial_moves: the static incidence of its selection and `kept` - the head's input
    x, the prefix table GP and pred of the latest eager or capturing predict() (a replay rewrites those same buffers), the math
    mode they were made in.  The rows of each design and their required times are predictor.slack's (rows_of(i), required).
    `stale`: an update() has run that no predict() has followed; `fresh()`: a predict() has."""

    def __init__(self, predictor):
        p = predictor
        placed, sel = p._placed, p._sel
        paths = sel.paths.cpu().numpy().astype(np.int64)
        self.rows_of_pin = rows_of_pin(placed.nodes.cpu().numpy(), placed.lens.cpu().numpy(), paths, placed.maxlen,
                                       int(placed.node_off[-1]))
        p.slack.groups                                       # uploaded here: no trial_moves call pays for it
        self.kept, self.stale = {}, False

    def fresh(self):
        """A predict() has completed: what trial_moves keeps is that of the resident designs again."""
        self.ready, self.stale = True, False


def _refuse_mode(p, who='trial_moves'):
    """ValueError unless the kept predict() and this call are what the bitwise contract covers: bf16 math mode, the
    regression head, the fused head kernel, h_cnn in the head's input."""
    st = p._trial
    x, mods = st.kept.get('x'), list(p.pmodel.mlp_fuse.layers)
    if st.kept.get('mode') != 'bf16' or lib.get_math_mode() != 'bf16':
        raise ValueError(f'{who}: bf16 math mode only (the generic fp32 layers do not promise the same bits for a row in '
                         f'another batch); predict() and {who}() must both run in it')
    p.slack.require_regression(p.pmodel, who)
    if len(mods) != 3 or x is None or st.kept.get('cnn_col') is None or st.kept.get('GP') is None or \
            not MF.head_mlp_usable(x, mods[0].weight, mods[0].bias, mods[2].weight, mods[2].bias, p.pmodel.mlp_fuse.negative_slope):
        raise ValueError(f'{who} needs the fused head (mmft_head_mlp_supported: 288 -> 576 -> 1, ReLU) over a head input '
                         'that holds h_cnn')
    if x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16:
        raise ValueError(f'{who}: the head\'s input rows are not 16-byte aligned')


def check_state(p, who='trial_moves', why='the pair list is host work done per call'):
    """The state and mode refusals of a call that reads what predict() kept (trial_moves, search_moves): RuntimeError without
    trials=True, under an outer stream capture, before the first predict() and after an update() no predict() has followed;
    ValueError outside bf16 math mode with the fused regression head.  Returns the TrialState."""
    st = getattr(p, '_trial', None)
    if st is None:
        raise RuntimeError(f'Predictor.{who}(): built without trials=True')
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f'Predictor.{who}() under an outer stream capture: {why}')
    st.check_ready(f'Predictor.{who}()')
    if st.stale:
        raise RuntimeError(f'Predictor.{who}(): update() has run since the last predict(); the kept rows are not those of '
                           'the resident designs - call predict() first')
    _refuse_mode(p, who)
    return st


def prepare(p, i, pins, pin_x, pin_y, cand_ptr=None):
    """Stage 1, host: state and mode refusals, validation, the pair list, ONE upload of the call's integer tables.  Returns the
    plan `launch` takes.  Nothing is launched."""
    st = check_state(p)
    p._check_design(i, 'trial_moves')
    if p.slack.rows_of(i).numel() == 0:
        raise ValueError(f'trial_moves: design {i} has no selected path')
    placed = p._placed
    off = int(placed.node_off[i])
    pins, x, y, cand_ptr = check_moves(int(placed.node_off[i + 1]) - off, pins, pin_x, pin_y, cand_ptr)
    pair_ptr, pair_row, pair_cand = expand_candidates(st.rows_of_pin, off, pins, cand_ptr)
    K, n_pairs, M = cand_ptr.shape[0] - 1, pair_row.shape[0], pins.shape[0]
    parts = [pair_row, pair_cand, pair_ptr, cand_ptr, pins + off, x, y]
    sizes = [a.shape[0] for a in parts]
    ints = torch.from_numpy(np.concatenate([a.astype(np.int32) for a in parts])).to(p.device)
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    dev = [ints[cuts[j]:cuts[j + 1]] for j in range(len(parts))]
    return dict(i=i, K=K, M=M, n_pairs=n_pairs, pair_ptr=pair_ptr, pair_row=pair_row, ints=ints, dev=dev)


def launch(p, plan):
    """Stage 2, device, on the current stream: mmft_trial_rows over the pairs, mmft_head_mlp_fwd over their rows,
    mmft_trial_reduce over the candidates and the base.  Writes buffers of its own only.  Returns the plan."""
    st, placed, b = p._trial, p._placed, p.batch
    kept = st.kept
    x, GP, pred = kept['x'], kept['GP'], kept['pred']
    K, n_pairs = plan['K'], plan['n_pairs']
    d_row, d_cand, d_pptr, d_mptr, d_node, d_mx, d_my = plan['dev']
    fcn, mods = p.pmodel.fcn, list(p.pmodel.mlp_fuse.layers)
    width, Dout = x.shape[1], fcn.weight.shape[0]
    T = pred.numel()
    raw = torch.empty(6 * (K + 1) + (n_pairs + 1) // 2, dtype=torch.float64, device=p.device)
    summary = raw[:6 * (K + 1)]
    pred_t = raw[6 * (K + 1):].view(torch.float32)[:n_pairs]
    if n_pairs:
        xt = torch.empty((n_pairs, width), dtype=torch.float32, device=p.device)
        abi('mmft_trial_rows', placed.nodes, placed.lens, placed.maxlen, placed.loc_x, placed.loc_y, placed.map_x, placed.map_y,
            p._sel.paths, p._sel.feat_off if b.B > 1 else None, T, d_row, d_cand, n_pairs, d_mptr, d_node, d_mx, d_my, K,
            GP, fcn.bias, x, x.stride(0), xt, width, width, kept['cnn_col'], Dout, b.masks.run_block, *lib.stream_args(x))
        lib.head('mmft_head_mlp_fwd', xt, width, mods[0].weight, mods[0].bias, mods[2].weight, mods[2].bias, None, pred_t,
                 n_pairs, mods[0].weight.shape[1], mods[0].weight.shape[0], 1, *lib.stream_args(x))
        plan['xt'] = xt
    rows = p.slack.rows_of(plan['i'])
    abi('mmft_trial_reduce', pred.reshape(-1), pred_t if n_pairs else None, p.slack.required, rows, rows.numel(), T,
        d_pptr if K else None, d_row if n_pairs else None, n_pairs, K, summary, *lib.stream_args(x))
    plan['raw'] = raw
    return plan


def fetch(plan):
    """Stage 3: ONE device -> host copy, decoded.  The result of trial_moves."""
    K, n_pairs = plan['K'], plan['n_pairs']
    raw = plan['raw'].cpu().numpy()
    figures = decode(raw[:6 * (K + 1)])
    res = {k: v[:K] for k, v in figures.items()}
    res['base'] = {k: (float(v[K]) if v.dtype == np.float64 else int(v[K])) for k, v in figures.items()}
    res['pair_ptr'], res['rows'] = plan['pair_ptr'], plan['pair_row']
    res['pred'] = raw[6 * (K + 1):].view(np.float32)[:n_pairs].copy()
    return res


def trial_moves(p, i, pins, pin_x, pin_y, cand_ptr=None):
    """Predictor.trial_moves: see there."""
    return fetch(launch(p, prepare(p, i, pins, pin_x, pin_y, cand_ptr)))
