"""Near pairs of a search plan's groups and their swap tables, built on the device (include/mmft_pairs.h).

A placer swaps a cell with cells near it, and who is near changes with every commit.  Predictor.near_swap_plan pairs the
groups of a search plan whose anchors lie within `reach` map cells of each other NOW - on the resident pins -, and builds the
pairs and every table of a swap plan on the device; Predictor.refine_swaps puts a loop on top: each pass pairs the cells that
are near each other at that moment, scores and commits a conflict-free set of their swaps, and - patch=True - writes the
changed rows into the kept head state, so that no pass needs a predict().

    check_reach / check_class         host validation of near_swap_plan's arguments
    near_pairs_host                   THE RULE of the header restated in numpy
    build / near_swap_plan            the six launches and three size reads of a plan; what Predictor.near_swap_plan delegates to
    refine_swaps                      what Predictor.refine_swaps delegates to

The entry points are bound by `abi`, an accessor of this module: the table of mmft.lib's accessors is pinned by its own ledger
and is not touched here.
"""
import numpy as np
import torch

from . import commit as CM
from . import lib
from . import search as SE
from . import swap as SW
from . import trial as TR

abi = lib.Header('mmft_pairs.h')         # near pairs: their count, the scan, the pairs, their rows' count, the swap tables
abi_decls = abi.decls

MAX_REACH = 2 ** 31 - 1
MAX_PINS = SW.MAX_PINS


# ------------------------------------------------------------------------------------------------ host validation
def check_reach(reach, who='near_swap_plan'):
    """int(reach), or ValueError unless it is an int in [1, 2^31 - 1]."""
    if isinstance(reach, bool) or not isinstance(reach, (int, np.integer)) or not 1 <= reach <= MAX_REACH:
        raise ValueError(f'{who}: reach must be an integer in [1, 2^31 - 1], got {reach!r}')
    return int(reach)


def check_class(group_class, G, who='near_swap_plan'):
    """int32 numpy array [G], or None for None; ValueError unless group_class is a numpy array or tensor of an integer dtype,
    1-D, of G elements that fit int32."""
    if group_class is None:
        return None
    h = group_class.detach().cpu().numpy() if torch.is_tensor(group_class) else group_class
    if not isinstance(h, np.ndarray) or h.dtype.kind not in 'iu':
        raise ValueError(f'{who}: group_class must be a numpy array or tensor of integers, got {getattr(h, "dtype", type(group_class).__name__)}')
    if h.shape != (int(G),):
        raise ValueError(f'{who}: group_class must hold one class per group, shape ({G},), got {h.shape}')
    if h.size and (int(h.min()) < -2 ** 31 or int(h.max()) > 2 ** 31 - 1):
        raise ValueError(f'{who}: group_class must fit int32')
    return np.ascontiguousarray(h.astype(np.int32))


# ------------------------------------------------------------------------------------------------ the rule on the host
def near_pairs_host(mv_ptr, mv_node, loc_x, loc_y, reach, group_class=None, block=256):
    """(pair_a int64 [K], pair_b int64 [K]) in ascending (a, b): THE RULE of include/mmft_pairs.h in numpy.  Groups a < b pair
    iff both are non-empty with anchors (first pins) inside loc_x / loc_y, hold at most 64 pins together, share a class
    (group_class None: one class) and their anchors lie 1 .. reach cells apart in the larger of the two axes, the differences
    formed in 64 bits.  Walks the groups a in blocks of `block` rows of the all-pairs table."""
    mv_ptr, mv_node = np.asarray(mv_ptr, dtype=np.int64), np.asarray(mv_node, dtype=np.int64)
    x, y = np.asarray(loc_x).astype(np.int64), np.asarray(loc_y).astype(np.int64)
    G, n = mv_ptr.shape[0] - 1, x.shape[0]
    size = np.diff(mv_ptr)
    anchor = mv_node[np.minimum(mv_ptr[:-1], max(mv_node.shape[0] - 1, 0))] if mv_node.size else np.zeros(G, dtype=np.int64)
    ok = (size >= 1) & (size <= MAX_PINS) & (anchor >= 0) & (anchor < n)
    at = np.where(ok, anchor, 0)
    ax, ay = (x[at], y[at]) if n else (np.zeros(G, dtype=np.int64),) * 2
    kl = np.zeros(G, dtype=np.int64) if group_class is None else np.asarray(group_class, dtype=np.int64)
    ids = np.arange(G, dtype=np.int64)
    out_a, out_b = [], []
    for a0 in range(0, G, int(block)):
        a1 = min(G, a0 + int(block))
        rows, cols = slice(a0, a1), slice(a0 + 1, G)               # b > a0 at least; the triangle is cut below
        d = np.maximum(np.abs(ax[rows, None] - ax[None, cols]), np.abs(ay[rows, None] - ay[None, cols]))
        near = (d >= 1) & (d <= int(reach)) & ok[rows, None] & ok[None, cols] & (kl[rows, None] == kl[None, cols])
        near &= (size[rows, None] + size[None, cols] <= MAX_PINS) & (ids[rows, None] < ids[None, cols])
        a, b = np.nonzero(near)                                      # row-major: ascending (a, b)
        out_a.append(a + a0)
        out_b.append(b + a0 + 1)
    cat = lambda v: np.concatenate(v).astype(np.int64) if v else np.zeros(0, dtype=np.int64)
    return cat(out_a), cat(out_b)


# ------------------------------------------------------------------------------------------------ the Predictor's side
def _checked(p, plan, who):
    """The refusals of swap_plan under the caller's name; T."""
    if getattr(p, '_trial', None) is None:
        raise RuntimeError(f'Predictor.{who}(): built without trials=True')
    if not isinstance(plan, SE.SearchPlan):
        raise TypeError(f'{who}: plan must come from search_plan(), got {type(plan).__name__}')
    if plan.owner is not p:
        raise ValueError(f'{who}: the plan belongs to another Predictor')
    CM.check_plan(plan)
    T = int(p._sel.paths.numel())
    if T + plan.G > SW.MAX_T:
        raise ValueError(f'{who}: {T} rows and {plan.G} groups do not fit the {SW.MAX_T} rows of the selection')
    return T


def _class_table(group_class, G, device, who):
    """The class table on the device: None, an int32 tensor [G] that lies there already (refine_swaps uploads it once), or
    check_class's array, uploaded."""
    if torch.is_tensor(group_class) and group_class.dtype == torch.int32 and group_class.device == torch.device(device) \
            and group_class.shape == (int(G),) and group_class.is_contiguous():
        return group_class
    h = check_class(group_class, G, who)
    return None if h is None else torch.from_numpy(h).to(device)


def build(p, plan, T, reach, klass, max_pairs, who='near_swap_plan', timed=None):
    """The launches of a plan on the current stream, with the two size reads between them: (ints, K, RP) - the int32 buffer in
    SwapPlan's layout -, or None where nothing is near.  klass: None or int32 [G] on the device.  `timed`: a callable that is
    handed each part as a function (tools/bench_placement.py times them apart)."""
    run = timed if timed is not None else (lambda name, fn: fn())
    placed, dev = p._placed, p.device
    d_gptr, d_grow, _, d_mptr, d_node = plan.dev
    G, M, R = plan.G, plan.M, plan.R
    d_node, lx, ly, n_nodes = d_node if M else None, placed.loc_x, placed.loc_y, placed.loc_x.numel()
    work = torch.empty(2 * G + 1, dtype=torch.int32, device=dev)          # cnt [G] | off [G + 1]
    total = torch.empty(2, dtype=torch.int64, device=dev)                 # K, RP
    cnt, off = work[:G], work[G:]
    run('near_count', lambda: abi('mmft_pairs_near_count', d_mptr, d_node, G, M, lx, ly, n_nodes, klass, reach, cnt, *lib.stream_args(work)))
    run('scan', lambda: abi('mmft_pairs_scan', cnt, G, off, total[:1], *lib.stream_args(work)))
    K = int(total[0].item())                                              # 8 bytes: the first size read
    if K == 0:
        return None
    if K > int(max_pairs):
        raise ValueError(f'{who}: K = {K} near pairs exceed max_pairs = {max_pairs}')
    head = torch.empty(4 * K + 1, dtype=torch.int32, device=dev)          # pair_a | pair_b | prow_ptr [K + 1] | cnt [K]
    pa, pb, pptr, pcnt = head[:K], head[K:2 * K], head[2 * K:3 * K + 1], head[3 * K + 1:]
    run('near_fill', lambda: abi('mmft_pairs_near_fill', d_mptr, d_node, G, M, lx, ly, n_nodes, klass, reach, off, K, pa, pb,
                                 *lib.stream_args(work)))
    run('rows_count', lambda: abi('mmft_pairs_rows_count', pa, pb, K, d_gptr, d_grow if R else None, G, R, pcnt, *lib.stream_args(work)))
    run('scan', lambda: abi('mmft_pairs_scan', pcnt, K, pptr, total[1:], *lib.stream_args(work)))
    RP = int(total[1].item())                                             # 8 bytes: the second size read
    if RP + 2 * K >= 2 ** 31:
        raise ValueError(f'{who}: {RP} entries and {K} pairs: RP + 2 K does not stay below 2^31')
    ints = torch.empty(6 * K + 2 + 3 * RP, dtype=torch.int32, device=dev)
    ints[:3 * K + 1].copy_(head[:3 * K + 1])
    at = 3 * K + 1
    prow, ppair, sptr, srow = ints[at:at + RP], ints[at + RP:at + 2 * RP], ints[at + 2 * RP:at + 2 * RP + K + 1], ints[at + 2 * RP + K + 1:]
    run('rows_fill', lambda: abi('mmft_pairs_rows_fill', ints[:K], ints[K:2 * K], ints[2 * K:3 * K + 1], K, RP, d_gptr, d_grow if R else None, G, R, T,
                                 prow if RP else None, ppair if RP else None, sptr, srow, *lib.stream_args(work)))
    return ints, K, RP


def near_swap_plan(p, plan, reach, group_class=None, max_pairs=1 << 20, who='near_swap_plan', timed=None):
    """Predictor.near_swap_plan: see there."""
    T = _checked(p, plan, who)
    reach = check_reach(reach, who)
    if isinstance(max_pairs, bool) or not isinstance(max_pairs, (int, np.integer)) or max_pairs < 1:
        raise ValueError(f'{who}: max_pairs must be an integer of at least 1, got {max_pairs!r}')
    klass = _class_table(group_class, plan.G, p.device, who)
    made = build(p, plan, T, reach, klass, max_pairs, who, timed)
    if made is None:
        return None
    return SW.SwapPlan.from_device(p, plan, *made, T)                      # the third read: the tables, once


def refine_swaps(p, plan, reach, passes=4, patch=True, group_class=None, **kw):
    """Predictor.refine_swaps: see there."""
    if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or passes < 1:
        raise ValueError(f'refine_swaps: passes must be an integer of at least 1, got {passes!r}')
    if not kw.get('apply', True):
        raise ValueError('refine_swaps: every pass applies its swaps (apply=False is commit_swaps\' alone)')
    _checked(p, plan, 'refine_swaps')
    reach = check_reach(reach, 'refine_swaps')
    TR.check_state(p, 'refine_swaps', 'every pass reads the number of near pairs on the host')
    klass = _class_table(group_class, plan.G, p.device, 'refine_swaps')    # uploaded once
    out = []
    for _ in range(int(passes)):
        sp = near_swap_plan(p, plan, reach, klass, who='refine_swaps')
        if sp is None:                                       # nothing is near: a normal end
            break
        out.append(SW.commit_swaps(p, sp, patch=bool(patch), **kw))
        out[-1]['pair_a'], out[-1]['pair_b'] = sp.pair_a, sp.pair_b
        if not patch:
            p.predict()                                      # the truth of the pass, and what the next one reads
        if out[-1]['n_selected'] == 0:
            break
    if patch:
        p.predict()                                          # the static output, report() and criticality() are current again
    return out
