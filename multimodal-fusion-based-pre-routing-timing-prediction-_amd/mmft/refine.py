"""Patch the kept head rows after a commit, so that the next search needs no predict() (include/mmft_refine.h).

commit_moves(apply=True) moves the selected groups' pins.  A pin feeds only the path masks, so the next predict() differs from
the last one only on the rows of the selected groups' entries, and there only in the h_cnn columns of the head's input and in
the prediction - rows the search has just shown it can recompute with the same bits.  commit_moves(patch=True) recomputes
them once more at each selected group's best offset, from the pins before they move, and writes them into the kept x and
pred: the trial state stays fresh, and refine_moves(resident=True) enqueues all its passes without a host round trip.

    selected_entries                  the entries of the selected groups: the rule both kernels apply
    rows_host                         which row of the window search mmft_refine_rows writes into each slot, restated
    patch_host                        mmft_refine_patch restated in numpy
    scratch / launch                  the xt / pred_t buffers of a plan, and the three launches between select and apply

The entry points are bound by `abi`, an accessor of this module: the table of mmft.lib's accessors is pinned by its own ledger
and is not touched here.
"""
import numpy as np
import torch

from . import lib
from . import search as SE

abi = lib.Header('mmft_refine.h')        # the kept head rows after a commit: the selected entries' rows, their write into x and pred
abi_decls = abi.decls


# ------------------------------------------------------------------------------------------------ the kernels on the host
def selected_entries(sel, best_w, radius, grow_ptr):
    """bool [R]: entry e belongs to a group g with sel[g] != 0 and 0 <= best_w[g] < W."""
    sel, best_w = np.asarray(sel), np.asarray(best_w, dtype=np.int64)
    grow_ptr = np.asarray(grow_ptr, dtype=np.int64)
    W = SE.offsets(radius)[0].shape[0]
    return np.repeat((sel != 0) & (best_w >= 0) & (best_w < W), np.diff(grow_ptr))


def rows_host(x, search_rows, sel, best_w, radius, grow_ptr, grow_row):
    """xt [R, width] of mmft_refine_rows from host arrays: search_rows [W, R, width] - what mmft_search_rows writes over the
    whole window, slot (w, e) - at w = best_w[g] for the selected entries, x[grow_row[e]] for the others, zeros for a row
    outside x."""
    x, search_rows = np.asarray(x), np.asarray(search_rows)
    grow_row, best_w = np.asarray(grow_row, dtype=np.int64), np.asarray(best_w, dtype=np.int64)
    R, width = grow_row.shape[0], search_rows.shape[2]
    on = selected_entries(sel, best_w, radius, grow_ptr)
    inside = (grow_row >= 0) & (grow_row < x.shape[0])
    w_of = np.repeat(best_w, np.diff(np.asarray(grow_ptr, dtype=np.int64)))
    xt = np.zeros((R, width), dtype=x.dtype)
    plain = inside & ~on
    xt[plain] = x[grow_row[plain], :width]
    took = inside & on
    xt[took] = search_rows[w_of[took], np.flatnonzero(took)]
    return xt


def patch_host(x, pred, xt, pred_t, sel, best_w, radius, grow_ptr, grow_row, cnn_col, Dout):
    """(x, pred, (patched, skipped)): copies of x [T, .] and pred [T] with, for every entry e of a selected group whose row
    r = grow_row[e] lies in [0, T), x[r, cnn_col:cnn_col + Dout] = xt[e, the same columns] and pred[r] = pred_t[e]; the
    selected entries whose row lies outside are counted as skipped.  The selected groups share no row."""
    x, pred = np.array(x), np.array(pred)
    xt, pred_t = np.asarray(xt), np.asarray(pred_t)
    grow_row = np.asarray(grow_row, dtype=np.int64)
    on = selected_entries(sel, best_w, radius, grow_ptr)
    inside = (grow_row >= 0) & (grow_row < pred.shape[0])
    e = np.flatnonzero(on & inside)
    x[grow_row[e], cnn_col:cnn_col + Dout] = xt[e, cnn_col:cnn_col + Dout]
    pred[grow_row[e]] = pred_t[e]
    return x, pred, (int(e.shape[0]), int((on & ~inside).sum()))


# ------------------------------------------------------------------------------------------------ the Predictor's side
def scratch(p, plan):
    """(xt [R, width], pred_t [R]) of a plan, kept with it: every patched commit of the plan uses them in stream order."""
    x = p._trial.kept['x']
    buf = getattr(plan, 'refine_scratch', None)
    if buf is None or buf[0].shape != (plan.R, x.shape[1]):
        buf = plan.refine_scratch = (torch.empty((plan.R, x.shape[1]), dtype=torch.float32, device=p.device),
                                     torch.empty(plan.R, dtype=torch.float32, device=p.device))
    return buf


def launch(p, call, sel, best_w, stats, run):
    """On the current stream, between mmft_commit_select and mmft_commit_apply: mmft_refine_rows over the plan's entries,
    mmft_head_mlp_fwd over their rows, mmft_refine_patch into the kept x and pred.  sel / best_w: the selection on the device;
    stats: int64 [2] on the device; run(name, fn): commit.launch's hook, which is handed each launch as a function."""
    plan, placed, b, kept = call['plan'], p._placed, p.batch, p._trial.kept
    x, GP, pred = kept['x'], kept['GP'], kept['pred'].reshape(-1)
    d_gptr, d_grow, d_ggrp, d_mptr, d_node = plan.dev
    fcn, mods = p.pmodel.fcn, list(p.pmodel.mlp_fuse.layers)
    width, Dout, T = x.shape[1], fcn.weight.shape[0], pred.numel()
    G, R, radius = plan.G, plan.R, call['radius']
    xt, pred_t = call['scratch']
    if R:
        run('rows', lambda: abi('mmft_refine_rows', placed.nodes, placed.lens, placed.maxlen, placed.loc_x, placed.loc_y, placed.map_x,
                                placed.map_y, p._sel.paths, p._sel.feat_off if b.B > 1 else None, T, d_grow, d_ggrp, R, d_mptr, d_node, G,
                                sel, best_w, radius, GP, fcn.bias, x, x.stride(0), xt, width, width, kept['cnn_col'], Dout,
                                b.masks.run_block, *lib.stream_args(x)))
        run('head', lambda: lib.head('mmft_head_mlp_fwd', xt, width, mods[0].weight, mods[0].bias, mods[2].weight, mods[2].bias, None,
                                     pred_t, R, mods[0].weight.shape[1], mods[0].weight.shape[0], 1, *lib.stream_args(x)))
    run('patch', lambda: abi('mmft_refine_patch', x, x.stride(0), pred, T, xt if R else None, width, pred_t if R else None, sel, best_w,
                             radius, d_grow if R else None, d_ggrp if R else None, R, G, kept['cnn_col'], Dout, stats,
                             *lib.stream_args(x)))
