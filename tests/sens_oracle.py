"""The reference gradient of mmft.sensitivity: oracle.restatement.pathmodel_level looped over the levels (what
restatement.sweep_forward does) with cell_feat / net_feat as leaf tensors and a GIVEN feature map, J = sum_r w_r pred_r and
J.backward().  dtype and rounding (None, or 'bf16': oracle/bf16.py's rounding map) are parameters, so one function gives the
plain fp64 reference, the fp64 rounding oracle and the same in fp32.

Rows of `pred` come level by level and, inside a level, in the order of `path_ids` - the order of DesignBatch.select for one
design; `batch_rows` maps a batch of several designs onto it."""
import numpy as np
import torch

from oracle import restatement as R


def oracle_sensitivity(d, path_ids, pm_state, feat_map, weights, dtype=torch.float64, rounding=None, cell_feat=None,
                       net_feat=None):
    """dict(pred [T], cell [N, Fc], net [N, Fn], targets): predictions and d J / d cell_feat, d J / d net_feat of design d in
    its own node order, as fp64 tensors.  pm_state: PathModel.state_dict() on the host; feat_map: the CNN's output for the
    design (any shape with map_size^2 elements); weights: [T]; cell_feat / net_feat: arrays used instead of the design's."""
    p = {k: (v.detach().to(dtype) if v.dtype.is_floating_point else v.clone()) for k, v in pm_state.items()}
    extra = dict(rounding=rounding) if rounding is not None else {}
    cf = torch.from_numpy(np.asarray(d.cell_feat if cell_feat is None else cell_feat)).to(dtype).requires_grad_(True)
    nf = torch.from_numpy(np.asarray(d.net_feat if net_feat is None else net_feat)).to(dtype).requires_grad_(True)
    fm = feat_map.detach().cpu().to(dtype).reshape(1, -1)
    csr = R.design_csr(d)
    h = torch.zeros((d.N, p['gnn.fc_cell_self.layers.2.weight'].shape[0]), dtype=dtype)
    ends, paths = R.bucket_paths(path_ids, d.path2level, d.path2endpoint)
    P = d.map_size * d.map_size
    outs, targets = [], []
    for level_id in range(d.L):
        tg, pids = ends.get(level_id, []), paths.get(level_id, [])
        targets.extend(tg)
        path_map = R.dense_mask_rows(d.mask_indptr, d.mask_cols, pids, P, dtype) * fm if len(pids) else None
        lvl = torch.tensor([float(level_id)], dtype=dtype)
        h, y = R.pathmodel_level(p, csr, h, cf, nf, d.levels[level_id], tg, level_id, lvl, path_map, **extra)
        if y is not None:
            outs.append(y)
    pred = torch.cat(outs, 0)
    w = torch.as_tensor(weights).detach().cpu().to(dtype)
    assert w.shape == pred.shape
    (pred * w).sum().backward()
    return dict(pred=pred.detach().double(), cell=cf.grad.double(), net=nf.grad.double(), targets=targets)


def level_parity_rows(d):
    """(rows of even levels, rows of odd levels) of design d as int64 arrays."""
    even = np.concatenate([np.asarray(d.levels[l], dtype=np.int64) for l in range(0, d.L, 2)])
    odd = np.concatenate([np.asarray(d.levels[l], dtype=np.int64) for l in range(1, d.L, 2)]) if d.L > 1 else np.zeros(0, np.int64)
    return even, odd


def batch_rows(designs, path_ids_per_design):
    """Per design the rows of a batch's `pred` that belong to it, in the order of that design's own oracle rows (the batch
    sorts the concatenated paths by level with a stable sort: DesignBatch.select)."""
    lv = np.concatenate([np.asarray(d.path2level)[np.asarray(p, dtype=np.int64)] for d, p in zip(designs, path_ids_per_design)])
    which = np.concatenate([np.full(len(p), i, dtype=np.int64) for i, p in enumerate(path_ids_per_design)])
    order = np.argsort(lv, kind='stable')
    return [np.nonzero(which[order] == i)[0] for i in range(len(designs))]
