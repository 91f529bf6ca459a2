"""Inference on resident designs: `Predictor` holds a batch of designs on the device, returns the predicted arrival time of
their endpoints and lets the caller push new features / layout images (a placement that keeps changing under one netlist).

The arithmetic is TrainStep.forward's whole-sweep form (train.forward_to_head, the one place that orders its launches) under
torch.no_grad(): the netlist sweep in its forward-only form
(mmft.sweep.FORWARD_ONLY: nothing kept for a reverse sweep), the U-Net from its running statistics
(evaluate.frozen_statistics; 19 launches in bf16 mode), masked projection, fusion head.  Nothing of the model is written: no
statistic, no counter, no gradient, no module mode.  In bf16 mode the whole call is captured once and replayed.
"""
import contextlib

import numpy as np
import torch

from . import cells as _cells, commit, gradsink, lib, ops, pairs, search, swap, trial
from .criticality import PredictorCriticality
from .evaluate import frozen_statistics
from .placement import batch_tables, placed_fc
from .report import PredictorReport, SlackRows
from .train import DesignBatch, forward_to_head


def design_permutations(old_of_new, node_off):
    """Per design i the int64 array p_i with p_i[k] = row of the batch's node tensors that holds node k of design i
    (DesignBatch renumbers the merged nodes level-major: row r holds merged node old_of_new[r])."""
    old_of_new = np.asarray(old_of_new, dtype=np.int64)
    new_of_old = np.empty_like(old_of_new)
    new_of_old[old_of_new] = np.arange(old_of_new.shape[0], dtype=np.int64)
    return [new_of_old[int(node_off[i]):int(node_off[i + 1])] for i in range(len(node_off) - 1)]


def _as_rows(x, name, shape, device):
    t = torch.from_numpy(x) if isinstance(x, np.ndarray) else x
    if not torch.is_tensor(t):
        raise TypeError(f'update: {name} must be a numpy array or a tensor')
    if t.dtype != torch.float32:
        raise TypeError(f'update: {name} must be float32, got {t.dtype}')
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'update: {name} has shape {tuple(t.shape)}, design expects {tuple(shape)}')
    return t.to(device, non_blocking=True)


def check_rows(rows, n_nodes, lengths=()):
    """update(rows=): the node ids of a sparse feature update as a host int64 array, or an exception - TypeError unless
    `rows` is a 1-D int64 numpy array or tensor, IndexError for an id outside [0, n_nodes), ValueError for a repeated id (the
    rows of one call are written concurrently) and for a feature array in `lengths` (name -> its number of rows) that does
    not hold one row per id.  Host only: no device is touched."""
    r = rows.detach().cpu().numpy() if torch.is_tensor(rows) else rows
    if not isinstance(r, np.ndarray) or r.dtype != np.int64:
        raise TypeError(f'update: rows must be an int64 numpy array or tensor, got {getattr(r, "dtype", type(rows).__name__)}')
    if r.ndim != 1:
        raise ValueError(f'update: rows must be 1-D, got shape {r.shape}')
    if r.size and (int(r.min()) < 0 or int(r.max()) >= n_nodes):
        raise IndexError(f'update: rows outside the design\'s {n_nodes} nodes')
    if np.unique(r).size != r.size:
        raise ValueError('update: rows must be distinct')
    for name, n in dict(lengths).items():
        if n != r.size:
            raise ValueError(f'update: {name} has {n} rows for {r.size} node ids in rows')
    return np.ascontiguousarray(r)


def update_design(batch, perm, i, cell_feat=None, net_feat=None, image=None, rows=None, seed=None, perm32=None):
    """Copy new features (rows in design i's own node order) / a new layout image of design i into the batch's static
    buffers, in place: addresses stay, the copies are ordered on the current stream.  perm = design_permutations(...)[i] as
    an int64 tensor on the batch's device.  rows (int64 node ids of design i, distinct): the feature arrays hold those rows
    only.  seed (uint8 per row of the batch): the features go through ops.update_rows_diff, which also flags the rows that
    changed bitwise (perm32: perm as int32, what that kernel indexes by, if the caller keeps one).  Everything is validated
    before anything is written."""
    if not 0 <= i < batch.B:
        raise IndexError(f'update: design {i} of {batch.B}')
    nd, n = batch.graph.ndata, int(batch.node_off[i + 1] - batch.node_off[i])
    feats = [(name, x) for name, x in (('cell_feat', cell_feat), ('net_feat', net_feat)) if x is not None]
    if rows is not None:
        if not feats:
            raise ValueError('update: rows= names feature rows, but neither cell_feat nor net_feat is given')
        rows = check_rows(rows, n, {name: x.shape[0] for name, x in feats if hasattr(x, 'shape') and len(x.shape) == 2})
        n = rows.size
    todo = []
    for name, x in feats:
        todo.append((nd[name], _as_rows(x, name, (n, nd[name].shape[1]), nd[name].device)))
    img = _as_rows(image, 'image', batch.images.shape[1:], batch.images.device) if image is not None else None
    if todo:
        if seed is not None:                                 # the diff kernel takes int32 rows
            perm = perm32 if perm32 is not None else perm.to(torch.int32)
        where = perm if rows is None else perm[torch.from_numpy(rows).to(perm.device)]
    for dst, new in todo:
        if seed is not None:
            ops.update_rows_diff(dst, new.contiguous(), seed, idx=where)
        else:
            dst.index_copy_(0, where, new)
    if img is not None:
        batch.images[i].copy_(img)


class ResidentDesigns:
    """What the front ends that keep a batch of designs on the device share (Predictor, sensitivity.Sensitivity): the
    DesignBatch, ONE Selection of paths made here (static_selection: its packed indices live in `_static_idx`, at addresses
    a replayed graph may keep) with the rows' slack inputs - `slack` (report.SlackRows); `required` (fp32 [T] on the device)
    and `row_design` (host int64 [T]) are its `required` and `design` -, h, the per-design row permutations, and the module
    modes of a call."""

    def __init__(self, who, pmodel, cnn, designs, device, path_ids_per_design, frozen_stats, overlap, static_selection=False):
        self.pmodel, self.cnn = pmodel, cnn
        self.device = torch.device(device)
        self.frozen_stats = bool(frozen_stats)
        self.overlap = bool(overlap) and pmodel.gnn is not None
        self.side = torch.cuda.Stream(device=self.device) if self.overlap else None
        b = self.batch = DesignBatch(designs, device, pmodel.gnn.out_feat_dim if pmodel.gnn is not None else 128)
        if path_ids_per_design is None:
            path_ids_per_design = [np.arange(d.num_paths) for d in designs]
        self.T = int(sum(len(p) for p in path_ids_per_design))
        if self.T == 0:
            raise ValueError(f'{who}: no path selected')
        self._static_idx = None
        if static_selection:
            self._static_idx = torch.zeros(6 * self.T + b.path2level.shape[0], dtype=torch.int32, device=self.device)
        self._sel = b.select(path_ids_per_design, static=self._static_idx)
        self.endpoints = np.asarray(self._sel.endpoints)    # the caller's numbering: node_off[design] + the design's own node id
        self.slack = SlackRows(self._sel, b)
        self.required, self.row_design = self.slack.required, self.slack.design
        self.h = torch.zeros((b.N, b.out_dim), dtype=torch.float32, device=self.device)
        self._perm = [torch.from_numpy(p).to(self.device) for p in design_permutations(b.old_of_new, b.node_off)]
        self._modules = [m for root in (pmodel, cnn) if root is not None for m in root.modules()]
        self._per_sample = [m for m in self._modules if hasattr(m, 'per_sample_stats')]

    @contextlib.contextmanager
    def _modes_kept(self):
        """Module modes and the U-Net's statistics-per-image switch (set for the call, as TrainStep sets it for good: with it
        a train-mode U-Net treats every design's image as the batch of one the reference feeds) back as found, also on an
        exception."""
        modes = [(m, m.training) for m in self._modules]
        per = [(m, m.per_sample_stats) for m in self._per_sample]
        try:
            for m in self._per_sample:
                m.per_sample_stats = True
            yield
        finally:
            for m, was in per:
                m.per_sample_stats = was
            for m, was in modes:
                m.training = was

    def _check_design(self, i, what):
        if not 0 <= i < self.batch.B:
            raise IndexError(f'{what}: design {i} of {self.batch.B}')

    def _update_design(self, i, cell_feat, net_feat, image, rows, **kw):
        self._check_design(i, 'update')
        update_design(self.batch, self._perm[i], i, cell_feat, net_feat, image, rows=rows, **kw)


class Predictor(ResidentDesigns):
    """Predictor(pmodel, cnn, designs, device).predict() -> (predictions, endpoint ids).

    path_ids_per_design   per design the paths whose endpoints are predicted (None: every path of every design); fixed for
                          the life of the object - one static selection, made here
    frozen_stats          the U-Net normalises with its running statistics for the call (evaluate.frozen_statistics)
    graphed               bf16 mode: the first predict() runs eagerly (builds weight packs, slot tables, sizes the scratch),
                          the second is captured, later ones replay.  Eager instead: launch profiler on, an outer capture,
                          fp32 mode, a U-Net that does not take its fused eval path.  Same results either way
    overlap               the netlist sweep on a side stream under the U-Net (as TrainStep)
    cone                  the sweep skips nodes outside the endpoints' fan-in cone (few endpoints of a large design)
    report                None, or dict(k=32, hist=(lo, hi, nbins) or None): every predict() also launches the timing report
                          kernel (mmft.report) on the predictions and the endpoints' required times, as the last launch of
                          the call - inside the replayed graph in bf16 mode; report() decodes the last call's buffers.
                          Regression task only.  predict() returns what it returns without it
    placement             True: the path masks follow the pins.  Every design carries placement data
                          (placement.attach_placement: path nodes, pin coordinates, masks rasterised from them); the masked
                          projection is computed from those tables (placement.placed_fc) instead of the static masks, and
                          update(i, pin_x=..., pin_y=...) moves design i's pins in place - inside the replayed graph too.
                          Predictions are bitwise those of placement=False until a pin moves.  Needs pmodel.fcn and a CNN
    incremental           True: h is kept from predict() to predict() and the netlist sweep runs only over the rows an update
                          can have changed.  update() writes features through a kernel that flags the rows that really changed
                          (`seed`); predict() turns them into `dirty`, their transitive fan-out (L - 1 small launches), runs the
                          feature MLPs and the level kernels over flagged rows only and clears the seeds - inside the replayed
                          graph too, which is the same graph for one edited cell and for a full sweep (all seeds set).  h, and
                          with it every prediction, stays bitwise what a full sweep gives.  The sweep is a FULL one on the
                          first predict(), after invalidate(), when the math mode, a module mode or the address of a parameter
                          or buffer changed, and when a parameter or buffer was written in place: the sum of their autograd
                          version counters moved, or gradsink.param_epoch() did - the project's own optimizer (FlatAdam, under
                          TrainStep / GraphedTrainStep / EpochTrainer) writes through raw pointers and bumps that instead.  A
                          write neither sees - `p.data.mul_()` (.data has a version counter of its own), a kernel of the
                          caller's on .data_ptr() - needs invalidate().  Not under an outer stream capture: the decision
                          is the host's, a caller's graph would bake it in, so predict() refuses there.  Where the sweep does not take the path on which every launch honours the row flags
                          (fp32 mode, the attention branch, an unfolded schedule: sweep.incremental_supported) predict() runs
                          the ordinary full sweep and `incremental_active` is False.  The U-Net, the masked projection and
                          the head run in full on every call
    criticality           None, True or dict(cells=True): every predict() also launches the criticality kernels
                          (mmft.criticality, include/mmft_crit.h) on the predictions, the endpoints' required times and the
                          paths' nodes, after the report launch, as the last launches of the call - inside the replayed graph in
                          bf16 mode; criticality() decodes the last call's buffers: per pin the worst slack of any predicted
                          path through it, that path's row, the number of violating paths and a criticality in [0, 1]; with
                          cells=True the worst slack and the number of violating paths per map cell, from the masks of the
                          pins as they are now (a map of a multiple of 64 cells, at most 65536).  Every design carries
                          placement data; placement=True is NOT needed: without it the option keeps tables of its own and
                          the pins never move, with it the same tables serve both and the cell maps follow
                          update(i, pin_x=..., pin_y=...).  Regression task only.  predict() returns what it returns without it.
                          dict(cells=..., sums=True, scale_log2=20): the launches are those of mmft_criticality_sums
                          (include/mmft_crit_sums.h) INSTEAD - the same outputs, bitwise, and from the same walk the sums of
                          negative slack per pin, per cell and per design as exact integer sums of quanta of 2^-scale_log2
                          (scale_log2 in [0, 30], refused without sums), every pin's and cell's share of its design's TNS and
                          the rows that hit the cap; criticality() then also returns node_tns, cell_tns, tns, node_share,
                          cell_share and saturated (mmft.criticality.decode_sums).  Without sums nothing about the call changes
    trials                True (needs placement=True): every predict() keeps the head's input rows, the prefix table of the
                          masked projection and its predictions, and trial_moves(i, pins, pin_x, pin_y, cand_ptr) returns the
                          exact predictions and WNS / TNS of design i under a batch of candidate pin moves, each taken alone,
                          without writing the placement (mmft.trial, include/mmft_trial.h).  bf16 math mode with the fused
                          regression head.  search_plan(i, pins, group_ptr) / search_moves(plan, radius) enumerate a window
                          of rigid displacements per pin group on the device instead and return every candidate's score and the
                          best offset per group (mmft.search, include/mmft_search.h); they need nothing more at construction.
                          commit_moves(plan) runs that search, selects on the device a set of groups whose best moves cannot
                          see each other and moves their pins in place; refine_moves(plan) repeats it with a predict() in
                          between (mmft.commit, include/mmft_commit.h).
                          Left at False, nothing about the object, its launches or its results changes

    Construction touches no module mode and no requires_grad; predict() leaves every module in the mode it found."""

    def __init__(self, pmodel, cnn, designs, device, path_ids_per_design=None, frozen_stats=True, graphed=True, overlap=True,
                 cone=False, report=None, placement=False, incremental=False, criticality=None, trials=False):
        criticality = self._criticality_spec(criticality)        # refusals before a device is touched
        if trials and not placement:
            raise ValueError('Predictor: trials=True needs placement=True (a trial move moves pins of the placement tables)')
        super().__init__('Predictor', pmodel, cnn, designs, device, path_ids_per_design, frozen_stats, overlap, static_selection=True)
        self.graphed, self.cone = bool(graphed), bool(cone)
        b = self.batch
        self._perm32 = None                                # incremental=True: the same as int32, what update_rows_diff indexes by
        self._tensors = [t for root in (pmodel, cnn) if root is not None for t in list(root.parameters()) + list(root.buffers())]
        self._replay = self._sig = self._out = None
        # incremental sweeps: which feature rows changed since the last predict() / which rows that predict() swept (static
        # addresses: the replayed graph reads and writes them); whether h may be trusted, and under which signature it was made
        self.incremental = bool(incremental) and pmodel.gnn is not None
        self.incremental_active = False
        self.seed = torch.zeros(b.N, dtype=torch.uint8, device=self.device) if self.incremental else None
        self.dirty = torch.zeros(b.N, dtype=torch.uint8, device=self.device) if self.incremental else None
        self._trusted, self._trust_sig, self._incr_ok = False, None, {}
        if self.incremental:
            self._perm32 = [q.to(torch.int32) for q in self._perm]
        # the options: what runs after the head (report.AfterHead) in the order of its launches, and what trial_moves keeps
        self._report = PredictorReport(self, report) if report is not None else None
        self._placed = self._make_placed(designs) if placement else None
        self._crit = PredictorCriticality(self, criticality) if criticality is not None else None
        self._trial = trial.TrialState(self) if trials else None

    _criticality_spec = staticmethod(PredictorCriticality.spec)      # criticality= as a dict or None: host only, callable on its own

    def _make_placed(self, designs):
        """The batch's placement tables; refuses designs without placement data and designs whose stored masks are not the
        masks of their pins (turning the mode on then changes no prediction until a pin moves)."""
        if self.pmodel.fcn is None or self.cnn is None:
            raise ValueError('Predictor: placement=True needs the masked projection (pmodel.fcn and a CNN)')
        return batch_tables(designs, self.batch, self.device, 'Predictor(placement=True)')

    def _unet_is_fused_eval(self):
        """Inside frozen_statistics: the U-Net call is unet16's eval forward (19 launches, nothing written)."""
        cnn = self.cnn
        if cnn is None:
            return True
        from . import cnn as C, unet16
        bns = [m for m in cnn.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        return bool(bns) and hasattr(cnn, 'inc') and all(C.bn_uses_running_stats(bn) for bn in bns) and \
            unet16.supported(cnn, self.batch.images, frozen_stats=True)

    def _run_sweep(self, run):
        """The sweep of a call (train.forward_to_head's sweep=)."""
        if not self.incremental_active:
            return run()
        # dirty = fan-out of the seeds, the sweep over the dirty rows, then the seeds are spent - in this order on one
        # stream, so a seed set by an update() after this predict() survives until the next one
        out = run(incremental=(self.seed, self.dirty))
        self.seed.zero_()
        return out

    def _placed_fc(self, pmap, feat):
        """h_cnn from the pins as they are now (train.forward_to_head's project=, placement=True); with trials=True the prefix
        table it projected through is kept for trial_moves."""
        b, fcn = self.batch, self.pmodel.fcn
        return placed_fc(self._placed, self._sel.paths, self._sel.feat_off if b.B > 1 else None, feat, fcn.weight, fcn.bias, b.masks,
                         keep=self._trial.kept if self._trial is not None else None)

    def _launches(self):
        b, pm_ = self.batch, self.pmodel
        h_gnn, _, pmap, h_cnn = forward_to_head(pm_, self.cnn, b, self._sel, self.h, side=self.side, cone=self.cone, sweep=self._run_sweep,
                                                project=self._placed_fc if self._placed is not None else None)
        pred = pm_.fuse_heads(h_gnn, pmap, self._sel.levels, b.L, h_cnn=h_cnn, keep=self._trial.kept if self._trial is not None else None)
        if self._trial is not None:
            # the references of the latest eager or capturing call: a replay rewrites those same buffers
            self._trial.kept['pred'], self._trial.kept['mode'] = pred, lib.get_math_mode()
        for option in (self._report, self._crit):                # after the head, in this order, as the last launches of the call
            if option is not None:
                option.launch(pred)
        return pred

    @torch.no_grad()
    def predict(self):
        """(pred, endpoints): pred [T] (or [T, nlabels]) on the device, one row per selected path in level order;
        endpoints: host int64 array [T], the rows' endpoint nodes in the caller's numbering (node offset of the design in
        the batch + the design's own node id).  A replayed call returns a STATIC buffer: the next predict() overwrites it -
        clone what must survive."""
        with self._modes_kept(), frozen_statistics(self.cnn, self.frozen_stats):
            replay = self.graphed and not lib.PROF_ON and not torch.cuda.is_current_stream_capturing() and \
                lib.get_math_mode() == 'bf16' and self._unet_is_fused_eval()
            if self.incremental:
                self._begin_incremental()
            if replay:
                out = self._replayed()
            else:
                out = self._launches()
            self._trusted = self.incremental_active
            if self._trial is not None:
                self._trial.fresh()
            return out, self.endpoints

    def _replayed(self):
        """predict()'s launches through the GraphReplay: their result on an eager or the capturing call, the static buffer the
        captured one returned on a replay."""
        # the graph bakes in where the model lives and which modes it ran in
        sig = (tuple(t.data_ptr() for t in self._tensors), tuple(m.training for m in self._modules))
        if self.incremental:
            sig += (self.incremental_active,)                    # ... and whether its sweep is the masked one
        if self._replay is None or sig != self._sig:
            self._sig = sig
            self._replay = lib.GraphReplay(keep=(self._static_idx, self.h, self.batch, self._tensors, self._report, self._placed,
                                                 self.seed, self.dirty, self._crit) +
                                           ((self._trial,) if self._trial is not None else ()))
        out = self._replay.run(self._launches)
        if out is not None:                                      # an eager or the capturing call
            self._out = out
        return self._out

    def trial_moves(self, i, pins, pin_x, pin_y, cand_ptr=None):
        """Exact predictions of design i under K candidate pin moves, each taken ALONE, from the last predict()
        (trials=True; mmft.trial, include/mmft_trial.h).  pins: int64 [M] node ids in design i's own numbering; pin_x / pin_y:
        int32 / int64 [M], the pins' NEW absolute map-cell coordinates (any 32-bit int: the mask rule clamps them, as for
        update); cand_ptr: int64 [K + 1], CSR over the moves - non-decreasing, from 0 to M -, None: every move is a candidate
        of its own.  A candidate is a set of at most 64 distinct pins that move together.  Everything is validated on the
        host before anything is launched.

        Returns host data (one device -> host copy): pair_ptr [K + 1] and rows [n_pairs] - per candidate the rows of `pred`
        whose path holds one of its pins, ascending: the only rows it can change -, pred fp32 [n_pairs] - that row under that
        candidate -, per candidate wns, tns (float64), wns_row, violations, n_nan, n (the slack rule of mmft_report.h over
        design i's rows) and `base`, the same figures on the pins as they are.  A candidate without pairs has the base's.

        Writes nothing another call reads - not loc_x / loc_y, h, the model or predict()'s static output.  Eager: refused
        under an outer stream capture.  RuntimeError without trials=True, before the first predict() and after an update() that
        no predict() has followed; ValueError outside bf16 math mode with the fused regression head."""
        return trial.trial_moves(self, i, pins, pin_x, pin_y, cand_ptr)

    def search_plan(self, i, pins, group_ptr=None):
        """The static tables of G pin groups of design i for search_moves (trials=True; mmft.search).  pins: int64 [M] node ids in
        design i's own numbering; group_ptr: int64 [G + 1], CSR over pins - non-decreasing, from 0 to M -, None: every pin a
        group of its own.  A group is a set of at most 64 distinct pins that move rigidly together (a cell).  Host work and ONE
        upload, no launch: per group the ascending union of its pins' rows (grow_ptr, grow_row), the group of each entry
        (grow_grp) and the groups' pins in the tables' numbering (mv_ptr, mv_node).  The plan stays valid for the life of this
        Predictor - the incidence is static, pin moves do not change it - and belongs to it alone.
        RuntimeError without trials=True; TypeError / IndexError / ValueError as trial_moves validates its pins."""
        return search.search_plan(self, i, pins, group_ptr)

    def search_moves(self, plan, radius=1, scale_log2=20, max_rows=65536):
        """Every displacement of every group of `plan` within a window, each taken ALONE, scored exactly from the last
        predict() (mmft.search, include/mmft_search.h).  radius r in [1, 8]: W = (2 r + 1)^2 offsets, offset w = (dx, dy) =
        (w // (2 r + 1) - r, w % (2 r + 1) - r), x the first map axis, the centre w = 2 r (r + 1) the zero move; under (g, w)
        the pins of group g sit at their resident coordinates + (dx, dy), saturated to int32.  The window is enumerated on
        the device in chunks of max(1, max_rows // R) offsets (R: the plan's entries), which bounds the buffer of head input
        rows; the results do not depend on max_rows.  No host table is built per call.

        Returns host data (one device -> host copy), tables [G, W]: dq int64 - the change of the design's sum of negative-slack
        quanta of 2^-scale_log2 (THE QUANTUM of mmft_crit_sums.h): -dq * 2^-scale_log2 is the candidate's TNS gain, negative dq
        an improvement -, dviol (change of the number of violating rows), new_nan (rows whose slack becomes NaN; a candidate
        is eligible iff 0), capped (rows at the quantum's cap), worst / worst_row (the smallest valid slack among the group's
        rows under the candidate, NaN / -1 without one); per group best_w, best_dx, best_dy, best_dq, best_gain - the eligible
        offset with the smallest (dq, |dx| + |dy|, w); best_w == centre: no move in the window helps -; base: nsum, violations,
        n_nan of design i on the pins as they are; grow_ptr and rows from the plan.

        Writes nothing another call reads.  Refusals as trial_moves: RuntimeError without trials=True, under an outer stream
        capture, before the first predict() and after an update() no predict() has followed; ValueError outside bf16 math mode
        with the fused regression head, for a radius outside [1, 8], a scale_log2 outside [0, 30], max_rows < 1, R * W >= 2^31
        and a plan of another Predictor."""
        return search.search_moves(self, plan, radius, scale_log2, max_rows)

    def commit_moves(self, plan, radius=1, scale_log2=20, max_rows=65536, min_gain=0.0, apply=True, patch=False):
        """search_moves, then the commit of a conflict-free set of its best moves, on the device (mmft.commit,
        include/mmft_commit.h).  A group is a CANDIDATE iff its best offset is not the centre and improves the design's sum
        by at least max(1, ceil(min_gain * 2^scale_log2)) quanta; two groups CONFLICT iff they share a row of the plan.  The
        selected set is the one a loop over the candidates in the order of (best_dq, g) gives that takes a group iff none of
        its rows belongs to a group already taken.  Its groups share no row and - the plan is checked once - no pin, so each
        row changes exactly as under its own group's move alone: the next predict() has the negative-slack sum
        predicted_nsum, to the quantum.

        Returns everything search_moves returns, and selected (bool [G]), n_selected, n_candidates, rounds (of the selection
        kernel), sum_dq (int, the sum of the selected groups' best_dq), gain (float64, -sum_dq * 2^-scale_log2) and
        predicted_nsum = base['nsum'] + sum_dq; one device -> host copy.

        apply=True: the selected groups' pins are moved in place by their best offsets (addresses stay: a replayed graph
        sees them), and the trial state is stale as after update(): trial_moves / search_moves / commit_moves refuse until a
        predict() has run.  apply=False: nothing another call reads is written.  Eager: refused under an outer stream
        capture.  Refusals: those of search_moves; ValueError for a plan in which two groups hold one pin, and for a
        min_gain that is negative, not finite or too large for 62 bits of quanta.

        patch=True (needs apply=True, else ValueError; mmft.refine, include/mmft_refine.h): before the pins move, the rows of
        the selected groups' entries are recomputed at their best offsets and written into the kept head state - the h_cnn
        columns of the head's input and the predictions -, which then holds, bit for bit, what a predict() on the moved
        pins would write.  The trial state stays fresh: trial_moves, search_moves and commit_moves may follow at once.  The
        result gains n_patched, the entries written, in the same copy.  The kept predictions ARE the static buffer a replayed
        predict() returned: a tensor the caller still holds from the last predict() changes in place.  report() and
        criticality() keep describing the last predict()."""
        return commit.commit_moves(self, plan, radius, scale_log2, max_rows, min_gain, apply, patch)

    def refine_moves(self, plan, radius=1, passes=4, resident=False, **kw):
        """commit_moves(plan, radius, **kw), then predict(), repeated until a pass selects nothing or `passes` have run: the
        list of the passes' results.  Each pass's predicted_nsum is the next pass's base['nsum'], and the sums never
        increase.  Needs a predict() before the call, like every trial call, and leaves one behind.

        resident=True: the same list without a predict() or a host decision between the passes.  Everything is validated
        once, then all `passes` commits are enqueued back to back with patch=True, each into a result buffer of its own; one
        copy brings them back, and the list is cut after the first pass that selected nothing (the later ones found the same
        state and did nothing).  One predict() follows, after which the static output, report() and criticality() are
        current again."""
        return commit.refine_moves(self, plan, radius, passes, resident, **kw)

    def swap_plan(self, plan, pair_a, pair_b):
        """K swaps of the groups of `plan` (from search_plan) for swap_moves / commit_swaps (trials=True; mmft.swap,
        include/mmft_swap.h).  pair_a, pair_b: int64 [K], K >= 1, group ids of the plan: pair k swaps the cells pair_a[k] and
        pair_b[k].  The ANCHOR of a group is its first pin: under the swap the two anchors exchange positions and every pin
        keeps its offset from its own anchor, the sums formed in 64 bits and saturated to int32; the anchors are read on the
        device at call time, so the plan stays valid while the placement moves.  Host work and ONE upload, no launch: per
        pair the ascending union of its two groups' rows (prow_ptr, prow_row, prow_pair) and the select table of
        commit_swaps.  The same pair twice, or (a, b) beside (b, a), is allowed: they conflict.  Valid for the life of this
        Predictor, and its alone.
        RuntimeError without trials=True; TypeError for something that is no search plan; IndexError for a group id outside
        the plan; ValueError for arrays that are not int64 [K], a pair of a group with itself, an empty group, groups of more
        than 64 pins together, a plan of another Predictor, a plan in which two groups hold one pin, and more than 2^24 rows
        and groups together."""
        return swap.swap_plan(self, plan, pair_a, pair_b)

    def swap_moves(self, splan, scale_log2=20, max_rows=65536):
        """Every swap of `splan`, each taken ALONE, scored exactly from the last predict() (mmft.swap, include/mmft_swap.h).
        The pairs are walked on the device in chunks cut at pair boundaries so that a chunk's entries stay within max_rows
        (a single larger pair goes alone), which bounds the buffer of head input rows; the results do not depend on
        max_rows.  No host table is built per call.

        Returns host data (one device -> host copy), tables [K] with search_moves' definitions, a pair's entries in the
        place of a group's: dq int64, dviol, new_nan, capped, worst, worst_row; eligible (bool: new_nan == 0); gain float64
        = -dq * 2^-scale_log2; base: nsum, violations, n_nan of the design on the pins as they are; prow_ptr and rows from
        the plan; and per group of the search plan best_pair [G] - the eligible pair that holds the group with the
        smallest key (dq, k), -1 without one - and best_pair_dq [G], both decoded on the host from that same copy.

        Writes nothing predict() returns and no pin.  Refusals as search_moves: RuntimeError without trials=True, under an
        outer stream capture, before the first predict() and after an update() or a commit no predict() has followed;
        ValueError outside bf16 math mode with the fused regression head, for a scale_log2 outside [0, 30], max_rows < 1 and a
        plan of another Predictor; TypeError for something that is no swap plan."""
        return swap.swap_moves(self, splan, scale_log2, max_rows)

    def commit_swaps(self, splan, scale_log2=20, max_rows=65536, min_gain=0.0, apply=True, patch=False):
        """swap_moves, then the commit of a conflict-free set of swaps, on the device (mmft.swap; the selection is
        mmft_commit_select of include/mmft_commit.h as it stands).  A pair is a CANDIDATE iff it is eligible and improves the
        design's sum by at least max(1, ceil(min_gain * 2^scale_log2)) quanta, commit_moves' own threshold; two pairs
        CONFLICT iff they share a row or a group - also a group that lies on no row.  The selected set is the one a loop over
        the candidates in the order of (dq, k) gives that takes a pair iff it conflicts with none already taken.  Its swaps
        cannot see each other: the next predict() has the negative-slack sum predicted_nsum, to the quantum.

        Returns everything swap_moves returns - the per-pair gain under the name pair_gain -, and selected (bool [K]),
        n_selected, n_candidates, rounds (of the selection kernel), sum_dq (int, the sum of the selected pairs' dq), gain
        (float64, -sum_dq * 2^-scale_log2) and predicted_nsum = base['nsum'] + sum_dq; one device -> host copy.

        apply=True: the pins of both groups of every selected pair are written in place at their swapped coordinates
        (addresses stay: a replayed graph sees them), and the trial state is stale exactly as after commit_moves():
        trial_moves / search_moves / swap_moves / commit_swaps refuse until a predict() has run.  apply=False: nothing
        another call reads is written.  Eager: refused under an outer stream capture.  Refusals: those of swap_moves, and
        ValueError for a min_gain that is negative, not finite or too large for 62 bits of quanta.

        patch=True (needs apply=True, else ValueError; mmft_refine_patch of include/mmft_refine.h as it stands, the pairs as
        its groups): before the pins move, the rows of the selected pairs' entries under their swaps are written into the
        kept head state - the h_cnn columns of the head's input and the predictions -, which then holds, bit for bit, what
        a predict() on the swapped pins would write.  A call of one chunk patches from the rows of its scoring pass; a call
        of several (max_rows) recomputes each chunk's rows first.  The trial state stays fresh: swap_moves, commit_swaps,
        near_swap_plan and the window calls may follow at once.  The result gains n_patched, the entries written, in the
        same copy.  The kept predictions ARE the static buffer a replayed predict() returned: a tensor the caller still
        holds from the last predict() changes in place.  report() and criticality() keep describing the last predict()."""
        return swap.commit_swaps(self, splan, scale_log2, max_rows, min_gain, apply, patch)

    def near_swap_plan(self, plan, reach, group_class=None, max_pairs=1 << 20):
        """The swap plan of the groups of `plan` that are NEAR each other on the resident pins as they are now, built on the
        device (trials=True; mmft.pairs, include/mmft_pairs.h).  Groups a < b pair iff both are non-empty, hold at most 64
        pins together, share a class - group_class: an int array [G], None for one class - and their anchors (first pins)
        lie 1 .. reach map cells apart in the larger of the two axes (differences in 64 bits; coinciding anchors are no
        pair).  The pairs come in ascending (a, b), K in all, and with them every table of swap_plan: the result is an
        ordinary swap plan for swap_moves and commit_swaps.

        Six launches - count, scan, fill of the pairs; count, scan, fill of their rows - and THREE small synchronisations
        per plan: the read of K (8 bytes), the read of RP (8 bytes), and one copy of the int32 buffer back, from which the
        plan's host tables are decoded.  No host table arithmetic.  The neighbour test is all-pairs on the device.

        None where nothing is near (K == 0): a normal end of a refinement.  Needs no predict() and does not look at the trial
        state: it reads pins only.  RuntimeError without trials=True; TypeError for something that is no search plan;
        ValueError for a plan of another Predictor, a plan in which two groups hold one pin, more than 2^24 rows and groups
        together, a reach that is not an int in [1, 2^31 - 1], a group_class that is not an int array [G], K > max_pairs
        (the message names K) and RP + 2 K >= 2^31."""
        return pairs.near_swap_plan(self, plan, reach, group_class, max_pairs)

    def refine_swaps(self, plan, reach, passes=4, patch=True, group_class=None, **kw):
        """near_swap_plan(plan, reach, group_class) on the pins as they are now, then commit_swaps(patch=patch, **kw),
        repeated until nothing is near, a pass selects nothing or `passes` have run: the list of the passes' results, each
        with its plan's pair_a / pair_b.  Every pass pairs the cells that are near each other at that moment.  Each pass's
        predicted_nsum is the next pass's base['nsum'], and the sums never increase.

        patch=True: no pass needs a predict() - the patched commit keeps the head state current -, and one predict() follows
        the loop, after which the static output, report() and criticality() are current again.  patch=False: a predict()
        follows every pass.  Needs a predict() before the call, like every trial call.  Refusals: those of near_swap_plan
        and commit_swaps; ValueError for passes that is not an integer of at least 1 and for apply=False; refused under an
        outer stream capture."""
        return pairs.refine_swaps(self, plan, reach, passes, patch, group_class, **kw)

    def cell_set(self, i, pins, cell_ptr=None):
        """C cells of design i for critical_plan / refine_cells (trials=True; mmft.cells, include/mmft_cells.h).  pins: int64
        [M] node ids in design i's own numbering; cell_ptr: int64 [C + 1], CSR over pins - non-decreasing, from 0 to M -,
        None: every pin a cell of its own.  Validated once, on the host, by search_plan's rules for groups - and no pin may
        belong to two cells: that is what lets every plan built from the set be committed without a check per plan.  ONE
        upload of cell_ptr | cell_node; the incidence of the selection is uploaded once per Predictor, on first use.  Valid
        for the life of this Predictor, and its alone.
        RuntimeError without trials=True; TypeError / IndexError / ValueError as search_plan validates its pins; ValueError
        for a pin in two cells (the message names the pin and the cells) and for a design without a selected path."""
        return _cells.cell_set(self, i, pins, cell_ptr)

    def critical_plan(self, cells, slack_below=0.0, max_groups=1 << 20):
        """The search plan of the cells of a cell set that VIOLATE NOW, built on the device from the kept predictions
        (trials=True; mmft.cells, include/mmft_cells.h).  A cell is selected iff it holds 1 .. 64 pins and one of the rows
        its pins lie on has a slack (required - pred) + 0.0f that is not NaN and strictly below slack_below, compared in
        fp32; slack_below=None selects every cell of 1 .. 64 pins.  The selected cells, in ascending order, are the G groups
        of an ordinary search plan - each with ALL its rows, word for word what search_plan gives for them - for
        search_moves, commit_moves, refine_moves, swap_plan and near_swap_plan.  The plan also carries cell (int64 [G], the
        cell of each group) and worst (fp32 [G], the smallest valid slack among its rows, NaN without one).

        Five launches - count, three scans, fill - and TWO small synchronisations: the read of G, R and M' (24 bytes) and
        one copy of the int32 buffer back.  No host table arithmetic, no download of the predictions.  The kept
        predictions are those of the last predict() or of the patched commits since: the call is fresh after predict() and
        after commit_moves(patch=True) / commit_swaps(patch=True), and refused after update() or an unpatched commit.

        None where no cell is selected.  Refusals: those of search_moves' state and mode (RuntimeError without trials=True,
        under an outer stream capture, before the first predict(), on a stale state; ValueError outside bf16 math mode
        with the fused regression head); TypeError for something that is no cell set; ValueError for a cell set of another
        Predictor, a slack_below that is NaN or no number, G > max_groups (the message names G) and a design whose rows
        span more than 65536 rows of the selection (cells.critical_host and search_plan remain)."""
        return _cells.critical_plan(self, cells, slack_below, max_groups)

    def refine_cells(self, cells, radius=1, passes=4, slack_below=0.0, patch=True, **kw):
        """critical_plan(cells, slack_below) on the state as it is now, then commit_moves(plan, radius, patch=patch, **kw),
        repeated until no cell violates, a pass selects nothing or `passes` have run: the list of the passes' results, each
        with its plan's `cell`.  Every pass searches the cells that violate at that moment, not those that violated before
        the first.

        patch=True: no pass needs a predict() - the patched commit keeps the head state current, and each pass's
        predicted_nsum is the next pass's base['nsum'] -, and one predict() follows the loop, after which the static
        output, report() and criticality() are current again.  patch=False: a predict() follows every pass.  Needs a
        predict() before the call, like every trial call.  Refusals: those of critical_plan and commit_moves; ValueError for
        passes that is not an integer of at least 1 and for apply=False."""
        return _cells.refine_cells(self, cells, radius, passes, slack_below, patch, **kw)

    def _begin_incremental(self):
        """Decides what this predict()'s sweep is: the ordinary full one (incremental_active False) where the masked path is
        not taken, else the masked one - over every row (all seeds set, here, on the current stream) unless h is the result
        of a predict() under the same math mode, module modes, tensor addresses and tensor contents (the sum of the autograd
        version counters, and gradsink.param_epoch() for FlatAdam's raw-pointer steps: host side, no launch)."""
        from . import sweep as _sweep
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('Predictor(incremental=True).predict() under an outer stream capture: whether h can be trusted is '
                               'decided on the host per call, a captured graph would replay one decision for ever')
        mode = lib.get_math_mode()
        ok = self._incr_ok.get(mode)
        if ok is None:
            self.batch.graph.ndata['h'] = self.h
            ok = self._incr_ok[mode] = bool(_sweep.incremental_supported(self.pmodel.gnn, self.batch.graph, self.batch.level_nodes))
        self.incremental_active = ok
        trusted, self._trusted = self._trusted, False            # (an exception below or in the launches: not to be trusted)
        if not ok:
            return
        sig = (mode, tuple(t.data_ptr() for t in self._tensors), tuple(m.training for m in self._modules),
               sum(t._version for t in self._tensors), gradsink.param_epoch())
        if not trusted or sig != self._trust_sig:
            self.seed.fill_(1)
        self._trust_sig = sig

    def invalidate(self):
        """The next predict() sweeps every row (incremental=True; a no-op otherwise): for a change of the model that the
        Predictor cannot see, or of h itself."""
        self._trusted = False

    def dirty_mask(self, i=None):
        """Host uint8 copy of the rows the LAST predict() swept: the whole batch in the batch's row order, or design i in
        the design's own node order.  All ones after a predict() that fell back to the ordinary sweep.  One device->host
        copy here, nothing in predict()."""
        if not self.incremental:
            raise RuntimeError('Predictor.dirty_mask(): built without incremental=True')
        if i is not None:
            self._check_design(i, 'dirty_mask')
        d = self.dirty.cpu().numpy() if self.incremental_active else np.ones(self.batch.N, dtype=np.uint8)
        return d if i is None else d[self._perm[i].cpu().numpy()]

    def report(self):
        """The timing report of the LAST predict(): one dict per design (mmft.report.decode: n, n_nan, violations, wns,
        wns_row, tns, worst, hist, wns_endpoint, worst_endpoints; rows are rows of `pred`, endpoints in the caller's
        numbering).  One small device->host copy."""
        if self._report is None:
            raise RuntimeError('Predictor.report(): no report was requested (report=dict(k=..., hist=...))')
        self._report.check_ready('Predictor.report()')
        return self._report.result()

    def criticality(self, i=None):
        """The criticality of the LAST predict(): one dict per design, or design i's (mmft.criticality.decode: node_slack,
        node_row, node_viol, node_crit in the design's own node order - node_row is a row of `pred` -, cell_slack and
        cell_viol as [map, map] arrays or None, n, n_nan; with sums=True also node_tns, cell_tns, tns, node_share, cell_share and
        saturated: mmft.criticality.decode_sums).  One device->host copy."""
        if self._crit is None:
            raise RuntimeError('Predictor.criticality(): no criticality was requested (criticality=True or dict(cells=...))')
        self._crit.check_ready('Predictor.criticality()')
        if i is not None:
            self._check_design(i, 'criticality')
        return self._crit.result(i)

    def update(self, i, cell_feat=None, net_feat=None, image=None, pin_x=None, pin_y=None, rows=None):
        """New features (rows in design i's own node order, float32 [N_i, width]) and / or a new layout image (float32, the
        design's image shape) for design i; numpy arrays or tensors.  Copied into the resident buffers on the current stream:
        the next predict() sees them, eager or replayed.  rows (int64 node ids in design i's own numbering, distinct): the
        feature arrays hold those rows only, float32 [len(rows), width].  pin_x / pin_y (placement=True only; both or
        neither): new map-cell coordinates of the design's pins, int32 / int64 [N_i]; any value is allowed, boxes are clamped to
        the map.  All arguments of a call are validated before any is written.
        With incremental=True the features - whole tables as well - are written by a kernel that flags every row whose bits
        changed: the next predict() sweeps the fan-out of exactly those rows.  Images and pins flag nothing (the U-Net and the
        projection run in full anyway)."""
        self._check_design(i, 'update')
        pins = None
        if pin_x is not None or pin_y is not None:
            if self._placed is None:
                raise ValueError('update: pin_x / pin_y need a Predictor built with placement=True')
            if pin_x is None or pin_y is None:
                raise ValueError('update: pin_x and pin_y go together')
            pins = self._placed.check_pins(i, pin_x, pin_y)
        self._update_design(i, cell_feat, net_feat, image, rows, seed=self.seed,
                            perm32=self._perm32[i] if self._perm32 is not None else None)
        if self._trial is not None:
            self._trial.stale = True                         # until the next predict(): trial_moves refuses in between
        if pins is not None:
            self._placed.set_pins(i, *pins)

    def masks(self, i):
        """Host (indptr, cols) int64 of design i's current path masks: rasterised from the pins as they are now with
        placement=True (synchronises), the design's stored masks otherwise."""
        b = self.batch
        self._check_design(i, 'masks')
        q0, q1 = int(b.path_off[i]), int(b.path_off[i + 1])
        if self._placed is not None:
            ip, cols = (t.cpu().numpy().astype(np.int64) for t in self._placed.csr())
        else:
            ip, cols = b.masks.host_indptr, b.masks.host_cols
        return ip[q0:q1 + 1] - ip[q0], cols[ip[q0]:ip[q1]].copy()
