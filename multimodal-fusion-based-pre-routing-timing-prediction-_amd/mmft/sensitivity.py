"""Sensitivity of the predicted timing: `Sensitivity` holds a batch of designs on the device like `infer.Predictor` and answers
"which change would help" with one reverse sweep - the gradient of a weighted sum of the predictions,

    J = sum_r w_r pred_r,

with respect to every row of cell_feat and net_feat, handed out per design in the design's own node order.

What runs.  The launches and their order are train.forward_to_head's, as for Predictor.  The U-Net, the masked projection and
h_cnn run under no_grad: they do not depend on the features.  The netlist sweep runs in its training form (sweep.SweepFn keeps A / LSE / the hidden rows) and the
fusion head on top of it; torch.autograd.grad seeds the existing reverse sweep with w as the gradient of the predictions.
After it the sweep's G holds, for every cell and net row, the gradient at the output of fc_cell_self / fc_net_self - the rows
mlp2_feat_bwd_kernel reads for the weight gradients.  The last hop, through the two feature MLPs to their inputs, is
mmft_mlp2_feat_dx_bf16 (include/mmft_sens.h, csrc/mlp_feat_dx.hip): two launches over the row ranges of
sweep._batched_param_grads, in bf16 mode on a schedule where the sweep's feat_fused holds.  In fp32 mode, or where the rows
are not a range, the same result comes from the generic layers (linear_fwd recomputes H, linear_dgrad(mask=H), linear_dgrad).

image=True adds the third input, the layout image.  The U-Net then runs through unet16.unet_forward_eval_taped (the same 19
launches and bits as the eval forward) and its output, the feature map, is a leaf of the autograd tape: the masked projection
runs on the tape, MaskedFcFn.backward hands back d J / d feature map (`feat_grad`, the map-level answer), and
unet16.unet_eval_input_grad carries it through the eval-mode U-Net to the image - data gradient only, 32 launches, the two
kernels of include/mmft_sens_image.h among them.  bf16 mode on the fused eval path only; everything else is refused on the host.

pins=True adds the placement, as a DISCRETE sensitivity (a pin is not differentiable through box masks: it moves a path's mask
by whole cells): grads[i]['pin_move'][n][d] is the first-order change of J when pin n of design i alone moves one map cell in
direction d (0: x + 1, 1: x - 1, 2: y + 1, 3: y - 1) - EXACT IN THE MASK (the set difference of the path masks under the rule of
include/mmft_place.h: clamping, boxes that vanish or appear at the map's edge, cells another box of the path keeps alive) and
LINEAR IN THE HEAD (the change of h_cnn is contracted with the gradient at h_cnn).  It is not a prediction of the moved design:
the exact answer remains update() followed by predict().  h_cnn then comes from placement.placed_fc (bitwise masked_fc) as a
leaf of the tape - with image=True it is on the tape already -, the one autograd.grad call also returns the gradient at it (a
column slice of the head's dx, which the head kernel writes either way), and mmft_pin_move_rows / mmft_pin_move_sum
(include/mmft_sens_pins.h, csrc/pin_move.hip) turn it into row_move and pin_move: two launches, no workspace, no atomics.

Eager only: the forward + backward pair is not captured and replayed.  Nothing of the model is written - no parameter, no
buffer, no .grad (torch.autograd.grad, not .backward()), no requires_grad flag, no module mode.  A model whose parameters carry
gradient sinks (mmft.gradsink: a trainer with the fused optimizer owns it) is refused: the reverse sweep would deliver its
weight gradients into that trainer's flat gradient buffer.
"""
import numpy as np
import torch

from . import gradsink, lib, ops
from .evaluate import frozen_statistics
from .infer import ResidentDesigns
from .train import forward_to_head

OBJECTIVES = ('tns', 'sum')


def check_model(pmodel):
    """The refusals that the model alone decides, on the host: no netlist branch, the attention branch, a head that is not the
    regression head (ValueError); gradient sinks on a parameter (RuntimeError)."""
    if getattr(pmodel, 'gnn', None) is None:
        raise ValueError('Sensitivity: the model has no netlist branch (pmodel.gnn is None): nothing depends on the features')
    if getattr(pmodel.gnn, 'flag_attn', False):
        raise ValueError('Sensitivity: PathConv(flag_attn=True) is not supported (the attention branch reads net_feat through '
                         'h_drive and keeps the per-level sweep)')
    nlabels = pmodel.mlp_fuse.layers[-1].out_features
    if nlabels != 1:
        raise ValueError(f'Sensitivity: needs the regression head (nlabels = 1), the model has {nlabels} labels')
    check_no_sinks(pmodel)


def check_no_sinks(pmodel):
    sunk = [n for n, p in pmodel.named_parameters() if gradsink.of(p) is not None]
    if sunk:
        raise RuntimeError(f'Sensitivity: {len(sunk)} parameters of the model carry gradient sinks ({sunk[0]}, ...): a trainer with '
                           'the fused optimizer owns it, and the reverse sweep would write into its flat gradient buffer')


def check_image_model(pmodel, cnn):
    """image=True at construction: there must be a CNN whose output reaches the predictions (ValueError otherwise)."""
    if cnn is None:
        raise ValueError('Sensitivity(image=True): there is no CNN, so nothing depends on the layout image')
    if getattr(pmodel, 'fcn', None) is None:
        raise ValueError('Sensitivity(image=True): the model has no masked projection (pmodel.fcn is None): the predictions '
                         'do not depend on the layout image')


def check_pins_model(pmodel, cnn, designs):
    """pins=True at construction: there must be a masked projection for the pins to move, and every design must carry
    placement data (ValueError otherwise).  Host only."""
    from . import placement as PL
    if cnn is None:
        raise ValueError('Sensitivity(pins=True): there is no CNN, so no prediction depends on the path masks')
    if getattr(pmodel, 'fcn', None) is None:
        raise ValueError('Sensitivity(pins=True): the model has no masked projection (pmodel.fcn is None): the predictions '
                         'do not depend on the pins\' coordinates')
    PL.require_placement(designs, 'Sensitivity(pins=True)')


def check_pin_update(pins, image, pin_x, pin_y):
    """update(pin_x=, pin_y=): True when the call moves pins, False when it names none; ValueError where it cannot."""
    if pin_x is None and pin_y is None:
        return False
    if not pins:
        raise ValueError('update: pin_x / pin_y need a Sensitivity built with pins=True')
    if image:
        raise ValueError('update: pin_x / pin_y with image=True: that route\'s masks are the rasterised ones, and moving masks '
                         'have no backward')
    if pin_x is None or pin_y is None:
        raise ValueError('update: pin_x and pin_y go together')
    return True


def check_image_route(cnn, images, frozen_stats):
    """image=True at run(): the U-Net call must be unet16's fused eval forward - the condition of
    Predictor._unet_is_fused_eval under the statistics the call would freeze.  ValueError before anything is launched."""
    from . import cnn as C, unet16
    why = None
    if lib.get_math_mode() != 'bf16':
        why = 'the math mode is fp32 (the eval-mode input gradient exists on the bf16-storage kernels only)'
    elif not hasattr(cnn, 'inc') or not hasattr(cnn, 'outc'):
        why = f'{type(cnn).__name__} is not the U-Net'
    else:
        bns = [m for m in cnn.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        with frozen_statistics(cnn, frozen_stats):
            frozen = bool(bns) and all(C.bn_uses_running_stats(bn) for bn in bns)
        if not frozen:
            why = 'a BatchNorm layer would normalise with batch statistics (frozen_stats=False on a net in train mode, or ' \
                  'no tracked running statistics): they couple the pixels of an image'
        elif not unet16.supported(cnn, images, frozen_stats=True):
            why = f'the image batch {tuple(images.shape)} is outside the fused eval path (unet16.supported)'
    if why is not None:
        raise ValueError(f'Sensitivity.run(image=True): {why}')


def check_objective(objective):
    if objective not in OBJECTIVES:
        raise ValueError(f'Sensitivity.run: unknown objective {objective!r} (expected one of {OBJECTIVES})')
    return objective


def check_weights(weights, T):
    """weights= of run(): None, or a float32 [T] numpy array or tensor (host or device); TypeError / ValueError otherwise."""
    if weights is None:
        return None
    w = torch.from_numpy(weights) if isinstance(weights, np.ndarray) else weights
    if not torch.is_tensor(w):
        raise TypeError('Sensitivity.run: weights must be a numpy array or a tensor')
    if w.dtype != torch.float32:
        raise TypeError(f'Sensitivity.run: weights must be float32, got {w.dtype}')
    if w.dim() != 1 or w.numel() != T:
        raise ValueError(f'Sensitivity.run: weights has shape {tuple(w.shape)}, one weight per predicted path expected ({T},)')
    return w


class Sensitivity(ResidentDesigns):
    """Sensitivity(pmodel, cnn, designs, device).run() -> (pred, endpoints, grads).

    path_ids_per_design   per design the paths that are predicted and weighted (None: every path of every design); one static
                          selection, made here
    frozen_stats          the U-Net normalises with its running statistics for the call (evaluate.frozen_statistics)
    overlap               the netlist sweep on a side stream under the U-Net (as Predictor)
    image                 run() also returns grads[i]['image'], fp32 [3, H, W]: the gradient of J with respect to design i's
                          layout image (bf16 mode, the U-Net on its fused eval path)
    pins                  run() also returns grads[i]['pin_move'], fp32 [N_i, 4] in design i's own node order: the first-order
                          change of J when that pin alone moves one map cell (x + 1, x - 1, y + 1, y - 1) - exact in the mask,
                          linear in the head (module docstring); 0 for pins on no selected path.  Every design carries placement
                          data (placement.attach_placement); update(i, pin_x=..., pin_y=...) then moves design i's pins in
                          place (not with image=True) and the next run() predicts and differentiates on the moved pins.
                          pred and the other gradients are bitwise those of pins=False

    Attributes: endpoints (host int64 [T], as Predictor's), required (fp32 [T] on the device: the rows' required times),
    row_design (host int64 [T]: the design of each row of pred), feat_map (the U-Net's output of the last run(), [B, P]),
    feat_grad (image=True: d J / d feat_map of the last run(), [B, P]),
    proj_grad (pins=True: d J / d h_cnn of the last run(), [T, Dout] - a view), row_move (pins=True: fp32 [T, maxlen, 4], the
    per-row terms of pin_move, include/mmft_sens_pins.h), placed (pins=True: the placement.PlacedPaths tables),
    last_hop ('fused' / 'layers': which route the last run() took through the feature MLPs).
    force_layers = True sends the last hop through the generic layers also where the fused kernel would run."""

    def __init__(self, pmodel, cnn, designs, device, path_ids_per_design=None, frozen_stats=True, overlap=True, image=False,
                 pins=False):
        check_model(pmodel)
        if image:
            check_image_model(pmodel, cnn)
        if pins:
            check_pins_model(pmodel, cnn, designs)
        self.image, self.pins = bool(image), bool(pins)
        super().__init__('Sensitivity', pmodel, cnn, designs, device, path_ids_per_design, frozen_stats, overlap)
        nd = self.batch.graph.ndata
        # rows outside the (even / odd) levels are never written: zero for the life of the object
        self._dx = {k: torch.zeros_like(nd[k]) for k in ('cell_feat', 'net_feat')}
        self.feat_map = self.last_hop = self.feat_grad = None
        self.force_layers = False
        self.placed = self.proj_grad = self.row_move = self._incidence = self._pin_move = None
        if self.pins:
            self._make_pins(designs)

    def _make_pins(self, designs):
        """The placement tables, the incidence CSR of the selection and the static outputs of pins=True; refuses a map the
        kernels do not take and designs whose stored masks are not the masks of their pins (pred would then differ from
        pins=False) - what Predictor(placement=True) refuses."""
        from . import placement as PL
        placed = PL.batch_tables(designs, self.batch, self.device, 'Sensitivity(pins=True)')
        if placed.maxlen > ops.PIN_MOVE_MAX_LEN:
            raise ValueError(f'Sensitivity(pins=True): paths of up to {ops.PIN_MOVE_MAX_LEN} nodes, the designs\' rows hold {placed.maxlen}')
        self.placed = placed
        self._incidence = PL.pin_incidence(placed, self._sel.paths)
        self.row_move = torch.zeros((self.T, placed.maxlen, 4), dtype=torch.float32, device=self.device)
        self._pin_move = torch.zeros((self.batch.N, 4), dtype=torch.float32, device=self.device)

    def update(self, i, cell_feat=None, net_feat=None, image=None, rows=None, pin_x=None, pin_y=None):
        """New features / a new layout image of design i, as Predictor.update (infer.update_design): the next run() sees them.
        pin_x / pin_y (pins=True without image=True; both or neither): new map-cell coordinates of the design's pins, int32 /
        int64 [N_i], any value (boxes are clamped to the map) - PlacedPaths.set_pins.  Everything is validated before anything
        is written."""
        xy = None
        if check_pin_update(self.pins, self.image, pin_x, pin_y):
            xy = self.placed.check_pins(i, pin_x, pin_y)
        self._update_design(i, cell_feat, net_feat, image, rows)
        if xy is not None:
            self.placed.set_pins(i, *xy)

    def _forward(self):
        """pred [T] with the sweep and the head on the autograd tape; everything in front of them under no_grad - but for
        image=True: the feature map is then a leaf and the masked projection runs on the tape too."""
        b, pm_, sel = self.batch, self.pmodel, self._sel
        self._tape = None

        def sweep(run):
            with torch.enable_grad():
                return run()

        def features():
            with torch.set_grad_enabled(self.image):
                if not self.image:
                    return self.cnn(b.images).reshape(b.B, -1) if self.cnn is not None else None
                from . import unet16
                with torch.no_grad():
                    out, self._tape = unet16.unet_forward_eval_taped(self.cnn, b.images)
                return out.reshape(b.B, -1).requires_grad_(True)

        def project(pmap, feat):
            with torch.set_grad_enabled(self.image):
                if not self.pins or self.image:
                    return pm_._fcn(pmap) if (pmap is not None and pm_.fcn is not None) else None
                # the masks of the pins as they are now: bitwise masked_fc on masks rasterised from them (placement.placed_fc)
                from .placement import placed_fc
                h_cnn = placed_fc(self.placed, sel.paths, sel.feat_off if b.B > 1 else None, feat, pm_.fcn.weight, pm_.fcn.bias, b.masks)
            return h_cnn.requires_grad_(True)             # a leaf of the tape: autograd.grad hands back the gradient at it

        h_gnn, feat, pmap, h_cnn = forward_to_head(pm_, self.cnn, b, sel, self.h, side=self.side, sweep=sweep, features=features,
                                                   project=project)
        st = b.graph._sweep
        self._proj = h_cnn if self.pins else None
        self.feat_map = feat.detach() if self.image else feat
        self._feat_leaf = feat if self.image else None
        with torch.enable_grad():
            pred = pm_.fuse_heads(h_gnn, pmap, sel.levels, b.L, h_cnn=h_cnn)
        return pred, st

    def _last_hop(self, st):
        """G -> d J / d cell_feat, d J / d net_feat over the rows of the even / odd levels (sweep._batched_param_grads' row sets)."""
        from .sweep import _cat_rows, _rows_of, _w
        P = [_w(p) for p in st.params]
        (w1c, b1c, w2c, _, w1n, b1n, w2n, _) = P[0:8]
        rc = _cat_rows(st, lambda l: l % 2 == 0)
        rn = _cat_rows(st, lambda l: l % 2 == 1)
        fused = bool(st.feat_fused) and not self.force_layers and all(isinstance(r, tuple) for r in (rc, rn) if r is not None)
        self.last_hop = 'fused' if fused else 'layers'
        for rows, X, w1, b1, w2, dx in ((rc, st.cell_feat, w1c, b1c, w2c, self._dx['cell_feat']),
                                        (rn, st.net_feat, w1n, b1n, w2n, self._dx['net_feat'])):
            if rows is None:
                continue
            if fused:
                ops.mlp2_feat_dx_bf16(st.G, X, rows, w1, b1, w2, dx=dx)
                continue
            Xv, idx = _rows_of(X, rows)
            Gv, _ = _rows_of(st.G, rows)
            Dv, _ = _rows_of(dx, rows)
            H = ops.linear_fwd(Xv, w1, b1, xidx=idx, act=ops.ACT_RELU)               # [n, 256], materialised
            dH = ops.linear_dgrad(Gv, w2, gidx=idx, mask=H)
            ops.linear_dgrad(dH, w1, dx=Dv, dxidx=idx)

    def _pin_moves(self, g):
        """proj_grad -> row_move -> pin_move (include/mmft_sens_pins.h): two launches on the current stream."""
        from . import fusion
        b, placed = self.batch, self.placed
        paths_d, foff_d = self._sel.paths, self._sel.feat_off
        self._proj = None
        if g is None:
            raise RuntimeError('Sensitivity(pins=True): the predictions do not depend on the masked projection')
        self.proj_grad = g = ops.strided_rows(g)      # a column slice of the head's dx: read in place
        wT = fusion.fc_weight_t(self.pmodel.fcn.weight)          # the cached transpose of this run's masked projection
        ops.pin_move_rows(placed.nodes, placed.lens, placed.loc_x, placed.loc_y, placed.map_x, placed.map_y, paths_d,
                          foff_d if b.B > 1 else None, self.feat_map.reshape(-1), wT, g, row_move=self.row_move)
        ops.pin_move_sum(self.row_move, *self._incidence, pin_move=self._pin_move)

    def run(self, weights=None, objective='tns'):
        """(pred, endpoints, grads).  pred [T] on the device and endpoints (host int64 [T]) are what Predictor.predict() returns;
        grads[i] = dict(cell_feat=[N_i, Fc], net_feat=[N_i, Fn]): fp32 device tensors in design i's own node order, the
        gradient of J = sum_r w_r pred_r.  weights: float32 [T], host or device, one per row of pred.  Without weights,
        objective='tns': w_r = 1 where required_r - pred_r < 0 on this call's own predictions (NaN rows get 0) - the gradient
        of the magnitude of the total negative slack; objective='sum': w_r = 1.  cell_feat gradients live on the rows of even
        levels, net_feat gradients on the rows of odd levels; every other row is exactly 0.  With image=True each
        dict also holds image=[3, H, W], the gradient with respect to the design's layout image; with pins=True pin_move=[N_i, 4],
        the change of J per one-cell move of each pin (class docstring)."""
        check_objective(objective)
        w = check_weights(weights, self.T)
        check_no_sinks(self.pmodel)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('Sensitivity.run() under an outer stream capture: the forward + backward pair runs eagerly '
                               '(its weights may depend on this call\'s predictions)')
        from .sweep import _MLP_KEYS, _mlp2_params
        if not any(p.requires_grad for k in _MLP_KEYS for p in _mlp2_params(getattr(self.pmodel.gnn, k))):
            raise RuntimeError('Sensitivity.run: no parameter of fc_cell_self / fc_net_self / fc_cell_neigh requires a gradient - the '
                               'sweep then runs in its forward-only form, which keeps nothing for a reverse sweep')
        if self.image:
            check_image_route(self.cnn, self.batch.images, self.frozen_stats)
        cur = torch.cuda.current_stream(self.device)
        with self._modes_kept(), frozen_statistics(self.cnn, self.frozen_stats):
            pred, st = self._forward()
            out = pred.detach()
            if w is not None:
                w = w.to(self.device, non_blocking=True).contiguous()
            elif objective == 'tns':
                w = ((self.required - out) < 0).to(torch.float32)
            else:
                w = torch.ones_like(out)
            inputs = [p for p in st.params if p.requires_grad]
            if self.pins:
                inputs = inputs + [self._proj]
            if self.image:
                inputs = inputs + [self._feat_leaf]
            got = torch.autograd.grad(pred, inputs, grad_outputs=w.reshape(pred.shape), allow_unused=True)
            if self.overlap:
                cur.wait_stream(self.side)            # the reverse sweep ran on the stream of its forward
            self._last_hop(st)
            if self.pins:
                self._pin_moves(got[-2] if self.image else got[-1])
            dimg = None
            if self.image:
                from . import unet16
                self.feat_grad = got[-1].reshape(self.batch.B, -1)
                dimg = unet16.unet_eval_input_grad(self.cnn, self._tape, self.feat_grad)
                self._tape = self._feat_leaf = None
        grads = [dict(cell_feat=self._dx['cell_feat'].index_select(0, p), net_feat=self._dx['net_feat'].index_select(0, p))
                 for p in self._perm]
        if dimg is not None:
            for i, gr in enumerate(grads):
                gr['image'] = dimg[i]                 # NCHW, the layout of DesignBatch.images: a view
        if self.pins:
            off = self.batch.node_off                 # PlacedPaths keeps the caller's numbering: a slice, no permutation
            for i, gr in enumerate(grads):
                gr['pin_move'] = self._pin_move[int(off[i]):int(off[i + 1])].clone()
        return out, self.endpoints, grads
