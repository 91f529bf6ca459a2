"""Levelized netlist sweep on the GPU: forward per level, deterministic reverse sweep, batched weight grads.

Mirrors PathConv.forward (reference src/model.py:158-213) one call per topological level, as the
reference loops demand (src/train.py:490-511), but keeps ONE set of [N, .] buffers updated in place
instead of DGL's out-of-place frame update per pull:

    h   [N, D]   node embeddings (= graph.ndata['h'], rows written once per sweep)
    A   [N, D]   softmax-weighted fan-in sums of cell-level nodes      LSE [N, D]  their log-sum-exp
    HS  [N, Hd]  hidden activations of the *_self MLPs                 HN  [N, Hd] of fc_cell_neigh
    G   [N, D]   d loss / d pre-activation (reverse sweep)             DA  [N, D]  d loss / d A

Every buffer but h is allocated by the first launch that needs it: a forward-only sweep (FORWARD_ONLY, under no_grad) of a
schedule whose cell levels all take a fused level kernel holds h and PRE alone.

Autograd sees a chain of LevelFn nodes linked by a 1-element token, so the engine runs the levels'
backward in strictly decreasing level order.  Each backward does: scatter the target gradients,
one pull kernel over the level's OUT-edges (no atomics, bitwise reproducible), and for cell levels the
two small GEMMs that turn G into DA.  Weight gradients are NOT computed per level: the level-0 node
(last to run) computes all of them in batched GEMMs over every node of the sweep.
"""
import contextlib
import torch
from . import ops, gradsink, lib

_MLP_KEYS = ('fc_cell_self', 'fc_net_self', 'fc_cell_neigh')


class SweepState:
    """State of one sweep of one graph.  Every field is declared here; __init__ gives each the value of a per-level sweep,
    the whole-sweep entry (_run_sweep, SweepFn) and the deferred head (model.py) overwrite theirs."""
    __slots__ = ('graph', 'h', 'N', 'D', 'Hd', 'relu', 'cell_feat', 'net_feat', 'params', 'need_grad', '_bufs',
                 'HN', 'G', 'DA', 'DHN', 'tflag', 'level_meta', 'levels', 'token', 'next_level',
                 'bwd_active', 'complete', 'fold', 'level_lists', 'PRE', 'attn', 'wpack', 'active', 'seed', 'record',
                 'spec_lists', 'spec_token', 'spec_tix', 'target_order', 'targets_unique',
                 'hid16', 'feat_fused', 'prep', 'row_sets', 'head_batch', '_empty_rows')
    # what a forward sweep decides and its backward needs: a replayed forward skips the code that sets these
    DECIDED = ('levels', 'wpack', 'hid16', 'HN', 'DHN', 'prep', 'row_sets', 'feat_fused', 'PRE', 'attn')
    assert set(DECIDED) <= set(__slots__)

    def decided(self):
        return {k: getattr(self, k) for k in self.DECIDED}

    def adopt(self, decided):
        for k, v in decided.items():
            setattr(self, k, v)

    def __init__(self, graph, conv):
        self.graph = graph
        h = graph.ndata['h']
        if not (torch.is_tensor(h) and h.is_cuda and h.dtype == torch.float32 and h.dim() == 2 and h.is_contiguous()):
            raise RuntimeError("PathConv: graph.ndata['h'] must be a contiguous float32 CUDA tensor [N, out_dim] "
                               "(the HIP sweep has no CPU fallback)")
        if h.shape[0] != graph.number_of_nodes() or h.shape[1] != conv.out_feat_dim:
            raise ValueError(f"graph.ndata['h'] has shape {tuple(h.shape)}, expected "
                             f"({graph.number_of_nodes()}, {conv.out_feat_dim})")
        self.h = h
        self.N, self.D = h.shape
        self.Hd = conv.fc_cell_self.layers[0].weight.shape[0]
        self.relu = conv.activation is not None
        self.cell_feat = _feat(graph, 'cell_feat', conv.cell_feat_dim)
        self.net_feat = _feat(graph, 'net_feat', conv.net_feat_dim)
        self.params = [p for k in _MLP_KEYS for p in _mlp2_params(getattr(conv, k))]
        self.need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.params)
        bufs = graph._sweep_bufs
        key = (self.N, self.D, self.Hd, h.device)
        if bufs.get('key') != key:
            bufs.clear()
            bufs['key'] = key
        self._bufs = bufs
        self.HN = None              # fc_cell_neigh's hidden rows: hidden_rows() / the whole-sweep entry; None: nothing kept
        self.G = self.DA = self.DHN = self.tflag = None
        self.level_meta = None      # per-level static facts (contiguous range, algorithmic bytes), whole-sweep entry
        self.levels = []            # (level_id, rows) in forward order
        self.token = None
        self.next_level = 0
        self.bwd_active = False
        self.complete = False               # level lists = a complete schedule of the graph (whole-sweep entry)
        self.fold = None                    # static facts for the folded level kernels (PinGraph.fold_schedule)
        self.level_lists = None
        self.PRE = None
        self.attn = None                    # attention branch (flag_attn): dict(key, c12, alpha, dcp, o2i)
        self.wpack = None                   # bf16 math mode: fc_cell_neigh pre-packed as bf16 (W1, W2, W2^T, W1^T)
        self.active = None                  # uint8 per node: fan-in cone of the step's endpoints (None: every node)
        self.seed = None                    # incremental sweep: uint8 per node, rows whose features changed (active = their fan-out)
        self.record = None                  # _SweepRecord of the schedule (static level lists), or None
        self.spec_lists = None              # speculative drop-in sweep: the level lists it ran with, its token, target rows
        self.spec_token = None
        self.spec_tix = []
        self.target_order = None
        self.targets_unique = None
        self.hid16 = self.feat_fused = False        # whole-sweep entry, bf16 mode: HN / DHN stored as bf16; *_self MLPs without HS
        self.prep = self.row_sets = None            # ... recorded launches (record.calls); rows of the (cell, net, cell >= 2) levels
        self.head_batch = self._empty_rows = None   # deferred head: model._HeadBatch of the step; [0, D] result of a level without endpoints

    def _buf(self, name, width, dtype=torch.float32):
        b = self._bufs.get(name)
        if b is None:
            # zeros, not empty: with fan-in-cone pruning rows outside the cone are never written, yet batched GEMMs read
            # them next to zero gradients - they must hold finite values
            b = torch.zeros((self.N, width), dtype=dtype, device=self.h.device)
            self._bufs[name] = b
        return b

    # allocated by the first launch that names them (a forward-only sweep of fused levels never does)
    A = property(lambda self: self._buf('A', self.D))
    LSE = property(lambda self: self._buf('LSE', self.D))
    HS = property(lambda self: self._buf('HS', self.Hd))

    def hidden_rows(self):
        """HN, the hidden activations of fc_cell_neigh: what the whole-sweep entry chose, else the fp32 buffer (first use allocates)."""
        if self.HN is None:
            self.HN = self._buf('HN', self.Hd)
        return self.HN

    def hidden_grads(self):
        """DHN, the hidden gradients of fc_cell_neigh, in the format the forward chose for HN; allocated on first use."""
        if self.DHN is None:
            self.DHN = self._buf('DHN16', self.Hd, torch.bfloat16) if self.hid16 else self._buf('DHN', self.Hd)
        return self.DHN

    @property
    def fast(self):
        """The reverse sweep may skip the fills of G / DA (2 x 268 MB per step at config B): the level lists are a complete
        schedule of the graph, so every row a pull reads was rewritten earlier in the same reverse sweep (a DA row by
        fc_cell_neigh's input gradient of its cell level >= 2).  A partial schedule (truncated lists; a per-level sweep may
        stop early) leaves consumers outside it with rows of an earlier step - or uninitialised memory - and fan-in-cone
        pruning skips rows, which must read as zero: both buffers are zero-filled, the own-gradient flags not used."""
        return self.complete and self.active is None

    def seed_targets(self, tix, gout, order=None, unique=None):
        """Zero / flag / fill the endpoint rows `tix` of G with `gout` (tix None or empty: only start the reverse sweep)."""
        self.begin_backward()
        if tix is not None and tix.numel():
            if self.fast:
                ops.target_rows_begin(self.G, tix, self.tflag)
            ops.scatter_add_targets(self.G, tix, ops.strided_rows(gout), order=order, unique=unique)

    def begin_backward(self):
        if not self.bwd_active:
            if self.G is None:
                self.G = self._buf('G', self.D)
                fresh = 'DA' not in self._bufs
                self.DA = self._buf('DA', self.D)
                if fresh:
                    self.DA.zero_()
            if self.fast:
                # only the sampled endpoints start with a gradient of their own; the reverse pull takes zero for every other row (flag per node)
                if 'tflag' not in self._bufs:
                    self._bufs['tflag'] = torch.zeros(self.N, dtype=torch.uint8, device=self.h.device)
                self.tflag = self._bufs['tflag']
            else:
                self.G.zero_()
                self.DA.zero_()
            self.bwd_active = True


def _attn_state(st, graph, c12):
    """Buffers of the attention branch (src/model.py:119-136,190-196): ndata['key'] as a flat vector, the two score
    coefficients on the device, alpha per cell in-edge, per-node score-gradient partials."""
    key = graph.ndata.get('key')
    if key is None:
        raise RuntimeError("PathConv(flag_attn=True) reads graph.ndata['key'] (src/model.py:132-136); no reference file "
                           "creates it (SURVEY D6) - provide a float32 [N, 1] tensor")
    if not (torch.is_tensor(key) and key.is_cuda and key.dtype == torch.float32 and key.numel() == st.N):
        raise RuntimeError("graph.ndata['key'] must be a float32 CUDA tensor with one value per node")
    E = graph.csr('in', 'cell')[1].numel()
    bufs = st._bufs
    if bufs.get('alpha') is None or bufs['alpha'].numel() != max(E, 1):
        bufs['alpha'] = torch.zeros(max(E, 1), dtype=torch.float32, device=st.h.device)
        bufs['dcp'] = torch.zeros((st.N, 2), dtype=torch.float32, device=st.h.device)
    return dict(key=key.reshape(-1).contiguous(), c12=c12.detach().reshape(2).contiguous(), alpha=bufs['alpha'],
                dcp=bufs['dcp'], o2i=graph.out2in('cell'))


def _cell_gather_fwd(st, g, rows):
    """A[rows] (and what the reverse sweep needs) for one cell level: per-channel softmax (src/model.py:113-116) or,
    with flag_attn, one softmax weight per edge (src/model.py:119-136)."""
    if st.attn is not None:
        a = st.attn
        ops.seg_attn_fwd(st.h, a['key'], a['c12'], g.csr('in', 'cell'), rows, st.A, a['alpha'])
    else:
        ops.seg_softmax_sum_fwd(st.h, g.csr('in', 'cell'), rows, st.A, st.LSE)


def _pull_bwd(st, g, rows, own=None, alg_bytes=0, heavy=None):
    if st.attn is not None:
        a = st.attn
        ops.level_bwd_pull_attn(st.G, st.h, rows, g.csr('out', 'net'), g.out_net_weight(), g.csr('out', 'cell'), a['o2i'],
                                a['alpha'], st.DA, relu=st.relu, own=own)
    else:
        ops.level_bwd_pull(st.G, st.h, rows, g.csr('out', 'net'), g.out_net_weight(), g.csr('out', 'cell'),
                           st.A, st.LSE, st.DA, relu=st.relu, alg_bytes=alg_bytes, own=own, heavy=heavy, active=st.active)


def _attn_scores_bwd(st, g, rows):
    a = st.attn
    ops.seg_attn_bwd_scores(st.DA, st.h, st.A, a['alpha'], a['key'], a['c12'], g.csr('in', 'cell'), rows, a['dcp'])


def _attn_c12_grad(st, rows):
    """d loss / d c12 (2, 1) = the column sums of the score-gradient partials of the cell rows (range or index)."""
    dcp = st.attn['dcp']
    if isinstance(rows, tuple):
        return ops.colsum(dcp[rows[0]:rows[0] + rows[1]]).reshape(2, 1)
    return ops.colsum(dcp, idx=rows).reshape(2, 1)


def _feat(graph, name, width):
    t = graph.ndata[name]
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2):
        raise RuntimeError(f"graph.ndata['{name}'] must be a float32 CUDA tensor")
    if t.shape[1] != width:
        raise ValueError(f"graph.ndata['{name}'] has {t.shape[1]} columns, the model expects {width}")
    if t.stride(1) != 1:
        t = t.contiguous()
        graph.ndata[name] = t
    return t


def _mlp2_params(mlp):
    lin = [m for m in mlp.layers if isinstance(m, torch.nn.Linear)]
    if len(lin) != 2 or len(mlp.layers) != 3 or getattr(mlp, 'negative_slope', 0) != 0:
        raise NotImplementedError('PathConv level kernels expect Linear-LeakyReLU(0)-Linear MLPs (src/model.py:48-51)')
    return [lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias]


def _w(p):
    d = p.detach()
    return d if d.is_contiguous() else d.contiguous()


def _cell_neigh_fwd(st, rows, w1g, b1g, w2g, b2g, act, keep=True):
    """h[rows] = act(h[rows] + fc_cell_neigh(A[rows])), HN[rows] saved: one fused launch when the widths allow.
    keep=False (forward-only sweep, bf16 mode): the hidden rows are not stored."""
    if st.wpack is not None:
        ops.mlp2_rows_bf16(st.A, rows, st.wpack[0], b1g, st.wpack[1], b2g, st.h, hid_out=st.hidden_rows() if keep else None,
                           add_act=True, relu_out=(act == ops.ACT_RELU), active=st.active)
    elif ops.mlp2_fusable(st.D, st.Hd, st.D):
        ops.mlp2_rows(st.A, rows, w1g, b1g, w2g, b2g, st.h, kmajor=False, hid_out=st.hidden_rows(), add_act=True,
                      relu_out=(act == ops.ACT_RELU), active=st.active)
    else:
        ops.linear_fwd(st.A, w1g, b1g, y=st.hidden_rows(), xidx=rows, yidx=rows, act=ops.ACT_RELU)
        ops.linear_fwd(st.HN, w2g, b2g, y=st.h, xidx=rows, yidx=rows, epi=ops.EPI_ADD_ACT, act=act)


def _cell_neigh_bwd(st, rows, w1g, w2g, keep_dhn=False):
    """DA[rows] = ((G[rows] W2g) * relu'(HN[rows])) W1g.  With keep_dhn the hidden gradient rows are also written to
    st.DHN, so the batched weight-gradient pass does not recompute them."""
    if ops.mlp2_fusable(st.D, st.Hd, st.D):
        dhn_out = st.hidden_grads() if keep_dhn else None
        if st.wpack is not None:
            ops.mlp2_rows_bf16(st.G, rows, st.wpack[2], None, st.wpack[3], None, st.DA, mask=st.HN, hid_out=dhn_out,
                               active=st.active)
            return
        ops.mlp2_rows(st.G, rows, w2g, None, w1g, None, st.DA, kmajor=True, mask=st.HN, hid_out=dhn_out, active=st.active)
    else:
        dhn = ops.linear_dgrad(st.G, w2g, gidx=rows, mask=st.HN, maskidx=rows)
        ops.linear_dgrad(dhn, w1g, dx=st.DA, dxidx=rows)


class LevelFn(torch.autograd.Function):
    """One PathConv.forward call. Inputs: chain token, the attention coefficients c12 (or None) (+ the 12 MLP parameters
    at level 0)."""

    @staticmethod
    def forward(ctx, token, state, level_id, rows, tix, c12, *params):
        st, g = state, state.graph
        if c12 is not None:
            st.attn = _attn_state(st, g, c12)
        P = [_w(p) for p in st.params]
        (w1c, b1c, w2c, b2c, w1n, b1n, w2n, b2n, w1g, b1g, w2g, b2g) = P
        n = rows.numel()
        act = ops.ACT_RELU if st.relu else ops.ACT_NONE
        if n:
            if level_id % 2 == 1:                                                     # net level :186-187
                ops.linear_fwd(st.net_feat, w1n, b1n, y=st.HS, xidx=rows, yidx=rows, act=ops.ACT_RELU)
                ops.linear_fwd(st.HS, w2n, b2n, y=st.h, xidx=rows, yidx=rows)
                ops.seg_mean_add_act_fwd(st.h, g.csr('in', 'net'), rows, relu=st.relu)
            elif level_id == 0:                                                       # :148-153
                ops.linear_fwd(st.cell_feat, w1c, b1c, y=st.HS, xidx=rows, yidx=rows, act=ops.ACT_RELU)
                ops.linear_fwd(st.HS, w2c, b2c, y=st.h, xidx=rows, yidx=rows, act=act)
            else:                                                                     # cell level :113-116,138-146
                _cell_gather_fwd(st, g, rows)
                ops.linear_fwd(st.cell_feat, w1c, b1c, y=st.HS, xidx=rows, yidx=rows, act=ops.ACT_RELU)
                ops.linear_fwd(st.HS, w2c, b2c, y=st.h, xidx=rows, yidx=rows)
                _cell_neigh_fwd(st, rows, w1g, b1g, w2g, b2g, act)
        st.levels.append((level_id, rows))
        out = ops.gather_rows(st.h, tix) if tix.numel() else st.h.new_zeros((0, st.D))       # :213
        ctx.state, ctx.level_id, ctx.rows, ctx.tix = st, level_id, rows, tix
        ctx.nparams = len(params)
        ctx.has_c12 = c12 is not None
        new_token = st.h.new_zeros(1)
        return new_token, out

    @staticmethod
    def backward(ctx, gtoken, gout):
        st, g, level_id, rows = ctx.state, ctx.state.graph, ctx.level_id, ctx.rows
        st.seed_targets(ctx.tix if gout is not None else None, gout, unique=g.targets_unique)
        P = [_w(p) for p in st.params]
        (w1c, b1c, w2c, b2c, w1n, b1n, w2n, b2n, w1g, b1g, w2g, b2g) = P
        dc = None
        if rows.numel():
            _pull_bwd(st, g, rows)
            if level_id % 2 == 0 and level_id > 0:
                _cell_neigh_bwd(st, rows, w1g, w2g)
                if ctx.has_c12 and st.attn is not None:
                    _attn_scores_bwd(st, g, rows)
                    dc = _attn_c12_grad(st, rows)
        grads = [None] * ctx.nparams
        if level_id == 0:
            if ctx.nparams:
                grads = _batched_param_grads(st, P)
            st.bwd_active = False
        return (torch.zeros_like(gtoken) if ctx.needs_input_grad[0] else None, None, None, None, None, dc, *grads)


def _cat_rows(st, pred):
    """Rows of the levels selected by `pred`, in level order: a (start, n) range when the levels are contiguous id
    ranges that follow each other (DesignBatch's renumbering makes them so), else one int32 index tensor."""
    sel = [(l, r) for (l, r) in st.levels if pred(l) and r.numel()]
    if not sel:
        return None
    if st.level_meta:
        rng = [st.level_meta[l]['range'] if st.level_meta[l] else None for l, _ in sel]
        if all(rng) and all(rng[i][0] + rng[i][1] == rng[i + 1][0] for i in range(len(rng) - 1)):
            return (rng[0][0], sum(n for _, n in rng))
    return sel[0][1] if len(sel) == 1 else torch.cat([r for _, r in sel])


def _rows_of(t, rows):
    """(tensor the kernel should see, index tensor or None) for a row set that is a range or an index tensor."""
    if isinstance(rows, tuple):
        return t[rows[0]:rows[0] + rows[1]], None
    return t, rows


def _linear_rows(x, w, b, y, rows, **kw):
    """y[rows] = epi(x[rows] @ w.T + b) for a range or an index row set."""
    xv, idx = _rows_of(x, rows)
    yv, _ = _rows_of(y, rows)
    return ops.linear_fwd(xv, w, b, y=yv, xidx=idx, yidx=idx, **kw)


def _mlp_grads(st, sinks, G, gidx, H, X, xidx, w2, dH_rows=None):
    """Gradients of one Linear-ReLU-Linear MLP over the rows `gidx`: (dW1, db1, dW2, db2); entries whose parameter
    has a gradient sink (mmft.gradsink) are written there and returned as None.
    dH_rows: [N, Hd] buffer already holding the hidden gradients of those rows (from the level loop)."""
    s1w, s1b, s2w, s2b = sinks
    Gv, gi = _rows_of(G, gidx)
    Hv, _ = _rows_of(H, gidx)
    Xv, xi = _rows_of(X, xidx)
    dW2, db2 = gradsink.deliver_pair(s2w, s2b, lambda ow, ob: ops.linear_wgrad(Gv, Hv, dw=ow, gidx=gi, xidx=gi, db=ob,
                                                                               with_bias=True))
    if dH_rows is not None:
        Dv, _ = _rows_of(dH_rows, gidx)
        dW1, db1 = gradsink.deliver_pair(s1w, s1b, lambda ow, ob: ops.linear_wgrad(Dv, Xv, dw=ow, gidx=gi, xidx=xi,
                                                                                   db=ob, with_bias=True))
    elif FUSED_FIRST_LAYER_GRADS and xidx is gidx and ops.first_layer_grads_fusable(X.shape[1], H.shape[1], G.shape[1]) \
            and w2.stride(0) % 4 == 0:
        # dH = (G W2) * relu'(H) never leaves the registers: one launch instead of GEMM -> 268 MB -> GEMM
        dW1, db1 = gradsink.deliver_pair(s1w, s1b, lambda ow, ob: ops.mlp2_first_layer_grads(G, H, X, gidx, w2, dw1=ow,
                                                                                             db1=ob))
    else:
        dH = ops.linear_dgrad(Gv, w2, gidx=gi, mask=Hv, maskidx=gi)
        dW1, db1 = gradsink.deliver_pair(s1w, s1b, lambda ow, ob: ops.linear_wgrad(dH, Xv, dw=ow, xidx=xi, db=ob,
                                                                                   with_bias=True))
    return [dW1, db1, dW2, db2]


def _batched_param_grads(st, P, dhn_ready=False):
    (w1c, b1c, w2c, b2c, w1n, b1n, w2n, b2n, w1g, b1g, w2g, b2g) = P
    # a sink is only usable when the kernel-side tensor IS the parameter's storage (contiguous weights)
    S = [gradsink.of(p) if p.is_contiguous() else None for p in st.params]
    rc = _cat_rows(st, lambda l: l % 2 == 0)
    rn = _cat_rows(st, lambda l: l % 2 == 1)
    rc2 = _cat_rows(st, lambda l: l % 2 == 0 and l > 0)
    zeros = lambda ps: [torch.zeros_like(p) for p in ps]
    if st.feat_fused:
        feat = lambda sinks, rows, X, w1, b1, w2: gradsink.deliver_many(
            sinks, lambda o1, ob1, o2, ob2: ops.mlp2_feat_bwd_bf16(st.G, X, rows, w1, b1, w2, dw1=o1, db1=ob1, dw2=o2, db2=ob2))
        gc = feat(S[0:4], rc, st.cell_feat, w1c, b1c, w2c) if rc is not None else zeros(P[0:4])
        gn = feat(S[4:8], rn, st.net_feat, w1n, b1n, w2n) if rn is not None else zeros(P[4:8])
    else:
        gc = _mlp_grads(st, S[0:4], st.G, rc, st.HS, st.cell_feat, rc, w2c) if rc is not None else zeros(P[0:4])
        gn = _mlp_grads(st, S[4:8], st.G, rn, st.HS, st.net_feat, rn, w2n) if rn is not None else zeros(P[4:8])
    gg = _mlp_grads(st, S[8:12], st.G, rc2, st.HN, st.A, rc2, w2g,
                    st.DHN if (dhn_ready and st.DHN is not None) else None) if rc2 is not None else zeros(P[8:12])
    return gc + gn + gg


def attention_coefficients(conv):
    """c12 (2, 1): <fc_attn.w[:dk], fc_key.w> and <fc_attn.w[dk:], fc_key.w> - the edge score of message_func_attn
    (src/model.py:132-136) is leaky_relu(c12[0] key_src + c12[1] key_dst) because fc_key / fc_attn have no bias.  One tiny
    GEMM through the autograd-aware dense kernel, so the gradient reaches both parameters."""
    from . import functional as MF
    dk = conv.fc_key.weight.shape[0]
    return MF.linear_act(conv.fc_attn.weight.view(2, dk), conv.fc_key.weight.view(1, dk), None, None)


def level_forward(conv, graph, cur_nodes, targets, level_id):
    """Body of PathConv.forward (both branches): one level of a speculative or of a strict per-level sweep."""
    spec = _start_sweep(conv, graph, cur_nodes) if level_id == 0 else (graph._sweep is not None and graph._sweep.spec_lists is not None)
    if not torch.is_tensor(cur_nodes):
        graph._seen_lists.append(cur_nodes)
    if not spec and (level_id == 0 or graph._sweep is None):
        if level_id != 0:
            raise RuntimeError('PathConv: a sweep must start at level 0 (src/train.py:489-490)')
        graph._sweep = SweepState(graph, conv)
    st = graph._sweep
    if st.h is not graph.ndata['h']:
        raise RuntimeError("graph.ndata['h'] was replaced in the middle of a sweep; restart from level 0")
    if level_id != st.next_level:
        raise RuntimeError(f'PathConv: levels must arrive in increasing order (got {level_id}, expected {st.next_level})')
    st.next_level = level_id + 1
    return (_spec_level if spec else _strict_level)(conv, graph, st, cur_nodes, targets, level_id)


def _start_sweep(conv, graph, cur_nodes):
    """Level-0 call: the lists the graph was just swept with become the ones to speculate with, and when this call's list
    is the first of them the WHOLE sweep runs now (SPECULATE below).  True when it did."""
    seen, spec = graph._seen_lists, graph._spec_lists
    if len(seen) >= 2 and (spec is None or len(seen) >= len(spec)):
        spec = graph._spec_lists = list(seen)            # the previous sweep's lists, levels 0 .. k
    del seen[:]
    if not (SPECULATE and spec is not None and not graph._spec_disabled and not torch.is_tensor(cur_nodes) and _same_list(cur_nodes, spec[0])):
        return False
    dev_ = graph.ndata['h'].device
    # (only with gradient sinks on every parameter - FlatAdam: parameters that accumulate through autograd's own
    # AccumulateGrad nodes, created under the caller's stream, would be fed from another stream)
    sinks_ = all(gradsink.of(p) is not None for k in _MLP_KEYS for p in _mlp2_params(getattr(conv, k)))
    if SPEC_SIDE_STREAM and sinks_ and not torch.cuda.is_current_stream_capturing():
        # the whole sweep runs on a stream of its own: its autograd node then runs its backward there as well, next to the
        # U-Net's backward on the caller's stream (the caller's loop has one stream; inside a captured step TrainStep forks
        # the streams itself).  The caller's stream waits for the sweep right away - every later level call reads h.
        side = graph._spec_stream
        if side is None or side.device != dev_:
            side = graph._spec_stream = torch.cuda.Stream(device=dev_)
        cur_ = torch.cuda.current_stream(dev_)
        side.wait_stream(cur_)
        with torch.cuda.stream(side):
            st, token = _run_sweep(conv, graph, spec, None)
        cur_.wait_stream(side)
    else:
        st, token = _run_sweep(conv, graph, spec, None)
    st.spec_lists, st.spec_token, st.spec_tix, st.next_level = spec, token, [], 0
    return True


def _spec_level(conv, graph, st, cur_nodes, targets, level_id):
    """One level of a speculative sweep: checks that the list is the one the level-0 call swept with, returns h[targets]."""
    if level_id >= len(st.spec_lists) or torch.is_tensor(cur_nodes) or not _same_list(cur_nodes, st.spec_lists[level_id]):
        graph._spec_lists = None
        if not st.need_grad:
            # inference with other lists than last time (e.g. validate() after a truncated sweep): the levels below this
            # one were computed from identical lists, so the sweep simply continues level by level from here
            graph._sweep = st = SweepState(graph, conv)
            st.next_level = level_id + 1
            return _strict_level(conv, graph, st, cur_nodes, targets, level_id)
        # training: the autograd node of the speculative sweep covers the recorded lists of ALL levels
        graph._spec_disabled = True
        graph._sweep = None
        raise RuntimeError(f'PathConv: level {level_id} arrived with a node list that differs from the one this graph was '
                           f'swept with before - the speculative whole-sweep of the level-0 call used the recorded lists. '
                           f'Speculation is now disabled for this graph: zero graph.ndata["h"] and run the step again '
                           f'(mmft.sweep.SPECULATE = False avoids the first failure for loops whose level lists change).')
    tix = graph.level_rows(level_id, targets, 'targets')
    if not tix.numel():
        if st._empty_rows is None:
            st._empty_rows = st.h.new_zeros((0, st.D))
        return st._empty_rows
    if st.need_grad:
        st.spec_tix.append(tix)
        if graph._head_takes_gradients:
            # the caller (PathModel's deferred head) gathers h[targets] inside its one-call level head and scatters the
            # endpoint gradients itself from its root node: no launch, no autograd node here
            return st.h.new_empty((tix.numel(), 0))
        return TargetGatherFn.apply(st.spec_token, st, tix, graph.targets_unique)
    return ops.gather_rows(st.h, tix)


def _strict_level(conv, graph, st, cur_nodes, targets, level_id):
    """One level of a strict per-level sweep: a LevelFn node on the sweep's token chain."""
    rows = graph.level_rows(level_id, cur_nodes, 'nodes')
    tix = graph.level_rows(level_id, targets, 'targets')
    c12 = None
    if getattr(conv, 'flag_attn', False) and level_id % 2 == 0:
        if level_id > 0:
            c12 = attention_coefficients(conv)                                           # src/model.py:132-136
        # second pull of the branch: ndata['h_drive'] = mean of net_feat over the NET in-edges (src/model.py:197-198)
        hd = graph.ndata.get('h_drive')
        if hd is None or hd.shape != st.net_feat.shape or hd.device != st.net_feat.device:
            hd = torch.zeros_like(st.net_feat)
            graph.ndata['h_drive'] = hd
        if rows.numel():
            ops.seg_mean_rows_any(st.net_feat, graph.csr('in', 'net'), rows, hd)
    token = st.h.new_zeros(1) if level_id == 0 else st.token
    params = st.params if (level_id == 0 and st.need_grad) else ()
    with contextlib.nullcontext() if st.need_grad else torch.no_grad():
        st.token, out = LevelFn.apply(token, st, level_id, rows, tix, c12, *params)
    return out


# ------------------------------------------------------------------------------------------------
# Whole-sweep entry: one autograd node for all L levels.
#   * the *_self MLPs do not depend on h, so they run ONCE over all nodes of a kind (three batched GEMM
#     pairs) and pre-fill h; the level-serial chain is then one gather kernel per net level and
#     gather + two GEMMs per cell level;
#   * targets are gathered once after the last level (rows are final once written);
#   * backward = scatter of all target gradients, the reverse pull sweep, batched weight gradients.
# Same arithmetic as the per-level path (same kernels, same per-row operation order).
# ------------------------------------------------------------------------------------------------
EDGE_DRIVERS = True                 # folded gather: per-edge driver table (3-deep load chain, four edges in flight)
FEAT_MLP_NO_HIDDEN = True           # bf16 mode: fc_cell_self / fc_net_self as one kernel each way, hidden activations recomputed
FUSE_LEVEL_FWD = True               # bf16 mode: folded gather + fused MLP of a level pair in one launch (mmft_level_fwd_bf16)
LEVEL_SLOTS = True                  # ... in its slot-table form where the level allows it (mmft_level_fwd_slots: fan-in <= 4, ranges)
RECORD_LAUNCHES = True              # eager sweeps: the per-level kernels' validated argument lists are kept and re-issued (ops.relaunch)
SPEC_SIDE_STREAM = True             # drop-in loop: the speculative whole sweep (and with it its backward) on a stream of its own
HIDDEN_BF16 = True                  # bf16 mode: fc_cell_neigh's hidden activations / hidden gradients stored as bf16
LEVEL_BWD_PAIRS = True              # reverse sweep: one launch per (cell level, net level above it) pair where the numbering
                                    # allows it (PinGraph.level_bwd_pairs; mmft_level_bwd_pair)
FOLD_LEVELS = True                  # folded forward chain (one gather per (net, cell) level PAIR) when the graph allows it
FUSED_FIRST_LAYER_GRADS = True      # mmft_mlp2_first_layer_grads for the *_self MLPs (False: dgrad GEMM + wgrad GEMM)
FORWARD_ONLY = True                 # a sweep without a backward (no_grad / frozen parameters, no attention branch) keeps nothing for
                                    # one: bf16 mode, folded chain - the fused levels run the *_infer kernels (no A / LSE / hidden
                                    # rows stored), heavy fan-in levels gather without LSE and run the MLP without hid_out


SWEEP_REPLAY = True      # drop-in loop: the speculative sweep's forward / reverse launches replayed from captured HIP graphs
# (tools/ab_dropin.py, flags toggled inside one process, config B, ms per drop-in step: plain 7.31, recorded launches
#  6.69, + own stream 6.59, + replay 5.94)


def _sweep_form(st, attn):
    """Which form a forward sweep of st's schedule takes (st.levels, st.level_meta, st.fold, st.need_grad set; attn: the
    attention branch runs) - decided HERE and nowhere else: SweepFn._forward_launches launches by it, incremental_supported
    answers from it.
      packed      bf16 mode and fusable widths: the level chain's MLP takes pre-packed bf16 weights
      r0s, rc2, rn, rc   the rows of level 0, of the cell levels >= 2, of the net levels, of all cell levels (range, index, None)
      hid16       bf16 mode on range-numbered graphs: fc_cell_neigh's hidden activations and their gradients are STORED as bf16 -
                  every consumer rounds them to bf16 anyway (MFMA operands of the weight gradients) or reads the sign only (ReLU
                  mask); only the first layer's bias gradient then sums the rounded hidden gradients instead of the fp32 ones
      fold        the folded chain's static facts, or None
      fwd_only    nobody will ask for this sweep's backward.  Only the bf16 folded chain has launches that keep less; fp32 mode,
                  the attention branch and unfolded schedules run what they always ran
      feat_fused  bf16 mode: the feature MLPs run as one kernel each and their hidden activations (268 MB per MLP at config B)
                  are never stored - the backward recomputes them (mmft_mlp2_feat_*); needs contiguous row ranges"""
    packed = lib.get_math_mode() == 'bf16' and ops.mlp2_fusable(st.D, st.Hd, st.D)
    r0s = _cat_rows(st, lambda l: l == 0)
    rc2 = _cat_rows(st, lambda l: l % 2 == 0 and l > 0)
    rn = _cat_rows(st, lambda l: l % 2 == 1)
    rc = _cat_rows(st, lambda l: l % 2 == 0)
    fold = st.fold if (FOLD_LEVELS and not attn) else None
    return dict(packed=packed, r0s=r0s, rc2=rc2, rn=rn, rc=rc, fold=fold,
                hid16=bool(HIDDEN_BF16 and packed and isinstance(rc2, tuple) and not attn),
                fwd_only=bool(FORWARD_ONLY and not st.need_grad and not attn and packed and fold is not None),
                feat_fused=bool(FEAT_MLP_NO_HIDDEN and packed and all(isinstance(r, tuple) for r in (r0s, rc2, rn) if r is not None)
                                and isinstance(rc, tuple) and ops.mlp2_feat_fusable(st.cell_feat.shape[1], st.Hd, st.D)
                                and ops.mlp2_feat_fusable(st.net_feat.shape[1], st.Hd, st.D)))


class _SweepRecord:
    """What eager sweeps of one schedule keep from step to step while the level list objects and the addresses of h, the
    features, the parameters and their gradient sinks stay (`sig`; the graph's buffers are persistent): `calls`, recorded
    launches of the two per-level kernels (ops.relaunch); `fwd` / `bwd`, the drop-in loop's level-0 sweep (~45 + ~70
    launches) as graphs, `state` the sweep state a replayed forward stands for; `keep` = (slot tables, reverse pair tables)
    that all of these read, which PinGraph's LRU may drop.  The sampled endpoints are handled by the per-level nodes."""
    def __init__(self, sig, lists):
        self.sig, self.lists, self.calls, self.state, self.keep = sig, lists, {}, None, (None, None)
        self.fwd, self.bwd = lib.GraphReplay(), lib.GraphReplay()


def _sweep_record(st):
    """The record of this sweep's schedule, or None (no static level lists, a fan-in cone, non-contiguous parameters)."""
    if st.level_lists is None or st.active is not None or not all(p.is_contiguous() for p in st.params):
        return None
    sinks = [gradsink.of(p) for p in st.params]
    sig = (tuple(id(n) for n in st.level_lists), lib.get_math_mode(), HIDDEN_BF16, st.relu, st.h.data_ptr(),
           tuple(p.data_ptr() for p in st.params), tuple(r[0].data_ptr() if r is not None else 0 for r in sinks),
           st.cell_feat.data_ptr(), st.net_feat.data_ptr())
    rec = st._bufs.get('replay')
    if rec is None or rec.sig != sig:
        rec = st._bufs['replay'] = _SweepRecord(sig, list(st.level_lists))     # (the lists are pinned: ids stay theirs)
    return rec


def _pinned(st, i, build):
    """build(level lists) - PinGraph.level_slots (i = 0) or .level_bwd_pairs (i = 1) - held in the sweep record's keep."""
    rec = st.record
    if rec is not None and rec.keep[i] is None:
        rec.keep = rec.keep[:i] + (build(st.level_lists),) + rec.keep[i + 1:]
    return build(st.level_lists) if rec is None else rec.keep[i]


def _recorded(prep, key, name, dev, stream, build):
    """The launch of entry point `name` that the sweep record holds under `key` (prep = its `calls`), issued again on `stream`;
    the first time build() - the checked ops wrapper - issues it and what it returns is kept.  prep None: no record, build()."""
    rec = prep.get(key) if prep is not None else None
    if rec is not None:
        ops.relaunch(name, rec, dev, stream)
    elif prep is not None:
        prep[key] = build()
    else:
        build()


class SweepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, level_rows, tix, c12, anchor, *params):
        st, g = state, state.graph
        st.record = rec = _sweep_record(st)
        ctx.state, ctx.tix, ctx.nparams, ctx.has_c12 = st, tix, len(params), c12 is not None
        # graph replay: speculative mode only (no target gather inside the node), gradient sinks on every parameter, bf16 mode,
        # no profiler, no outer capture
        ctx.replay = rec if (SWEEP_REPLAY and rec is not None and tix is None and c12 is None and st.need_grad and not lib.PROF_ON
                             and not torch.cuda.is_current_stream_capturing() and lib.get_math_mode() == 'bf16'
                             and all(gradsink.of(p) is not None for p in st.params)) else None
        launches = lambda: SweepFn._forward_launches(st, g, level_rows, c12)
        if ctx.replay is None:
            launches()
        else:
            if rec.fwd.graph is not None:
                st.adopt(rec.state)
            rec.fwd.run(launches)
            rec.state = st.decided()
        if tix is None:
            # speculative drop-in sweep: the per-level target gathers (TargetGatherFn) hang off this token
            return st.h.new_zeros(1)
        return ops.gather_rows(st.h, tix) if tix.numel() else st.h.new_zeros((0, st.D))

    @staticmethod
    def _forward_launches(st, g, level_rows, c12):
        """Every launch of the forward sweep (and the python-side state of `st` the backward needs)."""
        st.attn = _attn_state(st, g, c12) if c12 is not None else None
        P = [_w(p) for p in st.params]
        (w1c, b1c, w2c, b2c, w1n, b1n, w2n, b2n, w1g, b1g, w2g, b2g) = P
        act = ops.ACT_RELU if st.relu else ops.ACT_NONE
        st.levels = [(l, r) for l, r in enumerate(level_rows)]
        form = _sweep_form(st, c12 is not None)
        st.wpack = None
        if form['packed']:
            # the level chain's fused MLP takes its weights pre-packed as bf16 (forward: W1, W2; reverse: W2^T, W1^T)
            # (static buffers per graph: their addresses are part of the recorded launches below)
            wp = st._bufs.get('wpack')
            if wp is None or wp[0].device != st.h.device:
                mk = lambda *shape: torch.empty(shape, dtype=torch.bfloat16, device=st.h.device)
                wp = st._bufs['wpack'] = (mk(st.Hd, st.D), mk(st.D, st.Hd), mk(st.Hd, st.D), mk(st.D, st.Hd))
            st.wpack = (ops.pack_bf16(w1g, out=wp[0]), ops.pack_bf16(w2g, out=wp[1]), ops.pack_bf16(w2g, transpose=True, out=wp[2]),
                        ops.pack_bf16(w1g, transpose=True, out=wp[3]))
        r0s, rc2, rn, fold, fwd_only = form['r0s'], form['rc2'], form['rn'], form['fold'], form['fwd_only']
        st.hid16, st.feat_fused, st.row_sets = form['hid16'], form['feat_fused'], (form['rc'], rn, rc2)
        st.HN = None if fwd_only else (st._buf('HN16', st.Hd, torch.bfloat16) if st.hid16 else st._buf('HN', st.Hd))
        st.DHN = None
        # recorded launches of the two per-level kernels (ops.relaunch), kept in the sweep's record
        st.prep = prep = st.record.calls if (RECORD_LAUNCHES and st.record is not None) else None
        dev_, stream_ = lib.stream_args(st.h)
        # incremental sweep (sweep_forward_all(incremental=)): h and PRE hold the previous sweep's values and only stale rows
        # are written again.  A row that depends on features alone - level 0, PRE - is stale where the features changed
        # (seed); a cell row of a level >= 2 holds its self term before its level runs and its final value afterwards, so it
        # gets the self term again exactly where its level launch will run (dirty = st.active), and nowhere else
        seed, dirty = st.seed, (st.active if st.seed is not None else None)
        if seed is not None and not (fwd_only and st.feat_fused):
            raise RuntimeError('sweep_forward_all(incremental=): needs the forward-only folded bf16 sweep with fused feature MLPs '
                               '(bf16 math mode, a foldable schedule, no attention branch, no gradient) - every other path ignores '
                               '`active` somewhere and would leave stale rows; sweep.incremental_supported() tells beforehand')
        if r0s is not None:                                                              # level 0, :148-153
            if st.feat_fused:
                ops.mlp2_feat_fwd_bf16(st.cell_feat, r0s, w1c, b1c, w2c, b2c, st.h, relu_out=st.relu, active=seed)
            else:
                _linear_rows(st.cell_feat, w1c, b1c, st.HS, r0s, act=ops.ACT_RELU)
                _linear_rows(st.HS, w2c, b2c, st.h, r0s, act=act)
        if rc2 is not None:                                                              # fc_cell_self, all cell nodes
            if st.feat_fused:
                ops.mlp2_feat_fwd_bf16(st.cell_feat, rc2, w1c, b1c, w2c, b2c, st.h, active=dirty)
            else:
                _linear_rows(st.cell_feat, w1c, b1c, st.HS, rc2, act=ops.ACT_RELU)
                _linear_rows(st.HS, w2c, b2c, st.h, rc2)
        if fold is not None:
            # fc_net_self outputs live apart from h: the folded gather updates h in place.  PRE (like the weight packs above)
            # is a buffer of graph._sweep_bufs and PERSISTS from sweep to sweep: that is what makes an incremental sweep
            # correct - a net row whose features did not change still finds its fc_net_self output here, and a level kernel
            # that recomputes a clean in-neighbour from PRE gets the value h holds for it
            st.PRE = st._buf('PRE', st.D)
        if rn is not None:                                                               # fc_net_self, all net nodes
            if st.feat_fused:
                ops.mlp2_feat_fwd_bf16(st.net_feat, rn, w1n, b1n, w2n, b2n, st.PRE if fold is not None else st.h, active=seed)
            else:
                _linear_rows(st.net_feat, w1n, b1n, st.HS, rn, act=ops.ACT_RELU)
                _linear_rows(st.HS, w2n, b2n, st.PRE if fold is not None else st.h, rn)
        in_net, in_cell = g.csr('in', 'net'), g.csr('in', 'cell')
        if fold is not None:
            # folded chain: one gather launch per (net level l - 1, cell level l) pair + the fused MLP of the cell level
            L = len(level_rows)
            drv = g.cell_edge_drivers() if EDGE_DRIVERS else None
            slot_tabs = _pinned(st, 0, g.level_slots) if (LEVEL_SLOTS and FUSE_LEVEL_FWD and st.wpack is not None
                                                          and st.level_lists is not None) else None
            for level_id in range(2, L + 1, 2):
                net_l = level_id - 1
                has_cell = level_id < L and level_rows[level_id].numel() > 0
                if not has_cell and not fold[net_l]['n']:
                    continue
                meta_n = st.level_meta[net_l] if st.level_meta else None
                meta_c = st.level_meta[level_id] if (st.level_meta and level_id < L) else None
                crow = None
                if has_cell:
                    crow = fold[level_id]['range'] or level_rows[level_id]
                fused = has_cell and st.wpack is not None and fold[level_id]['heavy_in'] is None and FUSE_LEVEL_FWD
                # gather bytes of the pair + what the MLP part must move per cell row: h read and written (2 x 4 D) and the
                # hidden row kept for the reverse sweep (4 Hd or 2 Hd)
                kept_bytes = level_rows[level_id].numel() * (8 * st.D + (2 if st.hid16 else 4) * st.Hd) if (meta_c and has_cell) else 0
                level_bytes = (meta_n['bytes_mean'] if meta_n else 0) + (meta_c['bytes_softmax'] if meta_c else 0) + kept_bytes
                if fused:
                    # bf16 mode: gather + fc_cell_neigh of the pair in ONE launch, its form picked here.  Slot form: the static slot
                    # table instead of the per-edge index chain, net rows inside the cell workgroups; only its launches are recorded.
                    # Forward-only form: a key of its own (a training step after this sweep must not re-issue a launch that leaves
                    # A / LSE stale); bytes: A and LSE - which happen to weigh what h read + written does - and the hidden row are
                    # not moved
                    slot = slot_tabs is not None and fold[level_id]['range'] is not None and slot_tabs[2][level_id] <= 4 and \
                        (fold[net_l]['range'] is not None or not fold[net_l]['n'])
                    fn = (ops.level_fwd_slots_infer if slot else ops.level_fwd_bf16_infer) if fwd_only else \
                        (ops.level_fwd_slots if slot else ops.level_fwd_bf16)

                    def build():
                        net_range = fold[net_l]['range'] or (0, 0)
                        tabs = (slot_tabs[0], slot_tabs[1], net_range, fold[level_id]['range']) if slot else (in_net, in_cell, net_range, crow)
                        kept, hid = ((), ()) if fwd_only else ((st.A, st.LSE), (st.HN,))
                        opts = {} if slot else {'in_cell_driver': drv}
                        return fn(st.h, st.PRE, *tabs, *kept, st.wpack[0], b1g, st.wpack[1], b2g, *hid, relu=st.relu, active=st.active,
                                  alg_bytes=level_bytes - (kept_bytes if fwd_only else 0), **opts)
                    _recorded(prep if slot else None, ('fi' if fwd_only else 'f', level_id), 'mmft_' + fn.__name__, dev_, stream_, build)
                    continue
                # (forward-only: A is the transient between the two launches, LSE is not written, the hidden rows are not stored)
                ops.pair_fwd_gather(st.h, st.PRE, in_net, in_cell, fold[net_l]['range'] or (0, 0), crow,
                                    st.A if has_cell else None, None if (fwd_only or not has_cell) else st.LSE, relu=st.relu,
                                    heavy=fold[level_id]['heavy_in'] if has_cell else None, active=st.active, in_cell_driver=drv,
                                    alg_bytes=(meta_n['bytes_mean'] if meta_n else 0) + (meta_c['bytes_softmax'] if (meta_c and has_cell) else 0))
                if has_cell:
                    _cell_neigh_fwd(st, level_rows[level_id], w1g, b1g, w2g, b2g, act, keep=not fwd_only)
        for level_id, rows in enumerate(level_rows):
            if fold is not None or level_id == 0 or not rows.numel():
                continue
            meta = st.level_meta[level_id] if st.level_meta else None
            spec = meta['range'] if (meta and meta['range']) else rows       # contiguous levels: no index array
            if level_id % 2 == 1:
                ops.seg_mean_add_act_fwd(st.h, in_net, spec, relu=st.relu, alg_bytes=meta['bytes_mean'] if meta else 0)
            elif st.attn is not None:
                _cell_gather_fwd(st, g, spec)
                _cell_neigh_fwd(st, rows, w1g, b1g, w2g, b2g, act)
            else:
                ops.seg_softmax_sum_fwd(st.h, in_cell, spec, st.A, st.LSE, alg_bytes=meta['bytes_softmax'] if meta else 0)
                _cell_neigh_fwd(st, rows, w1g, b1g, w2g, b2g, act)

    @staticmethod
    def backward(ctx, gout):
        st, g = ctx.state, ctx.state.graph
        if ctx.tix is not None:
            st.bwd_active = False
        fast, tix = st.fast, ctx.tix
        st.seed_targets(tix, gout, st.target_order, st.targets_unique)
        own = st.tflag if fast else None
        if tix is None:
            # the TargetGatherFn nodes of this sweep have already zeroed / flagged / filled their rows of G
            tix = torch.cat(st.spec_tix) if st.spec_tix else st.h.new_zeros(0, dtype=torch.int32)
        rec, sinks = ctx.replay, [gradsink.of(p) for p in st.params]
        launches = lambda: SweepFn._backward_launches(ctx, st, g, fast, own)
        if not (rec is not None and fast and ctx.nparams == len(st.params) and not torch.cuda.is_current_stream_capturing()
                and not lib.PROF_ON and all(r is not None and r[1] != gradsink._epoch[0] for r in sinks)):   # sinks fresh
            grads = launches()
        elif rec.bwd.graph is not None:
            st.DHN = st._bufs.get('DHN16' if st.hid16 else 'DHN')
            rec.bwd.run(launches)
            for r in sinks:
                gradsink._mark(r)
            grads = [None] * ctx.nparams
        else:
            grads = rec.bwd.run(launches)
        dc = None
        if ctx.has_c12:
            rc2 = st.row_sets[2]
            dc = _attn_c12_grad(st, rc2) if rc2 is not None else torch.zeros((2, 1), dtype=torch.float32, device=st.h.device)
        if tix.numel() and fast:
            ops.target_rows_end(tix, st.tflag)
        st.bwd_active = False
        # `anchor` (see _run_sweep): a defined gradient, so that its AccumulateGrad node - a function without outputs, living on
        # this node's stream - makes the engine join that stream with the caller's at the end of backward()
        ga = st.h.new_empty(1) if ctx.needs_input_grad[4] else None      # its value is never read: no fill launch
        return (None, None, None, dc, ga, *grads)

    @staticmethod
    def _backward_launches(ctx, st, g, fast, own):
        """The reverse sweep's launches between the endpoint scatter and the flag reset: level chain + batched weight gradients."""
        P = [_w(p) for p in st.params]
        w1g, w2g = P[8], P[10]
        out_net, out_cell, in_net_ptr = g.csr('out', 'net'), g.csr('out', 'cell'), g.out_net_weight()
        pairs = None
        if LEVEL_BWD_PAIRS and fast and st.fold is not None and st.wpack is not None and st.attn is None \
                and st.level_lists is not None:
            pairs = _pinned(st, 1, g.level_bwd_pairs)
        paired = set()
        prep = st.prep if fast else None
        dev_b, stream_b = lib.stream_args(st.h)
        if pairs is not None:
            cslots, plist, pscratch, pcounters = pairs
            st.hidden_grads()
        for level_id, rows in reversed(st.levels):
            if level_id in paired:
                continue
            if pairs is not None:
                # one launch for the pair (cell level l, net level l + 1): the net level comes first in this reverse order
                cell_l = level_id - (level_id % 2)
                pr = plist[cell_l // 2]
                if pr is not None:
                    paired.add(cell_l)
                    mc = st.level_meta[cell_l] if st.level_meta else None
                    mn = st.level_meta[cell_l + 1] if (st.level_meta and cell_l + 1 < len(st.level_meta)) else None
                    nb = (mc['bytes_pull'] if mc else 0) + (mn['bytes_pull'] if mn else 0) + \
                        (pr['n_cell'] * (8 * st.D + (4 if st.hid16 else 8) * st.Hd) if cell_l > 0 else 0)
                    _recorded(prep, ('b', cell_l), 'mmft_level_bwd_pair', dev_b, stream_b, lambda: ops.level_bwd_pair(
                        st.G, st.h, st.A, st.LSE, st.DA, own, pr['tiles'], pr['ntiles'], out_net[0], pr['sink_shift'], cslots, out_cell,
                        pscratch, pcounters, st.wpack[2], st.wpack[3], st.HN, st.DHN, relu=st.relu, has_mlp=cell_l > 0, alg_bytes=nb))
                    continue
            if not rows.numel():
                continue
            meta = st.level_meta[level_id] if st.level_meta else None
            spec = meta['range'] if (meta and meta['range']) else rows
            _pull_bwd(st, g, spec, own=own, alg_bytes=meta['bytes_pull'] if meta else 0,
                      heavy=meta['heavy_out'] if meta else None)
            if level_id % 2 == 0 and level_id > 0:
                # (cone pruning: the hidden gradients of skipped rows would be stale - recompute them from G = 0 instead)
                _cell_neigh_bwd(st, rows, w1g, w2g, keep_dhn=st.active is None)
                if ctx.has_c12:
                    _attn_scores_bwd(st, g, spec)
        return _batched_param_grads(st, P, dhn_ready=st.active is None) if ctx.nparams else []


class TargetGatherFn(torch.autograd.Function):
    """h[targets] of one level of a SPECULATIVE drop-in sweep (the whole sweep ran at the level-0 call).  Backward: zero,
    flag and fill the endpoint rows of G - the reverse sweep itself is SweepFn.backward, which the engine runs after
    every node that consumes the sweep's token."""

    @staticmethod
    def forward(ctx, token, state, tix, unique):
        ctx.state, ctx.tix, ctx.unique = state, tix, unique
        return ops.gather_rows(state.h, tix)

    @staticmethod
    def backward(ctx, gout):
        ctx.state.seed_targets(ctx.tix, gout, unique=ctx.unique)
        return ctx.state.h.new_zeros(1), None, None, None


def _set_schedule(st, graph, conv, level_nodes):
    """The schedule's facts on a fresh sweep state (complete, fold, level_lists, level_meta); returns the levels' row tensors."""
    st.complete = graph.level_set_is_complete(level_nodes)
    st.fold = graph.fold_schedule(level_nodes) if (FOLD_LEVELS and st.complete and not getattr(conv, 'flag_attn', False)) else None
    st.level_lists = level_nodes if st.fold is not None else None       # key of the static slot tables (PinGraph.level_slots)
    st.level_meta = [graph.level_meta(l, nodes, st.D) if not torch.is_tensor(nodes) else None
                     for l, nodes in enumerate(level_nodes)]
    return [graph.level_rows(l, nodes, 'nodes') for l, nodes in enumerate(level_nodes)]


def _run_sweep(conv, graph, level_nodes, tix, target_order=None, targets_unique=None, active=None, seed=None):
    """Build the sweep state for the given level lists and run SweepFn (tix None: deferred per-level target gathers)."""
    graph._sweep = st = SweepState(graph, conv)
    st.active, st.seed = active, seed
    st.target_order, st.targets_unique = target_order, targets_unique
    if seed is not None and st.need_grad:
        raise RuntimeError('sweep_forward_all(incremental=): a sweep that will be differentiated runs over every row')
    level_rows = _set_schedule(st, graph, conv, level_nodes)
    st.next_level = len(level_rows)
    c12 = None
    if getattr(conv, 'flag_attn', False):
        c12 = attention_coefficients(conv)
        hd = torch.zeros_like(st.net_feat)                     # ndata['h_drive'] of the even levels (src/model.py:197-198)
        for l in range(0, len(level_rows), 2):
            if level_rows[l].numel():
                ops.seg_mean_rows_any(st.net_feat, graph.csr('in', 'net'), level_rows[l], hd)
        graph.ndata['h_drive'] = hd
    if st.need_grad or (c12 is not None and c12.requires_grad):
        # The sweep may run on a stream of its own and, with gradient sinks, returns no gradient to any leaf: nothing would
        # tell the engine to join that stream when backward() ends (it joins the streams of functions WITHOUT outputs, i.e.
        # of AccumulateGrad nodes that ran).  A one-element leaf created here, on the sweep's stream, is that node.
        anchor = st.h.new_empty(1, requires_grad=True)                   # (neither its value nor its gradient is ever read)
        return st, SweepFn.apply(st, level_rows, tix, c12, anchor, *st.params)
    with torch.no_grad():
        return st, SweepFn.apply(st, level_rows, tix, c12, None)


def _level_specs(graph, level_nodes):
    """Per level its (start, n) range where the list is one, else its device row tensor: what the cone launches take."""
    specs = []
    for l, nodes in enumerate(level_nodes):
        meta = graph.level_meta(l, nodes) if not torch.is_tensor(nodes) else None
        specs.append(meta['range'] if (meta and meta['range']) else graph.level_rows(l, nodes, 'nodes'))
    return specs


def incremental_supported(conv, graph, level_nodes):
    """True when a sweep of these lists, now, takes the one form in which every launch honours `active` - the forward-only
    folded bf16 sweep with fused feature MLPs (bf16 math mode, a foldable schedule of contiguous level ranges, no attention
    branch, no gradient) - so that sweep_forward_all(incremental=) is allowed.  The answer is _sweep_form's, the function
    SweepFn._forward_launches launches by."""
    st = SweepState(graph, conv)
    st.levels = list(enumerate(_set_schedule(st, graph, conv, level_nodes)))
    form = _sweep_form(st, bool(getattr(conv, 'flag_attn', False)))
    return form['fwd_only'] and form['feat_fused']


def sweep_forward_all(conv, graph, level_nodes, targets, target_order=None, targets_unique=None, cone=False, incremental=None):
    """All levels of one sweep in one call. level_nodes: list (per level) of python int lists or device int32
    tensors; targets: device int32 tensor (or list) of node ids whose embeddings are returned, in order.
    target_order: optional device int32 stable argsort of `targets` (the host has it for free when it packs a
    step's endpoints); targets_unique: True when the caller knows that no endpoint is repeated.
    cone=True: fan-in-cone pruning (the reference carries the idea unused, src/MyDataloader.py:4-59) -
    the level kernels skip every node that cannot influence `targets`.  The cone is a per-node flag array built ON THE
    DEVICE by L - 1 fixed-size launches (mmft_fanin_cone_step), the launches of the sweep keep their full grids and
    skip flagged-off rows, so a captured HIP graph of the step stays valid while the sampled endpoints - and with them
    the cone - change from replay to replay.
    incremental=(seed, dirty), two uint8[N] device arrays the caller owns: graph.ndata['h'] holds the result of an earlier
    sweep of the same lists with the same parameters, and since then only the feature rows flagged in `seed` changed.  The
    sweep writes `dirty` = the seeds and their transitive fan-out (prep.fanout_cone_mask; intersected with the fan-in cone
    under cone=True) and runs over those rows alone; every other row of h keeps its value, which is the value a full sweep
    would give it.  Only where incremental_supported() holds - anywhere else this raises.  `seed` is read, not cleared."""
    tix = graph.level_rows(-1, targets, 'sweep_targets')
    active = seed = None
    if cone or incremental is not None:
        from . import prep
        specs, csrs = _level_specs(graph, level_nodes), [graph.csr('in', 'net'), graph.csr('in', 'cell')]
    if cone:
        active = graph._cone_mask = prep.cone_mask(csrs, specs, tix, out=graph._cone_mask)
    if incremental is not None:
        seed, dirty = incremental
        active = prep.fanout_cone_mask(csrs, specs, seed, within=active, out=dirty)
        if active is not dirty:
            raise ValueError('sweep_forward_all(incremental=): dirty must be a contiguous uint8[N] tensor on the graph\'s device')
    return _run_sweep(conv, graph, level_nodes, tix, target_order, targets_unique, active, seed)[1]


# Speculative drop-in sweep.  The reference loop calls the model once per level with the SAME node lists every step
# (topo_levels of the design, src/train.py:490-503) and nothing a later call passes can change what an earlier level
# computes, so once a graph has been swept level by level with some lists, the next level-0 call runs the WHOLE sweep with
# them (the whole-sweep kernels: batched *_self MLPs, folded gathers, one autograd node) and every level call then only
# checks that its list is the recorded one and gathers h[targets].  A call whose list differs raises; set
# mmft.sweep.SPECULATE = False for loops that change their level lists between steps.
SPECULATE = True


def _same_list(a, b):
    return a is b or (len(a) == len(b) and (not len(a) or (a[0] == b[0] and a[-1] == b[-1] and a == b)))
