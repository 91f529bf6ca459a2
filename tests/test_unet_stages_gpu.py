"""Every stage of one real bf16-storage U-Net train step (mmft/unet16.py) against the fp64 stage reference, teacher-forced.

The step is driven the way UNet16Fn's eager branch drives it - the same _Packs, arenas, sinks, _run_forward and
_run_backward, on arenas this file owns - and is first shown to BE the product's step: a fresh copy of the network run
through the public `net(x)` / `backward` gives the same output, parameter gradients and running statistics bit for bit.
Then every stage's own inputs are copied out of the HIP arenas and tests/unet_stage_oracle.py computes that stage from
them in fp64 (`ref`) and in fp32 (`ref32`); the wiring - which buffer, which channel slice, which gradient target - comes
from the oracle's table, not from the product's.  Because each stage starts from the step's stored operands, the
amplification through 14 chained BatchNorm layers that loosens the whole-network bounds (test_bf16_oracle_gpu.py) does
not apply, and any wrong stage or wire changes most elements of a row.

Rules (every row is printed before the test fails):
  * tensors stored as bf16 (z, a, pooled, the transposed convolution's slice, g, dz, gcat, gp, OutConv dx):
      - bitwise where only exact decisions are made from stored values: max pooling and the pool backward with skip add;
      - every element within one bf16 step of the larger of the two values plus (n - 1) 2^-24 sum|terms| (1 + 1e-3), the
        sum of |terms| from the same stage on |operands| in fp64;
      - the share of elements that differ from `ref` at all is at most 1e-3 per tensor (test_unet_stages_cpu.py holds the
        fp32 evaluation below a third of that at these seeds);
  * fp32 results: e_hip <= max(floor, 3 e_32) in relative max norm, e_32 = ref32 against ref; floors 1e-6 (mean, invstd,
    var, scale, running statistics), 1e-5 (shift, output), 1e-4 (dgamma, dbeta), 2e-6 (every dW and db);
  * both halves of a concatenation buffer are compared at their channel offsets (after the step: the half a stage must
    not write holds the other stage's checked result), and the padding between the arenas' regions keeps its fill;
  * running_var has a second row under the same floor on what the step ADDED to it (the buffer minus 0.9^N of its start):
    the buffer starts at 1, which hides a first layer's variance of a few 1e-2 from a relative bound.
Teeth: the stage reference with ONE deliberate error (the mutants listed in MUTANTS) must miss the HIP result by 10 x the
row's bound, or differ in more than 10 x the share cap of a stored tensor; every layer the mutant applies to is checked.

Measured on one MI355X, worst row of each kind over the three geometries.  fp32 rows, e_hip / e_32 / largest e_hip : e_32
of one row:
  mean 6.5e-8 / 1.3e-7 / 1.5        invstd 3.3e-7 / 1.1e-7 / 3.4      var 4.9e-7 / 5.2e-8 / 16       scale 3.3e-7 / 1.0e-7 / 3.4
  shift 3.9e-7 / 1.8e-7 / 6.5       running_mean 6.9e-8 / 8.7e-8 / 1.6                               output 2.6e-7 / 2.6e-7 / 1.2
  running_var and what was added to it 7.8e-6 / 3.2e-5 / 0.66 (the added part carries the rounding of a buffer near 1)
  dgamma 4.3e-7 / 2.1e-7 / 2.6      dbeta 5.8e-8 / 8.4e-8 / 2.0       dW 3.8e-7 / 5.8e-7 / 2.3       db 5.9e-7 / 1.0e-6 / 5.4
(var, invstd, scale and shift pass on their floors, not on 3 e_32: the kernels form var as E[z^2] - mean^2 from fp32 tile
sums, a cancellation that torch's var of centred values does not have.)  Stored tensors, share of differing elements of the HIP result / of ref32 /
largest |difference| : (one bf16 step + accumulation term):
  z 2.4e-4 / 6.5e-4 / 0.94          a 0 / 0 / 0                       pooled (max and avg) 0 / 0 / 0
  convT slice 2.2e-4 / 0 / 0.95     OutConv dx 0 / 0 / 0              dz 3.4e-4 / 2.4e-4 / 0.99
  conv dx 4.9e-4 / 4.3e-4 / 0.99    convT dx 1.2e-4 / 1.2e-4 / 0.99   pool backward + skip add 0 / 0 / 0
(the deepest tensors hold 2560 .. 4608 elements: 4.9e-4 is two elements of 4096).  Mutants, smallest miss : bound over
all their rows: batch statistics 5.9e3, unbiased invstd 3.9e2, running_var 20, xhat term 8.4e2, last maximum 36, skip add
9.9e2, first half 1.0e3, unflipped weights 9.9e2, one bias tap 4.6e5.
"""
import pytest
import torch

import unet_stage_oracle as S
from conftest import rel_err
from mmft import lib, ops, unet16

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SHARE_CAP, K32, TEETH_ROW = 1e-3, 3.0, 10.0
FILL = -1984.0                          # exact in bf16; what the arenas hold before the step runs
FLOORS = dict(mean=1e-6, invstd=1e-6, var=1e-6, scale=1e-6, shift=1e-5, running_mean=1e-6, running_var=1e-6, output=1e-5,
              dgamma=1e-4, dbeta=1e-4, dW=2e-6, db=2e-6)
MUTANTS = ('statistics over the batch', 'unbiased variance inside invstd', 'running_var without n / (n - 1)',
           'BatchNorm backward without xhat mean(gm xhat)', 'max-pool gradient to the last maximum', 'skip add dropped',
           'transposed convolution into the first half', 'input gradient through unflipped weights',
           'transposed convolution bias gradient over one tap')


def _new_net(dev, N, H, W, pooling, seed):
    import Unet
    net, x, gout = S.seeded_case(Unet.UNet, N, H, W, pooling, seed)
    net = net.to(dev)
    net.set_per_sample_stats(True)
    net.train()
    return net, x, gout


def _covered(buf, table):
    m = torch.zeros(buf.numel(), dtype=torch.bool)
    for t in table.values():
        o = t.storage_offset() - buf.storage_offset()
        m[o:o + t.numel()] = True
    return m


def drive(dev, N, H, W, pooling, seed, batch_reduce=True):
    """One train step, launched as UNet16Fn.forward / backward launch it without a replay, on arenas pre-filled with FILL."""
    net, x, gout = _new_net(dev, N, H, W, pooling, seed)
    sd0 = S.cast_state(net.state_dict(), torch.float64)
    pool_mode = ops.POOL_MAX if pooling == 'max' else ops.POOL_AVG
    geom = (N, H, W)
    with lib.math_mode('bf16'):
        xd = x.to(dev)
        assert unet16.supported(net, xd)
        packs = unet16._Packs(net, dev)
        fs, ffs = unet16._fwd_sizes(N, H, W)
        xn = ops.to_nhwc(xd)
        abuf, T = unet16._arena(fs, BF, dev)
        fbuf, F = unet16._arena(ffs, torch.float32, dev, align=4)
        abuf.fill_(FILL)
        out = torch.empty((N, 1, H // 2, W // 2), dtype=torch.float32, device=dev)
        unet16._run_forward(net, xn, pool_mode, packs, T, F, out, geom)
        sinks = unet16._make_sinks(net)
        gs, ws_bytes = unet16._bwd_sizes(N, H, W)
        gbuf, G = unet16._arena(gs, BF, dev)
        gbuf.fill_(FILL)
        SL = unet16._arena(unet16._slab_sizes(N, H, W), torch.float32, dev, align=4)[1] if batch_reduce else None
        unet16._run_backward(net, xn, pool_mode, packs, T, F, gout.to(dev).contiguous(), G, lib.workspace(dev, ws_bytes), geom, sinks, SL)
        by_id = {k: s.done() for k, s in sinks.items()}
        torch.cuda.synchronize()
    grads = {k: by_id[id(p)].detach().cpu().contiguous() for k, p in net.named_parameters()}
    host = lambda d: {k: v.detach().cpu() for k, v in d.items()}
    return dict(geom=geom, pooling=pooling, x=x, gout=gout, sd0=sd0, out=out.cpu(), grads=grads, state=host(net.state_dict()),
                T=host(T), F=host(F), G=host(G), pad_T=abuf.cpu()[~_covered(abuf, T)], pad_G=gbuf.cpu()[~_covered(gbuf, G)])


@pytest.fixture(scope='module', params=S.GEOMETRIES, ids=lambda g: '%dx%dx%d-%s' % g[:4])
def step(request, dev):
    return drive(dev, *request.param), request.param


def test_driven_sequence_is_the_public_step(step, dev):
    """The sequence this file drives is the product's: bitwise the public net(x) / backward; with the per-layer slab
    reductions instead of the batched one the convolution gradients keep their bits and the others stay within the 1e-5 of
    test_batched_reduce_equals_per_layer_reduce; nothing outside the named arena regions is written."""
    s, param = step
    net, x, gout = _new_net(dev, *param)
    with lib.math_mode('bf16'):
        y = net(x.to(dev))
        y.backward(gout.to(dev))
        torch.cuda.synchronize()
    assert torch.equal(y.detach().cpu(), s['out'])
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.equal(p.grad.cpu(), s['grads'][k]), k
    running = [k for k in s['state'] if 'running' in k]
    assert len(running) == 28
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), s['state'][k]), k
        if 'num_batches' in k:
            assert int(v) == param[0]
    assert bool((s['pad_T'].float() == FILL).all()) and bool((s['pad_G'].float() == FILL).all())
    assert all(bool(torch.isfinite(v.float()).all()) for d in (s['T'], s['G']) for v in d.values())
    per_layer = drive(dev, *param, batch_reduce=False)
    assert torch.equal(per_layer['out'], s['out'])
    for k, a in s['grads'].items():
        b = per_layer['grads'][k]
        if a.dim() == 4 and a.shape[-1] == 3:
            assert torch.equal(a, b), k
        else:
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-7, k


# ------------------------------------------------------------------------------------------------ rows
class Rows:
    """The rules of the module docstring over many rows: each is measured and kept, verdict() prints all and then fails."""

    def __init__(self, title):
        self.title, self.rows, self.bad, self.teeth, self.kinds = title, [], [], [], {}

    def _kind(self, kind, **kv):
        k = self.kinds.setdefault(kind, {})
        for name, v in kv.items():
            k[name] = max(k.get(name, 0.0), v)

    def fp32(self, name, kind, hip, ref, ref32):
        floor = FLOORS[kind]
        e_hip, e_32 = rel_err(hip, ref), rel_err(ref32, ref)
        bound = max(floor, K32 * e_32)
        self.rows.append(f'{name:38s} e_hip {e_hip:.2e}  e_32 {e_32:.2e}  bound {bound:.2e}')
        self._kind(kind, e_hip=e_hip, e_32=e_32, ratio=e_hip / e_32 if e_32 > 0 else 0.0)
        if not e_hip <= bound:
            self.bad.append(f'{name}: e_hip {e_hip:.3e} > bound {bound:.3e}')
        return bound

    def stored(self, name, kind, hip, ref, ref32, mass=None, n=1, bitwise=False):
        ref32 = ref32.double()
        assert hip.shape == ref.shape == ref32.shape, (name, hip.shape, ref.shape)
        if not bool(torch.isfinite(hip).all()):
            self.bad.append(f'{name}: not finite')
        share, share32 = float((hip != ref).double().mean()), float((ref32 != ref).double().mean())
        big = torch.maximum(hip.abs(), ref.abs())
        tol = torch.ldexp(torch.ones_like(big), torch.frexp(big).exponent - 8)          # one bf16 step of the larger value
        if mass is not None:
            tol = tol + (n - 1) * 2.0 ** -24 * mass * (1 + 1e-3)
        worst = float(((hip - ref).abs() / tol).max())
        self.rows.append(f'{name:38s} share {share:.2e}  share_32 {share32:.2e}  worst |d| / (step + acc) {worst:.3f}'
                         + ('  [bitwise]' if bitwise else ''))
        self._kind(kind, share=share, share_32=share32, worst=worst)
        if bitwise and share > 0:
            self.bad.append(f'{name}: {share:.3e} of the elements differ, bitwise expected')
        if not share <= SHARE_CAP:
            self.bad.append(f'{name}: share {share:.3e} > {SHARE_CAP}')
        if not worst <= 1.0:
            self.bad.append(f'{name}: an element is {worst:.3f} x (one bf16 step + accumulation term) away')

    def mutant_stored(self, mutant, name, hip, ref_mut):
        share = float((hip != ref_mut).double().mean())
        self.teeth.append((mutant, name, share, SHARE_CAP))

    def mutant_fp32(self, mutant, name, hip, ref_mut, bound):
        self.teeth.append((mutant, name, rel_err(hip, ref_mut), bound))

    def verdict(self, mutants):
        print(f'\n== {self.title}')
        for row in self.rows:
            print('   ' + row)
        print('   -- per kind of row (worst):')
        for kind, k in self.kinds.items():
            print(f'   {kind:16s} ' + '  '.join(f'{a} {v:.2e}' for a, v in k.items()))
        print('   -- mutants: miss / bound')
        for mutant, name, miss, bound in self.teeth:
            print(f'   {mutant:52s} {name:24s} {miss:.2e} / {bound:.2e} = {miss / bound:.1f}')
            if not miss > TEETH_ROW * bound:
                self.bad.append(f'no teeth: "{mutant}" at {name} misses by {miss:.3e}, not {TEETH_ROW} x {bound:.3e}')
        seen = {t[0] for t in self.teeth}
        assert set(mutants) <= seen, sorted(set(mutants) - seen)
        assert not self.bad, self.bad


class Host:
    """The step's tensors by the ORACLE's names, as (N,C,H,W) fp64 on the CPU."""

    def __init__(self, s):
        self.s = s
        N, H, W = s['geom']
        self.N, self.lv = N, [(H >> k, W >> k) for k in range(4)]
        self.shape = {}                                   # oracle name -> (level, channels of the buffer that holds it)
        self.where = {'image': None}
        for L in S.LAYERS:
            name, lo, hi = L['dst']
            act = 'act%d' % L['i']
            if name in S.CHANNELS:
                self.shape[name] = (L['level'], S.CHANNELS[name])
                self.where[name] = ('T', name)
                self.where[act] = ('T', name, lo, hi)
            else:
                self.where[act] = ('T', 'a%d' % L['i'])
            self.shape[act] = (L['level'], L['co'])
            if L['pooled']:
                self.shape[L['pooled']] = (L['level'] + 1, L['co'])
                self.where[L['pooled']] = ('T', 'p' + L['pooled'][4:])

    def _nchw(self, flat, level, C):
        h, w = self.lv[level]
        return flat.view(self.N, h, w, C).permute(0, 3, 1, 2).double()

    def t(self, name):
        if name == 'image':
            return self.s['x'].double()
        w = self.where[name]
        if len(w) == 4:                                    # a channel slice of a concatenation buffer
            lv, C = self.shape[w[1]]
            return self._nchw(self.s['T'][w[1]], lv, C)[:, w[2]:w[3]]
        return self._nchw(self.s['T'][w[1]], *self.shape[name])

    def z(self, i):
        return self._nchw(self.s['T']['z%d' % i], *self.shape['act%d' % i])

    def g(self, name):
        """Gradient of an oracle tensor: act_i -> g_i, pool_k -> gp_k, cat_k -> gcat_k."""
        buf = 'g' + name[3:] if name.startswith('act') else 'gp' + name[4:] if name.startswith('pool') else 'g' + name
        return self._nchw(self.s['G'][buf], *self.shape[name])

    def dz(self, i):
        return self._nchw(self.s['G']['dz%d' % i], *self.shape['act%d' % i])

    def bnp(self, i):
        C = self.shape['act%d' % i][1]
        return self.s['F']['bnp%d' % i].view(5, self.N, C)


BNP_ROWS = ('mean', 'invstd', 'var', 'scale', 'shift')
f32 = lambda t: t.float()


def test_forward_stages(step):
    s, param = step
    N, H, W, pooling, _ = param
    h, p64 = Host(s), s['sd0']
    p32 = {k: (v.float() if v.dtype.is_floating_point else v) for k, v in p64.items()}
    q = Rows('forward stages %dx%dx%d %s' % (N, H, W, pooling))
    ups = {u['src']: u for u in S.UPS}
    for L in S.LAYERS:
        i, bn = L['i'], L['bn']
        src, w, hz = h.t(L['src']), L['conv'], h.z(i)
        q.stored(f'z{i}', 'z', hz, S.conv_fwd(src, p64[w]), S.conv_fwd(f32(src), p32[w]), *S.conv_fwd_mass(src, p64[w]))
        bnp = h.bnp(i)
        st = S.bn_stats(hz, p64[bn + 'weight'], p64[bn + 'bias'])
        st32 = S.bn_stats(f32(hz), p32[bn + 'weight'], p32[bn + 'bias'])
        bounds = {key: q.fp32(f'bnp{i}.{key}', key, bnp[j], st[key], st32[key]) for j, key in enumerate(BNP_ROWS)}
        if N > 1:
            q.mutant_fp32(MUTANTS[0], f'bnp{i}.mean', bnp[0], S.bn_stats(hz, p64[bn + 'weight'], p64[bn + 'bias'], per_image=False)['mean'],
                          bounds['mean'])
        q.mutant_fp32(MUTANTS[1], f'bnp{i}.invstd', bnp[1], S.bn_stats(hz, p64[bn + 'weight'], p64[bn + 'bias'], unbiased_invstd=True)['invstd'],
                      bounds['invstd'])
        # running statistics from the stored mean / var rows
        n = hz.shape[2] * hz.shape[3]
        rm0, rv0 = p64[bn + 'running_mean'], p64[bn + 'running_var']
        rm, rv = S.running_update(rm0, rv0, bnp[0].double(), bnp[2].double(), n)
        rm32, rv32 = S.running_update(f32(rm0), f32(rv0), bnp[0], bnp[2], n)
        q.fp32(f'running_mean {i}', 'running_mean', s['state'][bn + 'running_mean'], rm, rm32)
        q.fp32(f'running_var {i}', 'running_var', s['state'][bn + 'running_var'], rv, rv32)
        # the same floor on what the step ADDED to running_var (the buffer starts at 1 and keeps 0.9^N of it, which hides a
        # layer's small variance): the row the n / (n - 1) mutant is judged on
        added = lambda t: t.double() - (1 - S.MOMENTUM) ** N * rv0
        b = q.fp32(f'running_var {i}, added', 'running_var', added(s['state'][bn + 'running_var']), added(rv), added(rv32))
        q.mutant_fp32(MUTANTS[2], f'running_var {i}, added', added(s['state'][bn + 'running_var']),
                      added(S.running_update(rm0, rv0, bnp[0].double(), bnp[2].double(), n, unbiased=False)[1]), b)
        ha = h.t(f'act{i}')
        q.stored(f'a{i}' + (' (skip half of %s)' % L['dst'][0] if L['pooled'] else ''), 'a', ha, S.bn_apply(hz, bnp[3], bnp[4]),
                 S.bn_apply(f32(hz), bnp[3], bnp[4]), *S.bn_apply_mass(hz, bnp[3].double(), bnp[4].double()))
        if L['pooled']:
            mass, nt = S.pool_fwd_mass(ha)
            q.stored(L['pooled'], 'pooled', h.t(L['pooled']), S.pool_fwd(ha, pooling), S.pool_fwd(f32(ha), pooling), mass, nt,
                     bitwise=pooling == 'max')
        u = ups.get(f'act{i}')
        if u:
            cat, lo, hi = u['dst']
            wn, bnm = u['prefix'] + 'weight', u['prefix'] + 'bias'
            ref = S.convt_fwd(ha, p64[wn], p64[bnm])
            hcat = h.t(cat)
            q.stored(f'convT {u["k"]} ({cat}[{lo}:{hi}])', 'convT', hcat[:, lo:hi], ref, S.convt_fwd(f32(ha), p32[wn], p32[bnm]),
                     *S.convt_fwd_mass(ha, p64[wn], p64[bnm]))
            q.mutant_stored(MUTANTS[6], f'{cat}[0:{hi - lo}]', hcat[:, :hi - lo], ref)     # the slice written at channel 0 ...
            q.mutant_stored(MUTANTS[6], f'{cat}[{lo}:{hi}]', hcat[:, lo:hi], torch.full_like(ref, FILL))   # ... its own half keeps the fill
    O = S.WIRING['out']
    a14 = h.t(O['src'])
    q.fp32('output', 'output', s['out'], S.outconv_fwd(a14, p64[O['weight']], p64[O['bias']], pooling),
           S.outconv_fwd(f32(a14), p32[O['weight']], p32[O['bias']], pooling))
    q.verdict([m for j, m in enumerate(MUTANTS) if j in (1, 2, 6) or (j == 0 and N > 1)])


def test_backward_stages(step):
    s, param = step
    N, H, W, pooling, _ = param
    h, p64, gr = Host(s), s['sd0'], s['grads']
    p32 = {k: (v.float() if v.dtype.is_floating_point else v) for k, v in p64.items()}
    q = Rows('backward stages %dx%dx%d %s' % (N, H, W, pooling))
    O = S.WIRING['out']
    a14, gout = h.t(O['src']), s['gout']
    dx, dw, db = S.outconv_bwd(a14, p64[O['weight']], p64[O['bias']], gout.double(), pooling)
    dx32, dw32, db32 = S.outconv_bwd(f32(a14), p32[O['weight']], p32[O['bias']], gout, pooling)
    q.stored('g14 (OutConv dx)', 'OutConv dx', h.g(O['grad_to']), dx, dx32, *S.outconv_dx_mass(a14, p64[O['weight']], p64[O['bias']], gout.double(), pooling))
    q.fp32('dW OutConv', 'dW', gr[O['weight']], dw, dw32)
    q.fp32('db OutConv', 'db', gr[O['bias']], db, db32)
    ups_by_cat = {u['dst'][0]: u for u in S.UPS}
    skip_by_act = {k['act']: k for k in S.SKIPS}
    for L in reversed(S.LAYERS):
        i, bn, act = L['i'], L['bn'], 'act%d' % L['i']
        hg = h.g(act)
        if act in skip_by_act:
            k = skip_by_act[act]
            cat, lo, hi = k['cat']
            args = (h.t(act), h.g(cat)[:, lo:hi], h.g(k['pooled']))
            q.stored(f'g{i} (pool backward + skip)', 'pool backward', hg, S.pool_bwd(*args, pooling), S.pool_bwd(*map(f32, args), pooling), bitwise=True)
            if pooling == 'max':
                q.mutant_stored(MUTANTS[4], f'g{i}', hg, S.pool_bwd(*args, pooling, last_max=True))
            q.mutant_stored(MUTANTS[5], f'g{i}', hg, S.pool_bwd(*args, pooling, skip=False))
        hz, bnp = h.z(i), h.bnp(i)
        st = dict(zip(BNP_ROWS, bnp))                     # the HIP step's own fp32 rows
        dz, dg, dbt = S.bn_relu_bwd(hg, hz, st)
        dz32, dg32, dbt32 = S.bn_relu_bwd(f32(hg), f32(hz), st)
        hdz = h.dz(i)
        q.stored(f'dz{i}', 'dz', hdz, dz, dz32, *S.bn_relu_bwd_mass(hg, hz, st))
        q.fp32(f'dgamma {i}', 'dgamma', gr[bn + 'weight'], dg, dg32)
        q.fp32(f'dbeta {i}', 'dbeta', gr[bn + 'bias'], dbt, dbt32)
        q.mutant_stored(MUTANTS[3], f'dz{i}', hdz, S.bn_relu_bwd(hg, hz, st, xhat_term=False)[0])
        src, w = h.t(L['src']), L['conv']
        need = L['grad_to'] is not None
        dW, dxc = S.conv_bwd(src, p64[w], hdz, need_dx=need)
        dW32, dxc32 = S.conv_bwd(f32(src), p32[w], f32(hdz), need_dx=need)
        q.fp32(f'dW conv {i}', 'dW', gr[w], dW, dW32)
        if need:
            hdx = h.g(L['grad_to'])
            q.stored(f'g:{L["grad_to"]} (conv {i} dx)', 'conv dx', hdx, dxc, dxc32, *S.conv_dx_mass(src, p64[w], hdz))
            q.mutant_stored(MUTANTS[7], f'g:{L["grad_to"]}', hdx, S.conv_bwd(src, p64[w], hdz, flipped=False)[1])
        if L['src'] in ups_by_cat:
            u = ups_by_cat[L['src']]
            cat, lo, hi = u['dst']
            wn, bnm = u['prefix'] + 'weight', u['prefix'] + 'bias'
            xs, gs = h.t(u['src']), h.g(cat)[:, lo:hi]
            dWu, dbu, dxu = S.convt_bwd(xs, p64[wn], gs)
            dWu32, dbu32, dxu32 = S.convt_bwd(f32(xs), p32[wn], f32(gs))
            q.fp32(f'dW convT {u["k"]}', 'dW', gr[wn], dWu, dWu32)
            bb = q.fp32(f'db convT {u["k"]}', 'db', gr[bnm], dbu, dbu32)
            q.stored(f'g:{u["grad_to"]} (convT {u["k"]} dx)', 'convT dx', h.g(u['grad_to']), dxu, dxu32, *S.convt_dx_mass(p64[wn], gs))
            q.mutant_fp32(MUTANTS[8], f'db convT {u["k"]}', gr[bnm], S.convt_bwd(xs, p64[wn], gs, bias_taps=1)[1], bb)
    q.verdict([m for j, m in enumerate(MUTANTS) if j in (3, 5, 7, 8) or (j == 4 and pooling == 'max')])
