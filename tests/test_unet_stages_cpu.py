"""The stage reference of the bf16-storage U-Net train step (tests/unet_stage_oracle.py) IS the existing rounding oracle.

`reference_step` chains the hand-written stages - each stage's reference output feeds the next, the backward stages run
from a seeded gout - and must reproduce, in fp64, `oracle.restatement.unet_forward(rounding='bf16')` run image by image
under autograd: the output and every stored activation bit for bit, every parameter gradient and the running statistics
to 1e-10.  That pins the written-out backward formulas and the wiring table to autograd before they judge a kernel
(tests/test_unet_stages_gpu.py).  The oracle's stored tensors are taken in the order `oracle.bf16.stored` is called.

Also here, because it needs no GPU: the fp32 evaluation of every teacher-forced stage differs from the fp64 one in fewer
than a third of the share of elements the GPU file allows the kernels (its cap is 1e-3 per stored tensor).
"""
import pytest
import torch

import unet_stage_oracle as S
from oracle import bf16 as B
from oracle import restatement as R

# the order in which unet_forward(rounding='bf16') calls B.stored for one image (restatement.py: _conv_bn_relu_r stores z
# then a, _pool stores the pooled tensor, _up stores the concatenation)
STORED_ORDER = ['z1', 'act1', 'z2', 'act2', 'pool1', 'z3', 'act3', 'z4', 'act4', 'pool2', 'z5', 'act5', 'z6', 'act6', 'pool3',
                'z7', 'act7', 'z8', 'act8', 'cat1', 'z9', 'act9', 'z10', 'act10', 'cat2', 'z11', 'act11', 'z12', 'act12',
                'cat3', 'z13', 'act13', 'z14', 'act14']
SHARE_CAP = 1e-3


def rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def autograd_oracle(sd, x, gout, pooling, monkeypatch):
    pc = {k: (v.double().clone().requires_grad_('running' not in k) if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}
    seen = []
    plain = B.stored

    def recording(t, value=True, grad=True):
        out = plain(t, value, grad)
        seen.append(out.detach())
        return out
    monkeypatch.setattr(B, 'stored', recording)
    ys = [R.unet_forward(pc, x[i:i + 1].double(), pooling, update_running=True, rounding='bf16') for i in range(x.shape[0])]
    monkeypatch.setattr(B, 'stored', plain)
    yo = torch.cat(ys)
    yo.backward(gout.double())
    n = len(STORED_ORDER)
    assert len(seen) == n * x.shape[0]
    stored = {name: torch.cat([seen[i * n + j] for i in range(x.shape[0])]) for j, name in enumerate(STORED_ORDER)}
    return yo.detach(), stored, pc


@pytest.mark.parametrize('N,H,W,pooling,seed', S.GEOMETRIES)
def test_stage_chain_is_the_rounding_oracle(monkeypatch, N, H, W, pooling, seed):
    import Unet
    net, x, gout = S.seeded_case(Unet.UNet, N, H, W, pooling, seed)
    sd = net.state_dict()
    yo, stored, pc = autograd_oracle(sd, x, gout, pooling, monkeypatch)
    T, grads, run = S.reference_step(S.cast_state(sd, torch.float64), x.double(), gout.double(), pooling)
    assert torch.equal(T['out'], yo)
    for name, want in stored.items():
        assert torch.equal(T[name], want), name
    params = [k for k, v in pc.items() if v.dtype.is_floating_point and 'running' not in k]
    assert sorted(params) == sorted(grads) and len(params) == 14 * 3 + 3 * 2 + 2
    for k in params:
        assert grads[k].shape == pc[k].grad.shape and rel(grads[k], pc[k].grad) < 1e-10, k
    running = [k for k in pc if 'running' in k]
    assert sorted(running) == sorted(run) and len(running) == 28
    for k in running:
        assert rel(run[k], pc[k]) < 1e-10 and not torch.equal(pc[k], sd[k].double()), k


def share(a, b):
    return float((a != b).double().mean())


@pytest.mark.parametrize('N,H,W,pooling,seed', S.GEOMETRIES)
def test_fp32_stage_evaluation_stays_under_a_third_of_the_share_cap(N, H, W, pooling, seed):
    """Every stage that stores bf16, fed the fp64 chain's tensors, evaluated in fp32 and in fp64: the share of elements that
    differ at all stays below SHARE_CAP / 3 per tensor, so the cap leaves the kernels' own fp32 arithmetic room."""
    import Unet
    net, x, gout = S.seeded_case(Unet.UNet, N, H, W, pooling, seed)
    p64, p32 = S.cast_state(net.state_dict(), torch.float64), S.cast_state(net.state_dict(), torch.float32)
    T, _, _ = S.reference_step(p64, x.double(), gout.double(), pooling)
    f = lambda t: t.float()
    worst = {}

    def row(kind, a32, a64):
        s = share(a32.double(), a64)
        if s > 0:
            print(f'   {kind} {tuple(a64.shape)}: {s:.2e}')
        worst[kind] = max(worst.get(kind, 0.0), s)
    for L in S.LAYERS:
        i, bn = L['i'], L['bn']
        src, z, g = T[L['src']], T[f'z{i}'], T[f'g:act{i}']
        row('z', S.conv_fwd(f(src), p32[L['conv']]), S.conv_fwd(src, p64[L['conv']]))
        st = S.bn_stats(z, p64[bn + 'weight'], p64[bn + 'bias'])
        st32 = {k: f(v) for k, v in st.items()}
        row('a', S.bn_apply(f(z), st32['scale'], st32['shift']), S.bn_apply(z, st32['scale'], st32['shift']))
        if L['pooled']:
            row('pooled', S.pool_fwd(f(T[f'act{i}']), pooling), S.pool_fwd(T[f'act{i}'], pooling))
        row('dz', S.bn_relu_bwd(f(g), f(z), st32)[0], S.bn_relu_bwd(g, z, st32)[0])
        if L['grad_to']:
            row('conv dx', S.conv_bwd(f(src), p32[L['conv']], f(T[f'dz{i}']))[1], S.conv_bwd(src, p64[L['conv']], T[f'dz{i}'])[1])
    for u in S.UPS:
        cat, lo, hi = u['dst']
        w, b = u['prefix'] + 'weight', u['prefix'] + 'bias'
        row('convT', S.convt_fwd(f(T[u['src']]), p32[w], p32[b]), S.convt_fwd(T[u['src']], p64[w], p64[b]))
        gs = T['g:' + cat][:, lo:hi]
        row('convT dx', S.convt_bwd(f(T[u['src']]), p32[w], f(gs))[2], S.convt_bwd(T[u['src']], p64[w], gs)[2])
    for s in S.SKIPS:
        cat, lo, hi = s['cat']
        args = (T[s['act']], T['g:' + cat][:, lo:hi], T['g:' + s['pooled']])
        row('pool backward', S.pool_bwd(*map(f, args), pooling), S.pool_bwd(*args, pooling))
    O = S.WIRING['out']
    row('OutConv dx', S.outconv_bwd(f(T['act14']), p32[O['weight']], p32[O['bias']], gout, pooling)[0],
        S.outconv_bwd(T['act14'], p64[O['weight']], p64[O['bias']], gout.double(), pooling)[0])
    print('\nworst share of differing elements, fp32 against fp64 evaluation:', {k: f'{v:.1e}' for k, v in worst.items()})
    assert max(worst.values()) < SHARE_CAP / 3, worst
    assert worst['pool backward'] == 0.0 and (pooling != 'max' or worst['pooled'] == 0.0)
