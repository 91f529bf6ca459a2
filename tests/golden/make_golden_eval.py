"""Generate tests/golden/unet_eval_*.npz by running the REFERENCE's own src/Unet.py in EVAL mode.

Run only where the reference checkout exists, like make_golden.py (whose helpers it imports):

    python tests/golden/make_golden_eval.py

The reference's module is imported unmodified, filled with det_state_dict (non-trivial running statistics: mean in +-0.1,
variance in 0.5 .. 1.5), given an OutConv bias that lets about half of the outputs survive the final ReLU - chosen on
the EVAL-mode pre-activation - and called after .eval().  Outputs only are stored.  The script asserts that the reference
leaves every buffer bitwise unchanged in eval mode and that tests/unet_eval_oracle.py agrees with it (2e-6 fp32 / 1e-12
fp64, make_golden.py's tolerances).
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG                              # noqa: E402  (also puts the repository and the package on sys.path)
from mmft.detrand import det_uniform, det_state_dict  # noqa: E402
import unet_eval_oracle as E                          # noqa: E402

CASES = (('max', (64, 64), 21, 2), ('avg', (64, 64), 22, 2), ('max', (37, 45), 23, 1))


def _pre_activation(net, x):
    """Pooled 1x1-convolution output before the final ReLU (src/Unet.py:110-119 without outc.conv[2])."""
    x1 = net.inc(x)
    x2 = net.down1(x1)
    x3 = net.down2(x2)
    x4 = net.down3(x3)
    y = net.up3(net.up2(net.up1(x4, x3), x2), x1)
    return net.outc.conv[1](net.outc.conv[0](y))


def _buffers(net):
    return {k: v.clone() for k, v in net.state_dict().items() if 'running' in k or 'num_batches' in k}


def _assert_buffers_unchanged(net, before, tag):
    after = net.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), f'{tag}: the reference changed {k} in eval mode'


def golden_unet_eval(ref_unet):
    for pooling, (H, W), seed, N in CASES:
        outc_bias = None
        for dtype, tol in ((torch.float32, 2e-6), (torch.float64, 1e-12)):
            net = ref_unet.UNet(pooling).to(dtype)
            sd = det_state_dict(net, seed)
            xin = torch.from_numpy(det_uniform((N, 3, H, W), seed + 100, 0.0, 1.0))
            if outc_bias is None:
                probe = ref_unet.UNet(pooling)
                sd0 = dict(sd)
                sd0['outc.conv.0.bias'] = torch.zeros(1)
                probe.load_state_dict(sd0)
                probe.eval()
                with torch.no_grad():
                    outc_bias = round(-float(_pre_activation(probe, xin).median()), 3)
            sd['outc.conv.0.bias'] = torch.full((1,), outc_bias)
            cast = {k: v.to(dtype) if v.dtype.is_floating_point else v for k, v in sd.items()}
            net.load_state_dict(cast)
            net.eval()
            x = xin.to(dtype)
            before = _buffers(net)
            with torch.no_grad():
                y = net(x)
            _assert_buffers_unchanged(net, before, f'unet eval {pooling} {H}x{W}')
            share = float((y > 0).double().mean())
            yo = E.unet_eval_forward(E.cast_state(cast, dtype), x, pooling)
            e = MG.check(f'unet eval {pooling} {H}x{W} {dtype} out', yo, y, tol)
            print(f'  unet eval {pooling} {H}x{W} N={N} {dtype}: surviving share {share:.2f}, oracle vs reference {e:.2e}')
            if dtype != torch.float32:
                continue
            arrs = dict(seed=seed, outc_bias=outc_bias, out=y)
            if (pooling, H, W) == ('max', 64, 64):
                # the hand-off from train-mode running-statistic updates to the eval path: two train-mode forwards on image 0
                # alone, then .eval() and a forward of the whole batch
                net2 = ref_unet.UNet(pooling)
                net2.load_state_dict(cast)
                net2.train()
                with torch.no_grad():
                    net2(x[:1])
                    net2(x[:1])
                net2.eval()
                before = _buffers(net2)
                with torch.no_grad():
                    y2 = net2(x)
                _assert_buffers_unchanged(net2, before, 'unet eval after train')
                nsd = net2.state_dict()
                yo2 = E.unet_eval_forward(E.cast_state(nsd, dtype), x, pooling)
                MG.check('unet eval after train out', yo2, y2, tol)
                arrs.update(out_after_train=y2, rm_inc1=nsd['inc.double_conv.1.running_mean'],
                            rv_inc1=nsd['inc.double_conv.1.running_var'], rm_up2_4=nsd['up2.conv.double_conv.4.running_mean'],
                            rv_up2_4=nsd['up2.conv.double_conv.4.running_var'],
                            nbt=nsd['inc.double_conv.1.num_batches_tracked'])
            MG.save(f'unet_eval_{pooling}_{H}x{W}', **arrs)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    _, ref_unet = MG.import_reference()
    golden_unet_eval(ref_unet)
    print('eval fixtures written; the eval oracle agrees with the reference on every one of them')


if __name__ == '__main__':
    main()
