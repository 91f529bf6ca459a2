"""Generate tests/golden/unet_eval_input_grad_*.npz: the INPUT gradient of the REFERENCE's own src/Unet.py in EVAL mode.

Run only where the reference checkout exists, like make_golden_eval.py (whose helpers it imports):

    python tests/golden/make_golden_eval_grad.py

The reference's module is imported unmodified, filled with det_state_dict and the median OutConv bias of
make_golden_eval.py, called after .eval(), and dx = autograd.grad(y, x, gout) is taken with gout = det_uniform(-1, 1).
Only seed, outc_bias, gout and dx are stored.  The script asserts that the plain oracle of tests/sens_image_oracle.py
(unet_eval_vjp on its own forward's activations) equals the reference: 2e-6 in fp32, 1e-12 in fp64 (make_golden.py's
tolerances; the plain oracle forms the BatchNorm scale in the working dtype for the second one).
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG                              # noqa: E402  (also puts the repository and the package on sys.path)
import make_golden_eval as ME                         # noqa: E402
from mmft.detrand import det_uniform, det_state_dict  # noqa: E402
import unet_eval_oracle as E                          # noqa: E402
import sens_image_oracle as SI                        # noqa: E402

CASES = (('max', (8, 32), 31, 2), ('avg', (16, 64), 32, 1))


def golden_unet_eval_grad(ref_unet):
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
                    outc_bias = round(-float(ME._pre_activation(probe, xin).median()), 3)
            sd['outc.conv.0.bias'] = torch.full((1,), outc_bias)
            cast = {k: v.to(dtype) if v.dtype.is_floating_point else v for k, v in sd.items()}
            net.load_state_dict(cast)
            net.eval()
            x = xin.to(dtype).requires_grad_(True)
            before = ME._buffers(net)
            y = net(x)
            gout = torch.from_numpy(det_uniform(tuple(y.shape), seed + 200, -1.0, 1.0)).to(dtype)
            (dx,) = torch.autograd.grad(y, x, gout)
            ME._assert_buffers_unchanged(net, before, f'unet eval grad {pooling} {H}x{W}')
            p = E.cast_state(cast, dtype)
            yo, acts = SI.unet_eval_acts(p, x.detach(), pooling)
            MG.check(f'unet eval grad {pooling} {H}x{W} {dtype} out', yo, y.detach(), tol)
            dxo = SI.unet_eval_vjp(p, acts, gout, pooling, dtype)
            e = MG.check(f'unet eval grad {pooling} {H}x{W} {dtype} dx', dxo, dx, tol)
            share, nz = float((y > 0).double().mean()), float((dx != 0).double().mean())
            print(f'  unet eval grad {pooling} {H}x{W} N={N} {dtype}: surviving share {share:.2f}, dx max {float(dx.abs().max()):.2e}, '
                  f'non-zero share {nz:.2f}, plain oracle vs reference {e:.2e}')
            if dtype == torch.float32:
                MG.save(f'unet_eval_input_grad_{pooling}_{H}x{W}_n{N}', seed=seed, outc_bias=outc_bias, gout=gout, dx=dx)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    _, ref_unet = MG.import_reference()
    golden_unet_eval_grad(ref_unet)
    print('eval input-gradient fixtures written; the plain oracle agrees with the reference on both')


if __name__ == '__main__':
    main()
