"""CPU: the eval-mode U-Net oracle (tests/unet_eval_oracle.py) against the fixtures the REFERENCE's own src/Unet.py produced
after .eval() (tests/golden/make_golden_eval.py), and the spread of its bf16 rounding variant - the numbers the GPU test's
whole-net bound is built from."""
import os

import numpy as np
import pytest
import torch

from conftest import rel_err
from mmft.detrand import det_uniform, det_state_dict
from oracle import restatement as R
import unet_eval_oracle as E

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURES = [('max', 64, 64, 2), ('avg', 64, 64, 2), ('max', 37, 45, 1)]
CASES = [(2, 64, 64, 'max'), (3, 40, 96, 'avg'), (1, 256, 256, 'max'), (8, 64, 64, 'max')]     # the GPU test's geometries


def fixture_state(pooling, H, W, N):
    """(fixture, state_dict, input) exactly as make_golden_eval.py built them."""
    import Unet
    g = np.load(os.path.join(GOLD, f'unet_eval_{pooling}_{H}x{W}.npz'))
    seed = int(g['seed'])
    sd = det_state_dict(Unet.UNet(pooling), seed)
    sd['outc.conv.0.bias'] = torch.full((1,), float(g['outc_bias']))
    x = torch.from_numpy(det_uniform((N, 3, H, W), seed + 100, 0.0, 1.0))
    return g, sd, x


def recipe_a(N, H, W, pooling):
    """The GPU test's recipe on the CPU: default initialisation under torch.manual_seed(3), running statistics after two
    train-mode forwards (fp32 oracle), torch.rand input."""
    import Unet
    torch.manual_seed(3)
    sd = E.cast_state(Unet.UNet(pooling).state_dict(), torch.float32)
    x = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        for _ in range(2):
            R.unet_forward(sd, x, pooling, True)
    return sd, x


@pytest.mark.parametrize('pooling,H,W,N', FIXTURES)
def test_eval_oracle_matches_the_reference_fixtures(pooling, H, W, N):
    """The eval oracle reproduces the reference's eval-mode outputs (2e-6, fp32); the train-mode oracle on the same inputs
    is far outside that, so the fixtures tell the two modes apart."""
    g, sd, x = fixture_state(pooling, H, W, N)
    out = torch.from_numpy(g['out'])
    assert out.shape == (N, 1, H // 2, W // 2)
    share = float((out > 0).double().mean())
    assert 0.3 < share < 0.7, share
    e = rel_err(E.unet_eval_forward(E.cast_state(sd, torch.float32), x, pooling), out)
    e3 = rel_err(E.unet_eval_forward(E.cast_state(sd, torch.float32), x[0], pooling), out[:1])          # (C,H,W), SURVEY D3
    with torch.no_grad():
        e_train = rel_err(R.unet_forward(E.cast_state(sd, torch.float32), x, pooling, False), out)
    print(f'\nunet eval {pooling} {H}x{W}: eval oracle {e:.2e}, (C,H,W) {e3:.2e}, train-mode oracle {e_train:.2e}')
    assert e <= 2e-6 and e3 <= 2e-6
    assert e_train > 1.0, e_train


def test_eval_after_train_fixture():
    """Two train-mode forwards on image 0 (the train oracle's running-statistic updates), then the eval oracle: the
    reference's `out_after_train` and its running statistics."""
    g, sd, x = fixture_state('max', 64, 64, 2)
    p = E.cast_state(sd, torch.float32)
    with torch.no_grad():
        for _ in range(2):
            R.unet_forward(p, x[:1], 'max', True)
    for k, name in (('rm_inc1', 'inc.double_conv.1.running_mean'), ('rv_inc1', 'inc.double_conv.1.running_var'),
                    ('rm_up2_4', 'up2.conv.double_conv.4.running_mean'), ('rv_up2_4', 'up2.conv.double_conv.4.running_var')):
        assert rel_err(p[name], torch.from_numpy(g[k])) <= 2e-6, k
    assert int(g['nbt']) == 2
    before = {k: v.clone() for k, v in p.items()}
    e = rel_err(E.unet_eval_forward(p, x, 'max'), torch.from_numpy(g['out_after_train']))
    assert e <= 2e-6, e
    assert all(torch.equal(before[k], p[k]) for k in p)                          # the eval oracle writes nothing


@pytest.mark.parametrize('N,H,W,pooling', CASES)
def test_rounding_oracle_spread(N, H, W, pooling):
    """e_32 = rounding oracle in fp32 vs fp64, e_plain = plain fp64 oracle vs rounding fp64 oracle (max-norm relative),
    recipe (a).  The GPU test bounds the kernels' output by max(2e-3, 3 e_32) under the ceiling 3e-2: the reference alone
    must stay inside the ceiling."""
    sd, x = recipe_a(N, H, W, pooling)
    o64 = E.unet_eval_forward(E.cast_state(sd, torch.float64), x.double(), pooling, 'bf16')
    o32 = E.unet_eval_forward(E.cast_state(sd, torch.float32), x, pooling, 'bf16')
    op = E.unet_eval_forward(E.cast_state(sd, torch.float64), x.double(), pooling)
    e_32, e_plain = rel_err(o32, o64), rel_err(op, o64)
    print(f'\nunet eval {N}x{H}x{W} {pooling}: e_32 {e_32:.2e}  e_plain {e_plain:.2e}  3 e_32 {3 * e_32:.2e}')
    assert float(o64.abs().max()) > 0
    assert 3 * e_32 <= 3e-2, e_32


def test_fixture_recipe_spread_is_recorded():
    """Recipe (b), the fixtures' own state (OutConv bias tuned so that half of the outputs are clipped: the output is a
    small difference of large terms): printed, not bounded - the fixtures are checked in fp32 mode only."""
    for pooling, H, W, N in FIXTURES[:2]:
        _, sd, x = fixture_state(pooling, H, W, N)
        o64 = E.unet_eval_forward(E.cast_state(sd, torch.float64), x.double(), pooling, 'bf16')
        o32 = E.unet_eval_forward(E.cast_state(sd, torch.float32), x, pooling, 'bf16')
        op = E.unet_eval_forward(E.cast_state(sd, torch.float64), x.double(), pooling)
        print(f'\nfixture recipe {pooling} {H}x{W}: e_32 {rel_err(o32, o64):.2e}  e_plain {rel_err(op, o64):.2e}')
        assert torch.isfinite(o64).all()


def test_scale_shift_sequence():
    """The kernel's scale / shift sequence restated: every step rounded to fp32, the last one a fused multiply-add."""
    p = {'b.weight': torch.tensor([1.5, 0.75]), 'b.bias': torch.tensor([0.1, -0.2]),
         'b.running_mean': torch.tensor([0.3, -0.05]), 'b.running_var': torch.tensor([0.9, 1.3])}
    scale, shift = E.scale_shift(p, 'b.')
    assert scale.dtype == shift.dtype == torch.float32
    invstd = (1.0 / np.sqrt((p['b.running_var'].numpy() + np.float32(1e-5)).astype(np.float32))).astype(np.float32)
    want = (p['b.weight'].numpy() * invstd).astype(np.float32)
    assert np.array_equal(scale.numpy(), want)
    fma = (-p['b.running_mean'].numpy().astype(np.float64) * want.astype(np.float64) + p['b.bias'].numpy().astype(np.float64))
    assert np.array_equal(shift.numpy(), fma.astype(np.float32))
