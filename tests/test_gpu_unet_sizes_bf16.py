"""GPU: the score U-Net evaluator and the samplers in bf16 (conv precision "bf16", tcx_unet.precision 2) at image
sizes whose bottleneck token count (H/4)*(W/4) is no multiple of 256: 96x96 (576 tokens) and 32x32 (64), served
by tcx_attention_split_ragged, against the float64 numpy oracle on the inputs of test_gpu_unet_sizes.setup.

The bound is measured, not derived: bf16 evaluation error depends on the input and the size in no derivable
way.  Before this kernel existed, the same model (unet(32), the same input recipe) in bf16 at 64x64 (N = 256,
k_attention_split) measured rel_err PARENT_64 against the oracle; the new sizes get twice that.  A wrong key
mask or slot order shows at order 1."""
import warnings

import pytest
import torch

from test_gpu_models import rel_err
from test_gpu_unet_sizes import B, setup

pytestmark = pytest.mark.gpu

PARENT_64 = 6.8683e-3   # measured on the MI355X on the parent commit (128x128, N = 1024: 6.5831e-3)
BOUND = 2 * PARENT_64


@pytest.fixture
def bf16():
    from toycrystals_amd import _lib
    old = _lib.conv_precision()
    _lib.set_conv_precision("bf16")
    yield _lib
    _lib.set_conv_precision(old)


@pytest.mark.parametrize("H,W", [(96, 96), (32, 32)])
def test_bf16_cfg_evaluation_vs_oracle(H, W, bf16):
    from toycrystals_amd.models.sde_score_model import predict_eps_cfg
    m, _, args, ref = setup(H, W)
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # no fallback warning
        e = predict_eps_cfg(m, *(a.cuda() for a in args), 1.5).cpu().numpy()
    assert bf16.used_conv_precision() == "bf16"
    err = rel_err(e, ref)
    print(f"  bf16 {H}x{W}: rel_err {err:.3e}, bound {BOUND:.3e}")
    assert err < BOUND


def test_bf16_samplers_at_96(bf16):   # finite images in [0, 1] from one 2-step SDE call and one DPM-Solver++ call
    from toycrystals_amd.models.sde_score_model import VPSDE, sample_dpm_solver_pp, sample_reverse_sde_euler_maruyama
    m, _, (_, _, y_cat, y_cont), _ = setup(96, 96)
    noise = torch.randn(3, B, 1, 96, 96, generator=torch.Generator().manual_seed(7))
    kw = dict(n_steps=2, guidance_scale=1.5, t_end=0.005)
    outs = [sample_reverse_sde_euler_maruyama(m, VPSDE(0.1, 30.0), y_cat.cuda(), y_cont.cuda(), (B, 1, 96, 96),
                                              noise=noise.cuda(), **kw),
            sample_dpm_solver_pp(m, VPSDE(0.1, 30.0), y_cat.cuda(), y_cont.cuda(), (B, 1, 96, 96), seed=3, **kw)]
    assert bf16.used_conv_precision() == "bf16"
    for out in outs:
        assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
