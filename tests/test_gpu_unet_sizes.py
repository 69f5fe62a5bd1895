"""GPU: the score U-Net evaluator and the samplers at image sizes whose bottleneck token count (H/4)*(W/4) is
above 256 and no multiple of 256 (tcx_attention_ragged): 96x96 (576 tokens; the split path applies), 72x80 (360;
fp32 under either setting) and 100x100 (625), against the float64 numpy oracle."""
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

from test_gpu_models import prec, rel_err, unet  # noqa: F401  (prec: the conv-precision fixture)

pytestmark = pytest.mark.gpu

B = 2


@lru_cache(maxsize=None)
def setup(H, W):   # model, oracle, inputs, the oracle's CFG evaluation: shared by both precisions
    from oracle.score_model import ScoreUNet, predict_eps_cfg as o_cfg
    m = unet(32)
    x = torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(H + W))
    t, y_cat, y_cont = torch.tensor([0.42, 0.77]), torch.tensor([1, 3]), torch.zeros(B, 4)
    y_cont[:, 1] = torch.linspace(0, math.pi / 3, B)
    o = ScoreUNet({k: v.cpu().numpy() for k, v in m.state_dict().items()}, dt=np.float64)
    return m, o, (x, t, y_cat, y_cont), o_cfg(o, x.double().numpy(), t.numpy(), y_cat.numpy(), y_cont.numpy(), 1.5)


@pytest.mark.parametrize("H,W", [(96, 96), (72, 80), (100, 100)])
def test_cfg_evaluation_vs_oracle(H, W, prec):
    from toycrystals_amd.models.sde_score_model import predict_eps_cfg
    m, _, args, ref = setup(H, W)
    assert rel_err(predict_eps_cfg(m, *(a.cuda() for a in args), 1.5).cpu().numpy(), ref) < 2e-5


@lru_cache(maxsize=None)
def sde_ref():
    from oracle.score_model import VPSDE as OVPSDE, sample_reverse_sde_euler_maruyama as o_sde
    _, o, (_, _, y_cat, y_cont), _ = setup(96, 96)
    noise = torch.randn(3, B, 1, 96, 96, generator=torch.Generator().manual_seed(7))
    return noise, o_sde(o, OVPSDE(0.1, 30.0, dt=np.float64), y_cat.numpy(), y_cont.numpy(), noise.double().numpy(), 2,
                        1.5, 0.005, clamp=False)


def test_samplers_at_96(prec):   # 2-step SDE against the float64 oracle; DPM-Solver++: finite, in [0, 1]
    from toycrystals_amd.models.sde_score_model import VPSDE, sample_dpm_solver_pp, sample_reverse_sde_euler_maruyama
    m, _, (_, _, y_cat, y_cont), _ = setup(96, 96)
    noise, ref = sde_ref()
    kw = dict(n_steps=2, guidance_scale=1.5, t_end=0.005)
    x0 = sample_reverse_sde_euler_maruyama(m, VPSDE(0.1, 30.0), y_cat.cuda(), y_cont.cuda(), (B, 1, 96, 96),
                                           noise=noise.cuda(), return_x0_hat=True, **kw).cpu().numpy()
    assert rel_err(x0, ref) < 1e-4
    out = sample_dpm_solver_pp(m, VPSDE(0.1, 30.0), y_cat.cuda(), y_cont.cuda(), (B, 1, 96, 96), seed=3, **kw)
    assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
