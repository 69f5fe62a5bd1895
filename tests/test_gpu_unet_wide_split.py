"""GPU: the score U-Net evaluator and the samplers in bf16 (tcx_unet.precision 2) with a wide attention head
(head dim 80, 96 and 128: tcx_attention_split_wide), through the public model against the float64 numpy oracle.
The head dim is made wide as in test_gpu_unet_wide.py: base_ch 96 with 2 heads (d 96), base_ch 64 with 1 head
(d 128), whose convs the suite covers.  Head dim 80 is the real CondUNetTiny(4, 4, 160) at its four heads (the
only width with base_ch % 32 == 0 and d = 80): the split convs take that width in both precisions.

The bound is measured, not derived (test_gpu_unet_sizes_bf16.py says why).  The base-96 and base-64 nets with
their stock four heads (d 48 and d 32: k_attention_split_ragged, untouched here) measured the bf16 rel_err
below against the oracle on the same inputs at the same sizes; the wide head dims get twice the larger.  A
wrong key mask, slot order or transpose shows at order 1.  f16x3 takes the same kernel at these head dims by
default (fmt 0, h2 qkv): one evaluation at 96x96 at the 2e-5 of test_gpu_unet_wide.py."""
import warnings
from functools import partial

import numpy as np
import pytest
import torch

from test_gpu_models import rel_err
from test_gpu_unet_wide import inputs, net

pytestmark = pytest.mark.gpu

# measured on the MI355X with four heads, the parent commit's kernels: (base_ch, H, W) -> bf16 rel_err
PARENT_4HEADS = {(96, 32, 32): 8.1149e-3, (96, 32, 96): 8.1782e-3, (64, 32, 32): 5.6792e-3, (64, 32, 96): 8.1248e-3}
BOUND = 2 * max(PARENT_4HEADS.values())


@pytest.fixture
def precision(request):
    from toycrystals_amd import _lib
    old = _lib.conv_precision()
    _lib.set_conv_precision(request.param)
    yield _lib
    _lib.set_conv_precision(old)


bf16 = pytest.mark.parametrize("precision", ["bf16"], indirect=True)


# 32x32: N = 64, one query workgroup; 32x96: N = 192, two query workgroups, no multiple of 256; f16x3 at 96x96
EVAL = [(base, heads, H, W, "bf16", BOUND) for base, heads in ((160, 4), (96, 2), (64, 1))
        for H, W in ((32, 32), (32, 96))] + [(96, 2, 96, 96, "f16x3", 2e-5)]


@pytest.mark.parametrize("base,heads,H,W,precision,bound", EVAL, indirect=["precision"])
def test_cfg_evaluation_vs_oracle(base, heads, H, W, precision, bound):
    from oracle.score_model import ScoreUNet, predict_eps_cfg as o_cfg
    from toycrystals_amd.models.sde_score_model import predict_eps_cfg
    m = net(base, heads).eval()
    args = inputs(2, H, W)
    o = ScoreUNet({k: v.cpu().numpy() for k, v in m.state_dict().items()}, dt=np.float64)
    o.attn = partial(ScoreUNet.attn, o, heads=heads)
    ref = o_cfg(o, args[0].double().numpy(), *(a.numpy() for a in args[1:]), 1.5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # no fallback warning
        got = predict_eps_cfg(m, *(a.cuda() for a in args), 1.5).cpu().numpy()
    assert precision.used_conv_precision() == precision.conv_precision()
    err = rel_err(got, ref)
    print(f"  {precision.conv_precision()} base {base} heads {heads} {H}x{W}: rel_err {err:.3e}, bound {bound:.3e}")
    assert err < bound


@bf16
def test_bf16_samplers_at_head_dim_96(precision):   # finite images in [0, 1] from a 2-step SDE and a DPM-Solver++ call
    from toycrystals_amd.models.sde_score_model import VPSDE, sample_dpm_solver_pp, sample_reverse_sde_euler_maruyama
    m = net(96, 2).eval()
    _, _, y_cat, y_cont = inputs(2, 32, 32)
    noise = torch.randn(3, 2, 1, 32, 32, generator=torch.Generator().manual_seed(7))
    kw = dict(n_steps=2, guidance_scale=1.5, t_end=0.005)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        outs = [sample_reverse_sde_euler_maruyama(m, VPSDE(0.1, 30.0), y_cat.cuda(), y_cont.cuda(), (2, 1, 32, 32),
                                                  noise=noise.cuda(), **kw),
                sample_dpm_solver_pp(m, VPSDE(0.1, 30.0), y_cat.cuda(), y_cont.cuda(), (2, 1, 32, 32), seed=3, **kw)]
    assert precision.used_conv_precision() == "bf16"
    for out in outs:
        assert bool(torch.isfinite(out).all()) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
