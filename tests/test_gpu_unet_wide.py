"""GPU: the score U-Net with a wide attention head (head dim 80, 96, 128: tcx_attention_wide in the evaluator,
tcx_attention_wide_fwd_lse / _bwd under AttentionFn) through the public model.  The head dim is made wide on a
narrow net by replacing model.attn with fewer heads (base_ch 40 / 1 head: d 80; 96 / 2: d 96; 64 / 1: d 128),
which keeps the convs at widths the suite covers; one real wide net, CondUNetTiny(4, 4, 192) (d 96), is
evaluated too.  Gates: evaluation against the float64 numpy oracle at rel_err < 2e-5 (test_gpu_unet_sizes.py);
parameter gradients against float64 torch CPU autograd at 1e-4 x max(|g|max, 1e-3) (test_gpu_train.py)."""
import math
from functools import lru_cache, partial

import numpy as np
import pytest
import torch

from test_gpu_models import rel_err

pytestmark = pytest.mark.gpu

NETS = {80: (40, 1), 96: (96, 2), 128: (64, 1)}   # head dim: base_ch, heads


@lru_cache(maxsize=None)
def net(base, heads):
    from toycrystals_amd.models.sde_score_model import CondUNetTiny, SelfAttention2d
    torch.manual_seed(0)
    m = CondUNetTiny(4, 4, base)
    if heads != 4:
        m.attn = SelfAttention2d(2 * base, num_heads=heads)
    return m.cuda()


def inputs(B, H, W):
    x = torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(H + W))
    y_cont = torch.zeros(B, 4)
    y_cont[:, 1] = torch.linspace(0, math.pi / 3, B)
    return x, torch.tensor([0.42, 0.77, 0.1][:B]), torch.tensor([1, 3, 0][:B]), y_cont


# the three head dims at N = 16 and N = 60 in fp32; f16x3 (h2 records out of the attention) where the split
# convs apply, at N = 64; the real base_ch-192 net
EVAL = [(*NETS[d], H, W, "fp32") for d in NETS for H, W in ((16, 16), (24, 40))] + \
       [(*NETS[d], 32, 32, "f16x3") for d in (96, 128)] + [(192, 4, 16, 16, "fp32")]


@pytest.mark.parametrize("base,heads,H,W,precision", EVAL)
def test_cfg_evaluation_vs_oracle(base, heads, H, W, precision):
    from oracle.score_model import ScoreUNet, predict_eps_cfg as o_cfg
    from toycrystals_amd import _lib
    from toycrystals_amd.models.sde_score_model import predict_eps_cfg
    m = net(base, heads).eval()
    args = inputs(2, H, W)
    o = ScoreUNet({k: v.cpu().numpy() for k, v in m.state_dict().items()}, dt=np.float64)
    o.attn = partial(ScoreUNet.attn, o, heads=heads)
    ref = o_cfg(o, args[0].double().numpy(), *(a.numpy() for a in args[1:]), 1.5)
    old = _lib.conv_precision()
    _lib.set_conv_precision(precision)
    try:
        got = predict_eps_cfg(m, *(a.cuda() for a in args), 1.5).cpu().numpy()
    finally:
        _lib.set_conv_precision(old)
    e = rel_err(got, ref)
    print(f"  rel_err {e:.2e}")
    assert e < 2e-5


@pytest.mark.parametrize("d", sorted(NETS))
def test_loss_backward_vs_float64_autograd(monkeypatch, d):
    """diffusion_loss_eps at 24x40, B 2 (bottleneck N = 60) on injected draws, no condition dropout"""
    from oracle.score_model_torch import TorchScoreUNet
    from toycrystals_amd import functional as TF
    from toycrystals_amd.models.sde_score_model import VPSDE, diffusion_loss_eps
    base, heads = NETS[d]
    m = net(base, heads).train()
    m.zero_grad(set_to_none=True)
    B, H, W = 2, 24, 40
    g = torch.Generator().manual_seed(d)
    x0, y_cont = torch.rand(B, 1, H, W, generator=g), torch.rand(B, 4, generator=g)
    y_cat = torch.tensor([1, 3])
    u, eps = torch.rand(B, generator=g), torch.randn(B, 1, H, W, generator=g)
    routed = []
    apply = TF.AttentionFn.apply
    monkeypatch.setattr(TF.AttentionFn, "apply", lambda *a: routed.append(apply(*a)) or routed[-1])
    diffusion_loss_eps(m, VPSDE(0.1, 30.0), x0.cuda(), y_cat.cuda(), y_cont.cuda(), p_uncond=0.0,
                       draws=(u, eps, None)).backward()
    fn = routed.pop().grad_fn
    assert fn.wide and not fn.fused and not fn.ragged and not routed
    # the same loss in float64 on the CPU: t = u, x_t = alpha(t) (2 x0 - 1) + sigma(t) eps, mean (eps_hat - eps)^2
    o = TorchScoreUNet(m.state_dict(), dtype=torch.float64)
    o.w = {k: v.requires_grad_() if v.is_floating_point() else v for k, v in o.w.items()}
    o._attn = partial(TorchScoreUNet._attn, o, heads=heads)
    t = u.double()
    alpha = torch.exp(-0.5 * (0.1 * t + 0.5 * (30.0 - 0.1) * t ** 2)).view(B, 1, 1, 1)
    sigma = torch.sqrt(torch.clamp(1.0 - alpha ** 2, min=1e-8))
    with torch.enable_grad():
        x_t = alpha * (2.0 * x0.double() - 1.0) + sigma * eps.double()
        eps_hat = TorchScoreUNet.__call__.__wrapped__(o, x_t, t, y_cat, y_cont)
        ((eps_hat - eps.double()) ** 2).mean().backward()
    worst = 0.0
    for k, p in m.named_parameters():
        ref = o.w[k].grad
        tol = 1e-4 * max(float(ref.abs().max()), 1e-3)
        e = float((p.grad.double().cpu() - ref).abs().max())
        worst = max(worst, e / tol)
        assert e <= tol, (k, e, tol)
    print(f"  worst gradient error / gate {worst:.3f}")
