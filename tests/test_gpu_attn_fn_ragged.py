"""GPU: AttentionFn (toycrystals_amd/functional.py) at token counts outside the fused pair's set: routed to
tcx_attention_ragged_fwd_lse + tcx_attention_ragged_bwd by default and to the GEMM chain with the switch off,
both against float64 autograd at the training path's 2e-5 gate; the ragged path's peak memory (no
[B, heads, N, N] tensor); and one model backward at 40x40 (N = 100) against the chain."""
import pytest
import torch

from test_gpu_attn_train import err, reference

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("B,N,C,heads", [(2, 576, 192, 4), (1, 100, 32, 2)])
def test_attention_fn_both_paths(monkeypatch, fused, B, N, C, heads):
    from toycrystals_amd import functional as TF
    if not fused:
        monkeypatch.setattr(TF, "_ATTN_FUSED", False)
    qkv, dout, out_ref, _, dqkv_ref = reference(B, N, C, heads, 1)
    x = qkv.cuda().requires_grad_()
    y = TF.AttentionFn.apply(x, heads)
    assert y.grad_fn.ragged is fused and y.grad_fn.fused is False
    y.backward(dout.cuda())
    assert err(y.detach(), out_ref) < 2e-5
    assert err(x.grad, dqkv_ref) < 2e-5


def test_ragged_path_allocates_no_score_tensor():
    """(2, 1000, 64, 4): inputs and outputs together are under 3 MB, one score tensor is 32 MB and the GEMM
    chain allocates four"""
    from toycrystals_amd import functional as TF
    B, N, C, heads = 2, 1000, 64, 4
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, N, 3 * C, generator=g).cuda().requires_grad_()
    gy = torch.randn(B, N, C, generator=g).cuda()

    def step():
        y = TF.AttentionFn.apply(x, heads)
        assert y.grad_fn.ragged
        y.backward(gy)
        x.grad = None
        torch.cuda.synchronize()

    step()  # the grow-only workspace exists from here on
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    assert torch.cuda.max_memory_allocated() - base < B * heads * N * N * 4


def test_model_backward_reaches_the_kernels(monkeypatch):
    """diffusion_loss_eps of CondUNetTiny(4, 4, 32) at 40x40, B 2 (bottleneck N = 100, d 16): the parameter
    gradients of the default route against the GEMM chain's on the same draws, relative to the largest one"""
    from toycrystals_amd import functional as TF
    from toycrystals_amd.models.sde_score_model import CondUNetTiny, VPSDE, diffusion_loss_eps
    torch.manual_seed(0)
    model = CondUNetTiny(4, 4, 32).cuda().train()
    g = torch.Generator().manual_seed(1)
    x0 = torch.rand(2, 1, 40, 40, generator=g).cuda()
    y_cat, y_cont = torch.tensor([1, 3]).cuda(), torch.rand(2, 4, generator=g).cuda()
    draws = (torch.rand(2, generator=g), torch.randn(2, 1, 40, 40, generator=g), torch.rand(2, generator=g))
    routed = []
    apply = TF.AttentionFn.apply
    monkeypatch.setattr(TF.AttentionFn, "apply", lambda *a: routed.append(apply(*a)) or routed[-1])

    def grads(fused):
        monkeypatch.setattr(TF, "_ATTN_FUSED", fused)
        model.zero_grad(set_to_none=True)
        diffusion_loss_eps(model, VPSDE(0.1, 30.0), x0, y_cat, y_cont, p_uncond=0.1, draws=draws).backward()
        assert routed.pop().grad_fn.ragged is fused and not routed
        return [p.grad.double() for p in model.parameters()]

    ga, gb = grads(True), grads(False)
    top = max(float(b.abs().max()) for b in gb)
    worst = max(float((a - b).abs().max()) for a, b in zip(ga, gb)) / top
    print(f"  largest gradient {top:.3e}, worst difference / largest {worst:.2e}")
    assert top > 0 and worst < 2e-5
