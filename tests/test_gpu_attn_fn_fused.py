"""GPU: AttentionFn (toycrystals_amd/functional.py) on the fused path (tcx_attention_fwd_lse +
tcx_attention_bwd) and on the GEMM chain, both against float64 autograd at the training path's 2e-5 gate,
and the fused path's peak memory: no [B, heads, N, N] tensor is allocated."""
import pytest
import torch

from test_gpu_attn_train import err, reference

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("B,N,C,heads", [(2, 256, 192, 4), (1, 512, 64, 2)])
def test_attention_fn_both_paths(monkeypatch, fused, B, N, C, heads):
    from toycrystals_amd import functional as TF
    monkeypatch.setattr(TF, "_ATTN_FUSED", fused)
    qkv, dout, out_ref, _, dqkv_ref = reference(B, N, C, heads, 1)
    x = qkv.cuda().requires_grad_()
    y = TF.AttentionFn.apply(x, heads)
    assert y.grad_fn.fused == fused
    y.backward(dout.cuda())
    assert err(y.detach(), out_ref) < 2e-5
    assert err(x.grad, dqkv_ref) < 2e-5


def test_fused_path_allocates_no_score_tensor(monkeypatch):
    """(2, 1024, 64, 4): inputs and outputs together are under 3 MB, one score tensor is 33.5 MB and the
    GEMM chain allocates four"""
    from toycrystals_amd import functional as TF
    monkeypatch.setattr(TF, "_ATTN_FUSED", True)
    B, N, C, heads = 2, 1024, 64, 4
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, N, 3 * C, generator=g).cuda().requires_grad_()
    gy = torch.randn(B, N, C, generator=g).cuda()

    def step():
        TF.AttentionFn.apply(x, heads).backward(gy)
        x.grad = None
        torch.cuda.synchronize()

    step()  # the grow-only workspace exists from here on
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    assert torch.cuda.max_memory_allocated() - base < B * heads * N * N * 4
