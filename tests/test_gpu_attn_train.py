"""GPU: the fused training attention through the C ABI (tcx_attention_fwd_lse, tcx_attention_bwd:
csrc/attention.hip, csrc/attention_bwd.hip) against float64 torch on the CPU: SDPA forward, logsumexp of
the scaled logits, autograd for dqkv.

Gate: the training path's per-op bound of tests/test_gpu_train.py, max|a - ref| / max(1, max|ref|) < 2e-5,
applied separately to out, lse and the dq / dk / dv column blocks of dqkv (a zeroed block, a dropped head
or tile is an O(1) miss).  A float32 CPU evaluation of the same recomputing formulation stays <= 4.4e-6 on
all twelve case / amplitude pairs, so the gate has >= 4x room.  Outputs and the workspace sit between
canaries (test_gpu_train_ops.Arena); an element never written still holds 1.3e36 and fails its gate.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_ops import L, chk, st
from test_gpu_train_ops import Arena, P, bits

pytestmark = pytest.mark.gpu

EINVAL, EUNSUP, EWS = -1, -2, -4

# Bt, N, C, heads: the smallest shapes that reach each structure of the kernels
CASES = [
    (1, 32, 8, 1),      # one wave, one key tile
    (2, 96, 48, 2),     # three waves, d 24; head and batch strides
    (2, 256, 192, 4),   # the training shape (d 48: a second, part-used 32-row tile of d)
    (1, 256, 64, 2),    # d 32
    (1, 512, 32, 2),    # flash forward; two query / key blocks, four staged tiles
    (1, 768, 64, 1),    # odd block count; widest d
]


def err(a, ref):
    return float((a.double().cpu() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


@functools.lru_cache(maxsize=None)
def reference(Bt, N, C, heads, amp):
    """fp32-representable inputs (q and k scaled by amp: amp 3 gives peaked rows) and float64 results"""
    g = torch.Generator().manual_seed(N + C + amp)
    qkv = torch.randn(Bt, N, 3 * C, generator=g)
    qkv[..., :2 * C] *= amp
    dout = torch.randn(Bt, N, C, generator=g)
    x = qkv.double().requires_grad_()
    d = C // heads
    q, k, v = (t.view(Bt, N, heads, d).transpose(1, 2) for t in x.split(C, dim=2))
    out = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(Bt, N, C)
    out.backward(dout.double())
    lse = torch.logsumexp(q.detach() @ k.detach().transpose(-1, -2) / math.sqrt(d), dim=-1)
    return qkv, dout, out.detach(), lse, x.grad


@pytest.mark.parametrize("amp", [1, 3])
@pytest.mark.parametrize("Bt,N,C,heads", CASES)
def test_fwd_lse_and_bwd(Bt, N, C, heads, amp):
    qkv, dout, out_ref, lse_ref, dqkv_ref = reference(Bt, N, C, heads, amp)
    A = Arena()
    x, g = A.new(qkv.numel(), init=qkv.numpy()), A.new(dout.numel(), init=dout.numpy())
    out, plain, lse = A.new(Bt * N * C), A.new(Bt * N * C), A.new(Bt * heads * N)
    nb = L().tcx_attention_bwd_workspace(Bt, N, C, heads)
    assert nb == Bt * heads * N * 4
    ws = A.new(nb, torch.uint8)
    chk(L().tcx_attention_fwd_lse(P(x), P(out), P(lse), Bt, N, C, heads, st()))
    chk(L().tcx_attention(P(x), P(plain), Bt, N, C, heads, st()))
    dq = [A.new(3 * Bt * N * C) for _ in range(2)]
    for t in dq:
        chk(L().tcx_attention_bwd(P(x), P(out), P(g), P(lse), P(t), Bt, N, C, heads, P(ws), nb, st()))
    A.check()
    assert bits(out) == bits(plain), "out differs from tcx_attention"
    assert bits(dq[0]) == bits(dq[1]), "tcx_attention_bwd is not deterministic"
    got = dq[0].view(Bt, N, 3 * C)
    errs = {"out": err(out.view(Bt, N, C), out_ref), "lse": err(lse.view(Bt, heads, N), lse_ref)}
    for i, name in enumerate(("dq", "dk", "dv")):
        errs[name] = err(got[..., i * C:(i + 1) * C], dqkv_ref[..., i * C:(i + 1) * C])
    print("  " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 2e-5, f"{k}: {v:.3e}"


@pytest.mark.parametrize("kw,codes", [
    (dict(N=300), (EUNSUP, EINVAL)), (dict(N=576), (EUNSUP, EINVAL)), (dict(C=8), (EUNSUP, EINVAL)),  # d 4
    (dict(short=1), (EWS,)), (dict(Bt=0), (0,))], ids=str)
def test_refusals(kw, codes):
    """refused (or the empty batch accepted) before any launch: nothing written"""
    a = dict(Bt=1, N=256, C=32, heads=2, short=0)
    a.update(kw)
    A = Arena()
    x, g = A.new(256 * 96, init=torch.zeros(256 * 96).numpy()), A.new(256 * 32, init=torch.zeros(256 * 32).numpy())
    out, lse, dq, ws = A.new(256 * 32), A.new(2 * 256), A.new(256 * 96), A.new(2 * 256 * 4, torch.uint8)
    before = [bits(t) for t in (out, lse, dq, ws)]
    nb = L().tcx_attention_bwd_workspace(1, a["N"], a["C"], a["heads"]) - a["short"]
    if not a["short"]:
        assert L().tcx_attention_fwd_lse(P(x), P(out), P(lse), a["Bt"], a["N"], a["C"], a["heads"], st()) in codes
    rc = L().tcx_attention_bwd(P(x), P(out), P(g), P(lse), P(dq), a["Bt"], a["N"], a["C"], a["heads"], P(ws), nb, st())
    assert rc in codes, rc
    if rc == EWS:
        assert str(nb + 1) in L().tcx_last_error().decode()
    torch.cuda.synchronize()
    assert [bits(t) for t in (out, lse, dq, ws)] == before, "a refused call wrote"
    A.check()
