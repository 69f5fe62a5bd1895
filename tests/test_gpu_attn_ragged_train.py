"""GPU: the fused training attention for any token count through the C ABI (tcx_attention_ragged_fwd_lse,
tcx_attention_ragged_bwd: csrc/attention_ragged.hip, csrc/attention_ragged_bwd.hip) against float64 torch on
the CPU (test_gpu_attn_train.reference: SDPA forward, logsumexp of the scaled logits, autograd for dqkv).

Gate: the training path's per-op bound of tests/test_gpu_train.py, max|a - ref| / max(1, max|ref|) < 2e-5,
applied separately to out, lse and the dq / dk / dv column blocks of dqkv.  A float32 CPU evaluation of the
same recomputing formulation stays <= 4.8e-6 on all fourteen case / amplitude pairs (worst: out of
(1, 257, 64, 1) at amplitude 3), so the gate has >= 4x room and no pair is dropped.  Outputs and the workspace
sit between canaries (test_gpu_train_ops.Arena); an element never written still holds 1.3e36 and fails its gate.
"""
import pytest
import torch

from test_gpu_attn_train import EINVAL, EUNSUP, EWS, err, reference
from test_gpu_ops import L, chk, st
from test_gpu_train_ops import Arena, P, bits

pytestmark = pytest.mark.gpu

# Bt, N, C, heads: the smallest shapes that reach each structure of the kernels
CASES = [
    (1, 1, 8, 1),       # one row, one key: the whole workgroup but one lane is clamped
    (2, 63, 48, 2),     # under one tile; d 24; batch and head strides
    (1, 129, 16, 1),    # one live row in the second workgroup, one in the third tile's first sub-tile
    (1, 160, 64, 2),    # a tail of exactly one sub-tile; d 32
    (1, 257, 64, 1),    # widest d; one live row past four full tiles
    (1, 300, 32, 2),    # a ragged second sub-tile in the tail
    (2, 576, 192, 4),   # the 96x96 training shape: d 48, nine full tiles and an all-live peeled one
]


@pytest.mark.parametrize("amp", [1, 3])
@pytest.mark.parametrize("Bt,N,C,heads", CASES)
def test_fwd_lse_and_bwd(Bt, N, C, heads, amp):
    qkv, dout, out_ref, lse_ref, dqkv_ref = reference(Bt, N, C, heads, amp)
    A = Arena()
    x, g = A.new(qkv.numel(), init=qkv.numpy()), A.new(dout.numel(), init=dout.numpy())
    out, plain, lse = A.new(Bt * N * C), A.new(Bt * N * C), A.new(Bt * heads * N)
    nb = L().tcx_attention_ragged_bwd_workspace(Bt, N, C, heads)
    assert nb == Bt * heads * N * 4
    ws = A.new(nb, torch.uint8)
    chk(L().tcx_attention_ragged_fwd_lse(P(x), P(out), P(lse), Bt, N, C, heads, st()))
    chk(L().tcx_attention_ragged(P(x), P(plain), 0, Bt, N, C, heads, None, st()))
    dq = [A.new(3 * Bt * N * C) for _ in range(2)]
    for t in dq:
        chk(L().tcx_attention_ragged_bwd(P(x), P(out), P(g), P(lse), P(t), Bt, N, C, heads, P(ws), nb, st()))
    A.check()
    assert bits(out) == bits(plain), "out differs from tcx_attention_ragged"
    assert bits(dq[0]) == bits(dq[1]), "tcx_attention_ragged_bwd is not deterministic"
    got = dq[0].view(Bt, N, 3 * C)
    errs = {"out": err(out.view(Bt, N, C), out_ref), "lse": err(lse.view(Bt, heads, N), lse_ref)}
    for i, name in enumerate(("dq", "dk", "dv")):
        errs[name] = err(got[..., i * C:(i + 1) * C], dqkv_ref[..., i * C:(i + 1) * C])
    print("  " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 2e-5, f"{k}: {v:.3e}"


@pytest.mark.parametrize("kw,code", [
    (dict(C=8), EUNSUP), (dict(C=80), EUNSUP),  # d 4, d 40
    (dict(N=0), EINVAL), (dict(short=1), EWS), (dict(shift=4), EINVAL), (dict(Bt=0), 0)], ids=str)
def test_refusals(kw, code):
    """refused (or the empty batch accepted) before any launch, by name: nothing written"""
    a = dict(Bt=1, N=100, C=32, heads=2, short=0, shift=0)
    a.update(kw)
    A = Arena()
    n = 100 * 80
    x, g = A.new(3 * n, init=torch.zeros(3 * n).numpy(), shift=a["shift"]), A.new(n, init=torch.zeros(n).numpy())
    out, lse, dq, ws = A.new(n), A.new(2 * 100), A.new(3 * n), A.new(2 * 100 * 4, torch.uint8)
    before = [bits(t) for t in (out, lse, dq, ws)]
    nb = L().tcx_attention_ragged_bwd_workspace(1, a["N"], a["C"], a["heads"])
    assert nb == (0 if code in (EUNSUP, EINVAL) and not a["shift"] else a["N"] * a["heads"] * 4)
    rcs = [L().tcx_attention_ragged_bwd(P(x), P(out), P(g), P(lse), P(dq), a["Bt"], a["N"], a["C"], a["heads"], P(ws),
                                        nb - a["short"], st())]
    msgs = [L().tcx_last_error().decode()]
    if not a["short"]:
        rcs.append(L().tcx_attention_ragged_fwd_lse(P(x), P(out), P(lse), a["Bt"], a["N"], a["C"], a["heads"], st()))
        msgs.append(L().tcx_last_error().decode())
    assert rcs == [code] * len(rcs), rcs
    if code:
        assert msgs[0].startswith("tcx_attention_ragged_bwd:") and msgs[-1].startswith("tcx_attention_ragged_")
    if code == EWS:
        assert str(nb) in msgs[0]
    torch.cuda.synchronize()
    assert [bits(t) for t in (out, lse, dq, ws)] == before, "a refused call wrote"
    A.check()
