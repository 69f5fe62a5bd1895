"""GPU: the wide-head attention (head dim 80, 96, 128; csrc/attention_wide.hip, csrc/attention_wide_bwd.hip)
through the C ABI against float64: attn_ref.sdpa64 for the forward, test_gpu_attn_train.reference (torch CPU
float64 autograd) for lse and dqkv.  Buffers sit between canaries; every kernel runs twice, bit-equal.

Gates.  Forward, fp32 and h2 out: attn_ref.bound per element (the fp32-MFMA forms' score and softmax terms and
the output format's term) with this kernel's tile count, nt = ceil(N / 32) key tiles, in the 3 (nt - 1) term of
attn_ref.c1.  lse: 4 * 2^-24 * (|lse| + 1).  dq, dk, dv: 2e-5 of each block's maximum, the gate of
test_gpu_attn_ragged_train.py.  N: 1 and 31 are under one 32-key tile; 31 / 32 / 33 and 127 / 128 / 129 sit
around the key tile and the 128-query workgroup; 65 has one live key in its third tile; 200 and 576 span 7 and
18 tiles and 2 and 5 workgroups."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import attn_ref as R
import train_ops_ref as T
from attn_ref import U
from test_gpu_attn import values
from test_gpu_attn_train import EINVAL, EUNSUP, EWS, err, reference
from test_gpu_ops import L, chk, st
from test_gpu_train_ops import Arena, P, bits, gate, last_error

pytestmark = pytest.mark.gpu

HEADS, BT = 2, 3
NS = (1, 31, 32, 33, 65, 127, 128, 129, 200, 576)


@lru_cache(maxsize=None)
def forward_ref(N, D):
    return R.sdpa64(reference(BT, N, D * HEADS, HEADS, 1)[0].numpy(), HEADS)


def fwd_bound(c, ref):
    return R.bound(c, ref) + 3 * (-(-c.N // 32) - 1) * U * 2 * ref.A


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("D", [80, 96, 128])
def test_forward_lse_backward(D, N):
    C = D * HEADS
    qkv, dout, _, lse_ref, dqkv_ref = reference(BT, N, C, HEADS, 1)
    ref = forward_ref(N, D)
    A = Arena()
    x, g = A.new(qkv.numel(), init=qkv.numpy()), A.new(dout.numel(), init=dout.numpy())
    f32 = [A.new(BT * N * C) for _ in range(2)]
    h2 = [A.new(BT * N * C * 4, torch.uint8) for _ in range(2)]
    out, lse = A.new(BT * N * C), A.new(BT * HEADS * N)
    ovf = A.new(1, torch.int32, init=np.zeros(1))
    nb = L().tcx_attention_wide_bwd_workspace(BT, N, C, HEADS)
    assert nb == BT * HEADS * N * 4
    ws = A.new(nb, torch.uint8)
    dq = [A.new(3 * BT * N * C) for _ in range(2)]
    for y in f32:
        chk(L().tcx_attention_wide(P(x), P(y), 0, BT, N, C, HEADS, None, st()))
    for y in h2:
        chk(L().tcx_attention_wide(P(x), P(y), 1, BT, N, C, HEADS, P(ovf), st()))
    chk(L().tcx_attention_wide_fwd_lse(P(x), P(out), P(lse), BT, N, C, HEADS, st()))
    for t in dq:
        chk(L().tcx_attention_wide_bwd(P(x), P(out), P(g), P(lse), P(t), BT, N, C, HEADS, P(ws), nb, st()))
    A.check()
    assert bits(f32[0]) == bits(f32[1]) and bits(h2[0]) == bits(h2[1]), "tcx_attention_wide is not deterministic"
    assert bits(out) == bits(f32[0]), "out differs from tcx_attention_wide"
    assert bits(dq[0]) == bits(dq[1]), "tcx_attention_wide_bwd is not deterministic"
    assert int(ovf.item()) == 0
    for entry, y in (("attention", f32[0]), ("attention_h2", h2[0])):
        c = R.Case(entry, "wide", N, D, HEADS, BT, "gauss", 1.0)
        raw = y.cpu().numpy().view(np.uint8)
        gate(repr(c), T._worst(T._diff(values(c, raw), ref.o), fwd_bound(c, ref)))
    dl = (lse.view(BT, HEADS, N).double().cpu() - lse_ref).abs()
    print(f"  lse worst / bound {float((dl / (4 * U * (lse_ref.abs() + 1))).max()):.3f}")
    assert bool((dl <= 4 * U * (lse_ref.abs() + 1)).all())
    got = dq[0].view(BT, N, 3 * C)
    for i, name in enumerate(("dq", "dk", "dv")):
        e = err(got[..., i * C:(i + 1) * C], dqkv_ref[..., i * C:(i + 1) * C])
        print(f"  {name} {e:.2e}")
        assert e < 2e-5, f"{name}: {e:.3e}"


def test_h2_range_flag():
    """V scaled to 7e4 (past f16's 65504 at every output) raises the flag; the same call unscaled leaves 0"""
    N, C = 40, 80
    qkv = reference(1, N, C, 1, 1)[0]
    big = qkv.clone()
    big[..., 2 * C:] = 7e4
    for q, want in ((big, 1), (qkv, 0)):
        A = Arena()
        x, y = A.new(q.numel(), init=q.numpy()), A.new(N * C * 4, torch.uint8)
        ovf = A.new(1, torch.int32, init=np.zeros(1))
        chk(L().tcx_attention_wide(P(x), P(y), 1, 1, N, C, 1, P(ovf), st()))
        A.check()
        assert int(ovf.item()) == want


@pytest.mark.parametrize("kw,code", [
    (dict(C=128), EUNSUP), (dict(C=224), EUNSUP),  # d 64, d 112
    (dict(N=0), EINVAL), (dict(null=1), EINVAL), (dict(shift=4), EINVAL), (dict(Bt=65536), EINVAL),
    (dict(short=1), EWS), (dict(Bt=0), 0)], ids=str)
def test_refusals(kw, code):
    """all four entries refuse (or accept the empty batch) before any launch, by name: nothing written"""
    a = dict(Bt=1, N=100, C=160, heads=2, short=0, shift=0, null=0)
    a.update(kw)
    A = Arena()
    n = 100 * 224
    x, g = A.new(3 * n, init=np.zeros(3 * n), shift=a["shift"]), A.new(n, init=np.zeros(n))
    out, lse, dq, ws = A.new(n), A.new(2 * 100), A.new(3 * n), A.new(2 * 100 * 4, torch.uint8)
    before = [bits(t) for t in (out, lse, dq, ws)]
    nb = L().tcx_attention_wide_bwd_workspace(a["Bt"] or 1, a["N"], a["C"], a["heads"])
    assert nb == (0 if code in (EUNSUP, EINVAL) and not (a["shift"] or a["null"]) else a["N"] * a["heads"] * 4)
    px = None if a["null"] else P(x)
    sh = a["Bt"], a["N"], a["C"], a["heads"]
    rcs = [L().tcx_attention_wide_bwd(px, P(out), P(g), P(lse), P(dq), *sh, P(ws), nb - a["short"], st())]
    msgs = [last_error()]
    if not a["short"]:
        rcs += [L().tcx_attention_wide_fwd_lse(px, P(out), P(lse), *sh, st())]
        msgs += [last_error()]
        rcs += [L().tcx_attention_wide(px, P(out), 0, *sh, None, st())]
        msgs += [last_error()]
    assert rcs == [code] * len(rcs), rcs
    if code:
        assert msgs[0].startswith("tcx_attention_wide_bwd:") and all(m.startswith("tcx_attention_wide") for m in msgs)
    if code == EWS:
        assert str(nb) in msgs[0]
    torch.cuda.synchronize()
    assert [bits(t) for t in (out, lse, dq, ws)] == before, "a refused call wrote"
    A.check()
