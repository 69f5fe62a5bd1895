"""GPU: tcx_attention_ragged (k_attention_ragged<D>: 64-key tiles, a masked last tile) through the C ABI against
float64.  Arena buffers end at their last byte, so a tail read or a stray store shows; every call runs twice,
bit-equal.  Gate: the derived bound of attn_ref.py:323-373 with this kernel's tile count nt = ceil(N / 64)."""
import numpy as np
import pytest
import torch

import attn_ref as R
import train_ops_ref as T
from attn_ref import U
from test_gpu_attn import Bufs, put_bytes, values
from test_gpu_ops import L, chk, st
from test_gpu_train_ops import Arena, P, bits, gate, last_error

pytestmark = pytest.mark.gpu

# 1: one key, one query; 63: under one tile; 257: one live key in the last tile and one live query in the last
# workgroup; 288: a tail of exactly one sub-tile; 300: a ragged sub-tile; 576: the 96x96 bottleneck; 625: odd
NS = (1, 63, 257, 288, 300, 576, 625)


def _cases():
    out = []

    def mk(N, h2, D, family, arg=None):
        k = len(out) + 1
        out.append(R.Case("attention_h2" if h2 else "attention", "ragged", N, D, 1 + k % 4, 1 + (k // 3) % 2, family, arg))
    for j, (N, h2) in enumerate((N, h2) for N in NS for h2 in (0, 1)):
        fit = [d for d in R.DIMS if d >= max(8, int(N - 1).bit_length())]   # onehot codes the key index on D dims
        mk(N, h2, R.DIMS[j % 6], "gauss", 3.0 if j % 2 else 1.0)
        mk(N, h2, R.DIMS[(j + 3) % 6], "constv" if (j // 2 + h2) % 2 else "uniform")
        mk(N, h2, fit[(j + 1) % len(fit)], "onehot")
    return out


def call_case(c, x, y, ovf=None):
    return L().tcx_attention_ragged(P(x), P(y), int(c.entry == "attention_h2"), c.Bt, c.N, c.C, c.heads, P(ovf), st())


def bound(c, ref):
    o, A = np.abs(ref.o), ref.A
    if c.family == "onehot":
        return R.out_rounding(c, o) + 4 * U * o + 2 * c.N * np.exp(-39.0) * ref.vmax
    c1 = 2 + (c.N - 1) + c.N + 2 + 1 + 3 * (-(-c.N // 64) - 1)
    return (2 * (c.D + 2) * U * ref.sabs + c1 * U) * 2 * A + R.out_rounding(c, o)


@pytest.mark.parametrize("c", _cases(), ids=repr)
def test_ragged_against_float64(c):
    A, ref = Arena(), R.reference(c)
    x = put_bytes(A, R.encode(R.inputs(c), "f32"))
    outs = [A.new(c.Bt * c.N * c.C * 4, torch.uint8) for _ in range(2)]
    for y in outs:
        chk(call_case(c, x, y))
    A.check()
    assert bits(outs[0]) == bits(outs[1]), f"{c} is not deterministic"
    gate(repr(c), T._worst(T._diff(values(c, outs[0].cpu().numpy()), ref.o), bound(c, ref)))


def test_h2_range_flag():
    """onehot: one v value of 7e4 reaches one output element and raises the flag; else 0; ovf = NULL accepted"""
    c = R.Case("attention_h2", "ragged", 300, 16, 2, 1, "onehot", None)
    big = R.inputs(c).copy()
    big[0, 5, 2 * c.C + 3] = 7e4
    for qkv, want in ((big, 1), (R.inputs(c), 0)):
        A = Arena()
        x = put_bytes(A, R.encode(qkv, "f32"))
        y = A.new(c.Bt * c.N * c.C * 4, torch.uint8)
        ovf = A.new(1, torch.int32, init=np.zeros(1))
        chk(call_case(c, x, y, ovf))
        A.check()
        assert int(ovf.item()) == want
    chk(call_case(c, x, y, None))
    A.check()


REFUSALS = [
    (dict(x=None), "null pointer"), (dict(y=None), "null pointer"), (dict(heads=0), "bad args"),
    (dict(heads=3), "bad args"), (dict(N=0), "N must be"), (dict(N=-300), "N must be"), (dict(out_h2=2), "out_h2"),
    (dict(out_h2=-1), "out_h2"), (dict(C=80), "head dim 40"), (dict(C=24), "head dim 12"),
    (dict(x=4), "16-B aligned"), (dict(y=4), "16-B aligned"), (dict(Bt=-1), "Bt must be in [0, 65535]"),
    (dict(Bt=65536), "Bt must be in [0, 65535]"), (dict(C=8 * 65536, heads=65536), "heads must be in [1, 65535]"),
    (dict(out_h2=1, C=12, heads=1), "C % 8"), (dict(Bt=0, N=300, out_h2=1), None),
]


@pytest.mark.parametrize("kw,msg", REFUSALS, ids=str)
def test_refusals_and_empty_batch(kw, msg):   # msg None: Bt = 0 returns 0; nothing is written either way
    b = Bufs()
    a = dict(x=0, y=0, out_h2=0, Bt=1, N=256, C=32, heads=2)
    a.update(kw)
    x, y = (None if a[k] is None else P(t) + a[k] for k, t in (("x", b.x), ("y", b.y)))
    rc = L().tcx_attention_ragged(x, y, a["out_h2"], a["Bt"], a["N"], a["C"], a["heads"], P(b.ovf), st())
    assert rc == 0 if msg is None else rc != 0 and last_error().startswith("tcx_attention_ragged:") and msg in last_error()
    b.untouched()
