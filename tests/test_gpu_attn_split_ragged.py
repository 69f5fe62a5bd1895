"""GPU: tcx_attention_split_ragged (k_attention_split_ragged<D, FMT>: 128-query workgroups, 64-key tiles, a peeled
and masked last tile) through the C ABI against float64, in the three storage formats.  Arena buffers end at
their last byte, so a tail read or a stray store shows; every call runs twice, bit-equal.

Gate: attn_ref.bound with this kernel's tile count nt = ceil(N / 64).  For the two bf16 entries the two bf16
rounding terms are doubled (the output's 2^-9 |o|, and the P term 2 * 2^-9 sig or 2^-9 * 2 A): round-to-nearest
bf16 errs by up to 2^-8 relative just above a power of two, and with that true half-ulp the gate is derived
and needs no emulation fallback.  No case is left out."""
import numpy as np
import pytest
import torch

import attn_ref as R
import train_ops_ref as T
from test_gpu_attn import Bufs, put_bytes, values
from test_gpu_ops import L, chk, st
from test_gpu_train_ops import Arena, P, bits, gate, last_error

pytestmark = pytest.mark.gpu

# 1: one key, one query; 63: under one tile; 257: one live key in the last tile and one live query in the last
# workgroup; 288: a tail of exactly one sub-tile; 300: a tail that ends inside a 16-key k-step; 576: the 96x96
# bottleneck; 625: odd
NS = (1, 63, 257, 288, 300, 576, 625)
FMT = {"split": 0, "split_bf16": 1, "split_b2": 2}


class Case(R.Case):
    __slots__ = ()

    @property
    def ntile(self):
        return -(-self.N // 64)


def _cases():
    out = []

    def mk(e, N, D, family, arg=None):
        k = len(out) + 1
        out.append(Case(e, "ragged", N, D, 1 + k % 4, 1 + (k // 3) % 4, family, arg))
    for e in FMT:
        for j, N in enumerate(NS):
            fit = [d for d in R.DIMS_LONG if d >= max(8, int(N - 1).bit_length())]   # onehot codes the key index
            mk(e, N, R.DIMS_LONG[j % 4], "gauss", 1.0)
            mk(e, N, R.DIMS_LONG[(j + 1) % 4], "gauss", 3.0)
            mk(e, N, R.DIMS_LONG[(j + 2) % 4], "constv" if j % 2 else "uniform")
            mk(e, N, fit[(j + 3) % len(fit)], "onehot")
    return out


def call(x, y, fmt, Bt, N, C, heads):
    return L().tcx_attention_split_ragged(x, y, fmt, Bt, N, C, heads, st())


def bound(c, ref, lo):
    b = R.bound(c, ref, lo)
    if c.entry != "split":
        if not lo:
            b = b + 2.0 ** -9 * np.abs(ref.o)
        if c.family != "onehot":
            b = b + (2 * 2.0 ** -9 * ref.sig if c.ones else 2.0 ** -9 * 2 * ref.A)
    return b


@pytest.mark.parametrize("c", _cases(), ids=repr)
def test_split_ragged_against_float64(c):
    A, ref = Arena(), R.reference(c)
    x = put_bytes(A, R.encode(R.inputs(c), c.fmt_in))
    outs = [A.new(R.nbytes(c.Bt * c.N * c.C, c.fmt_out), torch.uint8) for _ in range(2)]
    for y in outs:
        chk(call(P(x), P(y), FMT[c.entry], c.Bt, c.N, c.C, c.heads))
    A.check()
    assert bits(outs[0]) == bits(outs[1]), f"{c} is not deterministic"
    raw = outs[0].cpu().numpy()
    for lo in ((False, True) if c.entry == "split_bf16" else (False,)):   # a bf16 record: the hi half, and hi + lo
        gate(repr(c) + (" [hi+lo]" if lo else ""), T._worst(T._diff(values(c, raw, lo), ref.o), bound(c, ref, lo)))


REFUSALS = [
    (dict(x=None), -1, "null pointer"), (dict(y=None), -1, "null pointer"), (dict(heads=0), -1, "bad args"),
    (dict(heads=3), -1, "bad args"), (dict(fmt=3), -1, "fmt must be"), (dict(fmt=-1), -1, "fmt must be"),
    (dict(C=16), -2, "head dim 8"), (dict(C=80), -2, "head dim 40"), (dict(N=0), -1, "N must be"),
    (dict(x=4), -1, "16-B aligned"), (dict(y=4), -1, "16-B aligned"), (dict(Bt=65536), -1, "Bt must be in [0, 65535]"),
    (dict(Bt=-1), -1, "Bt must be in [0, 65535]"), (dict(C=16 * 65536, heads=65536), -1, "heads must be in [1, 65535]"),
    (dict(Bt=0, N=300, fmt=1), 0, None),
]


@pytest.mark.parametrize("kw,rc,msg", REFUSALS, ids=str)
def test_refusals_and_empty_batch(kw, rc, msg):   # -1 TCX_EINVAL, -2 TCX_EUNSUP; Bt = 0 returns 0; nothing is written
    b = Bufs()
    a = dict(x=0, y=0, fmt=0, Bt=1, N=256, C=32, heads=2)
    a.update(kw)
    x, y = (None if a[k] is None else P(t) + a[k] for k, t in (("x", b.x), ("y", b.y)))
    assert call(x, y, a["fmt"], a["Bt"], a["N"], a["C"], a["heads"]) == rc
    assert msg is None or (last_error().startswith("tcx_attention_split_ragged:") and msg in last_error())
    b.untouched()
