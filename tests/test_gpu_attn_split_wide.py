"""GPU: tcx_attention_split_wide (k_attention_split_wide<D, FMT>, head dim 80 / 96 / 128: 128-query workgroups,
32-key tiles, a peeled and masked last tile) through the C ABI against float64, in the three storage formats.
Arena buffers end at their last byte, so a tail read or a stray store shows; every call runs twice, bit-equal.

Gate: attn_ref.bound with this kernel's tile count nt = ceil(N / 32), and the two bf16 rounding terms doubled as
in test_gpu_attn_split_ragged.bound (the true half-ulp of round-to-nearest bf16): derived, no emulation
fallback, no case left out.  attn_ref.Case.ones (D % 32 != 0) is this kernel's rule too: the ONES row at 80."""
import pytest
import torch

import attn_ref as R
import train_ops_ref as T
from test_gpu_attn import Bufs, put_bytes, values
from test_gpu_attn_split_ragged import FMT, bound
from test_gpu_ops import L, chk, st
from test_gpu_train_ops import Arena, P, bits, gate, last_error

pytestmark = pytest.mark.gpu

# 1: one key, one query; 31 / 32 / 33: one below, at and one above the key tile; 129: one live key in the last
# tile and one live query in the second workgroup; 137: a tail that ends inside a 16-key k-step; 576: 96x96
NS = (1, 31, 32, 33, 129, 137, 576)
DIMS = (80, 96, 128)


class Case(R.Case):
    __slots__ = ()

    @property
    def ntile(self):
        return -(-self.N // 32)


def _cases():
    out = []

    def mk(e, N, D, family, arg=None):   # heads 1..3: onehot's h2 values need C <= 511 (D = 128: 3 heads)
        k = len(out) + 1
        out.append(Case(e, "wide", N, D, 1 + k % 3, 1 + (k // 2) % 3, family, arg))
    for e in FMT:
        for j, N in enumerate(NS):
            mk(e, N, DIMS[j % 3], "gauss", 1.0)
            mk(e, N, DIMS[(j + 1) % 3], "gauss", 3.0)
            mk(e, N, DIMS[(j + 2) % 3], "onehot")
            if j % 2:
                mk(e, N, DIMS[j % 3], "constv" if j % 4 == 1 else "uniform")
    return out


def call(x, y, fmt, Bt, N, C, heads):
    return L().tcx_attention_split_wide(x, y, fmt, Bt, N, C, heads, st())


@pytest.mark.parametrize("c", _cases(), ids=repr)
def test_split_wide_against_float64(c):
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
    (dict(x=None), -1, "null pointer"), (dict(y=None), -1, "null pointer"), (dict(x=4), -1, "16-B aligned"),
    (dict(y=4), -1, "16-B aligned"), (dict(fmt=-1), -1, "fmt must be"), (dict(fmt=3), -1, "fmt must be"),
    (dict(C=128), -2, "head dim 64"), (dict(C=224), -2, "head dim 112"), (dict(N=0), -1, "N must be"),
    (dict(Bt=-1), -1, "Bt must be in [0, 65535]"), (dict(Bt=65536), -1, "Bt must be in [0, 65535]"),
    (dict(heads=0), -1, "bad args"), (dict(C=80 * 65536, heads=65536), -1, "heads must be in [1, 65535]"),
    (dict(Bt=0, N=137, fmt=1), 0, None),
]


@pytest.mark.parametrize("kw,rc,msg", REFUSALS, ids=str)
def test_refusals_and_empty_batch(kw, rc, msg):   # -1 TCX_EINVAL, -2 TCX_EUNSUP; Bt = 0 returns 0; nothing is written
    b = Bufs()
    a = dict(x=0, y=0, fmt=0, Bt=1, N=32, C=192, heads=2)
    a.update(kw)
    x, y = (None if a[k] is None else P(t) + a[k] for k, t in (("x", b.x), ("y", b.y)))
    assert call(x, y, a["fmt"], a["Bt"], a["N"], a["C"], a["heads"]) == rc
    assert msg is None or (last_error().startswith("tcx_attention_split_wide:") and msg in last_error())
    b.untouched()
