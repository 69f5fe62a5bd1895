"""GPU: the attention kernels of csrc/attention.hip and csrc/attention_split.hip through the C ABI at their
dispatch edges (tcx_attention, tcx_attention_h2, tcx_attention_split, _split_bf16, _split_b2), against the
float64 reference of tests/attn_ref.py (gates, input families, mutants and the restated dispatch are stated
there and proved in tests/test_attn_ref_cpu.py).

Every input and output lives in an Arena between runs of 0x7b bytes and ends at the last byte the call may
touch: a load past the end multiplies 1.3e36 in, a store outside trips the canary, an element never written
still holds the pattern and fails its gate.  Every call runs twice and the two outputs must agree bit for bit.
Errors are measured against float64 only.  Each test prints error against bound (pytest -s); the module
prints the worst error / bound per group at the end.

Reached here (attn_ref.GROUPS; test_attn_ref_cpu prints the instantiation of every group)
  valu        k_attention<8..64>, never run before: N 1 .. 255 off a multiple of 32 (N < 4: lanes that own no
              key; every last query block ragged), heads 1 / 3, Bt 1 / 2
  mfma        k_attention_mfma<8..64> at N 32 (one wave) .. 256, heads 1 / 2 / 5, Bt up to 3
  flash       k_attention_flash<16..64> at N 512 / 768, and the steered families at 768 / 1280
  h2          the out_h2 form of all six mfma and all four flash instances; the range flag raised, left alone, NULL
  split       k_attention_split<D, 0, 0> D 16 .. 64 at N 256 / 512 / 768, 1 / 3 / 9 / 15 / 17 workgroups
  split_bf16  k_attention_split<D, 1, 0 | 1>, split_b2: <D, 2, 0 | 1>: the same, N = 256 without and N >= 512 with
              the two-deep prefetch; both halves of a bf16 record are gated (hi at 2^-9, hi + lo at 2^-17)
  every refusal of the five entries, the new Bt / heads bounds included; the numpy codecs against the GPU
  writers; TCX_ATTN_XCD / TCX_ATTN_PF2 / TCX_ATTN_DEFER = 0 in child processes.
Not reached
  qkv extents past 2 GiB (N * 3C * 4 bytes), grids past 65535 rows (refused on the host, never launched),
  k_attn_block (csrc/attn_block.hip: one shape, held bit-identical to the launches it replaces).

4 x fallback (attn_ref.needs_emul: the form's own CPU emulation misses the derived gate): ten gauss(3) cases of
the bf16 forms' hi halves, listed by test_attn_ref_cpu.py.  The stated output term 2^-9 |o| is half of bf16's
round-to-nearest error just above a power of two; the emulation's error there is 1.4e-2 .. 3.1e-2 against
bounds of 1.3e-2 .. 2.4e-2, and the GPU's error equals the emulation's to three digits (2.871e-02 both).

Measured on the MI355X (430 tests; 3.1 s inside the module without the three child processes, which take
2.5 .. 2.8 s each, a Python start and library load; profiles/r10_attn_tests.txt), worst error / bound per group:
  valu 0.028   mfma 0.011   flash 0.002 (rising 0.002, threshold 0.001)   h2 0.029   split 0.038
  split_bf16 hi 0.770, hi + lo 0.406 (gauss(3)); rising 0.247, falling 0.203, threshold 0.053, uniform 0.080
  split_b2 0.382 (gauss(3)); rising 0.196, falling 0.170, threshold 0.038
  onehot 0 everywhere but 1e-7 relative in a few h2 / hi + lo cases; constv at most 0.011 (fp32 mfma)
  TCX_ATTN_DEFER=0: 0.416 against 0.416 at the default; max |exact - deferred| 2.4e-4 .. 6.3e-2 (one bf16 ulp)
TCX_ATTN_XCD=0 and TCX_ATTN_PF2=0 are bit-identical to the defaults.  No canary was touched, every rerun was
bit-equal.
Found: k_attention_split<32 | 64, 1 | 2> summed l from the unrounded p while the MFMA multiplied bf16(p); under
the deferred maximum the row's largest p is no longer the exact 2^10 and nine gauss(3) cases missed their gate
by 0.2 .. 8 % (err / bound 1.002 .. 1.084).  l now sums the rounded p (v_dot2c_f32_bf16 against packed ones,
DESIGN.md); the same cases sit at 0.11 .. 0.77.  The unbounded Bt / heads and the negative Bt of the five
entries were confirmed from the code and are refused now; no other kernel defect showed.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import attn_ref as R
import train_ops_ref as T
from attn_ref import F32
from test_gpu_ops import L, chk, st
from test_gpu_train_ops import Arena, P, bits, gate, last_error

pytestmark = pytest.mark.gpu

WORST = {}
T0 = [None]
ENTRY = {"attention": "tcx_attention", "attention_h2": "tcx_attention_h2", "split": "tcx_attention_split",
         "split_bf16": "tcx_attention_split_bf16", "split_b2": "tcx_attention_split_b2"}


@pytest.fixture(scope="module", autouse=True)
def report():
    T0[0] = time.time()
    yield
    print(f"\n  test_gpu_attn: {time.time() - T0[0]:.1f} s; worst error / bound per group:")
    for k, v in WORST.items():
        print(f"    {k:36s} {v:.3f}")


def put_bytes(A, a):
    """a numpy array's bytes in an Arena buffer that ends at its last byte"""
    b = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return A.new(b.size, torch.uint8, init=b)


def call(c, qkv, out, ovf=None, Bt=None):
    fn = getattr(L(), ENTRY[c.entry])
    Bt = c.Bt if Bt is None else Bt
    if c.entry == "attention_h2":
        return fn(P(qkv), P(out), Bt, c.N, c.C, c.heads, P(ovf), st())
    return fn(P(qkv), P(out), Bt, c.N, c.C, c.heads, st())


def run_case(c, qkv=None):
    """the raw output bytes of one call (numpy uint8); canaries, two bit-equal runs"""
    qkv = R.inputs(c) if qkv is None else qkv
    A = Arena()
    x = put_bytes(A, R.encode(qkv, c.fmt_in))
    nb = R.nbytes(c.Bt * c.N * c.C, c.fmt_out)
    outs = []
    for _ in range(2):
        y = A.new(nb, torch.uint8)
        chk(call(c, x, y))
        outs.append(y)
    A.check()
    assert bits(outs[0]) == bits(outs[1]), f"{c} is not deterministic"
    return outs[0].cpu().numpy()


def values(c, raw, lo=False):
    """the values the raw output stands for, through the numpy codec"""
    if c.fmt_out == "f32":
        return raw.view(F32).reshape(c.Bt, c.N, c.C).astype(np.float64)
    if c.fmt_out == "b2":
        return R.decode(raw.view(np.uint16).reshape(c.Bt, c.N, c.C), "b2")
    return R.decode(raw.view(np.uint16).reshape(c.Bt, c.N, c.C // 8, 2, 8), c.fmt_out, lo=(lo or c.fmt_out == "h2"))


def check_raw(group, c, raw, what=""):
    qkv, ref = R.inputs(c), R.reference(c)
    for lo in ((False, True) if c.entry == "split_bf16" else (False,)):
        em = R.emulate(c, qkv, lo) if R.needs_emul(c, lo) else None
        eb = R.gate(c, values(c, raw, lo), ref, em, lo)
        k = f"{group} {c.family}" + (" hi+lo" if lo else "")
        r = 0.0 if eb[0] == 0 else (eb[0] / eb[1] if eb[1] > 0 else float("inf"))
        WORST[k] = max(WORST.get(k, 0.0), r)
        gate(f"{c!r}{what}" + (" [hi+lo]" if lo else ""), eb)


def check_case(group, c):
    assert c.branch == R.branch(c.entry, c.N, c.D, c.Bt, c.heads)
    check_raw(group, c, run_case(c))


def cases(g):
    return pytest.mark.parametrize("c", R.GROUPS[g], ids=repr)


@cases("valu")
def test_attention_valu_fallback(c):
    """k_attention<D>: 4 lanes per query row, keys dealt 4 jj + sub; N < 4 leaves lanes without a key"""
    check_case("valu", c)


@cases("mfma")
def test_attention_mfma(c):
    """k_attention_mfma<D>: N / 32 waves, nkt = N / 32 of the 8 guarded key tiles"""
    check_case("mfma", c)


@cases("flash")
def test_attention_flash(c):
    """k_attention_flash<D>: 128-key tiles, running max with a rescale per tile"""
    check_case("flash", c)


@cases("h2")
def test_attention_h2(c):
    """tcx_attention_h2: the out_h2 stores of both kernels, decoded by the numpy codec"""
    check_case("h2", c)


@cases("split")
def test_attention_split(c):
    """k_attention_split<D, 0>: f16x3 products on h2 records"""
    check_case("split", c)


@cases("split_bf16")
def test_attention_split_bf16(c):
    """k_attention_split<D, 1, PF2>: bf16 records, deferred running max, ONES row at D = 16 / 48"""
    check_case("split_bf16", c)


@cases("split_b2")
def test_attention_split_b2(c):
    """k_attention_split<D, 2, PF2>: 2-byte bf16 qkv and output"""
    check_case("split_b2", c)


# ------------------------------------------------------------------------------------ the h2 range flag
@pytest.mark.parametrize("c", [c for c in R.GROUPS["h2"] if c.family == "onehot"], ids=repr)
def test_attention_h2_range_flag(c):
    """onehot: query i returns v[pi(i)], so ONE v value of 7e4 (above the f16 maximum 65504) reaches one output
    element of one row and raises the flag; without it the word stays 0; ovf = NULL is accepted"""
    big = R.inputs(c).copy()
    big[0, 5, 2 * c.C + 3] = 7e4
    for qkv, want in ((big, 1), (R.inputs(c), 0)):
        A = Arena()
        x = put_bytes(A, R.encode(qkv, "f32"))
        y = A.new(c.Bt * c.N * c.C * 4, torch.uint8)
        ovf = A.new(1, torch.int32, init=np.zeros(1))
        for _ in range(2):
            chk(call(c, x, y, ovf))
        A.check()
        assert int(ovf.item()) == want, f"{c}: ovf {int(ovf.item())}, expected {want}"
    A = Arena()
    x = put_bytes(A, R.encode(big, "f32"))
    y = A.new(c.Bt * c.N * c.C * 4, torch.uint8)
    chk(call(c, x, y, None))
    A.check()


# ------------------------------------------------------------------------------------ codecs against the GPU writers
def test_numpy_encoders_equal_the_gpu_writers():
    g = T.rng(5)
    v = (g.standard_normal((2, 64, 32)) * 10.0 ** g.uniform(-6, 4, (2, 64, 32))).astype(F32)
    A = Arena()
    x = put_bytes(A, v)
    one, zero = put_bytes(A, np.ones((2, 32), F32)), put_bytes(A, np.zeros((2, 32), F32))
    h2, bf, b2 = A.new(v.size * 4, torch.uint8), A.new(v.size * 4, torch.uint8), A.new(v.size * 2, torch.uint8)
    chk(L().tcx_f32_to_h2(P(x), P(h2), v.size, None, st()))
    chk(L().tcx_gn_apply_tab_bf16(P(x), P(bf), 2, 64, 32, P(one), P(zero), 0, st()))
    chk(L().tcx_gn_apply_tab_b2(P(x), P(b2), 2, 64, 32, P(one), P(zero), 0, 0, st()))
    A.check()
    assert bits(h2) == R.encode(v, "h2").tobytes()
    assert bits(bf) == R.encode(v, "bf16").tobytes()
    assert bits(b2) == R.encode(v, "b2").tobytes()


# ------------------------------------------------------------------------------------ refusals
class Bufs:
    """small valid buffers (Bt 1, N 256, C 32 in the widest format) between canaries"""

    def __init__(self):
        self.A = Arena()
        self.x = self.A.new(256 * 96 * 4, torch.uint8, init=np.zeros(256 * 96 * 4, np.uint8))
        self.y = self.A.new(256 * 32 * 4, torch.uint8)
        self.ovf = self.A.new(1, torch.int32, init=np.zeros(1))
        self.before = bits(self.y), bits(self.ovf)

    def untouched(self):
        torch.cuda.synchronize()
        assert (bits(self.y), bits(self.ovf)) == self.before, "a refused call wrote its output"
        self.A.check()


COMMON = [
    (dict(x=None), "bad args"), (dict(y=None), "bad args"), (dict(heads=0), "bad args"), (dict(heads=-2), "bad args"),
    (dict(heads=3), "bad args"), (dict(N=0), ""), (dict(N=-256), ""),
    (dict(C=80), "head dim 40"), (dict(C=24), "head dim 12"),                 # head dims 40 and 12
    (dict(N=512, C=16), "head dim 8"), (dict(N=512, C=48), "head dim 24"),    # 8 and 24: not on flash / split
    (dict(x=4), "16-B aligned"), (dict(y=4), "16-B aligned"),
    (dict(Bt=-1), "Bt must be in [0, 65535]"), (dict(Bt=65536), "Bt must be in [0, 65535]"),
    (dict(N=512, Bt=65536), "Bt must be in [0, 65535]"), (dict(Bt=1 << 30), "Bt must be in [0, 65535]"),
    (dict(C=8 * 65536, heads=65536), "heads must be in [1, 65535]"),
]
REFUSALS = (
    [("attention", kw, msg) for kw, msg in COMMON + [(dict(N=300), "N must be"), (dict(N=576), "N must be"),
                                                     (dict(N=100, Bt=65536), "Bt must be in [0, 65535]")]] +
    [("attention_h2", kw, msg) for kw, msg in COMMON + [(dict(N=100), "needs N"), (dict(N=288), "needs N"),
                                                        (dict(C=12, heads=1), "bad args")]] +
    [(e, kw, msg) for e in ("split", "split_bf16", "split_b2") for kw, msg in COMMON + [(dict(N=128), "needs N")]])


@pytest.mark.parametrize("entry,kw,msg", REFUSALS, ids=str)
def test_refusals(entry, kw, msg):
    """every host refusal: nonzero, tcx_last_error names the entry, output, flag word and canaries untouched.
    The Bt / heads bounds are refused before any launch (a grid of that extent is never asked for)."""
    b = Bufs()
    a = dict(x=0, y=0, Bt=1, N=256, C=32, heads=2)
    a.update(kw)
    x = None if a["x"] is None else P(b.x) + a["x"]
    y = None if a["y"] is None else P(b.y) + a["y"]
    fn = getattr(L(), ENTRY[entry])
    args = (x, y, a["Bt"], a["N"], a["C"], a["heads"]) + ((P(b.ovf),) if entry == "attention_h2" else ())
    assert fn(*args, st()) != 0, (entry, kw)
    name = "tcx_attention_split" if entry.startswith("split") else ENTRY[entry]
    assert last_error().startswith(name + ":") and msg in last_error(), last_error()
    b.untouched()


@pytest.mark.parametrize("entry", R.ENTRIES)
def test_empty_batch_returns_ok_and_writes_nothing(entry):
    b = Bufs()
    fn = getattr(L(), ENTRY[entry])
    args = (P(b.x), P(b.y), 0, 256, 32, 2) + ((P(b.ovf),) if entry == "attention_h2" else ())
    assert fn(*args, st()) == 0
    b.untouched()


# ------------------------------------------------------------------------------------ knob parity
CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests", sys.argv[1] + "/vae-diffusion-toy-crystals_amd"]
import attn_ref as R
import test_gpu_attn as G
np.savez(sys.argv[2], *[G.run_case(c) for c in R.KNOB_CASES[sys.argv[3]]])
"""


def _child(tmp_path, knob):
    """the knob's case list in a fresh process with the knob at 0 (the library reads its environment once)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / f"{knob}.npz")
    t = time.time()
    r = subprocess.run([sys.executable, "-c", CHILD, root, path, knob], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **{knob: "0"}))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(f"\n  {knob}=0 child: {time.time() - t:.1f} s")
    z = np.load(path)
    return [z[f"arr_{i}"] for i in range(len(R.KNOB_CASES[knob]))]


@pytest.mark.parametrize("knob", ["TCX_ATTN_XCD", "TCX_ATTN_PF2"])
def test_scheduling_knobs_are_bit_identical(tmp_path, knob):
    """XCD: the split forms at 9 and 17 workgroups; PF2: the bf16 forms at N = 512 / 768.  Pure scheduling:
    the outputs equal this process's (knobs at their defaults) bit for bit."""
    for k in ("TCX_ATTN_XCD", "TCX_ATTN_PF2", "TCX_ATTN_DEFER"):
        assert k not in os.environ, f"{k} is set: this process is not at the defaults"
    for c, raw in zip(R.KNOB_CASES[knob], _child(tmp_path, knob)):
        assert raw.tobytes() == run_case(c).tobytes(), f"{c}: {knob}=0 changes the output"


def test_exact_running_max_meets_the_same_gate(tmp_path):
    """TCX_ATTN_DEFER=0 (the exact running max) on rising, threshold and gauss(3): the same float64 gate as the
    deferred default; the difference between the two is printed"""
    for c, raw in zip(R.KNOB_CASES["TCX_ATTN_DEFER"], _child(tmp_path, "TCX_ATTN_DEFER")):
        check_raw("defer=0", c, raw, " DEFER=0")
        own = run_case(c)
        check_raw("defer=8", c, own, " default")
        d = np.abs(values(c, raw) - values(c, own)).max()
        print(f"  {c!r}: max |exact - deferred| {d:.3e}, {int((raw != own).sum())} of {raw.size} bytes differ")
