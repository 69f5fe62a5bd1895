"""GPU: the fp32 forward convolution through the C ABI at its dispatch edges: k_conv (csrc/conv.hip) behind
tcx_conv2d, tcx_conv_transpose2x / tcx_convT2x and tcx_linear, the epilogues of csrc/conv_common.hpp, the
one-channel forwards of csrc/thin.hip and the three weight packers, against the float64 references of
tests/conv_ref.py (gates, mutants and the restated dispatch are stated there and proved in
tests/test_conv_ref_cpu.py).

Every input, weight, table and output lives in an Arena between runs of 0x7b bytes and ends at the last
element the call may read or write: a load past a ragged tail multiplies 1.3e36 in and fails the gate, a
store outside the output trips the canary, an element never written still holds the pattern.  Every call
runs twice and the two outputs (and GroupNorm partials) must agree bit for bit.  Errors are measured against
the float64 reference only.  Each test prints error against bound (pytest -s); the module prints the worst
error / bound per group at the end.

Reached here and nowhere else in the suite
  most of the 24 fp32 k_conv<NT, MODE, CIRC, PRO>, all of which run here (conv_ref.GROUPS["a"]: cout_pad 32 /
  64 / 96 over Cout = 20; MODE 1 with Cin 3 / 6 and Cin 1 at stride 2; MODE 2 and the prologue at every NT;
  MODE 3 again with kpad > K, which drops to MODE 0); tiles that
  span several images with a ragged last tile, bias_b and residual (Ho*Wo = 1 and 35); the sub-pixel epilogue at
  M % 128 != 0; quad epilogue with an activation, column and general epilogues with GroupNorm partials, two
  128-pixel groups per image; bmod 1 / 2 / 3 with Bt % bmod != 0 at MODE 0 / 1 / 3 with residual and bias_b;
  x1 off by 4 bytes; MODE 2 on 1x1 .. 5x2 sources, with two sources, 1x1 and 4x4/s2 kernels; the prologue on
  source 2 only and at 384 channels; tcx_pack_conv_dgrad_weight and the data gradient it feeds; circular
  transposed conv in fp32, with Cin % 4 != 0 and non-square; tcx_linear on a column window of a wider weight;
  both sides of every condition of thin_conv_takes that the ABI can reach; every argument refusal.

Not reached
  M*Cout >= 2^29 (leaves the fast epilogue), operand extents past 2 GiB (clear bytes1 / bytes2 / bytesw and
  leave MODE 3) and B*Ho >= 2^31 (thin.hip declines): nothing of that size is allocated.  thin_conv_takes'
  aligned16(w): tcx_conv2d refuses a misaligned packed weight before the question is asked.  A residual in a
  sub-pixel phase: neither transposed-conv entry takes a residual.  tcx_conv2d's "empty output": with the new
  geometry refusals Ho, Wo >= 1 always.  The over-size k_thin_cin1 launch (more than 64 KB of dynamic LDS) is
  not provoked: thin_conv_takes now declines above 48 KB and both sides of that bound run.

Float32 fallback (4 x the float32 evaluation's error): used by no case; the sigmoid / SiLU, prologue and
upsample cases all hold the derived gates of conv_ref.py.

Measured on the MI355X (427 tests, 3.6 s in all, 1.4 s inside the module; slowest 0.39 s, the first call, which
loads the library; every other test below 0.1 s), worst error / bound per group:
  a instantiations 0.032 (rms 0.260)   b tile edges 0.039   c geometry 0.133 (rms 0.237)
  d sources 0.017 (rms 0.257)   e upsample 0.045   f prologue 0.0003 (rms 0.254; partials: own 0.010, ref 0.0002)
  g epilogues 0.014 (partials: own 0.039, ref 0.001)   h transposed 0.090   i dgrad 0.012   j linear 0.021
  k thin 0.267 (rms 0.246)
The RMS error of k_conv equals the plain-k-order float32 chain's (ratio 1/4 of the 4 x bound).  The prologue's
per-element bound carries |z| <= 20 and is loose (1e-3 against errors of 1e-6); its RMS gate is the one that
binds, so every prologue case takes it.  No kernel bug was found; the host changes that came with this module
are the three geometry / LDS refusals described in DESIGN.md.
"""
import time

import numpy as np
import pytest
import torch

import conv_ref as R
import train_ops_ref as T
from conv_ref import F32
from test_gpu_ops import L, chk, st
from test_gpu_train_ops import Arena, P, bits, cpu, gate, last_error

pytestmark = pytest.mark.gpu

WORST = {}
T0 = [None]


@pytest.fixture(scope="module", autouse=True)
def report():
    T0[0] = time.time()
    yield
    print(f"\n  test_gpu_conv: {time.time() - T0[0]:.1f} s; worst error / bound per group:")
    for k, v in WORST.items():
        print(f"    {k:28s} {v:.3f}")


def check(group, what, gates):
    for name, eb in gates:
        r = 0.0 if eb[0] == 0 else (eb[0] / eb[1] if eb[1] > 0 else float("inf"))
        WORST[f"{group} {name}"] = max(WORST.get(f"{group} {name}", 0.0), r)
        gate(f"{what} [{name}]", eb)


def put(A, a, shift=0):
    return None if a is None else A.new(a.size, init=a, shift=shift)


def run_case(c, inp):
    """the output (out_shape) and the GroupNorm partials of one call; canaries, determinism"""
    Hi, Wi, Ho, Wo, M = c.dims()
    A = Arena()
    x1, x2 = put(A, inp["x1"], c.shift_x), put(A, inp["x2"])
    bias, bias_b, resid = put(A, inp["bias"]), put(A, inp["bias_b"], c.shift_bb), put(A, inp["resid"], c.shift_r)
    tabs = [put(A, inp[k]) for k in ("sc1", "sh1", "sc2", "sh2")]
    if c.kind == "dgrad":   # through the GPU packer, over a NaN preset
        cof, cif, ci_lo, n_ci = c.fwd
        w = put(A, inp["w"])
        wpk = A.new(c.cout_pad * c.kpad, init=np.full(c.cout_pad * c.kpad, np.nan, F32))
        chk(L().tcx_pack_conv_dgrad_weight(P(w), P(wpk), cof, cif, c.ks, ci_lo, n_ci, c.cout_pad, c.kpad, st()))
        assert bits(wpk) == R.pack_dgrad(inp["w"], ci_lo, n_ci, c.cout_pad, c.kpad).tobytes(), f"{c}: dgrad pack"
    else:
        wpk = put(A, R.pack_case(c, inp))
    nsplit = R.cdiv(Ho * Wo, 128)
    n = int(np.prod(c.out_shape()))
    outs = []
    for _ in range(2):
        y = A.new(n, shift=c.shift_y)
        gn = A.new(c.Bt * nsplit * c.Cout * 2, torch.float64) if c.gn else None
        if c.kind == "convT" and c.entry == "convT2x":
            rc = L().tcx_convT2x(P(x1), c.Bt, c.H, c.W, c.Cin, P(wpk), P(bias), P(y), c.Cout, c.cout_pad, c.kpad, c.act, st())
        elif c.kind == "convT":
            rc = L().tcx_conv_transpose2x(P(x1), c.Bt, c.H, c.W, c.Cin, P(wpk), P(bias), P(y), c.Cout, c.cout_pad, c.kpad,
                                          c.act, c.circ, st())
        elif c.kind == "linear":
            rc = L().tcx_linear(P(x1), c.C1, P(x2), c.C2, P(wpk), P(bias), P(resid), P(y), c.Bt, c.Cout, c.cout_pad,
                                c.kpad, c.act, st())
        else:
            rc = L().tcx_conv2d(P(x1), P(x2), c.Bt, c.bmod, c.H, c.W, c.C1, c.C2, P(wpk), P(bias), P(bias_b), P(resid),
                                P(y), c.Cout, c.cout_pad, c.kpad, c.ks, c.stride, c.pad, c.circ, c.ups, c.act, P(gn),
                                *[P(t) for t in tabs], st())
        chk(rc)
        outs.append((y, gn))
    A.check()
    assert bits(outs[0][0]) == bits(outs[1][0]), f"{c} is not deterministic"
    if c.gn:
        assert bits(outs[0][1]) == bits(outs[1][1]), f"{c}: GroupNorm partials are not deterministic"
    y, gn = outs[0]
    return cpu(y, c.out_shape()), (cpu(gn, (c.Bt, nsplit, c.Cout, 2)) if c.gn else None)


def check_case(group, c):
    inp = c.inputs()
    got, part = run_case(c, inp)
    if got.size == 0:
        return
    ref = R.evaluate(c, inp)
    r32 = R.evaluate(c, inp, None, F32)["y"] if R.needs32(c) else None
    gs = R.gates(c, got, ref, r32)
    if c.gn:
        gs += R.gn_gates(c, part, got, ref, R.elem_bound(c, ref, r32))
    check(group, repr(c), gs)


def cases(g):
    return pytest.mark.parametrize("c", R.GROUPS[g], ids=repr)


@cases("a")
def test_conv_instantiations(c):
    """a. the 24 fp32 k_conv<NT, MODE, CIRC, PRO>, M = 70 (one ragged tile; the prologue: 3 tiles)"""
    check_case("a instantiations", c)


@cases("b")
def test_conv_tile_edges(c):
    """b. M 0 .. 257, Ho*Wo 1 / 35 / 128 / 256, Cout 1 .. 193, kpad = K and rup(K)"""
    check_case("b tile edges", c)


@cases("c")
def test_conv_geometry(c):
    """c. ks 1 .. 5, stride 1 .. 3, pad 0 .. ks - 1, both paddings, 7 x 5; one- and two-pixel images, pad == H"""
    check_case("c geometry", c)


@cases("d")
def test_conv_sources(c):
    """d. two sources, bmod with Bt % bmod != 0, x1 off by 4 bytes"""
    check_case("d sources", c)


@cases("e")
def test_conv_upsample(c):
    check_case("e upsample", c)


@cases("f")
def test_conv_prologue(c):
    check_case("f prologue", c)


@cases("g")
def test_conv_epilogues(c):
    """g. general / cols / quad / quad_act x GroupNorm partials x act 0..3"""
    check_case("g epilogues", c)


@cases("h")
def test_transposed_conv(c):
    check_case("h transposed", c)


@cases("i")
def test_conv_data_gradient(c):
    """i. tcx_pack_conv_dgrad_weight (bit-equal to the reference layout) feeding tcx_conv2d at pad' = ks - 1 - pad"""
    check_case("i dgrad", c)


@cases("j")
def test_linear(c):
    check_case("j linear", c)


@cases("k")
def test_thin_forwards(c):
    """k. thin.hip taken and declined (then k_conv) by one condition each"""
    check_case("k thin", c)


# ------------------------------------------------------------------------------------ packers
def _pack(fn, w, n, *args):
    A = Arena()
    wd = put(A, w)
    outs = []
    for _ in range(2):
        o = A.new(n, init=np.full(n, np.nan, F32))
        chk(fn(P(wd), P(o), *args, st()))
        outs.append(bits(o))
    A.check()
    assert outs[0] == outs[1]
    return outs[0]


@pytest.mark.parametrize("Cout,Cin,ks,cp,kp", [(5, 3, 3, 32, 32), (20, 12, 3, 32, 160), (33, 4, 1, 64, 32), (1, 7, 5, 32, 192),
                                               (97, 1, 2, 128, 32)])
def test_pack_conv_weight(Cout, Cin, ks, cp, kp):
    w = R.f32(T.rng(Cout).standard_normal((Cout, Cin, ks, ks)))
    assert _pack(L().tcx_pack_conv_weight, w, cp * kp, Cout, Cin, ks, cp, kp) == R.pack_conv(w, cp, kp).tobytes()


@pytest.mark.parametrize("Cin,Cout,cp,kp", [(3, 5, 32, 32), (32, 20, 32, 128), (36, 33, 64, 160), (4, 1, 32, 64)])
def test_pack_convT_weight(Cin, Cout, cp, kp):
    w = R.f32(T.rng(Cin).standard_normal((Cin, Cout, 4, 4)))
    assert _pack(L().tcx_pack_convT_weight, w, 4 * cp * kp, Cin, Cout, cp, kp) == R.pack_convT(w, cp, kp).tobytes()


@pytest.mark.parametrize("ks", [1, 3, 5])
@pytest.mark.parametrize("ci_lo,n_ci", [(0, 12), (5, 4), (5, 7), (0, 5)])
def test_pack_conv_dgrad_weight(ks, ci_lo, n_ci):
    """Cout 6, Cin 12: ci_lo in {0, 5, Cin - n_ci}; padding rows and columns zeroed over NaN"""
    w = R.f32(T.rng(ks).standard_normal((6, 12, ks, ks)))
    kp = R.rup(ks * ks * 6) + 32
    assert _pack(L().tcx_pack_conv_dgrad_weight, w, 32 * kp, 6, 12, ks, ci_lo, n_ci, 32, kp) == \
        R.pack_dgrad(w, ci_lo, n_ci, 32, kp).tobytes()


# ------------------------------------------------------------------------------------ refusals
class Bufs:
    def __init__(self):
        self.A = Arena()
        self.buf = self.A.new(1 << 16, init=np.zeros(1 << 16, F32))
        self.y = self.A.new(1 << 16)
        self.gn = self.A.new(4096, torch.float64)
        self.before = bits(self.y), bits(self.gn)

    def untouched(self):
        torch.cuda.synchronize()
        assert (bits(self.y), bits(self.gn)) == self.before, "a refused call wrote its output"
        self.A.check()


def conv2d_args(b, **kw):
    p = P(b.buf)
    a = dict(x1=p, x2=None, Bt=2, bmod=0, H=8, W=16, C1=32, C2=0, wpk=p, bias=None, bias_b=None, resid=None, y=P(b.y),
             Cout=20, cout_pad=32, kpad=None, ks=3, stride=1, pad=1, circ=1, ups=0, act=0, gn=None, sc1=None, sh1=None,
             sc2=None, sh2=None)
    a.update(kw)
    if a["kpad"] is None:
        a["kpad"] = R.rup(a["ks"] * a["ks"] * (a["C1"] + a["C2"]))
    return [a[k] for k in ("x1", "x2", "Bt", "bmod", "H", "W", "C1", "C2", "wpk", "bias", "bias_b", "resid", "y", "Cout",
                           "cout_pad", "kpad", "ks", "stride", "pad", "circ", "ups", "act", "gn", "sc1", "sh1", "sc2", "sh2")]


def _conv2d_refusals():
    X = "BUF"   # stands for the device buffer; BUF4: the same, 4 bytes on
    pro = dict(sc1=X, sh1=X)
    return [
        (dict(x1=None), "null pointer"), (dict(wpk=None), "null pointer"), (dict(y=None), "null pointer"),
        (dict(Bt=-1), "bad shape"), (dict(H=0), "bad shape"), (dict(W=0), "bad shape"), (dict(C1=0), "bad shape"),
        (dict(Cout=0), "bad shape"), (dict(C2=-4), "bad shape"),
        (dict(C2=4), "x2/C2 mismatch"), (dict(x2=X), "x2/C2 mismatch"),
        (dict(cout_pad=16), "cout_pad"), (dict(cout_pad=48), "cout_pad"),
        (dict(kpad=300), "kpad"), (dict(kpad=256), "kpad"),
        (dict(ks=0), "bad geometry"), (dict(stride=0), "bad geometry"), (dict(pad=-1), "bad geometry"),
        (dict(act=4), "bad act"), (dict(act=-1), "bad act"),
        (dict(ups=1, circ=0), "upsample needs"), (dict(ups=1, C1=6), "upsample needs"), (dict(ups=1, x1="BUF4"), "upsample needs"),
        (dict(C1=3, C2=4, x2=X), "single source"), (dict(C2=32, x2=X, x1="BUF4"), "single source"),
        (dict(H=5, W=7, gn=X), "GN stats"),
        (dict(sc1=X), "scale/shift pairs"), (dict(sc2=X, sh2=X, sh1=X), "scale/shift pairs"),
        (dict(C1=12, **pro), "GN prologue"), (dict(C1=16, C2=16, x2=X, **pro), "GN prologue"),
        (dict(circ=0, **pro), "GN prologue"), (dict(bmod=1, **pro), "GN prologue"), (dict(H=5, W=7, **pro), "GN prologue"),
        (dict(C1=416, **pro), "GN prologue"), (dict(sc2=X, sh2=X), "GN prologue"),
        (dict(C1=64, C2=32, x2=X, **pro), "GN prologue"), (dict(ks=5, pad=2, **pro), "GN prologue"),
        (dict(kpad=320, **pro), "GN prologue"), (dict(ups=1, H=8, W=8, **pro), "GN prologue"),
        (dict(wpk="BUF4"), "16-B aligned"),
    ] + [(dict(H=g[0], W=g[1], ks=g[2], stride=g[3], pad=g[4], circ=g[5], ups=g[6], C1=4), msg) for g, msg in R.BAD_GEOMETRY]


@pytest.mark.parametrize("kw,msg", _conv2d_refusals(), ids=str)
def test_conv2d_refusals(kw, msg):
    """l. every TCX_REQUIRE of tcx_conv2d, the two new geometry refusals included: refused on the host,
    tcx_last_error names it, output and canaries untouched"""
    b = Bufs()
    sub = {"BUF": P(b.buf), "BUF4": P(b.buf) + 4}
    kw = {k: sub.get(v, v) if isinstance(v, str) else v for k, v in kw.items()}
    if "gn" in kw:
        kw["gn"] = P(b.gn)
    assert L().tcx_conv2d(*conv2d_args(b, **kw), st()) != 0
    assert last_error().startswith("tcx_conv2d:") and msg in last_error(), last_error()
    b.untouched()


@pytest.mark.parametrize("H,ks,stride,pad,circ,msg", [(2, 3, 2, 0, 0, "larger than the padded input"),
                                                      (2, 3, 2, 0, 1, "larger than the padded input"),
                                                      (2, 4, 1, 3, 1, "wraps more than once")])
def test_conv2d_h2_geometry_refusals(H, ks, stride, pad, circ, msg):
    b = Bufs()
    p = P(b.buf)
    rc = L().tcx_conv2d_h2_pro(p, None, 1, 0, H, H, 32, 0, p, None, p, None, None, None, P(b.y), 0, 20, 32, ks * ks * 32, ks,
                               stride, pad, circ, 0, None, None, None, None, None, 0, None, st())
    assert rc != 0
    assert last_error().startswith("tcx_conv2d_h2:") and msg in last_error(), last_error()
    b.untouched()


def test_other_entry_refusals():
    """l. tcx_conv_transpose2x / tcx_convT2x, tcx_linear and the three packers"""
    b = Bufs()
    p, y = P(b.buf), P(b.y)
    lib = L()

    def ct(x=p, Bt=2, H=5, W=5, Cin=4, w=p, yy=y, Cout=20, cp=32, kp=32, act=0):
        return lib.tcx_conv_transpose2x(x, Bt, H, W, Cin, w, None, yy, Cout, cp, kp, act, 0, st())

    for kw, msg in ((dict(x=None), "null"), (dict(w=None), "null"), (dict(yy=None), "null"), (dict(cp=16), "bad padding"),
                    (dict(cp=48), "bad padding"), (dict(kp=16), "bad padding"), (dict(Cin=12), "bad padding"),
                    (dict(Bt=-1), "bad shape"), (dict(H=0), "bad shape"), (dict(W=0), "bad shape"), (dict(Cout=0), "bad shape"),
                    (dict(act=4), "bad act"), (dict(act=-1), "bad act")):
        assert ct(**kw) != 0, kw
        assert last_error().startswith("tcx_convT2x:") and msg in last_error(), (kw, last_error())
    assert lib.tcx_convT2x(p, 2, 5, 5, 4, p, None, y, 20, 32, 32, 7, st()) != 0 and "bad act" in last_error()

    def lin(x1=p, K1=8, x2=None, K2=0, w=p, yy=y, M=4, N=20, npad=32, kpad=32, act=0):
        return lib.tcx_linear(x1, K1, x2, K2, w, None, None, yy, M, N, npad, kpad, act, st())

    for kw, msg in ((dict(x1=None), "bad args"), (dict(w=None), "bad args"), (dict(yy=None), "bad args"), (dict(M=-1), "bad args"),
                    (dict(N=0), "bad args"), (dict(K1=0), "bad args"), (dict(K2=-4), "bad args"), (dict(K2=4), "x2/K2"),
                    (dict(x2=p), "x2/K2"), (dict(npad=16), "bad padding"), (dict(npad=48), "bad padding"),
                    (dict(kpad=48), "bad padding"), (dict(K1=40), "bad padding"), (dict(act=4), "bad act"),
                    (dict(K1=6, x2=p, K2=4), "two-source"), (dict(x1=p + 4, x2=p, K2=4), "two-source")):
        assert lin(**kw) != 0, kw
        assert last_error().startswith("tcx_linear:") and msg in last_error(), (kw, last_error())

    for call, name in (
            (lambda: lib.tcx_pack_conv_weight(None, y, 5, 3, 3, 32, 32, st()), "tcx_pack_conv_weight"),
            (lambda: lib.tcx_pack_conv_weight(p, None, 5, 3, 3, 32, 32, st()), "tcx_pack_conv_weight"),
            (lambda: lib.tcx_pack_conv_weight(p, y, 33, 3, 3, 32, 32, st()), "tcx_pack_conv_weight"),
            (lambda: lib.tcx_pack_conv_weight(p, y, 5, 4, 3, 32, 32, st()), "tcx_pack_conv_weight"),
            (lambda: lib.tcx_pack_convT_weight(None, y, 3, 5, 32, 32, st()), "tcx_pack_convT_weight"),
            (lambda: lib.tcx_pack_convT_weight(p, None, 3, 5, 32, 32, st()), "tcx_pack_convT_weight"),
            (lambda: lib.tcx_pack_convT_weight(p, y, 3, 33, 32, 32, st()), "tcx_pack_convT_weight"),
            (lambda: lib.tcx_pack_convT_weight(p, y, 9, 5, 32, 32, st()), "tcx_pack_convT_weight"),
            (lambda: lib.tcx_pack_conv_dgrad_weight(None, y, 6, 12, 3, 0, 4, 32, 64, st()), "tcx_pack_conv_dgrad_weight"),
            (lambda: lib.tcx_pack_conv_dgrad_weight(p, None, 6, 12, 3, 0, 4, 32, 64, st()), "tcx_pack_conv_dgrad_weight"),
            (lambda: lib.tcx_pack_conv_dgrad_weight(p, y, 6, 12, 3, -1, 4, 32, 64, st()), "tcx_pack_conv_dgrad_weight"),
            (lambda: lib.tcx_pack_conv_dgrad_weight(p, y, 6, 12, 3, 0, 0, 32, 64, st()), "tcx_pack_conv_dgrad_weight"),
            (lambda: lib.tcx_pack_conv_dgrad_weight(p, y, 6, 12, 3, 9, 4, 32, 64, st()), "tcx_pack_conv_dgrad_weight"),
            (lambda: lib.tcx_pack_conv_dgrad_weight(p, y, 6, 40, 3, 0, 33, 32, 64, st()), "tcx_pack_conv_dgrad_weight"),
            (lambda: lib.tcx_pack_conv_dgrad_weight(p, y, 6, 12, 3, 0, 4, 32, 32, st()), "tcx_pack_conv_dgrad_weight")):
        assert call() != 0, name
        assert last_error().startswith(name + ":"), last_error()
    b.untouched()
