"""GPU: the fp32 GEMM and conv weight-gradient kernels of csrc/gemm.hip (k_gemm, k_gemm_reduce, k_wgrad,
k_wgrad_reduce) through the C ABI at their dispatch edges, against the float64 references of
tests/gemm_ref.py (gates, mutants and the plan arithmetic are stated there and proved in
tests/test_gemm_ref_cpu.py).

Every input, output and workspace lives in an Arena between runs of 0x7b bytes, and every operand
buffer ends at the last element the call may read: a vector load past a ragged tail multiplies 1.3e36
in and fails the gate, a store outside the output trips the canary or the "elements the call does not
own" comparison.  Every call runs twice and must agree bit for bit.  Each test prints error against
bound (pytest -s); the module prints the worst error / bound per group at the end.

Reached here and nowhere else in the suite
  tcx_gemm (the entry without scratch) at all; k_gemm load modes (1,0), (0,2), (2,0), (1,2), (2,1) at
  every NT; the scalar fallback for each reason but one (neither stride 1, contiguous extent % 4, base
  pointer off by 4 bytes, a batch stride % 4); K = 0 with NULL operands; beta = 0 over NaN; bdiv 3 and 6;
  zero batch strides; transposed and strided C; head dim 3 in the attention layouts; ragged split-K plans
  (a 4-wide last chunk, a short last split, nsplit below the first estimate, 16 splits over three
  n-blocks), split-K in modes (1,1), (2,2), (0,1) and with bdiv = 2; both scratch fallbacks; argument
  errors; the GEMM-split branch of tcx_linear_ws with two sources, residual and every activation;
  k_wgrad with beta != 0, over NaN, with no pixels, with a misaligned x1 / dy / workspace, at 5x5 pad 2,
  on a one-pixel image; uneven pixel splits (9 + 8, 9 + 9 + 9 + 9 + 5); the shapes thin.hip declines.

k_gemm<NT, LA, LB>: test_gemm_load_modes[modes N=28|60|100 la=LA lb=LB] is <1|2|3, LA, LB>, 27 in all.
k_wgrad<NT, ASC, BSC>, test_wgrad_instantiations at (1, 9, 7, C1, C2, Cout, 3, 1, 1, 1):
  <1,0,0> (12,4) Cout 20   <1,0,1> (12,4) Cout 21   <1,1,0> (6,0) Cout 20   <1,1,1> (6,0) Cout 21
  <2,0,0> (12,4) Cout 36   <2,0,1> (12,4) Cout 37   <2,1,0> (6,0) Cout 36   <2,1,1> (6,0) Cout 37
  <3,0,0> (12,4) Cout 100  <3,0,1> (12,4) Cout 101  <3,1,0> (6,0) Cout 100  <3,1,1> (6,0) Cout 101
  and for the alignment reason: <1,1,0> x1 + 4 B, <2,0,1> dy + 4 B, <3,1,1> both.
tests/test_gemm_ref_cpu.py asserts these tables from the restated predicates; the workspace-size
assertions here fail if a plan changes.

Not reached (nothing of that size is allocated)
  k_wgrad_h2_r2: needs an h2 operand past 2 GiB (k_wgrad_h2 forms 32-bit buffer offsets below that).
  grid.y = batch * nsplit of k_gemm: a batch past 65535 (unsplit) is a refused launch, reported through
  check_launch, not a wrong result.  k_gemm and the reduces index with 64-bit strides and size_t; the
  host forms M = Bt * Ho * Wo and the pixel index m = chunk * 32 + px in int, past 2^31 pixels only.
  k_thin_wgrad's look-ahead on a one-pixel-wide circular input read one float past the thin operand
  (wrap_idx(2, 1) = 1, value unused): tcx_conv_wgrad now keeps that shape on k_wgrad, tested here as
  the "W=1 circular" boundary case; the thin kernel itself is not run at W = 1.

Measured on the MI355X (157 tests, 3.4 s in all, slowest 0.37 s), worst error / bound per group:
  a load modes 0.024   b scalar fallback 0.009   c size edges 0.273   d batch layouts 0.050
  e split-K 0.003 (unsplit rerun, ws NULL, ws short 0.002)   non-splitting 0.003   g linear_ws 0.002
  h wgrad instantiations 0.005, geometry 0.070, splits 0.001, beta 0.003   i thin boundary 0.016
RMS gate (GPU RMS error, float32-chain RMS error on the CPU; bound = 4 x the latter):
  gemm (132,100,544)x3   split 2.6e-6  unsplit 4.9e-6   chain 4.9e-6
  gemm (36,28,1056)x2    split 3.9e-6  unsplit 9.3e-6   chain 9.4e-6
  gemm (8,200,2048)      split 5.0e-6  unsplit 1.8e-5   chain 1.8e-5
  linear_ws (65,40,260,132), act 0..3: 1.9e-7 / 1.3e-7 / 4.0e-8 / 1.4e-7, chain 3.7e-7 / 2.7e-7 / 6.6e-8 / 2.7e-7
  wgrad 512 / 544 / 1312 pixels: 6.2e-7 / 7.1e-7 / 1.1e-6, chain 9.0e-7 / 9.7e-7 / 2.3e-6
The unsplit GEMM's RMS error equals the plain-k-order chain's: the MFMA sums in k order.  No linear_ws
case needs the ref32 fallback: the float32 evaluation meets the stated gate for sigmoid and SiLU
(tests/test_gemm_ref_cpu.py::test_linear_gate asserts it).
"""
import time

import numpy as np
import pytest
import torch

import gemm_ref as R
from gemm_ref import F32
from test_gpu_ops import L, chk, st
from test_gpu_train_ops import Arena, P, bits, cpu, gate, last_error

pytestmark = pytest.mark.gpu

WORST = {}
T0 = [None]


@pytest.fixture(scope="module", autouse=True)
def report():
    T0[0] = time.time()
    yield
    print(f"\n  test_gpu_gemm: {time.time() - T0[0]:.1f} s; worst error / bound per group:")
    for k, v in WORST.items():
        print(f"    {k:28s} {v:.3f}")


def check(group, what, gates):
    for name, eb in gates:
        r = 0.0 if eb[0] == 0 else (eb[0] / eb[1] if eb[1] > 0 else float("inf"))
        WORST[f"{group} {name}"] = max(WORST.get(f"{group} {name}", 0.0), r)
        gate(f"{what} [{name}]", eb)


def put(A, a, shift=0):
    return A.new(a.size, init=a, shift=shift)


# ------------------------------------------------------------------------------------ tcx_gemm / tcx_gemm_ws
def run_gemm(c, inp, how="plain", null_ab=False, c_init=None):
    """how: plain (tcx_gemm) | ws (tcx_gemm_ws, the queried scratch) | ws_null | ws_short.  Returns the
    whole C buffer after the call; checks canaries, determinism and the elements the call does not own."""
    A = Arena()
    a = None if null_ab else put(A, inp["A"], c.shift_a)
    b = None if null_ab else put(A, inp["B"], c.shift_b)
    bias = put(A, inp["bias"]) if c.bias else None
    c0 = inp["C"] if c_init is None else c_init
    nws = int(L().tcx_gemm_workspace(c.M, c.N, c.K, c.batch))
    assert nws == R.gemm_workspace(c.M, c.N, c.K, c.batch), "the split plan changed: the tables no longer hold"
    pa = None if a is None else P(a) + 4 * c.A[4]
    pb = None if b is None else P(b) + 4 * c.B[4]
    outs = []
    for _ in range(2):
        cd = A.new(c0.size, init=c0)
        args = (c.M, c.N, c.K, c.alpha, pa, c.A[0], c.A[1], pb, c.B[0], c.B[1], c.beta, P(cd) + 4 * c.C[4], c.C[0],
                c.C[1], P(bias), c.batch, c.bdiv, c.A[2], c.A[3], c.B[2], c.B[3], c.C[2], c.C[3])
        if how == "plain":
            chk(L().tcx_gemm(*args, st()))
        else:
            nb = {"ws": nws, "ws_null": 0, "ws_short": nws - 4}[how]
            ws = A.new(nb, torch.uint8) if how != "ws_null" else None
            chk(L().tcx_gemm_ws(*args, P(ws), nb, st()))
            if how == "ws_short":
                assert bool((ws == 0x7B).all()), "a too-small workspace was written"
        outs.append(cd)
    A.check()
    assert bits(outs[0]) == bits(outs[1]), f"{c} [{how}] is not deterministic"
    out = cpu(outs[0])
    own = np.zeros(out.size, bool)
    own[c.idx("C").reshape(-1)] = True
    assert out[~own].tobytes() == np.asarray(c0, F32)[~own].tobytes(), f"{c}: wrote an element it does not own"
    return out


def check_gemm(group, c, how="plain", **kw):
    inp = c.inputs()
    ref, S = R.ref_gemm(c, inp)
    out = run_gemm(c, inp, how, **kw)
    ns = c.nsplit if how == "ws" and c.nsplit > 1 else 0
    ref32 = R.f32_gemm(c, inp) if c.K > R.LONG else None
    check(group, f"{c} [{how}]", R.gemm_gates(c, out[c.idx("C")], ref, S, ns, ref32))


@pytest.mark.parametrize("c", R.GEMM_MODES, ids=repr)
def test_gemm_load_modes(c):
    """a. all 27 k_gemm<NT, LA, LB>: M = 132 (128 + 4), K = 68 (32 + 32 + 4), N = 28 / 60 / 100 (96 + 4)"""
    check_gemm("a modes", c)


@pytest.mark.parametrize("c", R.GEMM_SCALAR, ids=repr)
def test_gemm_scalar_fallback_reasons(c):
    """b. each term of gemm_impl's predicate alone sends A (then B) to the scalar loads"""
    check_gemm("b scalar", c)


@pytest.mark.parametrize("c", R.GEMM_EDGES, ids=repr)
def test_gemm_size_edges(c):
    """c. one dimension at a time around (36, 40, 36); K = 0 with A = B = NULL; beta = 0 over NaN"""
    kw = {}
    if c.K == 0:
        kw["null_ab"] = True
    if "NaN" in c.name:
        kw["c_init"] = np.full(c.size("C"), np.nan, F32)
    check_gemm("c edges", c, **kw)


@pytest.mark.parametrize("c", R.GEMM_BATCH, ids=repr)
def test_gemm_batch_layouts(c):
    """d. bdiv 1 / 3 / 6 with distinct hi / lo strides, broadcast B, transposed C, the attention products
    as column slices of qkv / dqkv (the other columns keep their bits)"""
    check_gemm("d batch", c, "ws")


@pytest.mark.parametrize("c", R.GEMM_SPLIT, ids=repr)
def test_gemm_split_k(c):
    """e. ragged split plans through tcx_gemm_ws, the same inputs unsplit through tcx_gemm, and the two
    fallbacks (no scratch, scratch one float short) which must leave the scratch alone"""
    check_gemm("e split", c, "ws")
    check_gemm("e split (unsplit run)", c, "plain")
    check_gemm("e split (ws NULL)", c, "ws_null")
    check_gemm("e split (ws short)", c, "ws_short")


@pytest.mark.parametrize("c", R.GEMM_NOSPLIT, ids=repr)
def test_gemm_shapes_that_do_not_split(c):
    assert L().tcx_gemm_workspace(c.M, c.N, c.K, c.batch) == 0
    check_gemm("e nosplit", c, "ws")


def test_gemm_argument_errors():
    """f. refused on the host, C untouched; empty problems are TCX_OK and touch nothing"""
    A = Arena()
    buf = A.new(64 * 64, init=np.ones(64 * 64, F32))
    cd = A.new(64 * 64)
    before = bits(cd)
    p, pc = P(buf), P(cd)

    def call(M=8, N=8, K=8, a=p, b=p, c=pc, batch=1, bdiv=1):
        return L().tcx_gemm(M, N, K, 1.0, a, K, 1, b, 1, K, 0.0, c, N, 1, None, batch, bdiv, 0, 0, 0, 0, 0, 0, st())

    for kw in (dict(M=-1), dict(bdiv=0), dict(c=None), dict(a=None), dict(b=None)):
        assert call(**kw) != 0, kw
        assert "tcx_gemm" in last_error(), last_error()
    for kw in (dict(M=0), dict(N=0), dict(batch=0)):
        assert call(**kw) == 0, kw
    torch.cuda.synchronize()
    assert bits(cd) == before
    A.check()


# ------------------------------------------------------------------------------------ tcx_linear_ws
@pytest.mark.parametrize("shape,act,rb", R.LINEAR_CASES, ids=str)
def test_linear_ws_gemm_split(shape, act, rb):
    """g. M = 65 > 64: the skinny path declines, each source is a split-K k_gemm<3, 0, 0> into raw partials
    and k_gemm_reduce applies bias, residual and activation"""
    M, N, K1, K2 = shape
    inp = R.linear_inputs(*shape)
    s1, _, s2, _ = R.linear_plan(*shape)
    nws = int(L().tcx_linear_workspace(M, N, K1, K2))
    assert nws == (s1 + s2) * M * N * 4, "the linear plan changed"
    npad, kpad = 64, (K1 + K2 + 31) // 32 * 32
    wpk = np.full((npad, kpad), np.nan, F32)   # the padding is never read on this path
    wpk[:N, :K1 + K2] = inp["w"]
    A = Arena()
    x1 = A.new(M * K1, init=inp["x1"])
    x2 = A.new(M * K2, init=inp["x2"]) if K2 else None
    wd = A.new(wpk.size, init=wpk)
    b = A.new(N, init=inp["b"]) if rb else None
    resid = A.new(M * N, init=inp["resid"]) if rb else None
    outs = []
    for _ in range(2):
        ws, y = A.new(nws, torch.uint8), A.new(M * N)
        chk(L().tcx_linear_ws(P(x1), K1, P(x2), K2, P(wd), P(b), P(resid), P(y), M, N, npad, kpad, act, P(ws), nws,
                              st()))
        outs.append(y)
    A.check()
    assert bits(outs[0]) == bits(outs[1]), "tcx_linear_ws is not deterministic"
    ref, S = R.ref_linear(inp, act, rb)
    r32 = R.f32_linear(inp, act, rb) if act >= 2 else None
    got = cpu(outs[0], (M, N))
    gates = [("elem", R.gate_linear(got, ref, S, K1 + K2, s1 + s2, r32))]
    if K1 + K2 > R.LONG:
        gates.append(("rms", R.gate_rms(got, ref, R.f32_linear(inp, act, rb))))
    check("g linear", f"linear_ws {shape} act {act} resid/bias {rb}", gates)


# ------------------------------------------------------------------------------------ tcx_conv_wgrad
def run_wgrad(c, inp, ws_shift=0):
    B, H, W, C1, C2, Cout, ks, s, p, circ = c.shape
    Ho, Wo, M, K = c.dims()
    A = Arena()
    x1 = put(A, inp["x1"], c.shift_x)
    x2 = put(A, inp["x2"]) if C2 else None
    dy = put(A, inp["dy"], c.shift_dy)
    nws = int(L().tcx_conv_wgrad_workspace(B, Ho, Wo, C1 + C2, Cout, ks))
    assert nws == R.wgrad_workspace(B, Ho, Wo, C1 + C2, Cout, ks), "the wgrad plan changed: the tables no longer hold"
    d0 = np.full(inp["dw0"].shape, np.nan, F32) if c.nan_dw else inp["dw0"]
    outs = []
    for _ in range(2):
        ws, dw = A.new(nws, torch.uint8, shift=ws_shift), A.new(d0.size, init=d0)
        chk(L().tcx_conv_wgrad(P(x1), P(x2), B, H, W, C1, C2, P(dy), Cout, ks, s, p, circ, c.beta, P(dw), P(ws), nws,
                               st()))
        outs.append(dw)
    A.check()
    assert bits(outs[0]) == bits(outs[1]), f"tcx_conv_wgrad {c} is not deterministic"
    return cpu(outs[0], inp["dw0"].shape)


def check_wgrad(group, c, **kw):
    inp = c.inputs()
    ref, S = R.ref_wgrad(c, inp)
    got = run_wgrad(c, inp, **kw)
    check(group, f"wgrad {c}", R.wgrad_gates(c, got, ref, S, R.f32_wgrad(c, inp) if c.dims()[2] > R.LONG else None))


@pytest.mark.parametrize("c", R.WGRAD_INST, ids=repr)
def test_wgrad_instantiations(c):
    """h. all 12 k_wgrad<NT, ASC, BSC> at M = 63 pixels (a ragged chunk); K = 144 is a ragged second k-block;
    the scalar forms also for the alignment reason"""
    check_wgrad("h wgrad inst", c)


@pytest.mark.parametrize("c", R.WGRAD_GEOM, ids=repr)
def test_wgrad_geometry(c):
    check_wgrad("h wgrad geometry", c)


@pytest.mark.parametrize("c", R.WGRAD_SPLIT, ids=repr)
def test_wgrad_splits(c):
    """16 chunks as 8 + 8, 17 as 9 + 8, 41 as 9 + 9 + 9 + 9 + 5"""
    check_wgrad("h wgrad split", c)


@pytest.mark.parametrize("c", R.WGRAD_BETA, ids=repr)
def test_wgrad_beta(c):
    check_wgrad("h wgrad beta", c)


@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_wgrad_no_pixels(beta):
    """Bt = 0: dw = beta * dW0"""
    c = R.Wc((0, 5, 6, 8, 0, 20, 3, 1, 1, 1), beta=beta)
    inp = c.inputs()
    got = run_wgrad(c, inp)
    assert (got == F32(beta) * inp["dw0"]).all()


def test_wgrad_workspace_edges():
    """ws shifted by 4 bytes with the queried size (which includes the 256 bytes of the internal align-up);
    one byte below nsplit * K * Cout * 4: refused, dw untouched"""
    c = R.WGRAD_SPLIT[1]
    check_wgrad("h wgrad ws+4B", c, ws_shift=4)
    B, H, W, C1, C2, Cout, ks, s, p, circ = c.shape
    Ho, Wo, M, K = c.dims()
    inp = c.inputs()
    A = Arena()
    x1, dy, dw = A.new(inp["x1"].size, init=inp["x1"]), A.new(inp["dy"].size, init=inp["dy"]), A.new(inp["dw0"].size)
    nb = len(c.splits) * K * Cout * 4 - 1
    ws = A.new(nb, torch.uint8)
    before = bits(dw)
    rc = L().tcx_conv_wgrad(P(x1), None, B, H, W, C1, 0, P(dy), Cout, ks, s, p, circ, 0.0, P(dw), P(ws), nb, st())
    assert rc != 0
    assert "workspace" in last_error()
    torch.cuda.synchronize()
    assert bits(dw) == before and bool((ws == 0x7B).all())
    A.check()


@pytest.mark.parametrize("c", R.WGRAD_THIN_EDGE, ids=repr)
def test_wgrad_thin_path_boundary(c):
    """i. shapes thin_wgrad_plan (thin.hip) declines by one condition each run k_wgrad; the last shape runs
    both ways (x1 off by 4 bytes: k_wgrad; aligned: k_thin_wgrad)"""
    check_wgrad("i thin boundary", c)


@pytest.mark.parametrize("entry", ["tcx_conv_wgrad", "tcx_conv_wgrad_h2"])
@pytest.mark.parametrize("H,ks,pad,stride,circ", R.WGRAD_BAD_GEOMETRY)
def test_wgrad_refuses_invalid_geometry(entry, H, ks, pad, stride, circ):
    """j. a kernel larger than the padded input (C division made Ho = 1 of it), a circular pad that wraps
    more than once, an empty input: refused on the host before any launch, as torch refuses them"""
    A = Arena()
    buf = A.new(4096, init=np.zeros(4096, F32))
    dw = A.new(8 * 8 * ks * ks)
    before = bits(dw)
    p = P(buf)
    if entry == "tcx_conv_wgrad":
        rc = L().tcx_conv_wgrad(p, None, 1, H, H, 8, 0, p, 8, ks, stride, pad, circ, 0.0, P(dw), p, 4096 * 4, st())
    else:
        rc = L().tcx_conv_wgrad_h2(p, None, 1, H, H, 8, 0, p, 8, ks, stride, pad, circ, 0.0, p, P(dw), p, 4096 * 4,
                                   st())
    assert rc != 0
    msg = last_error()
    assert msg.startswith(entry + ":"), msg
    assert any(w in msg for w in ("empty input", "larger than the padded input", "wraps more than once")), msg
    torch.cuda.synchronize()
    assert bits(dw) == before
    A.check()
