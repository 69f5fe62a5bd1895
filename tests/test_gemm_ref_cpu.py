"""CPU: the gates of tests/test_gpu_gemm.py can fail, a correct fp32 evaluation meets them, and the
case tables reach the branches of csrc/gemm.hip they claim.

For every case of tests/gemm_ref.py: (a) the reference evaluated as a float32 fma chain passes the
per-element gate against the float64 reference; (b) every applicable mutant fails a gate (the
10-bit operand truncation must fail the per-element gate up to K = 300 and the RMS gate beyond);
(c) the plan arithmetic restated from gemm.hip gives the load modes, kernel instantiations and split
shapes the tables state.  Needs no libtcx and no GPU."""
import numpy as np
import pytest

import gemm_ref as R
from gemm_ref import ok


def passes(gates, what=""):
    for name, eb in gates:
        assert ok(eb), f"{what} {name}: err {eb[0]:.3e} > bound {eb[1]:.3e}"


# ------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("c", R.GEMM_ALL, ids=repr)
def test_gemm_gate(c):
    inp = c.inputs()
    ref, S = R.ref_gemm(c, inp)
    r32 = R.f32_gemm(c, inp)
    # (a) the chain is unsplit; a split evaluation has shorter chains and the larger bound
    passes([("elem", R.gate_sum(r32, ref, S, c.K))], repr(c))
    if c.K > R.LONG:
        e, b = R.gate_rms(r32, ref, r32)
        print(f"  {c}: float32 chain RMS {e:.3e}, RMS bound {b:.3e}")
    # (b)
    for mut in R.GEMM_MUTANTS:
        if not R.gemm_applies(c, mut):
            continue
        got, _ = R.ref_gemm(c, inp, mut)
        gates = R.gemm_gates(c, got, ref, S, c.nsplit if c.nsplit > 1 else 0, r32)
        if mut == "trunc10":
            which = dict(gates)["elem" if c.K <= R.LONG else "rms"]
            assert not ok(which), f"{c}: truncated operands pass: err {which[0]:.3e} <= bound {which[1]:.3e}"
        else:
            assert not R.all_ok(gates), f"{c}: mutant {mut} passes: {gates}"


def test_gemm_exact_where_the_sum_is_empty():
    c = next(c for c in R.GEMM_EDGES if c.name == "edge K=0 no bias beta=0")
    ref, S = R.ref_gemm(c, c.inputs())
    assert (S == 0).all() and (ref == 0).all()
    assert not ok(R.gate_sum(ref + 1e-30, ref, S, 0)) and not ok(R.gate_sum(ref * np.nan, ref, S, 0))


def test_every_mutant_is_exercised():
    for mut in R.GEMM_MUTANTS:
        assert sum(R.gemm_applies(c, mut) for c in R.GEMM_ALL) >= 3, mut
    for mut in R.WGRAD_MUTANTS:
        assert sum(R.wgrad_applies(c, mut) for c in R.WGRAD_ALL) >= 2, mut


def test_gemm_tables_reach_what_they_claim():
    seen = set()
    for c in R.GEMM_ALL:
        if c.modes is not None:
            assert c.expect_modes() == c.modes, (c, c.expect_modes())
        ns, kcs = R.gemm_split_plan(c.M, c.N, c.K, c.batch)
        assert ns == c.nsplit, (c, ns)
        if ns > 1:
            assert R.split_chunks(c.K, ns, kcs) == c.chunks, c
            assert R.gemm_workspace(c.M, c.N, c.K, c.batch) == ns * c.batch * c.M * c.N * 4
        else:
            assert R.gemm_workspace(c.M, c.N, c.K, c.batch) == 0
        seen.add((R.gemm_nt(c.N),) + c.expect_modes())
    assert len(seen) == 27, "not all 27 k_gemm<NT, LA, LB>"
    assert {R.gemm_nt(c.N) for c in R.GEMM_MODES} == {1, 2, 3}
    # the split table: a 4-wide last chunk, a first estimate of 8 splits ending at 7, three n-blocks
    s = {c.name: c for c in R.GEMM_SPLIT}
    assert s["split (36,40,260) transposed"].K % 32 == 4
    c = s["split (36,28,1056)x2 bdiv=2"]
    assert min(min(R.cdiv(512, 2), 16), 33 // 4) == 8 and c.nsplit == 7
    assert R.cdiv(200, 96) == 3
    assert {c.expect_modes() for c in R.GEMM_SPLIT} >= {(1, 1), (2, 2)}
    assert any(c.C[1] != 1 and c.beta != 0 and c.bias for c in R.GEMM_SPLIT)
    # every scalar case is scalar for exactly the stated operand
    assert [c.expect_modes() for c in R.GEMM_SCALAR] == [(2, 1)] * 7 + [(1, 2)] * 7
    # the attention layouts: d = 3 is scalar everywhere k- or d-contiguous, d = 8 is vector
    assert all(2 in c.expect_modes() for c in R.GEMM_BATCH if c.name.startswith("attn d=3"))
    assert all(2 not in c.expect_modes() for c in R.GEMM_BATCH if c.name.startswith("attn d=8"))


# ------------------------------------------------------------------------------------ tcx_linear_ws
def test_linear_plan():
    for M, N, K1, K2 in R.LINEAR_SHAPES:
        assert M > 64 and R.linear_wants_split(M, N, K1, K2)
    assert R.linear_plan(65, 40, 260, 132) == (3, 3, 2, 3)   # 9 chunks as 3 + 3 + 3, 5 as 3 + 2, each last chunk 4 wide
    assert R.linear_plan(65, 40, 260, 0) == (3, 3, 0, 0)


@pytest.mark.parametrize("shape,act,rb", R.LINEAR_CASES, ids=str)
def test_linear_gate(shape, act, rb):
    M, N, K1, K2 = shape
    inp = R.linear_inputs(*shape)
    ref, S = R.ref_linear(inp, act, rb)
    s1, _, s2, _ = R.linear_plan(*shape)
    r32 = R.f32_linear(inp, act, rb)
    eb = R.gate_linear(r32, ref, S, K1 + K2, 0)
    assert ok(eb), f"float32 evaluation misses the stated gate: {eb} (the GPU test then needs ref32)"
    muts = ["drop_last_k", "trunc10"] + (["no_bias", "no_resid"] if rb else []) + (["no_act"] if act else []) \
        + (["x2_from_x1"] if K2 else [])
    for mut in muts:
        got, _ = R.ref_linear(inp, act, rb, mut)
        eb = R.gate_linear(got, ref, S, K1 + K2, s1 + s2, r32)
        if mut == "trunc10":   # K1 + K2 = 392 > 300: the aggregate gate
            eb = R.gate_rms(got, ref, r32)
        assert not ok(eb), f"{shape} act {act}: mutant {mut} passes: {eb}"


# ------------------------------------------------------------------------------------ conv weight gradient
@pytest.mark.parametrize("c", R.WGRAD_ALL, ids=repr)
def test_wgrad_gate(c):
    inp = c.inputs()
    ref, S = R.ref_wgrad(c, inp)
    r32 = R.f32_wgrad(c, inp)
    M = c.dims()[2]
    passes([("elem", R.gate_sum(r32, ref, S, M))], repr(c))
    if M > R.LONG:
        e, b = R.gate_rms(r32, ref, r32)
        print(f"  {c}: float32 chain RMS {e:.3e}, RMS bound {b:.3e}")
    for mut in R.WGRAD_MUTANTS:
        if R.wgrad_applies(c, mut):
            got, _ = R.ref_wgrad(c, inp, mut)
            assert not R.all_ok(R.wgrad_gates(c, got, ref, S, r32)), f"{c}: mutant {mut} passes"


def test_wgrad_truncated_operands_fail():
    for c in R.WGRAD_INST[:2] + R.WGRAD_SPLIT:
        inp = c.inputs()
        ref, S = R.ref_wgrad(c, inp)
        t = dict(inp, x1=R.trunc10(inp["x1"]), dy=R.trunc10(inp["dy"]),
                 x2=R.trunc10(inp["x2"]) if inp["x2"] is not None else None)
        got, _ = R.ref_wgrad(c, t)
        g = dict(R.wgrad_gates(c, got, ref, S))
        assert not ok(g["rms" if c.dims()[2] > R.LONG else "elem"]), c


def test_wgrad_tables_reach_what_they_claim():
    seen = set()
    for c in R.WGRAD_ALL:
        if c.inst is not None:
            assert c.expect_inst() == c.inst, (c, c.expect_inst())
        if c.splits is not None:
            assert c.expect_splits() == c.splits, (c, c.expect_splits())
        B, H, W, C1, C2, Cout, ks, s, p, circ = c.shape
        Ho, Wo, M, K = c.dims()
        assert R.wgrad_workspace(B, Ho, Wo, C1 + C2, Cout, ks) == len(c.expect_splits()) * K * Cout * 4 + 256
        seen.add(c.expect_inst())
    assert len(seen - {"thin"}) == 12, "not all 12 k_wgrad<NT, ASC, BSC>"
    assert "thin" in seen
    c = R.WGRAD_INST[0]
    assert c.dims()[2] == 63 and c.dims()[3] == 144        # a ragged pixel chunk, a ragged second k-block
    assert [c.dims()[2] for c in R.WGRAD_SPLIT] == [512, 544, 1312]
    # the thin boundary: each declined shape is one condition away from the taken one
    assert [R.thin_takes(c.shape, c.shift_x) for c in R.WGRAD_THIN_EDGE] == [False] * 5 + [True]
    # the refused geometries: torch's output size is < 1, or the wrap would go round more than once
    for H, ks, pad, stride, circ in R.WGRAD_BAD_GEOMETRY:
        assert H <= 0 or H + 2 * pad < ks or (circ and pad > H)
        if 0 < H and H + 2 * pad < ks:
            assert int((H + 2 * pad - ks) / stride) + 1 == 1, "C's truncating division admitted this one"
