"""CPU: tests/conv_ref.py proves itself.  (1) its float64 references equal torch's float64 CPU operators to
1e-12, for every kind; (2) its float32 evaluation (sequential k order) passes every gate, plain sums without
the float32 fallback, and the fallback is used by at most a tenth of the cases; (3) every mutant fails the
gate of at least one case that names the mutated branch; (4) every case reaches the branch it names by the
restated predicates of conv.hip / thin.hip, the 24 fp32 instantiations of k_conv included."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import train_ops_ref as T
from conv_ref import F32, F64


@functools.lru_cache(maxsize=None)
def _ev(name, dt):
    c = BY_NAME[name]
    return R.evaluate(c, c.inputs(), None, dt)


BY_NAME = {c.name: c for c in R.ALL}


def ev(c, dt=F64):
    return _ev(c.name, dt)


def t64(a):  # NHWC numpy -> NCHW float64 tensor
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, F64).transpose(0, 3, 1, 2)))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def torch_reference(c, inp):
    """the same operation from torch's own float64 operators (NCHW)"""
    act = {0: lambda v: v, 1: torch.relu, 2: torch.sigmoid, 3: F.silu}[c.act]
    if c.kind == "linear":
        x = np.concatenate([inp["x1"]] + ([inp["x2"]] if c.C2 else []), 3).reshape(c.Bt, c.K).astype(F64)
        y = torch.from_numpy(x) @ torch.from_numpy(inp["w"].reshape(c.Cout, -1)[:, :c.K].astype(F64)).T
        y = y.reshape(c.Bt, c.Cout, 1, 1)
    elif c.kind == "convT":
        x, w = t64(inp["x1"]), torch.from_numpy(inp["w"].astype(F64))
        if not c.circ:
            y = F.conv_transpose2d(x, w, stride=2, padding=1)
        else:   # the adjoint of the circularly padded 4x4 / stride-2 conv
            u = torch.zeros(c.Bt, c.Cout, 2 * c.H, 2 * c.W, dtype=torch.float64, requires_grad=True)
            F.conv2d(F.pad(u, (1, 1, 1, 1), mode="circular"), w, stride=2).backward(x)
            y = u.grad
    elif c.kind == "dgrad":
        cof, cif, ci_lo, n_ci = c.fwd
        pf = c.ks - 1 - c.pad   # the forward conv's pad
        Hf, Wf = c.H - 2 * pf + c.ks - 1, c.W - 2 * pf + c.ks - 1
        u = torch.zeros(c.Bt, cif, Hf, Wf, dtype=torch.float64, requires_grad=True)
        up = F.pad(u, (pf,) * 4, mode="circular") if c.circ and pf else F.pad(u, (pf,) * 4)
        F.conv2d(up, torch.from_numpy(inp["w"].astype(F64))).backward(t64(inp["x1"]))
        y = u.grad[:, ci_lo:ci_lo + n_ci]
    else:
        b = np.arange(c.Bt)
        bs = b % c.bmod if c.bmod else b
        srcs = []
        for i in (1, 2):
            if inp[f"x{i}"] is None:
                continue
            x = t64(inp[f"x{i}"][bs])
            if inp[f"sc{i}"] is not None:
                sc, sh = (torch.from_numpy(inp[k].astype(F64))[:, :, None, None] for k in (f"sc{i}", f"sh{i}"))
                x = F.silu(x * sc + sh)
            srcs.append(x)
        x = torch.cat(srcs, 1)
        if c.ups:
            x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        if c.pad:
            x = F.pad(x, (c.pad,) * 4, mode="circular") if c.circ else F.pad(x, (c.pad,) * 4)
        y = F.conv2d(x, torch.from_numpy(inp["w"].astype(F64)), stride=c.stride)
    if inp["bias"] is not None:
        y = y + torch.from_numpy(inp["bias"].astype(F64))[None, :, None, None]
    if inp["bias_b"] is not None:
        y = y + torch.from_numpy(inp["bias_b"].astype(F64))[:, :, None, None]
    if inp["resid"] is not None:
        y = y + t64(inp["resid"])
    return nhwc(act(y))


@pytest.mark.parametrize("group", list(R.GROUPS))
def test_references_equal_torch_float64(group):
    for c in R.GROUPS[group]:
        if c.dims()[4] == 0:
            assert ev(c)["y"].size == 0
            continue
        ref, want = ev(c)["y"], torch_reference(c, c.inputs())
        assert ref.shape == want.shape, c
        scale = max(1.0, float(np.abs(want).max()))
        assert float(np.abs(ref - want).max()) <= 1e-12 * scale, (c, float(np.abs(ref - want).max()))
        if c.gn:
            v = want.reshape(c.Bt, -1, 128, c.Cout)
            assert np.allclose(ev(c)["gn"][..., 0], v.sum(2), rtol=1e-12, atol=1e-12)
            assert np.allclose(ev(c)["gn"][..., 1], (v * v).sum(2), rtol=1e-12, atol=1e-12)


def test_packers_are_the_reference_weights():
    """the packed layouts reproduce the conv through a plain [pixels][K] x [K][Cout] product"""
    r = T.rng(5)
    w = R.f32(r.standard_normal((5, 3, 3, 3)))
    p = R.pack_conv(w, 32, 32)
    assert p.shape == (32, 32) and (p[5:] == 0).all() and (p[:, 27:] == 0).all()
    assert p[4, (1 * 3 + 2) * 3 + 1] == w[4, 1, 1, 2]
    wt = R.f32(r.standard_normal((3, 5, 4, 4)))
    pt = R.pack_convT(wt, 32, 32)
    assert pt.shape == (4, 32, 32) and pt[0, 4, 0 * 3 + 2] == wt[2, 4, 3, 3] and pt[3, 4, 3 * 3 + 2] == wt[2, 4, 0, 0]
    assert pt[1, 4, 1 * 3 + 2] == wt[2, 4, 3, 0]    # phase (ry 0, rx 1), tap (dy 0, dx 1): ky 3, kx 0
    pd = R.pack_dgrad(w, 1, 2, 32, 64)
    assert pd[1, (0 * 3 + 2) * 5 + 4] == w[4, 2, 2, 0] and (pd[2:] == 0).all() and (pd[:, 45:] == 0).all()


def test_float32_evaluation_passes_every_gate():
    fallback = []
    for c in R.ALL:
        if c.dims()[4] == 0:
            continue
        ref, r32 = ev(c), ev(c, F32)["y"]
        gs = R.gates(c, r32, ref, r32)
        if T.FALLBACK:
            fallback.append((c.name, T.FALLBACK))
        assert not (c.plain() and T.FALLBACK)
        assert R.all_ok(gs), (c, gs)
        if c.gn:
            assert R.all_ok(R.gn_gates(c, _own_gn(c, r32), r32, ref, R.elem_bound(c, ref, r32))), c
    T.FALLBACK = None
    print(f"\n  float32 fallback used by {len(fallback)} of {len(R.ALL)} cases: {fallback}")
    assert len(fallback) * 10 <= len(R.ALL)
    for name, _ in fallback:   # never in groups a-d, h-j with act 0 / 1
        c = BY_NAME[name]
        assert not (name[0] in "abcdhij" and c.act < 2), name


def _own_gn(c, y):
    v = np.asarray(y, F64).reshape(c.Bt, -1, 128, c.Cout)
    return np.stack([v.sum(2), (v * v).sum(2)], -1)


@pytest.mark.filterwarnings("ignore:overflow encountered")   # a mutant may multiply the 0x7b pattern in
@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_mutant_is_caught(mut):
    named = [c for c in R.ALL if R.applies(c, mut)]
    assert named, f"no case names the branch of {mut}"
    caught = []
    for c in named:
        if c.K * c.dims()[4] * c.Cout > 2e7:   # the float64 matmul of the largest cases is not needed here
            continue
        ref = ev(c)
        r32 = ev(c, F32)["y"] if R.needs32(c) else None
        m = R.evaluate(c, c.inputs(), mut)
        if mut == "gn_neighbour_group":
            bad = not R.all_ok(R.gn_gates(c, m["gn"], ref["y"], ref, R.elem_bound(c, ref, r32)))
        else:
            bad = not R.all_ok(R.verdict(c, R.flat_output(c, m, mut), ref, r32))
        if bad:
            caught.append(c.name)
        # the unmutated reference passes the same check
        assert R.all_ok(R.verdict(c, R.flat_output(c, ref), ref, r32)), c
    T.FALLBACK = None
    print(f"\n  {mut}: fails {len(caught)} of {len(named)} cases that name it")
    assert caught, f"{mut} passes every gate"


def test_every_case_reaches_the_branch_it_names():
    for c in R.ALL:
        if c.inst is not None:
            assert R.dispatch(c) == c.inst, (c, R.dispatch(c), c.inst)
        if c.epi is not None:
            assert not isinstance(R.dispatch(c), str) and R.epilogue(c) == c.epi, (c, R.epilogue(c))
        Hi, Wi, Ho, Wo, M = c.dims()
        assert Hi + 2 * c.pad >= c.ks and Wi + 2 * c.pad >= c.ks and (not c.circ or c.pad <= min(Hi, Wi)), c
        assert c.kpad % 32 == 0 and c.kpad >= c.K and c.cout_pad % 32 == 0 and c.cout_pad >= c.Cout, c
        if c.pro:
            assert (Ho * Wo) % 128 == 0 and c.circ and not c.bmod and max(c.C1, c.C2) <= R.PRO_MAXC and c.kpad == c.K, c
        if c.gn:
            assert (Ho * Wo) % 128 == 0, c


def test_all_24_fp32_instantiations_are_named():
    want = {(nt, m, circ, False) for nt in (1, 2, 3) for m in (0, 1, 3) for circ in (True, False)}
    want |= {(nt, 2, True, False) for nt in (1, 2, 3)} | {(nt, 3, True, True) for nt in (1, 2, 3)}
    assert len(want) == 24
    got = {R.dispatch(c) for c in R.GROUPS["a"]}
    assert got == want, want ^ got
    for c in R.GROUPS["a"]:
        assert c.inst == R.dispatch(c), c


def test_table_covers_the_listed_edges():
    al = R.ALL
    conv = [c for c in al if c.kind == "conv" and not isinstance(R.dispatch(c), str)]
    assert {0, 1, 127, 128, 129, 257} <= {c.dims()[4] for c in conv}
    assert {1, 35, 128, 256} <= {c.dims()[2] * c.dims()[3] for c in conv}
    assert {1, 31, 32, 33, 95, 96, 97, 193} <= {c.Cout for c in conv}
    assert {4, 28} <= {c.K % 32 for c in conv} and any(c.kpad == c.K for c in conv)
    assert {1, 2, 3, 4, 5} <= {c.ks for c in conv} and {1, 2, 3} <= {c.stride for c in conv}
    for mode in (0, 1, 3):   # bmod 1, 2, 3 with residual and bias_b at each mode
        assert {1, 2, 3} <= {c.bmod for c in conv if R.dispatch(c)[1] == mode and c.bias_b and c.resid}
    eps = {(R.epilogue(c), c.gn, c.act) for c in conv}
    for form in ("general", "cols", "quad"):
        for gn in (False, True):
            for act in range(4):
                f = "quad_act" if form == "quad" and act else form
                assert (f, gn, act) in eps, (f, gn, act)
    thin = [c for c in al if isinstance(R.dispatch(c), str)]
    for kern in ("cin1", "cout1"):
        t = [c for c in thin if R.dispatch(c) == kern]
        assert {1, 2, 3, 4, 7} <= {c.ks for c in t} and {0, 1, 2, 3} <= {c.act for c in t}
        assert any(c.bias_b for c in t) and any(c.resid for c in t) and any(c.Bt * c.dims()[2] > 2048 for c in t)
        assert {1, 5, 65} <= {c.W for c in t} and any(c.dims()[3] > 64 for c in t)
        assert any(c.dims()[3] != c.W for c in t)
    ct = [c for c in al if c.kind == "convT"]
    assert {(1, 1), (1, 3), (5, 5), (3, 7), (8, 16)} <= {(c.H, c.W) for c in ct}
    assert {3, 4, 32, 36} <= {c.C1 for c in ct} and {1, 20, 33, 96} <= {c.Cout for c in ct}
    assert {0, 1, 2, 3} <= {c.act for c in ct} and {0, 1} <= {c.circ for c in ct} and {True, False} <= {c.bias for c in ct}
    assert any(c.dims()[4] % 128 for c in ct)
