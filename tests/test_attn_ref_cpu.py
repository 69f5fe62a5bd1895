"""CPU: the float64 attention reference, codecs, restated dispatch, input families, gates and mutants of
tests/attn_ref.py, which tests/test_gpu_attn.py applies to the HIP kernels.  No GPU.

Shown here (pytest -s): every case sits on the dispatch branch it names and the case lists reach all 36 kernel
instantiations; the per-form CPU emulations (float32 chain; P rounded to bf16; P split into f16 hi + lo) meet
every derived gate, the 4 x fallbacks listed; every mutant misses at least one gate; onehot, constv and
threshold have the properties the GPU tests lean on."""
import math

import numpy as np
import pytest
import torch

import attn_ref as R
import train_ops_ref as T
from attn_ref import F32, F64


# ------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize("Bt,N,heads,d", [(2, 37, 3, 8), (1, 256, 2, 48), (3, 5, 1, 64)])
def test_sdpa64_equals_torch_float64(Bt, N, heads, d):
    C = heads * d
    qkv = T.rng(N).standard_normal((Bt, N, 3 * C)) * 2.0
    ref = R.sdpa64(qkv, heads)
    t = torch.from_numpy(qkv)
    sp = lambda a: a.reshape(Bt, N, heads, d).transpose(1, 2)  # noqa: E731
    q, k, v = sp(t[..., :C]), sp(t[..., C:2 * C]), sp(t[..., 2 * C:])
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(Bt, N, C).numpy()
    assert np.abs(ref.o - o).max() <= 1e-12
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), -1)
    assert np.abs(ref.P - p.numpy()).max() <= 1e-12
    assert np.abs(ref.A - (p @ v.abs()).transpose(1, 2).reshape(Bt, N, C).numpy()).max() <= 1e-12
    assert (ref.A >= np.abs(ref.o) - 1e-12).all()
    dev = (p.unsqueeze(-1) * (v.unsqueeze(2) - (p @ v).unsqueeze(3)).abs()).sum(3)    # sum_j P |v_j - o|
    assert (dev.transpose(1, 2).reshape(Bt, N, C).numpy() <= ref.sig + 1e-12).all()


# ------------------------------------------------------------------------------------ codecs
def _wide(shape, seed=3):
    g = T.rng(seed)
    return (g.standard_normal(shape) * 10.0 ** g.uniform(-6, 4, shape)).astype(F32)


def test_codecs_equal_torch_casts_bit_for_bit():
    x = _wide((3, 7, 32))
    x[0, 0, :4] = [0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8]    # two bf16 ties: to even, down and up
    t = torch.from_numpy(x)
    hb = t.to(torch.bfloat16)
    lb = (t - hb.float()).to(torch.bfloat16)
    assert np.array_equal(R.encode(x, "b2"), hb.view(torch.int16).numpy().view(np.uint16))
    rec = R.encode(x, "bf16")
    assert rec.shape == (3, 7, 4, 2, 8) and rec.dtype == np.uint16
    assert np.array_equal(rec[..., 0, :].reshape(x.shape), hb.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(rec[..., 1, :].reshape(x.shape), lb.view(torch.int16).numpy().view(np.uint16))
    hh = t.to(torch.float16)
    lh = (t - hh.float()).to(torch.float16)
    rec = R.encode(x, "h2")
    assert np.array_equal(rec[..., 0, :].reshape(x.shape), hh.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(rec[..., 1, :].reshape(x.shape), lh.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(R.decode(rec, "h2"), (hh.double() + lh.double()).numpy())
    assert np.array_equal(R.decode(R.encode(x, "bf16"), "bf16", lo=False), hb.double().numpy())


@pytest.mark.parametrize("fmt", ["f32", "h2", "bf16", "b2"])
def test_codecs_round_trip(fmt):
    """representable() is a projection; encode(decode(.)) gives the storage back; the layout is [C/8][2][8]"""
    x = _wide((2, 5, 16), 4)
    r = R.representable(x, fmt)
    assert np.array_equal(R.representable(r, fmt), r)
    u = R.encode(r, fmt)
    if fmt == "h2":
        assert np.array_equal(R.encode(R.decode(u, fmt), fmt), u)
    else:
        assert np.array_equal(R.encode(R.decode(u, fmt, lo=False), fmt)[..., 0, :] if fmt == "bf16" else
                              R.encode(R.decode(u, fmt), fmt), u[..., 0, :] if fmt == "bf16" else u)
    tol = {"f32": 0.0, "h2": 2.0 ** -21, "bf16": 2.0 ** -8, "b2": 2.0 ** -8}[fmt]
    assert (np.abs(r - x) <= tol * np.abs(x) + (2.0 ** -24 if fmt == "h2" else 0)).all()
    assert u.nbytes == R.nbytes(x.size, fmt)
    if fmt in ("h2", "bf16"):   # channel 8 g + e of a pixel: hi at [g][0][e], lo at [g][1][e]
        one = np.zeros((1, 16), F32)
        one[0, 11] = 1.0 + 2.0 ** -12
        rec = R.encode(one, fmt)
        assert rec[0, 1, 0, 3] != 0 and rec[0, 1, 1, 3] != 0 and np.count_nonzero(rec) == 2


# ------------------------------------------------------------------------------------ dispatch
def test_branch_restates_the_host_code():
    b = R.branch
    assert [b("attention", n, 48) for n in (1, 31, 32, 255, 256, 300, 512, 576, 0)] == \
        ["valu", "valu", "mfma", "valu", "mfma", "refused", "flash", "refused", "refused"]
    assert b("attention", 512, 8) == b("attention", 512, 24) == "unsupported"
    assert b("attention", 100, 40) == b("attention", 64, 12) == "unsupported"
    assert [b("attention_h2", n, 16) for n in (32, 100, 256, 288, 512)] == ["mfma", "refused", "mfma", "refused", "flash"]
    assert b("attention_h2", 64, 12, heads=1) == "refused" and b("attention_h2", 64, 12, heads=2) == "unsupported"
    for e in ("split", "split_bf16", "split_b2"):
        assert b(e, 128, 16) == "refused" and b(e, 512, 8) == b(e, 512, 24) == b(e, 256, 40) == "unsupported"
        assert b(e, 256, 16) == "split"
        assert b(e, 512, 16) == b(e, 768, 64) == ("split" if e == "split" else "split_pf2")
    for e in R.ENTRIES:
        assert b(e, 256, 16, Bt=-1) == b(e, 256, 16, Bt=65536) == b(e, 256, 16, heads=65536) == "refused"
        assert b(e, 256, 16, heads=0) == "refused" and b(e, 256, 16, Bt=65535, heads=65535) != "refused"


@pytest.mark.parametrize("c", R.ALL_CASES + [c for cs in R.KNOB_CASES.values() for c in cs], ids=repr)
def test_every_case_is_on_the_branch_it_names(c):
    assert c.branch == R.branch(c.entry, c.N, c.D, c.Bt, c.heads)
    assert c.branch in ("valu", "mfma", "flash", "split", "split_pf2")


def test_the_case_lists_reach_what_the_issue_names():
    G = R.GROUPS
    reached = {}
    for name, cs in G.items():
        for c in cs:
            reached.setdefault(R.instantiation(c.entry, c.N, c.D), set()).add(name)
    print()
    for k in R.ALL_INSTANTIATIONS:
        print(f"  {k:32s} {', '.join(sorted(reached.get(k, ())))}")
    assert set(reached) == set(R.ALL_INSTANTIATIONS)
    valu = [c for c in G["valu"] if c.family == "gauss"]
    assert {(c.N, c.D) for c in valu} == {(n, d) for n in R.VALU_N for d in R.DIMS}
    assert {c.heads for c in valu} == {1, 3} and {c.Bt for c in valu} == {1, 2}
    assert all(c.branch == "valu" and c.N % 64 for c in G["valu"])
    mf = [c for c in G["mfma"] if c.family == "gauss"]
    assert {(c.N, c.D) for c in mf} == {(n, d) for n in R.MFMA_N for d in R.DIMS}
    assert {c.heads for c in mf} == {1, 2, 5} and max(c.Bt for c in mf) == 3
    fl = [c for c in G["flash"] if c.family == "gauss"]
    assert {(c.N, c.D) for c in fl} == {(n, d) for n in (512, 768) for d in R.DIMS_LONG}
    assert len({(c.Bt, c.heads) for c in fl}) >= 3
    h2 = [c for c in G["h2"] if c.family == "gauss"]
    assert {c.D for c in h2 if c.branch == "mfma"} == set(R.DIMS)
    assert {c.D for c in h2 if c.branch == "flash"} == set(R.DIMS_LONG)
    for e in ("split", "split_bf16", "split_b2"):
        gs = [c for c in G[e] if c.family == "gauss"]
        assert {(c.N, c.D) for c in gs} >= {(n, d) for n in (256, 512) for d in R.DIMS_LONG} | {(768, 16), (768, 48)}
        assert {c.N // 256 * c.Bt * c.heads for c in gs} >= {1, 3, 9, 15, 17}
    # onehot, uniform and constv on every branch at every head dim; the steered families on flash and the split forms
    for fam in ("onehot", "uniform", "constv"):
        got = {(c.entry, c.branch, c.D) for c in R.ALL_CASES if c.family == fam}
        want = {("attention", "valu", d) for d in R.DIMS} | {("attention", "mfma", d) for d in R.DIMS} | \
            {("attention", "flash", d) for d in R.DIMS_LONG} | {("split", "split", d) for d in R.DIMS_LONG} | \
            {(e, b, d) for e in ("split_bf16", "split_b2") for b in ("split", "split_pf2") for d in R.DIMS_LONG}
        assert got >= want, want - got
    for fam in ("rising", "falling", "threshold"):
        for e in ("attention", "split", "split_bf16", "split_b2"):
            cs = [c for c in R.ALL_CASES if c.family == fam and c.entry == e]
            assert 16 in {c.D for c in cs} and len({c.D for c in cs}) >= 2 and all(c.N in (768, 1280) for c in cs)
    assert {c.arg for c in R.ALL_CASES if c.family == "rising"} == {3.0, 12.0}


# ------------------------------------------------------------------------------------ emulations meet the gates
FALLBACKS = []


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print(f"\n  4 x fallbacks (the form's own CPU emulation misses the derived gate): {len(FALLBACKS)}")
    for line in FALLBACKS:
        print("    " + line)


@pytest.mark.parametrize("c", R.ALL_CASES, ids=repr)
def test_emulation_meets_the_gate(c):
    """the form's CPU emulation against float64 under the derived bound; where it misses (only where
    attn_ref.needs_emul allows an emulation into the gate), the 4 x rule applies and the case is listed"""
    qkv, ref = R.inputs(c), R.reference(c)
    assert np.array_equal(R.representable(qkv, c.fmt_in), qkv)
    for lo in ((False, True) if c.entry == "split_bf16" else (False,)):
        em = R.emulate(c, qkv, lo)
        eb = R.gate(c, em, ref, None, lo)
        if not R.ok(eb):
            assert R.needs_emul(c, lo), f"{c} lo={lo}: emulation err {eb[0]:.3e} > bound {eb[1]:.3e}"
            eb2 = R.gate(c, em, ref, em, lo)
            assert T.FALLBACK is not None and R.ok(eb2)
            FALLBACKS.append(f"{c!r}: emulation err {eb[0]:.3e}, derived bound {eb[1]:.3e}, gate 4 x {T.FALLBACK:.3e}")
        T.FALLBACK = None


def test_unrounded_l_under_the_deferred_max_misses_the_gate():
    """The finding of tests/test_gpu_attn.py, reproduced on the CPU: at D = 32 / 64 the bf16 kernel summed l from
    the unrounded p.  With the exact running maximum a row's largest p is 2^10, exact in bf16; under the deferred
    maximum it is not, and its rounding stays in the output of a peaked row.  That arithmetic (l_rounded=False)
    misses the gate on the gauss(3) cases below, to the digits measured on the GPU; with l summed from the
    rounded p (the kernel now), or with the exact maximum, it is well inside."""
    print()
    for name in ("split_bf16-split-N256-D32-h2-B2-gauss(3)", "split_bf16-split_pf2-N512-D64-h1-B3-gauss(3)",
                 "split_b2-split-N256-D64-h1-B3-gauss(3)", "split_b2-split_pf2-N512-D32-h2-B2-gauss(3)"):
        c = next(c for c in R.ALL_CASES if repr(c) == name)
        qkv, ref = R.inputs(c), R.reference(c)
        r = {}
        for what, kw in (("before", dict(l_rounded=False)), ("exact max", dict(l_rounded=False, defer=0.0)), ("now", {})):
            e, b = R.gate(c, R.emulate(c, qkv, **kw), ref)
            r[what] = e / b
        print(f"  {name}: err / bound before {r['before']:.3f}, with the exact maximum {r['exact max']:.3f}, now {r['now']:.3f}")
        assert r["before"] > 1.0 and r["exact max"] < 0.5 and r["now"] < 0.5


# ------------------------------------------------------------------------------------ mutants
def _probe_cases(m):
    """per (entry, branch, family): the first case the mutant applies to"""
    seen, out = set(), []
    for c in R.ALL_CASES:
        k = (c.entry, c.branch, c.family, c.arg)
        if k not in seen and R.applies(m, c):
            seen.add(k)
            out.append(c)
    return out


@pytest.mark.parametrize("m", R.MUTANTS)
def test_every_mutant_fails(m):
    failed = []
    cs = _probe_cases(m)
    for c in cs:
        qkv, ref = R.inputs(c), R.reference(c)
        got = R.mutant(c, qkv, m)
        los = (False, True) if c.entry == "split_bf16" else (False,)
        if any(not R.ok(R.gate(c, got, ref, R.emulate(c, qkv, lo) if R.needs_emul(c, lo) else None, lo)) for lo in los):
            failed.append(c)
        T.FALLBACK = None
    fams = sorted({f"{c.branch}/{c.family}" for c in failed})
    print(f"\n  {m}: misses the gate on {len(failed)} of {len(cs)} probed cases: {', '.join(fams)}")
    assert failed, m
    if m in ("no_rescale_O", "no_rescale_l", "max_per_tile"):
        assert any(c.family == "rising" for c in failed)
    if m == "p_bf16_l_unrounded":
        assert any(c.family == "constv" and c.D == 16 for c in failed)


def test_the_truth_is_no_mutant():
    c = R.GROUPS["flash"][0]
    assert R.ok(R.gate(c, R.reference(c).o, R.reference(c)))


# ------------------------------------------------------------------------------------ the families' properties
def _scores(c):
    q, k, _ = R.heads_of(R.inputs(c), c.heads)
    return q @ k.transpose(0, 1, 3, 2) / math.sqrt(c.D)


@pytest.mark.parametrize("c", [c for c in R.ALL_CASES if c.family == "onehot"], ids=repr)
def test_onehot_leads_by_40_and_names_key_and_channel(c):
    s = _scores(c)
    ref = R.reference(c)
    _, _, v = R.heads_of(R.inputs(c), c.heads)
    for b in range(c.Bt):
        for h in range(c.heads):
            pi = R.onehot_perm(c.N, b, h)
            assert sorted(pi) == list(range(c.N))
            if c.N > 1:
                top = s[b, h, np.arange(c.N), pi]
                rest = s[b, h].copy()
                rest[np.arange(c.N), pi] = -np.inf
                assert (top - rest.max(-1) >= 40.0).all()
            assert np.abs(ref.o[b, :, h * c.D:(h + 1) * c.D] - v[b, h, pi]).max() <= 1e-12 * np.abs(v).max()
    # pi crosses sub-tiles, key tiles and query blocks
    pi, i = R.onehot_perm(c.N), np.arange(c.N)
    if c.N >= 64:
        assert (pi // 32 != i // 32).any() and len({int(x) for x in pi[:32] % 32}) > 16
    if c.N >= 512:
        assert (pi // 128 != i // 128).any() and (pi // 256 != i // 256).any()
    # v names (key, channel): exact in the format, distinct over keys at a channel and over channels at a key
    vv = R.onehot_v(c.N, c.C, c.fmt_in)
    assert np.array_equal(R.representable(vv, c.fmt_in), vv)
    assert all(len(set(vv[:, ch])) == c.N for ch in range(c.C)) and all(len(set(vv[j])) == c.C for j in (0, c.N - 1))


@pytest.mark.parametrize("c", [c for c in R.ALL_CASES if c.family in ("constv", "uniform")], ids=repr)
def test_constv_and_uniform(c):
    ref = R.reference(c)
    _, _, v = R.heads_of(R.inputs(c), c.heads)
    if c.family == "constv":
        assert np.abs(ref.o - R.merge(v)).max() <= 1e-13 * np.abs(v).max()
        # the only terms left of a bf16 ONES bound: output rounding and the fp32 chain
        assert (ref.sig <= 1e-6 * np.abs(v).max()).all()
    else:
        assert np.abs(ref.P - 1.0 / c.N).max() <= 1e-15
        assert np.abs(ref.o - R.merge(np.broadcast_to(v.mean(2, keepdims=True), v.shape))).max() <= 1e-12


@pytest.mark.parametrize("c", [c for c in R.ALL_CASES if c.family in ("rising", "falling", "threshold")], ids=repr)
def test_steered_families(c):
    s2 = _scores(c)[0, 0] * R.LOG2E                        # log2 units of p
    tmax = s2.reshape(c.N, c.N // 128, 128).max(-1)        # [query, tile]
    rise = np.diff(tmax, axis=1)
    if c.family == "rising":
        assert (np.abs(rise - c.arg) <= 1.5).all()         # each tile raises the row maximum by the step
        assert (c.arg < 8.0) == (c.arg == 3.0)             # 3: deferred until the stale offset passes 8; 12: never
        if c.arg == 3.0:
            assert (tmax[:, 3] - tmax[:, 0] > 8.0).all() and (tmax[:, 2] - tmax[:, 0] < 8.0).all()
    elif c.family == "falling":
        # the first tile holds the maximum; each later one lies a further ~30 log2 units down (k's steering value
        # is rounded to the input format: within 2.5), so from the fifth on p underflows float32
        assert (np.abs(rise + c.arg) <= 2.5).all() and (tmax.argmax(1) == 0).all()
        assert (tmax[:, -1] - tmax[:, 0] < -126).all()
    else:
        first = rise[:, 0]
        assert (np.abs(rise[:, 1:]) < 0.1).all()
        for w in range(c.N // 32):                         # every wave's 32 queries: both sides of the threshold
            r = first[32 * w:32 * w + 32]
            assert ((r > 7.5) & (r < 7.95)).sum() == 16 and ((r > 8.05) & (r < 8.5)).sum() == 16
