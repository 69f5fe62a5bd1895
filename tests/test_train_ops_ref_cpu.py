"""CPU: the gates of tests/test_gpu_train_ops.py can fail, and a correct fp32 evaluation meets them.

For every gate: (a) the reference formula evaluated in float32 passes it against the float64
reference, on the inputs the GPU test uses; (b) a deliberately wrong variant fails it.  A mutant
that passed would mean the case or the gate is too weak.  Needs no libtcx and no GPU."""
import numpy as np
import pytest

import train_ops_ref as R
from train_ops_ref import F32, F64, ok


def passes(eb, what=""):
    assert ok(eb), f"{what}: err {eb[0]:.3e} > bound {eb[1]:.3e}"


def fails(eb, what=""):
    assert not ok(eb), f"mutant passed: {what}: err {eb[0]:.3e} <= bound {eb[1]:.3e}"


# ------------------------------------------------------------------------------------ column sums
COLSUM_SHAPES = ([(1, r, c) for r, c, _ in R.COLSUM_SMALL if _ == 0.0] + [R.COLSUM_PAST_SMALL] + R.COLSUM_VEC
                 + R.COLSUM_SCALAR + [(1, 16448, 8), (2, 20000, 4)])


@pytest.mark.parametrize("shape", COLSUM_SHAPES, ids=str)
def test_colsum_gate(shape):
    x = R.colsum_input(*shape)
    pb, tot, sa = R.ref_colsum(x)
    # (a) float64 accumulation rounded once to float32, as the kernels do
    passes(R.gate_colsum(pb.astype(F32), pb, sa), "per_batch")
    passes(R.gate_colsum(tot.astype(F32), tot, sa), "total")
    t0 = R.f32(R.rng(7).standard_normal(shape[2]))
    passes(R.gate_colsum((F32(0.5) * t0 + tot.astype(F32)).astype(F32), 0.5 * t0.astype(F64) + tot, sa, 0.5, t0), "beta")
    # (b)
    if shape[1] > 1:
        mpb, mtot, _ = R.ref_colsum(x, mutant="drop_last_row")
        fails(R.gate_colsum(mtot.astype(F32), tot, sa), "total without the last row")
        fails(R.gate_colsum(mpb.astype(F32), pb, sa), "per_batch without the last row")
    ns = R.colsum_nsplit(shape[0], shape[1])
    if shape[1] % ns:
        _, mtot, _ = R.ref_colsum(x, mutant="floor_split")
        fails(R.gate_colsum(mtot.astype(F32), tot, sa), "rows past nsplit*floor(HW/nsplit) dropped")
    if shape[0] > 32:
        _, mtot, _ = R.ref_colsum(x, mutant="first32")
        fails(R.gate_colsum(mtot.astype(F32), tot, sa), "total over the first 32 batches")


def test_colsum_cases_reach_the_uneven_split_and_second_trip():
    assert any(hw % R.colsum_nsplit(bt, hw) for bt, hw, _ in R.COLSUM_VEC)
    assert any(bt > 32 for bt, _, _ in R.COLSUM_VEC)
    assert R.colsum_nsplit(1, 16448) == 257 and R.colsum_nsplit(2, 20000) > 256


# ------------------------------------------------------------------------------------ GroupNorm
def _gn_all(case, offset=0.0):
    Bt, HW, C, groups, silu = case
    x, dy, gamma, beta = R.gn_inputs(Bt, HW, C, offset=offset)
    return x, dy, gamma, beta, R.ref_gn_bwd(x, dy, gamma, beta, groups, silu)


@pytest.mark.parametrize("case", R.GN_CASES, ids=str)
def test_gn_bwd_gate(case):
    Bt, HW, C, groups, silu = case
    x, dy, gamma, beta, (dx, dg, db) = _gn_all(case)
    # the closed form of the kernels is the autograd result
    fx, fg, fb = R.gn_bwd_formula(x, dy, gamma, beta, groups, silu)
    passes(R.gate_max(fx, dx, 1e-9), "formula dx")
    passes(R.gate_max(fg, dg, 1e-9), "formula dgamma")
    passes(R.gate_max(fb, db, 1e-9), "formula dbeta")
    # (a)
    hx, hg, hb = R.gn_bwd_formula(x, dy, gamma, beta, groups, silu, dt=F32)
    for name, h, ref in (("dx", hx, dx), ("dgamma", hg, dg), ("dbeta", hb, db)):
        eb = R.gate_max(h, ref)
        print(f"GN {case} {name}: fp32 reference err {eb[0]:.3e} bound {eb[1]:.3e}")
        passes(eb, name)
    # (b)
    mx, _, _ = R.gn_bwd_formula(x, dy, gamma, beta, groups, silu, mutant="no_k3")
    fails(R.gate_max(mx, dx), "dx without k3")
    if HW * (C // groups) <= 1600:  # beyond that 1/n and 1/(n-1) differ by less than the 2e-5 gate
        mx, _, _ = R.gn_bwd_formula(x, dy, gamma, beta, groups, silu, mutant="n_minus_1")
        fails(R.gate_max(mx, dx), "dx with n - 1")
    if Bt > 32:
        _, mg, mb = R.gn_bwd_formula(x, dy, gamma, beta, groups, silu, mutant="first32")
        fails(R.gate_max(mg, dg), "dgamma over 32 batches")
        fails(R.gate_max(mb, db), "dbeta over 32 batches")


def test_gn_bwd_cases_cover_the_mutants():
    assert sum(hw * (c // g) <= 1600 for _, hw, c, g, _ in R.GN_CASES) >= 3
    assert any(bt > 32 for bt, *_ in R.GN_CASES)


def test_gn_bwd_offset_input_fp32_reference():
    """x = 100 + randn at (2, 200, 96, 8, silu): prints the float32 reference error that the GPU
    test prints next to the kernel's error; the GPU test keeps the plain 2e-5 * max|ref| there."""
    case = (2, 200, 96, 8, 1)
    x, dy, gamma, beta, (dx, dg, db) = _gn_all(case, offset=100.0)
    hx, hg, hb = R.gn_bwd_formula(x, dy, gamma, beta, 8, 1, dt=F32)
    for name, h, ref in (("dx", hx, dx), ("dgamma", hg, dg), ("dbeta", hb, db)):
        e = float(np.abs(h.astype(F64) - ref).max())
        print(f"GN offset {name}: fp32 reference err {e:.3e}, 2e-5*max|ref| {2e-5 * np.abs(ref).max():.3e}")
    mx, _, _ = R.gn_bwd_formula(x, dy, gamma, beta, 8, 1, mutant="no_k3")
    fails(R.gate_max(mx, dx), "offset dx without k3")


def test_gn_stats_gate():
    for case in R.GN_CASES:
        Bt, HW, C, groups, _ = case
        x, _, gamma, beta = R.gn_inputs(Bt, HW, C)
        ref = R.ref_gn_stats(x, gamma, beta, groups)
        for name, r in zip(("mean", "rstd", "scale", "shift"), ref):
            passes(R.gate_rel(r.astype(F32), r, 1e-6), f"{case} {name} rounded once")
        sc32, sh32 = R.gn_tables_f32(ref[0], ref[1], gamma, beta)
        passes(R.gate_rel(sc32, ref[2], 1e-6), "scale formed in fp32")
        passes(R.gate_rel(sh32, ref[3], 1e-6, ref32=sh32), "shift formed in fp32")
        fails(R.gate_rel(beta[None] + 0 * sh32, ref[3], 1e-6, ref32=sh32), "shift without mean*scale")
        fails(R.gate_rel(ref[1] * (1 + 3e-6), ref[1], 1e-6), "rstd off by 3e-6")
        # unbiased variance instead of the biased one
        n = HW * (C // groups)
        if 1 < n < 100000:
            fails(R.gate_rel(ref[1] * np.sqrt((n - 1) / n), ref[1], 1e-6), "rstd of the unbiased variance")


# ------------------------------------------------------------------------------------ upsample
@pytest.mark.parametrize("case", R.UPS_CASES, ids=str)
def test_upsample_bwd_gate(case):
    Bt, H, W, C = case
    x, dy = R.ups_inputs(*case)
    ref = R.ref_upsample_bwd(dy)
    passes(R.gate_max(R.upsample_bwd_formula(dy), ref, 1e-12), "matrix form is the autograd adjoint")
    passes(R.gate_upsample_bwd(R.upsample_bwd_formula(dy, dt=F32), ref, dy), "fp32")
    passes(R.gate_upsample_bwd(R.ref_upsample_bwd(dy, torch_f32()), ref, dy), "torch fp32")
    fails(R.gate_upsample_bwd(R.upsample_bwd_formula(dy, mutant="no_clamp"), ref, dy), "no edge clamp")
    if H != W:
        fails(R.gate_upsample_bwd(R.upsample_bwd_formula(dy, mutant="swap_hw"), ref, dy), "H and W swapped")
    # adjoint identity <up(x), g> = <x, up_bwd(g)>
    lhs, rhs = float((R.ref_upsample(x) * dy).sum()), float((x.astype(F64) * ref).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)


def torch_f32():
    import torch
    return torch.float32


def test_upsample_cases_have_non_square_shapes():
    assert sum(h != w for _, h, w, _ in R.UPS_CASES) >= 3


# ------------------------------------------------------------------------------------ softmax
@pytest.mark.parametrize("family", R.SOFTMAX_FAMILIES)
@pytest.mark.parametrize("case", R.SOFTMAX_CASES, ids=str)
def test_softmax_gates(case, family):
    S, dP = R.softmax_input(*case, family)
    P = R.ref_softmax(S)
    P32 = R.ref_softmax(S, dt=F32)
    passes(R.gate_softmax_p(P32, P), "P fp32")
    passes(R.gate_rowsum(P32), "row sums fp32")
    dS = R.ref_softmax_bwd(P32, dP)  # the backward kernel receives the fp32 P
    passes(R.gate_softmax_ds(R.ref_softmax_bwd(P32, dP, dt=F32), dS, P32, dP), "dS fp32")
    if family == "offset":
        fails(R.gate_softmax_p(R.ref_softmax(S, dt=F32, mutant="no_max"), P), "no max subtraction")
    fails(R.gate_softmax_ds(R.ref_softmax_bwd(P32, dP, mutant="no_dot"), dS, P32, dP), "no dot term")
    if case[1] > 1 and family != "peaked":  # a peaked row's last entry may be below the 1e-10 floor
        Pm = P.copy()
        Pm[:, -1] = 0  # the last column never written
        fails(R.gate_softmax_p(Pm, P), "last column dropped")


# ------------------------------------------------------------------------------------ activations
@pytest.mark.parametrize("n", R.ACT_SIZES)
@pytest.mark.parametrize("act", (1, 2, 3))
def test_act_gates(act, n):
    z, dy = R.act_inputs(n)
    y, d = R.ref_act_fwd(z, act), R.ref_act_bwd(z, dy, act)
    assert np.isfinite(y).all() and np.isfinite(d).all()
    passes(R.gate_rel(R.ref_act_fwd(z, act, dt=F32), y, 1e-5, 1e-12), "fwd fp32")
    d32 = R.ref_act_bwd(z, dy, act, dt=F32)
    if act == 1:
        passes(R.gate_rel(d32, d, 1e-5, 1e-12), "relu bwd fp32")
    else:
        # s*(1-s) at z = +20 and 1 + z*(1-s) near z = -1.28 cancel in fp32: the stated gate cannot hold there
        eb = R.gate_rel(d32, d, 1e-5, 1e-12)
        print(f"act {act} n {n}: fp32 reference bwd err {eb[0]:.3e} at a bound of {eb[1]:.3e}; "
              f"4x its worst error {4 * np.abs(d32.astype(F64) - d).max():.3e}")
        passes(R.gate_rel(d32, d, 1e-5, 1e-12, ref32=d32), "bwd fp32")
    if act == 3:
        fails(R.gate_rel(R.ref_act_bwd(z, dy, 3, mutant="no_z_term"), d, 1e-5, 1e-12, ref32=d32), "silu' without z(1-s)")
    if act == 2:
        fails(R.gate_rel(dy * R.ref_act_fwd(z, 2), d, 1e-5, 1e-12, ref32=d32), "sigmoid' without (1-s)")
    if act == 1 and n > 1:
        assert d[z == 0].size and (d[z == 0] == 0).all()  # relu'(+-0) = 0
        fails(R.gate_rel(np.where(z >= 0, dy, 0), d, 1e-5, 1e-12), "relu'(0) = 1")


def test_act_saturation_values():
    z = np.array([100.0, -100.0], dtype=F32)
    assert R.ref_act_fwd(z, 2)[0] == 1.0 and 0 < R.ref_act_fwd(z, 2)[1] < 1e-43
    assert R.ref_act_fwd(z, 3)[0] == 100.0 and abs(R.ref_act_fwd(z, 3)[1]) < 1e-41


# ------------------------------------------------------------------------------------ MSE
@pytest.mark.parametrize("n", R.MSE_SIZES)
def test_mse_gates(n):
    a, b = R.mse_inputs(n)
    loss = R.ref_mse(a, b)
    d = (a - b).astype(F32)  # the kernel's fp32 difference and square, summed in fp64
    passes(R.gate_rel(F32((d * d).astype(F64).mean()), loss, 1e-6), "loss")
    fails(R.gate_rel(loss * n / (n + 1), loss, 1e-6), "loss over n + 1")
    for g in (3.0, 0.0):
        ref = R.ref_mse_bwd(a, b, g)
        passes(R.gate_rel(R.ref_mse_bwd(a, b, g, dt=F32), ref, 1e-6), "grad fp32")
        if g:
            fails(R.gate_rel(R.ref_mse_bwd(a, b, g, mutant="n_plus_1"), ref, 1e-6), "grad with n + 1")
            # the old gate |err| / max(1, |ref|max) < 2e-5 lets the same mutant through
            assert n < 1000 or np.abs(R.ref_mse_bwd(a, b, g, mutant="n_plus_1") - ref).max() / max(1, np.abs(ref).max()) < 2e-5


# ------------------------------------------------------------------------------------ embedding
def test_embedding_gate():
    r = R.rng(11)
    for E in (1, 24):
        idx = np.full(300, 2, np.int64)
        dout = R.f32(r.standard_normal((300, E)))
        ref, sa = R.ref_embedding_bwd(idx, dout, 5)
        got, _ = R.ref_embedding_bwd(idx, dout, 5, dt=F32)
        passes(R.gate_embedding(got, ref, sa, 300), "serial fp32 sum")
        m, _ = R.ref_embedding_bwd(idx[:-1], dout[:-1], 5)
        fails(R.gate_embedding(m, ref, sa, 300), "last batch row dropped")


# ------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("offset", (0.0, 50.0))
@pytest.mark.parametrize("film", (False, True))
@pytest.mark.parametrize("case", R.LN_CASES, ids=str)
def test_ln_gates(case, film, offset):
    M, Wd = case
    x, dh, w, b, gb = R.ln_inputs(M, Wd, 2 * Wd if film else 0, offset=offset)
    stats = R.ln_stats_f32(x)
    ref = R.ref_ln(x, dh, w, b, gb)
    passes(R.gate_max(ref["dx"], R.ref_ln_dx_autograd(x, dh, w, b, gb), 1e-7 if offset else 1e-9),
           "formula dx is autograd's")
    h = R.ref_ln(x, dh, w, b, gb, dt=F32)
    for k in ("y", "dx"):
        eb = R.gate_max(h[k], ref[k])
        print(f"LN {case} film={film} offset={offset} {k}: fp32 reference err {eb[0]:.3e} bound {eb[1]:.3e}")
        passes(eb, k)  # the plain 2e-5 * max|ref| in every case, x = 50 + randn included
    for k in ("mean", "rstd"):  # the kernel forms both in float64 and rounds once
        passes(R.gate_rel(ref[k].astype(F32), ref[k], 1e-6), k)
    fails(R.gate_rel(ref["rstd"] * np.sqrt((Wd - 1) / Wd) if Wd > 1 else ref["rstd"] * 1.01, ref["rstd"], 1e-6),
          "rstd of the unbiased variance")
    # the backward on the float32 statistics it is given; l = xhat*w + b cancels, so dgb's float32
    # evaluation forms l in float64 as the kernel does
    rs, hs = R.ref_ln(x, dh, w, b, gb, stats=stats), R.ref_ln(x, dh, w, b, gb, dt=F32, stats=stats)
    passes(R.gate_max(hs["dx"], rs["dx"]), "dx on the given statistics")
    for k in ("dwrow", "dbrow") + (("dgb",) if film else ()):
        got = rs[k].astype(F32) if k == "dgb" else hs[k]
        passes(R.gate_rel(got, rs[k], 1e-5, 1e-9), k)
        if Wd > 1:  # Wd = 1: xhat = 0
            fails(R.gate_rel(1.001 * rs[k], rs[k], 1e-5, 1e-9), k + " off by 1e-3")
    m = R.ref_ln(x, dh, w, b, gb, mutant="no_m2")
    if Wd > 1:
        fails(R.gate_max(m["dx"], ref["dx"]), "dx without xh*m2")


# ------------------------------------------------------------------------------------ Adam / EMA
@pytest.mark.parametrize("step", (1, 1000))
@pytest.mark.parametrize("wd", (0.0, 0.01))
def test_adam_gates(wd, step):
    ts = R.adam_inputs(3, step)
    ps, ms, vs = R.ref_adam(ts, step, wd)
    for (p, g, m, v), rp, rm, rv in zip(ts, ps, ms, vs):
        fp, fm, fv = R.adam_formula(p, g, m, v, step, wd)
        passes(R.gate_abs(fp, rp, 1e-6), "param")
        sm, sv = R.ref_adam_slack(p, g, m, wd)
        # numpy rounds every product (no fma) where torch's vector loops fuse: about 1 % of exp_avg at step
        # 1000 is then beyond 1e-6 relative alone, so this unfused formula gets ref_adam_slack; the kernel
        # fuses as torch does and is held to 1e-6 relative alone in the GPU test
        for name, f, r in (("exp_avg", fm, rm), ("exp_avg_sq", fv, rv)):
            n_over = int((np.abs(f.astype(F64) - r) > 1e-6 * np.abs(r.astype(F64))).sum())
            print(f"adam wd={wd} step={step} n={p.size} {name}: {n_over} elements beyond 1e-6 relative alone")
        passes(R.gate_adam_moment(fm, rm, sm), "exp_avg")
        passes(R.gate_adam_moment(fv, rv, sv), "exp_avg_sq")
        if step == 1:
            mp, _, _ = R.adam_formula(p, g, m, v, step, wd, mutant="no_bias_correction")
            fails(R.gate_abs(mp, rp, 1e-6), "no bias correction")
        if wd:
            _, mm, mv = R.adam_formula(p, g, m, v, step, 0.0)
            fails(R.gate_adam_moment(mm, rm, sm), "exp_avg without weight decay")
            fails(R.gate_adam_moment(mv, rv, sv), "exp_avg_sq without weight decay")


def test_adam_sizes_cross_the_chunk_and_the_grid():
    for nt in R.ADAM_NT:
        s = R.adam_sizes(nt)
        assert len(s) == nt and max(s) == R.ADAM_BIG > 1024 * 256
    assert {48, 49} <= set(R.ADAM_NT)


def test_ema_gate():
    p, g = R.mse_inputs(257, seed=3)
    ref = R.ref_ema(p, g)
    passes(R.gate_ema(R.ref_ema(p, g, dt=F32), ref, p, g, R.EMA_DECAY), "fp32")
    fails(R.gate_ema(R.ref_ema(p, g, mutant="swapped"), ref, p, g, R.EMA_DECAY), "d and 1-d swapped")


# ------------------------------------------------------------------------------------ VAE
def test_reparam_gates():
    for n in R.REPARAM_SIZES:
        mu, lv, eps, dz, dmu0, dlv0 = R.reparam_inputs(n)
        passes(R.gate_rel(R.ref_reparam(mu, lv, eps, dt=F32), R.ref_reparam(mu, lv, eps), 1e-5, 1e-9), "z")
        fails(R.gate_rel(R.ref_reparam(mu, 2 * lv, eps), R.ref_reparam(mu, lv, eps), 1e-5, 1e-9), "exp(lv)")
        for beta in (0.0, 1.0):
            ref = R.ref_reparam_bwd(lv, eps, dz, dmu0, dlv0, beta)
            got = R.ref_reparam_bwd(lv, eps, dz, dmu0, dlv0, beta, dt=F32)
            for a, b in zip(got, ref):
                passes(R.gate_rel(a, b, 1e-5, 1e-9, ref32=a), f"reparam_bwd beta={beta}")
            m = R.ref_reparam_bwd(2 * lv, eps, dz, dmu0, dlv0, beta)
            fails(R.gate_rel(m[1], ref[1], 1e-5, 1e-9, ref32=got[1]), "dlv with exp(lv)")
        r0, r1 = R.ref_reparam_bwd(lv, eps, dz, dmu0, dlv0, 0.0), R.ref_reparam_bwd(lv, eps, dz, dmu0, dlv0, 1.0)
        fails(R.gate_rel(r0[0], r1[0], 1e-5, 1e-9), "beta ignored")


@pytest.mark.parametrize("fb", R.KL_FREE_BITS)
@pytest.mark.parametrize("shape", R.KL_SHAPES, ids=str)
def test_kl_gates(shape, fb):
    mu, lv = R.kl_inputs(*shape, fb, plant_tie=fb > 0)
    ref = R.ref_kl(mu, lv, fb)
    passes(R.gate_rel(R.ref_kl(mu, lv, fb, dt=F32), ref, 1e-6), "kl fp32 terms")
    dmu0, dlv0 = R.kl_inputs(*shape, 0.0, seed=5)
    for beta in (0.0, 1.0):
        rm, rl = R.ref_kl_bwd(mu, lv, fb, 0.7, dmu0, dlv0, beta)
        gm, gl = R.ref_kl_bwd(mu, lv, fb, 0.7, dmu0, dlv0, beta, dt=F32)
        passes(R.gate_rel(gm, rm, 1e-5, 1e-9, ref32=gm), "dmu fp32")
        passes(R.gate_rel(gl, rl, 1e-5, 1e-9, ref32=gl), "dlv fp32")
        if shape[0] > 1:
            ml = R.ref_kl_bwd(mu, lv, fb, 0.7 * shape[0] / (shape[0] + 1), dmu0, dlv0, beta)[1]
            fails(R.gate_rel(ml, rl, 1e-5, 1e-9, ref32=gl), "dlv over B + 1")
        if fb > 0:
            assert abs(rm.flat[0] - beta * dmu0.flat[0] - 0.5 * 0.7 / shape[0]) < 1e-15  # tie weight 0.5
            mm, _ = R.ref_kl_bwd(mu, lv, fb, 0.7, dmu0, dlv0, beta, mutant="tie_weight_1")
            fails(R.gate_rel(mm, rm, 1e-5, 1e-9, ref32=gm), "tie weight 1")


def test_kl_inputs_stay_off_the_tie():
    for shape in R.KL_SHAPES:
        mu, lv = R.kl_inputs(*shape, 0.5, plant_tie=True)
        kd = R._kl_dim(mu.astype(F64), lv.astype(F64)).reshape(-1)
        assert kd[0] == 0.5 and (np.abs(kd[1:] - 0.5) >= 1e-3).all()
        kd32 = (F32(0.5) * (mu * mu + np.exp(lv) - F32(1) - lv)).reshape(-1)
        assert kd32[0] == F32(0.5)
        if kd.size > 100:
            assert (kd[1:] > 0.5).any() and (kd[1:] < 0.5).any()


# ------------------------------------------------------------------------------------ data path
def test_cond_inputs_gate():
    t = np.array([0.0, 1e-3, 1.0, 0.37], dtype=F32)
    y_cat = np.array([-1, 0, 4, 7], dtype=np.int64)
    y_cont = R.f32(R.rng(3).standard_normal((4, 4)))
    for E in (2, 3, 7, 128):
        te, yv, yc = R.ref_cond_inputs(t, y_cat, y_cont, E, 4)
        te32, yv32, _ = R.ref_cond_inputs(t, y_cat, y_cont, E, 4, dt=F32)
        passes(R.gate_abs(te32, te, 1e-6), "te fp32")
        passes(R.gate_abs(yv32, yv, 1e-6), "yv fp32")
        fails(R.gate_abs(R.ref_cond_inputs(t, y_cat, y_cont, E, 4, mutant="no_2pi")[0], te, 1e-6), "no 2 pi")
        assert np.isfinite(te).all() and (E % 2 == 0 or (te[:, -1] == 0).all())
        assert yc.tolist() == [0, 0, 4, 4]


def test_prior_temb_and_qsample_gates():
    t = np.array([0, 999, 17], dtype=np.int64)
    for E in (2, 7, 64):
        fr = R.prior_freqs(E)
        te = R.ref_prior_temb(t, fr, E)
        passes(R.gate_abs(R.ref_prior_temb(t, fr, E, dt=F32), te, 1e-6), "prior temb fp32")
        fails(R.gate_abs(np.roll(te, E // 2, 1) if E % 2 == 0 else te[:, ::-1], te, 1e-6), "sin and cos swapped")
    r = R.rng(5)
    u = np.array([0.0, 0.3, 1.0], dtype=F32)
    for HW in (1, 257):
        x0, eps = R.f32(r.random((3, HW))), R.f32(r.standard_normal((3, HW)))
        for tp in (1.0, 2.0, 0.5):
            t64, xt = R.ref_qsample_vp(x0, eps, u, tp, 0.1, 14.95)
            t32, xt32 = R.ref_qsample_vp(x0, eps, u, tp, 0.1, 14.95, dt=F32)
            passes(R.gate_rel(t32, t64, 1e-5, 1e-9), "t")
            passes(R.gate_rel(xt32, xt, 1e-5, 1e-9, ref32=xt32), "x_t fp32")
            assert t64[0] == 0 and abs(xt[0, 0] - ((2 * float(x0[0, 0]) - 1) + np.sqrt(float(F32(1e-8))) * eps[0, 0])) < 1e-12
            m = R.ref_qsample_vp(x0, eps, u, 1.0 if tp != 1.0 else 2.0, 0.1, 14.95)[1]
            fails(R.gate_rel(m, xt, 1e-5, 1e-9, ref32=xt32), "wrong t_power")


def test_prior_qsample_reference_clamps_and_truncates():
    T = 1000
    u = np.array([0.0, 0.5, 1.0, 0.99999994], dtype=F32)
    sab = R.f32(np.linspace(1.0, 0.1, T))
    s1 = R.f32(np.sqrt(1 - sab.astype(F64) ** 2))
    r = R.rng(2)
    z0, eps = R.f32(r.standard_normal((4, 5))), R.f32(r.standard_normal((4, 5)))
    t, zt = R.ref_prior_qsample(z0, eps, u, sab, s1, T)
    assert t.tolist() == [0, 250, 999, 999]
    zt32 = R.ref_q_sample(z0, t, eps, sab, s1, dt=F32)
    passes(R.gate_rel(zt32, zt, 1e-5, 1e-9, ref32=zt32), "z_t fp32")
    fails(R.gate_rel(R.ref_q_sample(z0, np.minimum(t + 1, T - 1), eps, sab, s1), zt, 1e-5, 1e-9, ref32=zt32), "t off by one")


def test_first_conv_gates():
    r = R.rng(9)
    for B, C0, nm, ks in ((1, 4, 1, 3), (3, 32, 16, 3)):
        maps, w = R.f32(r.standard_normal((B, nm))), R.f32(r.standard_normal((C0, 1 + nm, ks, ks)))
        bias, S = R.f32(r.standard_normal(C0)), R.f32(r.standard_normal((B, C0)))
        dwx = R.f32(r.standard_normal((C0, ks, ks)))
        bb, bb32 = R.ref_first_conv_bias(maps, w, bias), R.ref_first_conv_bias(maps, w, bias, dt=F32)
        passes(R.gate_rel(bb32, bb, 1e-5, 1e-9, ref32=bb32), "bias_b fp32")
        fails(R.gate_rel(R.ref_first_conv_bias(maps, w, None), bb, 1e-5, 1e-9, ref32=bb32), "bias dropped")
        ref = R.ref_first_conv_bwd(S, maps, w, dwx)
        r32 = R.ref_first_conv_bwd(S, maps, w, dwx, dt=F32)
        for name, a, b in zip(("dmaps", "dw", "db"), r32, ref):
            passes(R.gate_rel(a, b, 1e-5, 1e-9, ref32=a), name)
        if B > 1:
            mm = R.ref_first_conv_bwd(S[:-1], maps[:-1], w, dwx)
            fails(R.gate_rel(mm[1], ref[1], 1e-5, 1e-9, ref32=r32[1]), "dw without the last batch")
            fails(R.gate_rel(mm[2], ref[2], 1e-5, 1e-9, ref32=r32[2]), "db without the last batch")
