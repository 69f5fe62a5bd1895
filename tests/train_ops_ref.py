"""References, inputs and gates for the training-path kernels of csrc/train.hip (no GPU import).

Every reference is written from the formula in the kernel's comment and PyTorch's documented
semantics, and is evaluated in float64 on the float32-rounded inputs the kernel receives.  Most
take `dt` (np.float64 | np.float32): the float32 evaluation shows that a correct fp32 kernel can
meet the gate; and `mutant`, a named deliberate error that the gate has to reject
(tests/test_train_ops_ref_cpu.py).  The GPU tests (tests/test_gpu_train_ops.py) use the same
input builders and the same gates.

Every gate returns (measured error, bound) at the element where error - bound is largest; a
non-finite result counts as an infinite error.  `ok(eb)` is `error <= bound`.
"""
import math

import numpy as np
import torch

F32, F64 = np.float32, np.float64
U24 = 2.0 ** -24


def f32(a):
    return np.ascontiguousarray(a, dtype=F32)


def rng(seed):
    return np.random.default_rng(seed)


# ------------------------------------------------------------------------------------ gates
def _worst(err, bound):
    err = np.asarray(err, dtype=F64)
    bound = np.broadcast_to(np.asarray(bound, dtype=F64), err.shape)
    if err.size == 0:
        return 0.0, 0.0
    err = np.where(np.isfinite(err), err, np.inf)
    i = int(np.argmax(err.reshape(-1) - bound.reshape(-1)))
    return float(err.reshape(-1)[i]), float(bound.reshape(-1)[i])


def _diff(got, ref):
    got, ref = np.asarray(got, dtype=F64), np.asarray(ref, dtype=F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return np.abs(got - ref)


def ok(eb):
    return eb[0] <= eb[1]


FALLBACK = None  # set by the last gate_rel / gate_max call: the float32-reference error if its floor was used


def _f32_floor(ref32, ref, bound):
    """The issue's fallback, per case: where the float32 CPU evaluation of the reference (`ref32`) itself
    misses the stated `bound` against float64, the case's bound becomes at least 4 x that evaluation's
    error (the factor covers another valid fp32 order).  Where it meets the bound, nothing changes.
    Never derived from a kernel's output."""
    global FALLBACK
    FALLBACK = None
    if ref32 is None:
        return 0.0
    e = _diff(ref32, ref)
    if not np.isfinite(e).all() or (e <= bound).all():
        return 0.0
    FALLBACK = float(e.max())
    return 4.0 * FALLBACK


def gate_rel(got, ref, rel, floor=0.0, ref32=None):
    """per element |err| <= rel * |ref| + floor; `ref32`: see _f32_floor"""
    b = rel * np.abs(np.asarray(ref, dtype=F64)) + floor
    return _worst(_diff(got, ref), np.maximum(b, _f32_floor(ref32, ref, b)))


def gate_abs(got, ref, tol):
    return _worst(_diff(got, ref), tol)


def gate_max(got, ref, tol=2e-5, ref32=None):
    """max |err| <= tol * max|ref| of the tensor (the project's 2e-5 without a floor at 1), plus
    1e-12 for the float64 reference's own rounding where the exact result is 0; `ref32`: see _f32_floor"""
    ref = np.asarray(ref, dtype=F64)
    b = tol * (float(np.abs(ref).max()) if ref.size else 0.0) + 1e-12
    return _worst(_diff(got, ref), max(b, _f32_floor(ref32, ref, b)))


def gate_exact(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.count_nonzero(got != ref)), 0.0


def gate_colsum(got, ref, sumabs, beta=0.0, total0=None):
    """fp64 accumulation rounded once to fp32 (+ one rounding of beta*total0 + sum):
    |err| <= 3 * 2^-24 * (|beta*total0| + |ref|) + 1e-12 * sum|x|"""
    ref = np.asarray(ref, dtype=F64)
    pre = np.abs(beta * np.asarray(total0, dtype=F64)) if total0 is not None else 0.0
    return _worst(_diff(got, ref), 3 * U24 * (pre + np.abs(ref)) + 1e-12 * np.asarray(sumabs, dtype=F64))


def gate_upsample_bwd(got, ref, dy):
    """at most 16 fp32 fmas with weights totalling at most 4: |err| <= 5e-6 * max|dy|"""
    return _worst(_diff(got, ref), 5e-6 * float(np.abs(dy).max()))


def gate_softmax_p(got, ref):
    return _worst(_diff(got, ref), 2e-5 * np.asarray(ref, dtype=F64) + 1e-10)


def gate_rowsum(P):
    return _worst(np.abs(np.asarray(P, dtype=F64).sum(-1) - 1.0), 1e-6)


def gate_softmax_ds(got, ref, P, dP):
    P, dP = np.asarray(P, dtype=F64), np.asarray(dP, dtype=F64)
    s = (P * np.abs(dP)).sum(-1, keepdims=True)
    return _worst(_diff(got, ref), 2e-5 * P * (np.abs(dP) + s) + 1e-10)


def gate_embedding(got, ref, sumabs, B):
    """a serial fp32 sum of at most B terms: |err| <= B * 2^-24 * sum|terms|"""
    return _worst(_diff(got, ref), max(B, 1) * U24 * np.asarray(sumabs, dtype=F64))


def gate_ema(got, ref, p, g, d):
    p, g = np.abs(np.asarray(p, dtype=F64)), np.abs(np.asarray(g, dtype=F64))
    return _worst(_diff(got, ref), 2.0 ** -22 * (p * d + g * (1.0 - d)))


def gate_adam_moment(got, ref, slack):
    """1e-6 relative per element, plus `slack` (ref_adam_slack): only for the unfused numpy adam_formula
    of the CPU check; the kernel is held to 1e-6 relative alone"""
    return _worst(_diff(got, ref), 1e-6 * np.abs(np.asarray(ref, dtype=F64)) + slack)


# ------------------------------------------------------------------------------------ column sums
COLSUM_SMALL = [(r, c, b) for r in (1, 7, 8, 9, 4096) for c in (4, 128, 132) for b in (0.0, 0.5)]
COLSUM_PAST_SMALL = (1, 4097, 8)
COLSUM_VEC = [(3, 200, 96), (2, 130, 1028), (33, 64, 8)]
COLSUM_SCALAR = [(2, 200, 1), (2, 200, 6), (2, 200, 258)]  # nsplit 3, uneven; 258 takes two column passes
COLSUM_WIDE = [(1, 16448, 8, False), (1, 70000, 8, False), (2, 20000, 4, True)]


def colsum_input(Bt, HW, C, seed=0):
    return f32(3.0 + rng(1000 + seed).standard_normal((Bt, HW, C)))


def colsum_nsplit(Bt, HW):
    """the split count tcx_colsum picks (train.hip colsum_nsplit)"""
    ns = max(1, -(-2048 // max(Bt, 1)))
    ns = min(ns, max(1, HW // 64))
    return min(ns, 4096)


def ref_colsum(x, dt=F64, mutant=None):
    """x [Bt][HW][C] -> per_batch [Bt][C], total [C], sum|x| per column [C]"""
    x = np.asarray(x)
    Bt, HW, C = x.shape
    xs = x
    if mutant == "drop_last_row":
        xs = x[:, :HW - 1]
    elif mutant == "floor_split":
        ns = colsum_nsplit(Bt, HW)
        xs = x[:, :ns * (HW // ns)]
    elif mutant == "first32":
        xs = x[:32]
    pb = xs.astype(dt).sum(1, dtype=dt)
    if mutant == "first32":
        pb = np.concatenate([pb, x[32:].astype(dt).sum(1, dtype=dt)], 0)
        return pb, pb[:32].sum(0, dtype=dt), np.abs(x).astype(F64).sum((0, 1))
    return pb, pb.sum(0, dtype=dt), np.abs(x).astype(F64).sum((0, 1))


# ------------------------------------------------------------------------------------ GroupNorm
# (Bt, HW, C, groups, silu)
GN_CASES = [(2, 1, 4, 1, 1), (3, 63, 8, 2, 0), (2, 200, 96, 8, 1), (2, 4160, 192, 8, 1), (33, 64, 12, 4, 1),
            (1, 128, 1024, 8, 0)]
GN_EPS = float(np.float32(1e-5))  # the float the kernel receives


def gn_inputs(Bt, HW, C, seed=0, offset=0.0):
    r = rng(2000 + seed)
    x = f32(offset + r.standard_normal((Bt, HW, C)))
    dy = f32(r.standard_normal((Bt, HW, C)))
    gamma = f32(1.0 + 0.5 * r.standard_normal(C))
    beta = f32(0.5 * r.standard_normal(C))
    return x, dy, gamma, beta


def ref_gn_stats(x, gamma, beta, groups, eps=GN_EPS):
    """mean / rstd [Bt][groups] (biased variance) and the tables scale = rstd*gamma,
    shift = beta - mean*scale [Bt][C]"""
    x = np.asarray(x, dtype=F64)
    Bt, HW, C = x.shape
    cpg = C // groups
    xg = x.reshape(Bt, HW, groups, cpg)
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    rstd = 1.0 / np.sqrt(var + eps)
    gm = np.ones(C) if gamma is None else np.asarray(gamma, dtype=F64)
    bt = np.zeros(C) if beta is None else np.asarray(beta, dtype=F64)
    scale = np.repeat(rstd, cpg, 1) * gm
    shift = bt - np.repeat(mean, cpg, 1) * scale
    return mean, rstd, scale, shift


def gn_tables_f32(mean, rstd, gamma, beta):
    """the tables as the kernel documents them, formed in float32 from the float32 mean / rstd:
    scale = rstd*gamma, shift = beta - mean*scale"""
    Bt, groups = mean.shape
    C = gamma.shape[0] if gamma is not None else None
    cpg = (C // groups) if C else 1
    m, r = np.repeat(f32(mean), cpg, 1), np.repeat(f32(rstd), cpg, 1)
    sc = r * (f32(gamma) if gamma is not None else F32(1))
    return sc, ((f32(beta) if beta is not None else F32(0)) - m * sc).astype(F32)


def ref_gn_bwd(x, dy, gamma, beta, groups, silu, eps=GN_EPS, tdt=torch.float64):
    """torch group_norm (+ silu) autograd: dx [Bt][HW][C], dgamma [C], dbeta [C]"""
    Bt, HW, C = x.shape
    xt = torch.from_numpy(np.asarray(x)).to(tdt).permute(0, 2, 1).contiguous().requires_grad_(True)
    g = torch.from_numpy(np.ones(C, F32) if gamma is None else np.asarray(gamma)).to(tdt).requires_grad_(True)
    b = torch.from_numpy(np.zeros(C, F32) if beta is None else np.asarray(beta)).to(tdt).requires_grad_(True)
    y = torch.nn.functional.group_norm(xt, groups, g, b, eps)
    if silu:
        y = torch.nn.functional.silu(y)
    y.backward(torch.from_numpy(np.asarray(dy)).to(tdt).permute(0, 2, 1).contiguous())
    return (xt.grad.permute(0, 2, 1).contiguous().numpy(), g.grad.numpy(), b.grad.numpy())


def _sigmoid(z):
    z = np.asarray(z)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e)).astype(z.dtype)


def gn_bwd_formula(x, dy, gamma, beta, groups, silu, eps=GN_EPS, dt=F64, mutant=None):
    """The closed form the kernels implement (train.hip, GroupNorm backward): dz = dy*act'(z),
    S1 = sum dz, S2 = sum dz*xhat per (b, c); dx = k1*dz + k2*x + k3."""
    x, dy = np.asarray(x, dtype=dt), np.asarray(dy, dtype=dt)
    Bt, HW, C = x.shape
    cpg = C // groups
    gm = (np.ones(C) if gamma is None else np.asarray(gamma)).astype(dt)
    bt = (np.zeros(C) if beta is None else np.asarray(beta)).astype(dt)
    xg = x.reshape(Bt, HW, groups, cpg)
    mean = xg.mean((1, 3), dtype=dt)
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3), dtype=dt)
    rstd = (1.0 / np.sqrt(var + dt(eps))).astype(dt)
    mu_c, rs_c = np.repeat(mean, cpg, 1)[:, None, :], np.repeat(rstd, cpg, 1)[:, None, :]
    xh = (x - mu_c) * rs_c
    z = xh * gm + bt
    if silu:
        s = _sigmoid(z)
        dz = dy * (s * (1 + z * (1 - s)))
    else:
        dz = dy
    S1 = dz.sum(1, dtype=dt)
    S2 = (dz * xh).sum(1, dtype=dt)
    n = dt(HW * cpg - (1 if mutant == "n_minus_1" else 0))
    A = (gm * S1).reshape(Bt, groups, cpg).sum(2, dtype=dt)
    Bg = (gm * S2).reshape(Bt, groups, cpg).sum(2, dtype=dt)
    a2, a3 = -rstd * A / n, -rstd * Bg / n
    k1 = rs_c * gm
    k2 = np.repeat(a3 * rstd, cpg, 1)[:, None, :]
    k3 = np.repeat(a2 - a3 * rstd * mean, cpg, 1)[:, None, :]
    if mutant == "no_k3":
        k3 = 0 * k3
    dx = k1 * dz + k2 * x + k3
    nb = 32 if mutant == "first32" else Bt
    return dx.astype(dt), S2[:nb].sum(0, dtype=dt), S1[:nb].sum(0, dtype=dt)


# ------------------------------------------------------------------------------------ upsample x2
UPS_CASES = [(1, 1, 1, 4), (2, 1, 5, 4), (2, 5, 1, 8), (2, 3, 7, 12), (1, 16, 4, 4)]


def ups_inputs(Bt, H, W, C, seed=0):
    r = rng(3000 + seed)
    return f32(r.standard_normal((Bt, H, W, C))), f32(r.standard_normal((Bt, 2 * H, 2 * W, C)))


def ref_upsample(x, tdt=torch.float64):
    xt = torch.from_numpy(np.asarray(x)).to(tdt).permute(0, 3, 1, 2)
    y = torch.nn.functional.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=False)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def ref_upsample_bwd(dy, tdt=torch.float64):
    """adjoint of F.interpolate(scale_factor=2, bilinear, align_corners=False); dy [Bt][2H][2W][C]"""
    Bt, Ho, Wo, C = dy.shape
    xt = torch.zeros((Bt, C, Ho // 2, Wo // 2), dtype=tdt, requires_grad=True)
    y = torch.nn.functional.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=False)
    y.backward(torch.from_numpy(np.asarray(dy)).to(tdt).permute(0, 3, 1, 2))
    return xt.grad.permute(0, 2, 3, 1).contiguous().numpy()


def _up_matrix(n, dt, clamp=True):
    """[2n][n]: output row d takes (1-l) * in[i0] + l * in[i1], src = max(0, (d+0.5)/2 - 0.5)"""
    U = np.zeros((2 * n, n), dtype=dt)
    for d in range(2 * n):
        s = 0.5 * (d + 0.5) - 0.5
        if clamp:
            s = max(s, 0.0)
            i0 = int(s)
            i1 = i0 + (1 if i0 < n - 1 else 0)
            U[d, i0] += 1.0 - (s - i0)
            U[d, i1] += s - i0
        else:  # taps outside the image are dropped instead of clamped to the edge
            i0 = math.floor(s)
            for i, wt in ((i0, 1.0 - (s - i0)), (i0 + 1, s - i0)):
                if 0 <= i < n:
                    U[d, i] += wt
    return U


def upsample_bwd_formula(dy, dt=F64, mutant=None):
    dy = np.asarray(dy, dtype=dt)
    Bt, Ho, Wo, C = dy.shape
    H, W = Ho // 2, Wo // 2
    if mutant == "swap_hw":
        H, W = W, H
        dy = dy.reshape(Bt, 2 * H, 2 * W, C)
    UH, UW = _up_matrix(H, dt, mutant != "no_clamp"), _up_matrix(W, dt, mutant != "no_clamp")
    dx = np.einsum("yh,byxc,xw->bhwc", UH, dy, UW).astype(dt)
    return dx.reshape(Bt, Ho // 2, Wo // 2, C) if mutant == "swap_hw" else dx


# ------------------------------------------------------------------------------------ softmax rows
SOFTMAX_CASES = [(1, 1), (3, 63), (5, 64), (4, 65), (7, 257), (2, 1024), (9, 1500)]
SOFTMAX_FAMILIES = ("randn", "peaked", "const", "offset")


def softmax_input(rows, n, family, seed=0):
    r = rng(4000 + seed).standard_normal((rows, n))
    S = {"randn": r, "peaked": 30.0 * r, "const": np.full((rows, n), 0.75), "offset": r + 1e4}[family]
    return f32(S), f32(rng(4100 + seed).standard_normal((rows, n)))


def ref_softmax(S, dt=F64, mutant=None):
    S = np.asarray(S, dtype=dt)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(S if mutant == "no_max" else S - S.max(-1, keepdims=True))
        return (e / e.sum(-1, keepdims=True, dtype=dt)).astype(dt)


def ref_softmax_bwd(P, dP, dt=F64, mutant=None):
    P, dP = np.asarray(P, dtype=dt), np.asarray(dP, dtype=dt)
    dot = 0 if mutant == "no_dot" else (P * dP).sum(-1, keepdims=True, dtype=dt)
    return (P * (dP - dot)).astype(dt)


# ------------------------------------------------------------------------------------ activations
ACT_SIZES = (1, 255, 257, 8192 * 256 + 3)
ACT_PLANTED = (0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0)


def act_inputs(n, seed=0):
    r = rng(5000 + seed)
    z, dy = f32(r.standard_normal(n)), f32(r.standard_normal(n))
    if n >= 255:
        for i, v in enumerate(ACT_PLANTED):
            z[i * 31] = v
    return z, dy


def ref_act_fwd(z, act, dt=F64):
    z = np.asarray(z, dtype=dt)
    if act == 1:
        return np.maximum(z, 0)
    s = _sigmoid(z)
    return s if act == 2 else z * s


def ref_act_bwd(z, dy, act, dt=F64, mutant=None):
    z, dy = np.asarray(z, dtype=dt), np.asarray(dy, dtype=dt)
    if act == 1:
        return np.where(z > 0, dy, 0).astype(dt)
    s = _sigmoid(z)
    if act == 2:
        return dy * (s * (1 - s))
    return dy * s if mutant == "no_z_term" else dy * (s * (1 + z * (1 - s)))


# ------------------------------------------------------------------------------------ MSE
MSE_SIZES = (1, 257, 1024 * 256 + 5)
MSE_BWD_STRIDE_SIZE = 8192 * 256 + 3  # k_mse_bwd's grid cap: its second stride


def mse_inputs(n, seed=0):
    r = rng(6000 + seed)
    return f32(r.standard_normal(n)), f32(r.standard_normal(n))


def ref_mse(a, b, dt=F64):
    d = np.asarray(a, dtype=dt) - np.asarray(b, dtype=dt)
    return (d * d).mean(dtype=dt)


def ref_mse_bwd(a, b, g, dt=F64, mutant=None):
    n = a.size + (1 if mutant == "n_plus_1" else 0)
    return (dt(2.0) * dt(g) / dt(n)) * (np.asarray(a, dtype=dt) - np.asarray(b, dtype=dt))


# ------------------------------------------------------------------------------------ embedding
def ref_embedding_bwd(idx, dout, rows, dt=F64):
    """dW[r] = sum of dout[b] over idx[b] == r, and the sum of |terms|"""
    B, E = dout.shape
    dW, sa = np.zeros((rows, E), dtype=dt), np.zeros((rows, E), dtype=F64)
    for b in range(B):  # in batch order, as the kernel's serial loop
        dW[idx[b]] = dW[idx[b]] + dout[b].astype(dt)
        sa[idx[b]] += np.abs(dout[b]).astype(F64)
    return dW, sa


# ------------------------------------------------------------------------------------ LayerNorm + FiLM
LN_CASES = [(2, 1), (3, 7), (6, 64), (2, 255), (2, 257), (2, 1024)]
LN_EPS = float(np.float32(1e-5))


def ln_inputs(M, Wd, ld_gb=0, seed=0, offset=0.0):
    r = rng(7000 + seed)
    x = f32(offset + r.standard_normal((M, Wd)))
    dh = f32(r.standard_normal((M, Wd)))
    w = f32(1.0 + 0.5 * r.standard_normal(Wd))
    b = f32(0.5 * r.standard_normal(Wd))
    gb = f32(0.5 * r.standard_normal((M, ld_gb))) if ld_gb else None
    return x, dh, w, b, gb


def ln_stats_f32(x, eps=LN_EPS):
    """the float32 mean / rstd rows that tcx_ln_bwd receives (float64 statistics rounded once)"""
    x = np.asarray(x, dtype=F64)
    mean = x.mean(1)
    return f32(mean), f32(1.0 / np.sqrt(((x - mean[:, None]) ** 2).mean(1) + eps))


def ref_ln(x, dh, w, b, gb, eps=LN_EPS, dt=F64, mutant=None, stats=None):
    """y = l*(1+gm)+bt, l = xhat*w + b; returns dict(y, mean, rstd, dx, dwrow, dbrow, dgb).  `stats`:
    the (mean, rstd) float32 rows the backward kernel is given; the backward is then evaluated on
    them, as on every other float32 input."""
    x, dh, w, b = (np.asarray(a, dtype=dt) for a in (x, dh, w, b))
    M, Wd = x.shape
    mean = x.mean(1, dtype=dt)
    var = ((x - mean[:, None]) ** 2).mean(1, dtype=dt)
    rstd = (1.0 / np.sqrt(var + dt(eps))).astype(dt)
    if stats is not None:
        mean, rstd = np.asarray(stats[0], dtype=dt), np.asarray(stats[1], dtype=dt)
    xh = (x - mean[:, None]) * rstd[:, None]
    l = xh * w + b
    out = dict(mean=mean, rstd=rstd)
    dl = dh
    if gb is not None:
        gm, bt = np.asarray(gb[:, :Wd], dtype=dt), np.asarray(gb[:, Wd:2 * Wd], dtype=dt)
        out["y"] = l * (1 + gm) + bt
        out["dgb"] = np.concatenate([dh * l, dh], 1)
        dl = dh * (1 + gm)
    else:
        out["y"] = l
    dxh = dl * w
    m1 = dxh.mean(1, dtype=dt)[:, None]
    m2 = (dxh * xh).mean(1, dtype=dt)[:, None]
    if mutant == "no_m2":
        m2 = 0 * m2
    out.update(dx=rstd[:, None] * (dxh - m1 - xh * m2), dwrow=dl * xh, dbrow=dl * np.ones_like(xh))
    return out


def ref_ln_dx_autograd(x, dh, w, b, gb, eps=LN_EPS):
    """dx of the same map from torch float64 layer_norm autograd (cross-check of ref_ln)"""
    Wd = x.shape[1]
    xt = torch.from_numpy(np.asarray(x)).double().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xt, (Wd,), torch.from_numpy(w).double(), torch.from_numpy(b).double(), eps)
    if gb is not None:
        g = torch.from_numpy(gb).double()
        y = y * (1 + g[:, :Wd]) + g[:, Wd:2 * Wd]
    y.backward(torch.from_numpy(dh).double())
    return xt.grad.numpy()


# ------------------------------------------------------------------------------------ Adam / EMA
def _f(v):
    return float(F32(v))


# test_adam_matches_torch_adam's hyper-parameters, as the floats the C ABI receives (tcx_adam takes
# float lr / betas / eps / weight_decay: 1 - 0.99f and 1 - 0.99 differ by 9.5e-7 relative)
ADAM_HP = dict(lr=_f(3e-3), betas=(_f(0.8), _f(0.99)), eps=_f(1e-6))
ADAM_NT = (1, 48, 49, 97)
ADAM_BIG = 1024 * 256 + 3
EMA_DECAY = float(F32(0.999))


def adam_sizes(nt):
    """1, 255, 257 in turn, and one tensor past the capped grid (the last of the first chunk)"""
    s = [(1, 255, 257)[i % 3] for i in range(nt)]
    s[min(nt, 48) - 1] = ADAM_BIG
    return s


def adam_inputs(nt, step, seed=0):
    r = rng(8000 + seed)
    out = []
    for n in adam_sizes(nt):
        p, g = f32(r.standard_normal(n)), f32(r.standard_normal(n))
        if step == 1:
            m, v = np.zeros(n, F32), np.zeros(n, F32)
        else:
            m, v = f32(0.3 * r.standard_normal(n)), f32(0.5 + r.random(n))
        out.append((p, g, m, v))
    return out


def ref_adam(tensors, step, wd):
    """one torch.optim.Adam step (CPU fp32) at step number `step`: lists of p, exp_avg, exp_avg_sq"""
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p, _, _, _ in tensors]
    opt = torch.optim.Adam(ps, weight_decay=_f(wd), **ADAM_HP)
    for q, (_, g, m, v) in zip(ps, tensors):
        q.grad = torch.from_numpy(g.copy())
        opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(m.copy()),
                            exp_avg_sq=torch.from_numpy(v.copy()))
    opt.step()
    return ([q.detach().numpy() for q in ps], [opt.state[q]["exp_avg"].numpy() for q in ps],
            [opt.state[q]["exp_avg_sq"].numpy() for q in ps])


def ref_adam_slack(p, g, m, wd):
    """What torch's own fp32 step leaves open in (exp_avg, exp_avg_sq): ATen rounds the products of
    g + wd*p and of m + w*(g - m) before the add in its scalar loops and fuses them (fma) in its
    vector loops, so two correct fp32 evaluations differ by up to an ulp of g_eff, dg = 2^-23 (|g| +
    wd |p|), and by one rounding of w*(g - m).  exp_avg: w1 (dg + 2^-23 (|g_eff| + |m|));
    exp_avg_sq = v*b2 + w2*g_eff^2: w2 * 2 |g_eff| dg."""
    b1, b2 = ADAM_HP["betas"]
    ge = np.abs(g.astype(F64)) + wd * np.abs(p.astype(F64))
    dg = 2.0 ** -23 * ge if wd else 0.0 * ge
    return (1.0 - b1) * (dg + 2.0 ** -23 * (ge + np.abs(m.astype(F64)))), (1.0 - b2) * 2.0 * ge * dg


def adam_formula(p, g, m, v, step, wd, mutant=None):
    """torch/optim/adam.py's single-tensor step written out in float32"""
    b1, b2 = ADAM_HP["betas"]
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    if mutant == "no_bias_correction":
        bc1 = bc2 = 1.0
    g = (g + F32(wd) * p).astype(F32) if wd else g
    w1 = F32(1.0 - b1)
    m = (m + w1 * (g - m)).astype(F32)
    v = (v * F32(b2) + (F32(1.0 - b2) * g) * g).astype(F32)
    denom = (np.sqrt(v) / F32(math.sqrt(bc2)) + F32(ADAM_HP["eps"])).astype(F32)
    return (p + (F32(-(ADAM_HP["lr"] / bc1)) * m) / denom).astype(F32), m, v


def ref_ema(p, g, d=EMA_DECAY, dt=F64, mutant=None):
    p, g = np.asarray(p, dtype=dt), np.asarray(g, dtype=dt)
    d = dt(d)
    if mutant == "swapped":
        return p * (1 - d) + d * g
    return p * d + (1 - d) * g


# ------------------------------------------------------------------------------------ VAE ops
REPARAM_SIZES = (1, 257)
KL_SHAPES = [(1, 1), (5, 51), (4, 32), (8, 125)]  # B*Z = 1, 255, 128, 1000
KL_FREE_BITS = (0.0, 0.5)


def reparam_inputs(n, seed=0):
    r = rng(9000 + seed)
    return tuple(f32(r.standard_normal(n)) for _ in range(6))  # mu, lv, eps, dz, dmu0, dlv0


def ref_reparam(mu, lv, eps, dt=F64):
    return np.asarray(mu, dtype=dt) + np.exp(dt(0.5) * np.asarray(lv, dtype=dt)) * np.asarray(eps, dtype=dt)


def ref_reparam_bwd(lv, eps, dz, dmu0, dlv0, beta, dt=F64):
    lv, eps, dz = (np.asarray(a, dtype=dt) for a in (lv, eps, dz))
    dl = dz * eps * (dt(0.5) * np.exp(dt(0.5) * lv))
    return dt(beta) * np.asarray(dmu0, dtype=dt) + dz, dt(beta) * np.asarray(dlv0, dtype=dt) + dl


def _kl_dim(mu, lv):
    return 0.5 * (mu * mu + np.exp(lv) - 1 - lv)


def kl_inputs(B, Z, fb, seed=0, plant_tie=False):
    """mu, lv [B][Z]; with plant_tie the first element is (1, 0): kl_dim is exactly 0.5 in fp32
    and fp64.  Every other element is kept at least 1e-3 away from kl_dim == fb."""
    r = rng(9500 + seed)
    mu, lv = f32(r.standard_normal((B, Z))), f32(0.7 * r.standard_normal((B, Z)))
    if fb > 0:
        for _ in range(100):
            near = np.abs(_kl_dim(mu.astype(F64), lv.astype(F64)) - fb) < 1e-3
            if not near.any():
                break
            mu[near] = f32(mu[near] + 0.01)
    if plant_tie:
        mu.flat[0], lv.flat[0] = 1.0, 0.0
    return mu, lv


def ref_kl(mu, lv, fb, dt=F64):
    """{mean_b sum_d max(kl_dim, fb) (fb > 0), mean_b sum_d kl_dim}"""
    kd = _kl_dim(np.asarray(mu, dtype=dt), np.asarray(lv, dtype=dt))
    used = np.maximum(kd, dt(fb)) if fb > 0 else kd
    B = mu.shape[0]
    return np.array([used.sum(dtype=dt) / B, kd.sum(dtype=dt) / B], dtype=dt)


def ref_kl_bwd(mu, lv, fb, g, dmu0, dlv0, beta, dt=F64, mutant=None):
    """grad of g * kl_used; torch.maximum passes 1 where kl_dim > fb, 0.5 on a tie, 0 below"""
    mu, lv = np.asarray(mu, dtype=dt), np.asarray(lv, dtype=dt)
    w = np.ones_like(mu)
    if fb > 0:
        kd = _kl_dim(mu, lv)
        tie = 1.0 if mutant == "tie_weight_1" else 0.5
        w = np.where(kd > fb, 1.0, np.where(kd == dt(fb), tie, 0.0)).astype(dt)
    s = dt(g) / dt(mu.shape[0])
    gm, gl = s * w * mu, s * w * dt(0.5) * (np.exp(lv) - 1)
    return dt(beta) * np.asarray(dmu0, dtype=dt) + gm, dt(beta) * np.asarray(dlv0, dtype=dt) + gl


def ref_vae_yvec(y_cat, y_cont, keep_u, cond_drop, n_types):
    B = y_cat.shape[0]
    oh = (y_cat[:, None] == np.arange(n_types)[None, :]).astype(F32)
    out = np.concatenate([oh, y_cont.reshape(B, -1)], 1).astype(F32)
    if keep_u is not None:
        out = out * (keep_u >= F32(cond_drop)).astype(F32)[:, None]
    return out


# ------------------------------------------------------------------------------------ data path
def ref_cond_inputs(t, y_cat, y_cont, E, n_types, dt=F64, mutant=None):
    """te = [cos | sin]((2 pi t) * freqs), freqs = exp(-ln(1e4) k / max(half-1, 1)); odd E leaves the
    last column 0.  The argument is formed in float32 as the kernel documents; cos/sin in `dt`."""
    t = np.asarray(t, dtype=F32)
    B, half = t.shape[0], E // 2
    k = np.arange(half, dtype=F32)
    fr = np.exp((F32(-9.210340371976184) * k) / F32(max(half - 1, 1)), dtype=F64).astype(F32)
    # fr is exp() of a float32 argument, rounded to float32 (the kernel's expf)
    tp = F32(1.0) if mutant == "no_2pi" else F32(6.283185307179586)
    arg = ((tp * t)[:, None] * fr[None, :]).astype(F32)
    te = np.zeros((B, E), dtype=dt)
    te[:, :half] = np.cos(arg.astype(dt))
    te[:, half:2 * half] = np.sin(arg.astype(dt))
    yv = np.asarray(y_cont, dtype=dt).copy()
    th = np.asarray(y_cont[:, 1], dtype=dt)
    yv[:, 1] = np.sin(th)
    yv[:, 2] = np.cos(np.sin(th))
    return te, yv, np.clip(y_cat, 0, n_types).astype(np.int64)


def prior_freqs(E):
    half = E // 2
    return torch.exp(-torch.linspace(0, math.log(10000.0), half)).numpy().astype(F32)


def ref_prior_temb(t, freqs, E, dt=F64):
    """[sin | cos](t * freqs), argument formed in float32"""
    half = E // 2
    arg = (t.astype(F32)[:, None] * freqs[None, :half]).astype(F32)
    te = np.zeros((t.shape[0], E), dtype=dt)
    te[:, :half] = np.sin(arg.astype(dt))
    te[:, half:2 * half] = np.cos(arg.astype(dt))
    return te


def ref_qsample_vp(x0, eps, u, t_power, bmin, c2, dt=F64):
    """t = u^p; ib = bmin t + c2 t^2; a = exp(-ib/2); s = sqrt(max(1-a^2, 1e-8)); x_t = a(2 x0 - 1) + s eps.
    Returns t, x_t."""
    u = np.asarray(u, dtype=dt)
    t = u if t_power == 1.0 else (u * u if t_power == 2.0 else np.power(u, dt(t_power)))
    ib = dt(bmin) * t + dt(c2) * (t * t)
    a = np.exp(dt(-0.5) * ib)
    s = np.sqrt(np.maximum(1 - a * a, dt(F32(1e-8))))
    return t, a[:, None] * (np.asarray(x0, dtype=dt) * 2 - 1) + s[:, None] * np.asarray(eps, dtype=dt)


def ref_cond_drop(y_cat, y_cont, r, p, n_types):
    d = np.zeros(y_cat.shape[0], bool) if r is None else (r < F32(p))
    return np.where(d, n_types, y_cat).astype(np.int64), np.where(d[:, None], F32(0), y_cont).astype(F32)


def ref_prior_qsample(z0, eps, u, sab, s1mab, T, dt=F64):
    """t = clamp(trunc(u*u*T), 0, T-1) with u*u*T formed in float32; z_t = sab[t] z0 + s1mab[t] eps"""
    u = np.asarray(u, dtype=F32)
    t = np.clip(((u * u).astype(F32) * F32(T)).astype(F32).astype(np.int64), 0, T - 1)
    return t, ref_q_sample(z0, t, eps, sab, s1mab, dt)


def ref_q_sample(z0, t, eps, sab, s1mab, dt=F64):
    return (np.asarray(sab, dtype=dt)[t][:, None] * np.asarray(z0, dtype=dt)
            + np.asarray(s1mab, dtype=dt)[t][:, None] * np.asarray(eps, dtype=dt))


def ref_first_conv_bias(maps, w, bias, dt=F64):
    """bias_b[b][co] = bias[co] + sum_c maps[b][c] * sum_tap w[co][1+c][tap]"""
    ws = np.asarray(w, dtype=dt)[:, 1:].sum((2, 3), dtype=dt)  # [C0][nm]
    bb = np.zeros(w.shape[0], dtype=dt) if bias is None else np.asarray(bias, dtype=dt)
    m = np.asarray(maps, dtype=dt)
    return bb[None] + m @ ws.T


def ref_first_conv_bwd(S, maps, w, dwx, dt=F64):
    """dmaps [B][nm], dw [C0][1+nm][ks][ks], db [C0]"""
    S, m, wd = np.asarray(S, dtype=dt), np.asarray(maps, dtype=dt), np.asarray(w, dtype=dt)
    C0, nm1, ks, _ = w.shape
    ws = wd[:, 1:].sum((2, 3), dtype=dt)
    dmaps = S @ ws
    dw = np.zeros(w.shape, dtype=dt)
    dw[:, 0] = np.asarray(dwx, dtype=dt).reshape(C0, ks, ks)
    dw[:, 1:] = (S.T @ m)[:, :, None, None]
    return dmaps, dw, S.sum(0, dtype=dt)
