"""GPU: the training-path kernels of csrc/train.hip through the C ABI, at the shapes where their
dispatch changes, against the float64 references of tests/train_ops_ref.py (the gates are stated
there and proved able to fail in tests/test_train_ops_ref_cpu.py).

Every output and workspace lives inside a larger buffer filled with the byte 0x7b (0x7b7b7b7b as a
word: a finite float) with at least 64 elements of it on both sides; after the calls the bytes
around the buffer must be untouched, and an output element the kernel never wrote still holds the
pattern (1.3e36) and fails its gate.  Kernels whose header claims fixed-order reductions run twice
and must agree bit for bit.  Each test prints measured error against bound (pytest -s).

Branches reached here and nowhere else in the suite: k_colsum_fold_wide (nsplit > 256), the second
column pass of k_colsum_part (vector and scalar), its scalar form on a misaligned pointer, beta != 0,
the second trip of the b += 32 / sp += 32 loops of k_gn_bwd_affine, k_colsum_total and k_colsum_fold,
the second grid stride of k_adam, k_ema, k_act_*, k_sqdiff_part and k_mse_bwd, the 48-tensor chunking,
non-square and one-pixel-wide upsample backward, softmax rows off a multiple of 64.
Not reached: k_colsum_fold with nsplit > 256, which needs Bt*C > 65535 at nsplit > 256, more than
4 GB of input.

Gates are the stated ones.  A per-element relative gate cannot hold where the output is a difference
of rounded terms and the element is near 0; a gate given `ref32` (the float32 CPU evaluation of the
reference) becomes 4 x that evaluation's worst error in exactly the cases where that evaluation itself
misses the stated gate (train_ops_ref._f32_floor), and stays as stated in all others.  Those cases,
with the float32 reference's error and the error measured on the MI355X:
  gn_stats shift (33, 64, 12, 4, 1), beta - mean*scale ............ 8.4e-8   2.7e-8
  act_bwd sigmoid' n = 255 / 257 / 8192*256+3, s(1-s) at z = +20 .. 5.7e-8 / 7.3e-8 / 2.1e-7   3.4e-9 / 2.5e-9 / 1.5e-7
  act_bwd SiLU' n = 8192*256+3, 1 + z(1-s) near z = -1.28 ......... 6.2e-7   6.9e-8
  reparam_bwd dlv n = 257, beta = 1, beta*old + new ............... 1.7e-7   6.4e-8
  vae_kl_bwd dlv, exp(l) - 1 near l = 0: (5, 51), (4, 32) fb 0 beta 0;
    (8, 125) fb 0 beta 0 / 1 and fb 0.5 beta 0 ..................... 2.2e-8 to 8.3e-8   2.7e-9 to 1.5e-8
  qsample_vp x_t HW = 257, t_power 1 / 2, a(2 x0 - 1) + s eps ...... 2.8e-7 / 3.6e-7   3.9e-8 / 2.8e-7
  ddim_step last = 0 .............................................. 6.4e-7   1.6e-7
  first_conv_bias (3, 32, 16, 3), bias given / NULL, 16-term sums . 3.1e-6 / 3.2e-6   1.1e-6 / 1.3e-6
Every other case, LayerNorm and the x = 100 + randn GroupNorm included, holds the stated gate."""
import numpy as np
import pytest
import torch

import train_ops_ref as R
from test_gpu_ops import L, chk, dev, st
from train_ops_ref import F32, F64

pytestmark = pytest.mark.gpu

PAT = 0x7B


def P(t):
    """device address of a tensor (None -> NULL); valid for an empty view too"""
    if t is None:
        return None
    return t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()


class Arena:
    """Outputs and workspaces with canaries: each buffer sits between two runs of 0x7b bytes."""

    def __init__(self):
        self.bufs = []

    def new(self, n, dtype=torch.float32, init=None, shift=0):
        isz = torch.empty((), dtype=dtype).element_size()
        pad = max(64 * isz, 256)
        raw = torch.full((pad + shift + n * isz + pad,), PAT, dtype=torch.uint8, device="cuda")
        view = raw[pad + shift:pad + shift + n * isz].view(dtype)
        if init is not None:
            view.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)).to(dtype))
        self.bufs.append((raw, pad + shift, n * isz))
        return view

    def check(self):
        for raw, lo, nb in self.bufs:
            assert bool((raw[:lo] == PAT).all()) and bool((raw[lo + nb:] == PAT).all()), "a canary was overwritten"


def cpu(t, shape=None):
    a = t.cpu().numpy()
    return a if shape is None else a.reshape(shape)


def bits(t):
    return t.cpu().numpy().tobytes()


def idev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def gate(what, eb):
    fb = f"  [float32 reference misses the stated gate: its err {R.FALLBACK:.3e}, bound 4x that]" if R.FALLBACK else ""
    R.FALLBACK = None
    print(f"  {what}: err {eb[0]:.3e} bound {eb[1]:.3e}{fb}")
    assert R.ok(eb), f"{what}: err {eb[0]:.3e} > bound {eb[1]:.3e}"


def last_error():
    return L().tcx_last_error().decode(errors="replace")


# ------------------------------------------------------------------------------------ tcx_colsum
def run_colsum(x, want_pb, want_tot, beta=0.0, total0=None, misalign=False):
    """returns (per_batch, total) as numpy (None where not requested); runs twice (determinism)"""
    Bt, HW, C = x.shape
    A = Arena()
    xd = A.new(x.size, init=x, shift=4 if misalign else 0)
    nws = L().tcx_colsum_workspace(Bt, HW, C)
    outs = []
    for _ in range(2):
        ws = A.new(nws, torch.uint8)
        pb = A.new(Bt * C) if want_pb else None
        tot = A.new(C, init=total0) if want_tot else None
        chk(L().tcx_colsum(P(xd), Bt, HW, C, P(pb), P(tot), beta, P(ws), nws, st()))
        outs.append((pb, tot))
    A.check()
    for a, b in zip(*outs):
        assert a is None or bits(a) == bits(b), "tcx_colsum is not deterministic"
    pb, tot = outs[0]
    return (cpu(pb, (Bt, C)) if want_pb else None), (cpu(tot) if want_tot else None)


def check_colsum(x, want_pb, want_tot, beta=0.0, misalign=False, tag=""):
    C = x.shape[2]
    rpb, rtot, sa = R.ref_colsum(x)
    t0 = R.f32(R.rng(7).standard_normal(C)) if beta else None
    pb, tot = run_colsum(x, want_pb, want_tot, beta, t0, misalign)
    if want_pb:
        gate(f"colsum {x.shape}{tag} per_batch", R.gate_colsum(pb, rpb, sa))
    if want_tot:
        ref = rtot + (beta * t0.astype(F64) if beta else 0.0)
        gate(f"colsum {x.shape}{tag} total beta={beta}", R.gate_colsum(tot, ref, sa, beta, t0))


@pytest.mark.parametrize("rows,C,beta", R.COLSUM_SMALL)
def test_colsum_small_path(rows, C, beta):
    """k_colsum_small: Bt = 1, total only, rows <= 4096; C = 132 is 33 quads, two blocks."""
    check_colsum(R.colsum_input(1, rows, C), False, True, beta)


def test_colsum_just_past_the_small_path():
    check_colsum(R.colsum_input(*R.COLSUM_PAST_SMALL), False, True)
    check_colsum(R.colsum_input(*R.COLSUM_PAST_SMALL), False, True, 0.5)


@pytest.mark.parametrize("want", ["both", "per_batch", "total"])
@pytest.mark.parametrize("shape", R.COLSUM_VEC, ids=str)
def test_colsum_vector_path(shape, want):
    """(3, 200, 96): 24 quads, 10 lanes, HW % nsplit != 0; (2, 130, 1028): 257 quads, two column
    passes; (33, 64, 8): second trip of the b += 32 loop of k_colsum_total."""
    check_colsum(R.colsum_input(*shape), want != "total", want != "per_batch", 0.5 if want == "both" else 0.0)


@pytest.mark.parametrize("shape", R.COLSUM_SCALAR, ids=str)
def test_colsum_scalar_path(shape):
    """C % 4 != 0: k_colsum_part<false>; C = 258 takes two column passes."""
    check_colsum(R.colsum_input(*shape), True, True)


def test_colsum_scalar_path_on_a_misaligned_pointer():
    check_colsum(R.colsum_input(2, 200, 8), True, True, misalign=True, tag=" x+4B")
    check_colsum(R.colsum_input(1, 100, 8), False, True, 0.5, misalign=True, tag=" x+4B")  # not the small path


@pytest.mark.parametrize("Bt,HW,C,pb", R.COLSUM_WIDE)
def test_colsum_wide_fold(Bt, HW, C, pb):
    """nsplit > 256 (257 at 16448 rows): k_colsum_fold_wide.  k_colsum_fold with nsplit > 256 needs
    Bt*C > 65535 at the same time, more than 4 GB of input: not reached."""
    assert R.colsum_nsplit(Bt, HW) > 256
    check_colsum(R.colsum_input(Bt, HW, C), pb, True)


def test_colsum_degenerate():
    x = np.zeros((2, 0, 8), F32)
    pb, tot = run_colsum(x, True, True)
    assert (pb == 0).all() and (tot == 0).all()
    _, tot = run_colsum(np.zeros((1, 0, 8), F32), False, True)  # the small path with no rows
    assert (tot == 0).all()
    t0 = R.f32(R.rng(7).standard_normal(8))
    _, tot = run_colsum(np.zeros((0, 5, 8), F32), False, True, 0.5, t0)
    assert (tot == F32(0.5) * t0).all()


def test_colsum_bad_args():
    buf = torch.zeros(1024, device="cuda")
    for args in [(0, 1, 4, 4), (P(buf), -1, 4, 4), (P(buf), 1, 4, 0)]:
        assert L().tcx_colsum(args[0], args[1], args[2], args[3], None, P(buf), 0.0, P(buf), 4096, st()) != 0
    assert L().tcx_colsum(P(buf), 2, 4, 4, None, P(buf), 0.0, P(buf), 16, st()) != 0
    assert "workspace" in last_error()


# ------------------------------------------------------------------------------------ GroupNorm
def run_gn(case, gamma_null=False, offset=0.0, amax=False, const_group=False, bwd=True):
    Bt, HW, C, groups, silu = case
    x, dy, gamma, beta = R.gn_inputs(Bt, HW, C, offset=offset)
    if gamma_null:
        gamma = beta = None
    if const_group:
        x[:, :, :C // groups] = 2.5
    A = Arena()
    xd, dyd = dev(x), dev(dy)
    gd, bd = (dev(gamma), dev(beta)) if gamma is not None else (None, None)
    ns = max(1, min(4, HW // 32))
    part = A.new(Bt * ns * C * 2, torch.float64)
    chk(L().tcx_gn_partials(P(xd), Bt, HW, C, ns, P(part), st()))
    sc, sh, mean, rstd = A.new(Bt * C), A.new(Bt * C), A.new(Bt * groups), A.new(Bt * groups)
    chk(L().tcx_gn_stats(P(part), Bt, HW, C, groups, ns, P(gd), P(bd), R.GN_EPS, P(sc), P(sh), P(mean), P(rstd), st()))
    out = dict(x=x, dy=dy, gamma=gamma, beta=beta, mean=cpu(mean, (Bt, groups)), rstd=cpu(rstd, (Bt, groups)),
               scale=cpu(sc, (Bt, C)), shift=cpu(sh, (Bt, C)))
    if bwd:
        nws = L().tcx_gn_bwd_workspace(Bt, HW, C)
        runs = []
        for _ in range(2):
            ws = A.new(nws, torch.uint8)
            dx = A.new(Bt * HW * C)
            dg, db = (A.new(C), A.new(C)) if not gamma_null else (None, None)
            slot = A.new(1, torch.int32, init=np.zeros(1, np.int32)) if amax else None
            if amax:
                chk(L().tcx_gn_bwd_absmax(P(xd), P(dyd), P(sc), P(sh), P(mean), P(rstd), P(gd), Bt, HW, C, groups, silu,
                                          P(dx), P(dg), P(db), P(slot), P(ws), nws, st()))
            else:
                chk(L().tcx_gn_bwd(P(xd), P(dyd), P(sc), P(sh), P(mean), P(rstd), P(gd), Bt, HW, C, groups, silu,
                                   P(dx), P(dg), P(db), P(ws), nws, st()))
            runs.append((dx, dg, db, slot))
        for a, b in zip(*runs):
            assert a is None or bits(a) == bits(b), "tcx_gn_bwd is not deterministic"
        dx, dg, db, slot = runs[0]
        out.update(dx=cpu(dx, (Bt, HW, C)), dgamma=cpu(dg) if dg is not None else None,
                   dbeta=cpu(db) if db is not None else None, amax=int(cpu(slot)[0]) if amax else None)
    A.check()
    return out


def check_gn_stats(o, case, tag=""):
    ref = R.ref_gn_stats(o["x"], o["gamma"], o["beta"], case[3])
    C = o["x"].shape[2]
    t32 = R.gn_tables_f32(ref[0], ref[1], o["gamma"] if o["gamma"] is not None else np.ones(C, F32), o["beta"])
    for name, r, r32 in zip(("mean", "rstd", "scale", "shift"), ref, (None, None) + t32):
        # shift = beta - mean*scale cancels: where the float32 evaluation misses 1e-6, 4 x its error
        gate(f"gn_stats {case}{tag} {name}", R.gate_rel(o[name], r, 1e-6, ref32=r32 if name == "shift" else None))
    return ref


@pytest.mark.parametrize("case", R.GN_CASES, ids=str)
def test_gn_stats_and_bwd(case):
    """(3, 63, 8, 2, 0): nsplit 1, 128 lanes; (2, 200, 96, 8, 1): nsplit 3, uneven, 24 quads;
    (2, 4160, 192, 8, 1): the nsplit cap of 64; (33, 64, 12, 4, 1): second trip of k_gn_bwd_affine;
    (1, 128, 1024, 8, 0): C / 4 = 256, the last supported width.  amax at the first and third case
    must be exactly max|dx| of the returned dx (the first has fewer elements than one block)."""
    amax = case in ((2, 1, 4, 1, 1), (2, 200, 96, 8, 1))
    o = run_gn(case, amax=amax)
    check_gn_stats(o, case)
    dx, dg, db = R.ref_gn_bwd(o["x"], o["dy"], o["gamma"], o["beta"], case[3], case[4])
    gate(f"gn_bwd {case} dx", R.gate_max(o["dx"], dx))
    gate(f"gn_bwd {case} dgamma", R.gate_max(o["dgamma"], dg))
    gate(f"gn_bwd {case} dbeta", R.gate_max(o["dbeta"], db))
    if amax:
        assert o["amax"] == int(np.abs(o["dx"]).max().view(np.uint32)), "amax is not the bit pattern of max|dx|"


def test_gn_bwd_without_affine():
    """gamma = beta = NULL, dgamma = dbeta = NULL"""
    case = (2, 200, 96, 8, 1)
    o = run_gn(case, gamma_null=True)
    check_gn_stats(o, case, " no affine")
    dx, _, _ = R.ref_gn_bwd(o["x"], o["dy"], None, None, 8, 1)
    gate("gn_bwd no affine dx", R.gate_max(o["dx"], dx))


def test_gn_bwd_large_mean():
    """x = 100 + randn at (2, 200, 96, 8, silu): the large mean must not upset the scale / shift tables.
    The float32 CPU evaluation of the reference misses 2e-5 * max|ref| here (dx 2.4e-4 against 1.7e-4,
    dgamma 1.3e-3 against 7.6e-4, dbeta 5.5e-4 against 5.9e-4): it forms xhat = (x - mean)*rstd from a
    float32 mean.  The kernels keep the fp64 statistics up to the tables and hold the plain gate on the
    MI355X (dx 2.3e-5, dgamma 1.3e-4, dbeta 8.3e-5), so this case keeps 2e-5 * max|ref| too."""
    case = (2, 200, 96, 8, 1)
    o = run_gn(case, offset=100.0)
    check_gn_stats(o, case, " x=100+randn")
    dx, dg, db = R.ref_gn_bwd(o["x"], o["dy"], o["gamma"], o["beta"], 8, 1)
    hx, hg, hb = R.gn_bwd_formula(o["x"], o["dy"], o["gamma"], o["beta"], 8, 1, dt=F32)
    for name, ref, h in (("dx", dx, hx), ("dgamma", dg, hg), ("dbeta", db, hb)):
        print(f"  fp32 reference err {name}: {np.abs(h.astype(F64) - ref).max():.3e}, "
              f"2e-5*max|ref| {2e-5 * np.abs(ref).max():.3e}")
        gate(f"gn_bwd x=100+randn {name}", R.gate_max(o[name], ref))


def test_gn_stats_constant_group():
    """a constant group has variance exactly 0 in the fp64 partials: rstd = 1 / sqrt(eps)"""
    case = (2, 200, 96, 8, 1)
    o = run_gn(case, const_group=True, bwd=False)
    check_gn_stats(o, case, " const group")
    assert (o["rstd"][:, 0] == F32(1.0 / np.sqrt(R.GN_EPS))).all() and (o["mean"][:, 0] == 2.5).all()


def test_gn_bwd_bad_args():
    """C = 0 (a host division by zero without the guard), C = 1028 (channel quads past 256 were never
    reduced), C = 6, a misaligned x, a short workspace: refused, nothing launched."""
    buf = torch.zeros(4096, device="cuda")
    p = P(buf)
    big = 1 << 24

    def call(x, C, groups, nws):
        return L().tcx_gn_bwd_absmax(x, p, p, p, p, p, None, 1, 1, C, groups, 0, p, None, None, None, p, nws, st())

    assert call(p, 0, 1, big) != 0
    assert "1024" in last_error()
    assert call(p, 1028, 1, big) != 0
    assert "1024" in last_error()
    assert call(p, 6, 1, big) != 0
    assert call(p + 4, 8, 1, big) != 0
    assert "align" in last_error()
    assert call(p, 8, 1, L().tcx_gn_bwd_workspace(1, 1, 8) - 1) != 0
    assert "workspace" in last_error()
    assert L().tcx_gn_bwd(p, p, p, p, p, p, None, 1, 1, 1028, 1, 0, p, None, None, p, big, st()) != 0


# ------------------------------------------------------------------------------------ upsample x2
@pytest.mark.parametrize("case", R.UPS_CASES, ids=str)
def test_upsample2x_bwd(case):
    Bt, H, W, C = case
    x, dy = R.ups_inputs(*case)
    A = Arena()
    dx = A.new(x.size)
    dyd = dev(dy)
    chk(L().tcx_upsample2x_bwd(P(dyd), P(dx), Bt, H, W, C, st()))
    y = A.new(dy.size)
    xd = dev(x)
    chk(L().tcx_upsample2x(P(xd), P(y), Bt, H, W, C, None, None, st()))
    A.check()
    got = cpu(dx, x.shape)
    gate(f"upsample2x_bwd {case}", R.gate_upsample_bwd(got, R.ref_upsample_bwd(dy), dy))
    lhs = float((cpu(y, dy.shape).astype(F64) * dy).sum())
    rhs = float((x.astype(F64) * got).sum())
    scale = float((np.abs(R.ref_upsample(x)) * np.abs(dy)).sum())
    print(f"  adjoint {case}: <up(x), g> {lhs:.9e} <x, up_bwd(g)> {rhs:.9e}")
    assert abs(lhs - rhs) <= 1e-5 * scale


# ------------------------------------------------------------------------------------ softmax rows
@pytest.mark.parametrize("family", R.SOFTMAX_FAMILIES)
@pytest.mark.parametrize("case", R.SOFTMAX_CASES, ids=str)
def test_softmax_rows_fwd_bwd(case, family):
    rows, n = case
    S, dP = R.softmax_input(rows, n, family)
    A = Arena()
    Sd, dPd = dev(S), dev(dP)
    Pd, dS = A.new(rows * n), A.new(rows * n)
    chk(L().tcx_softmax_rows(P(Sd), P(Pd), rows, n, st()))
    chk(L().tcx_softmax_bwd_rows(P(Pd), P(dPd), P(dS), rows, n, st()))
    A.check()
    Pg = cpu(Pd, (rows, n))
    gate(f"softmax {case} {family} P", R.gate_softmax_p(Pg, R.ref_softmax(S)))
    gate(f"softmax {case} {family} row sums", R.gate_rowsum(Pg))
    gate(f"softmax {case} {family} dS", R.gate_softmax_ds(cpu(dS, (rows, n)), R.ref_softmax_bwd(Pg, dP), Pg, dP))


# ------------------------------------------------------------------------------------ activations
@pytest.mark.parametrize("n", R.ACT_SIZES)
@pytest.mark.parametrize("act", (1, 2, 3))
def test_act_fwd_bwd(act, n):
    """n = 8192*256 + 3 takes a second grid stride.  1e-5 |ref| + 1e-12; for Sigmoid' and SiLU' at the
    sizes where the float32 reference misses it, 4 x that reference's error (module docstring).  The
    planted +-88 and +-100 are also checked alone at the stated gate."""
    z, dy = R.act_inputs(n)
    A = Arena()
    zd, dyd = dev(z), dev(dy)
    y, dz = A.new(n), A.new(n)
    chk(L().tcx_act_fwd(P(zd), P(y), n, act, st()))
    chk(L().tcx_act_bwd(P(zd), P(dyd), P(dz), n, act, st()))
    A.check()
    yg, dg = cpu(y), cpu(dz)
    assert np.isfinite(yg).all() and np.isfinite(dg).all()
    ref = R.ref_act_bwd(z, dy, act)
    gate(f"act {act} n={n} fwd", R.gate_rel(yg, R.ref_act_fwd(z, act), 1e-5, 1e-12))
    r32 = R.ref_act_bwd(z, dy, act, dt=F32) if act != 1 else None
    if r32 is not None:
        print(f"  fp32 reference err act {act} bwd: {np.abs(r32.astype(F64) - ref).max():.3e}")
    gate(f"act {act} n={n} bwd", R.gate_rel(dg, ref, 1e-5, 1e-12, ref32=r32))
    if act == 1:
        assert (dg[z == 0] == 0).all()  # ReLU'(+-0) = 0
    if n >= 255:  # the planted +-88 and +-100: saturated, finite
        sat = np.abs(z) >= 88
        gate(f"act {act} n={n} saturated fwd", R.gate_rel(yg[sat], R.ref_act_fwd(z, act)[sat], 1e-5, 1e-12))
        gate(f"act {act} n={n} saturated bwd", R.gate_rel(dg[sat], ref[sat], 1e-5, 1e-12))


def test_act_bad_args():
    buf = torch.zeros(64, device="cuda")
    assert L().tcx_act_fwd(P(buf), P(buf), 8, 0, st()) != 0
    assert L().tcx_act_bwd(P(buf), P(buf), P(buf), 8, 4, st()) != 0


# ------------------------------------------------------------------------------------ MSE
def mse_ws_bytes(n):
    return min(-(-n // 256), 1024) * 8 + 256


@pytest.mark.parametrize("n", R.MSE_SIZES + (R.MSE_BWD_STRIDE_SIZE,))
def test_mse_loss_and_bwd(n):
    """n = 1024*256 + 5: second stride of k_sqdiff_part; 8192*256 + 3: second stride of k_mse_bwd.
    The gradient gate is 1e-6 |ref| per element with no floor."""
    a, b = R.mse_inputs(n)
    A = Arena()
    ad, bd = dev(a), dev(b)
    nws = mse_ws_bytes(n)
    losses = []
    for _ in range(2):
        ws, out = A.new(nws, torch.uint8), A.new(1)
        chk(L().tcx_mse_loss(P(ad), P(bd), n, P(out), P(ws), nws, st()))
        losses.append(out)
    assert bits(losses[0]) == bits(losses[1]), "tcx_mse_loss is not deterministic"
    gate(f"mse n={n} loss", R.gate_rel(cpu(losses[0])[0], R.ref_mse(a, b), 1e-6))
    for g in (3.0, 0.0):
        da = A.new(n)
        gd = dev(np.array([g]))
        chk(L().tcx_mse_bwd(P(ad), P(bd), n, P(gd), P(da), st()))
        gate(f"mse n={n} grad_out={g} grad", R.gate_rel(cpu(da), R.ref_mse_bwd(a, b, g), 1e-6))
    A.check()


def test_mse_bad_args():
    buf = torch.zeros(1024, device="cuda")
    assert L().tcx_mse_loss(P(buf), P(buf), 0, P(buf), P(buf), 4096, st()) != 0
    assert L().tcx_mse_loss(P(buf), P(buf), 1024, P(buf), P(buf), mse_ws_bytes(1024) - 1, st()) != 0
    assert L().tcx_mse_bwd(P(buf), P(buf), 8, None, P(buf), st()) != 0


# ------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("E", (1, 24))
def test_embedding_fwd_bwd(E):
    rows = 5
    r = R.rng(11 + E)
    W = R.f32(r.standard_normal((rows, E)))
    Wd = dev(W)
    for name, idx in (("repeats", np.array([0, 2, 2, 4, 0, 2])), ("same", np.full(300, 2)), ("empty", np.zeros(0))):
        idx = idx.astype(np.int64)
        B = idx.size
        dout = R.f32(r.standard_normal((B, E)))
        A = Arena()
        ix = A.new(B, torch.int64, init=idx)
        do = A.new(B * E, init=dout)
        out, dW = A.new(B * E), A.new(rows * E)
        chk(L().tcx_embedding_fwd(P(ix), P(Wd), B, E, P(out), st()))
        chk(L().tcx_embedding_bwd(P(ix), P(do), B, rows, E, P(dW), st()))
        A.check()
        gate(f"embedding_fwd E={E} {name}", R.gate_exact(cpu(out, (B, E)), W[idx]))
        ref, sa = R.ref_embedding_bwd(idx, dout, rows)
        got = cpu(dW, (rows, E))
        gate(f"embedding_bwd E={E} {name}", R.gate_embedding(got, ref, sa, B))
        unused = np.setdiff1d(np.arange(rows), idx)
        assert unused.size and (got[unused] == 0).all(), "an unused row of dW is not exactly 0"


# ------------------------------------------------------------------------------------ LayerNorm + FiLM
@pytest.mark.parametrize("offset", (0.0, 50.0))
@pytest.mark.parametrize("film", (0, 2, 3))
@pytest.mark.parametrize("case", R.LN_CASES, ids=str)
def test_ln_fwd_bwd(case, film, offset):
    """gb = NULL, ld_gb = 2 Wd, and ld_gb = 3 Wd (forward only).

    y and dx: 2e-5 * max|ref| in every case.  Two cases failed it before the kernels were changed, both
    at (2, 1), where rstd = 1/sqrt(eps) = 316 and the exact xhat and dx are 0:
      y, x = 50 + randn: 1.2e-4 to 1.6e-4 against 1.1e-5 (float32 reference 3e-8): k_ln_fwd formed
        fma(x, rstd, -mean*rstd), which leaves the rounding of mean*rstd (15800) in xhat;
      dx, either offset: 2.3e-6 to 5.2e-6 against 1e-12 (float32 reference 0): k_ln_bwd's second pass
        fused dl*w into dxh - m1, m1 being the mean of the rounded products.
    mean, rstd: 1e-6 relative.  The backward is given the float64 statistics rounded once to float32,
    and its reference is evaluated on those.  dwrow, dbrow, dgb: 1e-5 |ref| + 1e-9 in every case; dgb =
    [dh*l | dh] missed it at (2, 257), ld_gb = 2 Wd (1.6e-8 against 3.5e-9 where l = xhat*w + b is
    2.5e-4) until k_ln_bwd formed l in fp64."""
    M, Wd = case
    x, dh, w, b, gb = R.ln_inputs(M, Wd, film * Wd, offset=offset)
    A = Arena()
    xd, dhd, wd, bd = dev(x), dev(dh), dev(w), dev(b)
    gbd = dev(gb) if film else None
    stats = R.ln_stats_f32(x)  # the backward's mean / rstd inputs: float64 statistics rounded once
    md, rd = dev(stats[0]), dev(stats[1])
    runs = []
    for _ in range(2):
        y, mean, rstd = A.new(M * Wd), A.new(M), A.new(M)
        chk(L().tcx_ln_fwd(P(xd), P(y), M, Wd, P(wd), P(bd), P(gbd), film * Wd, R.LN_EPS, P(mean), P(rstd), st()))
        outs = [y, mean, rstd]
        if film != 3:
            dx, dwrow, dbrow = A.new(M * Wd), A.new(M * Wd), A.new(M * Wd)
            dgb = A.new(M * 2 * Wd) if film else None
            chk(L().tcx_ln_bwd(P(xd), P(dhd), M, Wd, P(wd), P(bd), P(gbd), film * Wd, P(md), P(rd), P(dx),
                               P(dwrow), P(dbrow), P(dgb), st()))
            outs += [dx, dwrow, dbrow] + ([dgb] if film else [])
        runs.append(outs)
    A.check()
    for t0, t1 in zip(*runs):
        assert bits(t0) == bits(t1), "tcx_ln is not deterministic"
    fwd, ref = R.ref_ln(x, dh, w, b, gb), R.ref_ln(x, dh, w, b, gb, stats=stats)
    r32 = R.ref_ln(x, dh, w, b, gb, dt=F32, stats=stats)
    for k in ("y", "mean", "rstd"):
        ref[k] = fwd[k]
    r32["y"] = R.ref_ln(x, dh, w, b, gb, dt=F32)["y"]
    names = ["y", "mean", "rstd"] + (["dx", "dwrow", "dbrow"] + (["dgb"] if film else []) if film != 3 else [])
    tag = f"ln {case} ld_gb={film}Wd offset={offset}"
    for name, t in zip(names, runs[0]):
        got = cpu(t, ref[name].shape)
        if name in ("y", "dx"):
            print(f"  fp32 reference err {name}: {np.abs(r32[name].astype(F64) - ref[name]).max():.3e}")
            gate(f"{tag} {name}", R.gate_max(got, ref[name]))
        elif name in ("mean", "rstd"):
            gate(f"{tag} {name}", R.gate_rel(got, ref[name], 1e-6))
        else:
            gate(f"{tag} {name}", R.gate_rel(got, ref[name], 1e-5, 1e-9))


def test_ln_bad_args():
    buf = torch.zeros(64, device="cuda")
    p = P(buf)
    assert L().tcx_ln_fwd(p, p, 1, 0, p, p, None, 0, 1e-5, p, p, st()) != 0
    assert L().tcx_ln_bwd(p, p, 1, 4, p, p, p, 8, p, p, p, p, p, None, st()) != 0  # gb without dgb


# ------------------------------------------------------------------------------------ Adam / EMA
def lay_out(A, arrays):
    """one buffer per tensor, each between its own canaries"""
    return [A.new(a.size, init=a) for a in arrays]


def table_of(ps, gs, ms, vs):
    from toycrystals_amd._lib import TcxAdamTensor
    tab = (TcxAdamTensor * len(ps))()
    for i, p in enumerate(ps):
        tab[i].p, tab[i].g = P(p), P(gs[i])
        tab[i].m, tab[i].v = (P(ms[i]), P(vs[i])) if ms else (None, None)
        tab[i].n = p.numel()
    return tab


@pytest.mark.parametrize("step", (1, 1000))
@pytest.mark.parametrize("wd", (0.0, 0.01))
@pytest.mark.parametrize("nt", R.ADAM_NT)
def test_adam_vs_torch_adam(nt, wd, step):
    """ntensors 1 / 48 / 49 / 97: one, exactly one, two and three launches of 48; sizes 1, 255, 257 and
    one tensor of 1024*256 + 3 (second grid stride).  torch.optim.Adam on CPU fp32 with the
    hyper-parameters (as the floats the ABI receives) and the 1e-6 absolute parameter gate of
    test_adam_matches_torch_adam; exp_avg and exp_avg_sq to 1e-6 relative per element."""
    ts = R.adam_inputs(nt, step)
    A = Arena()
    ps, gs, ms, vs = (lay_out(A, [t[k] for t in ts]) for k in range(4))
    tab = table_of(ps, gs, ms, vs)
    hp = R.ADAM_HP
    chk(L().tcx_adam(tab, nt, max(t[0].size for t in ts), hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], wd,
                     step, st()))
    A.check()
    rp, rm, rv = R.ref_adam(ts, step, wd)
    worst = [(0.0, 0.0)] * 3
    for i, (p, g, m, v) in enumerate(ts):
        assert bits(gs[i]) == g.tobytes(), "tcx_adam wrote a gradient"
        for k, eb in enumerate((R.gate_abs(cpu(ps[i]), rp[i], 1e-6), R.gate_rel(cpu(ms[i]), rm[i], 1e-6),
                                R.gate_rel(cpu(vs[i]), rv[i], 1e-6))):
            assert R.ok(eb), f"tensor {i} (n={p.size}) {('param', 'exp_avg', 'exp_avg_sq')[k]}: {eb}"
            worst[k] = max(worst[k], eb, key=lambda e: e[0] - e[1])
    for k, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
        print(f"  adam nt={nt} wd={wd} step={step} {name}: err {worst[k][0]:.3e} bound {worst[k][1]:.3e}")


@pytest.mark.parametrize("nt", R.ADAM_NT)
def test_ema(nt):
    ts = R.adam_inputs(nt, 1, seed=5)
    A = Arena()
    es, qs = lay_out(A, [t[0] for t in ts]), lay_out(A, [t[1] for t in ts])
    chk(L().tcx_ema(table_of(es, qs, None, None), nt, max(t[0].size for t in ts), R.EMA_DECAY, st()))
    A.check()
    worst = (0.0, 0.0)
    for i, (p, g, _, _) in enumerate(ts):
        eb = R.gate_ema(cpu(es[i]), R.ref_ema(p, g), p, g, R.EMA_DECAY)
        assert R.ok(eb), f"tensor {i}: {eb}"
        assert bits(qs[i]) == g.tobytes()
        worst = max(worst, eb, key=lambda e: e[0] - e[1])
    print(f"  ema nt={nt}: err {worst[0]:.3e} bound {worst[1]:.3e}")


def test_adam_bad_args():
    assert L().tcx_adam(None, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, st()) != 0
    assert L().tcx_adam(None, 0, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, st()) != 0  # step is 1-based
    assert L().tcx_ema(None, 1, 1, 0.5, st()) != 0
    chk(L().tcx_adam(None, 0, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, st()))


# ------------------------------------------------------------------------------------ VAE ops
@pytest.mark.parametrize("n", R.REPARAM_SIZES)
def test_reparam_fwd_bwd(n):
    """1e-5 |ref| + 1e-9; dlv at n = 257, beta = 1 (beta*old + new cancels) takes the float32-reference
    floor (module docstring)."""
    mu, lv, eps, dz, dmu0, dlv0 = R.reparam_inputs(n)
    A = Arena()
    mud, lvd, epd, dzd = dev(mu), dev(lv), dev(eps), dev(dz)
    z = A.new(n)
    chk(L().tcx_reparam(P(mud), P(lvd), P(epd), n, P(z), st()))
    gate(f"reparam n={n}", R.gate_rel(cpu(z), R.ref_reparam(mu, lv, eps), 1e-5, 1e-9,
                                      ref32=R.ref_reparam(mu, lv, eps, dt=F32)))
    for beta in (0.0, 1.0):
        dmu, dlv = (A.new(n, init=dmu0), A.new(n, init=dlv0)) if beta else (A.new(n), A.new(n))
        chk(L().tcx_reparam_bwd(P(lvd), P(epd), P(dzd), n, P(dmu), P(dlv), beta, st()))
        ref = R.ref_reparam_bwd(lv, eps, dz, dmu0, dlv0, beta)
        r32 = R.ref_reparam_bwd(lv, eps, dz, dmu0, dlv0, beta, dt=F32)
        gate(f"reparam_bwd n={n} beta={beta} dmu", R.gate_rel(cpu(dmu), ref[0], 1e-5, 1e-9, ref32=r32[0]))
        gate(f"reparam_bwd n={n} beta={beta} dlv", R.gate_rel(cpu(dlv), ref[1], 1e-5, 1e-9, ref32=r32[1]))
    A.check()


@pytest.mark.parametrize("fb", R.KL_FREE_BITS)
@pytest.mark.parametrize("shape", R.KL_SHAPES, ids=str)
def test_vae_kl_fwd_bwd(shape, fb):
    """With free bits the first element is mu = 1, logvar = 0: kl_dim is exactly 0.5 = free_bits in both
    precisions, and torch.maximum gives the tie a gradient weight of 0.5 (every other element is at
    least 1e-3 from the tie).  dlv in the cases listed in the module docstring (exp(l) - 1 cancels
    near l = 0) takes the float32-reference floor; dmu and every other case hold 1e-5 |ref| + 1e-9."""
    B, Z = shape
    mu, lv = R.kl_inputs(B, Z, fb, plant_tie=fb > 0)
    dmu0, dlv0 = R.kl_inputs(B, Z, 0.0, seed=5)
    A = Arena()
    mud, lvd = dev(mu), dev(lv)
    outs = [A.new(2), A.new(2)]
    for o in outs:
        chk(L().tcx_vae_kl(P(mud), P(lvd), B, Z, fb, P(o), st()))
    assert bits(outs[0]) == bits(outs[1]), "tcx_vae_kl is not deterministic"
    gate(f"vae_kl {shape} fb={fb}", R.gate_rel(cpu(outs[0]), R.ref_kl(mu, lv, fb), 1e-6))
    g = 0.7
    gd = dev(np.array([g]))
    for beta in (0.0, 1.0):
        dmu, dlv = (A.new(B * Z, init=dmu0), A.new(B * Z, init=dlv0)) if beta else (A.new(B * Z), A.new(B * Z))
        chk(L().tcx_vae_kl_bwd(P(mud), P(lvd), B, Z, fb, P(gd), P(dmu), P(dlv), beta, st()))
        gf = float(F32(g))
        ref = R.ref_kl_bwd(mu, lv, fb, gf, dmu0, dlv0, beta)
        r32 = R.ref_kl_bwd(mu, lv, fb, gf, dmu0, dlv0, beta, dt=F32)
        gm, gl = cpu(dmu, shape), cpu(dlv, shape)
        gate(f"vae_kl_bwd {shape} fb={fb} beta={beta} dmu", R.gate_rel(gm, ref[0], 1e-5, 1e-9, ref32=r32[0]))
        gate(f"vae_kl_bwd {shape} fb={fb} beta={beta} dlv", R.gate_rel(gl, ref[1], 1e-5, 1e-9, ref32=r32[1]))
        if fb > 0:  # the tie alone, at the stated gate
            gate("vae_kl_bwd tie dmu", R.gate_rel(gm.flat[0], ref[0].flat[0], 1e-5, 1e-9))
    A.check()


def test_vae_kl_bad_args():
    buf = torch.zeros(64, device="cuda")
    p = P(buf)
    assert L().tcx_vae_kl(p, p, 0, 4, 0.0, p, st()) != 0
    assert L().tcx_vae_kl_bwd(p, p, 2, 0, 0.0, p, p, p, 0.0, st()) != 0


def test_vae_yvec():
    B, n_types, ycd = 5, 4, 3
    r = R.rng(13)
    y_cat = np.array([0, 3, 4, -1, 2], dtype=np.int64)  # 4 and -1: outside [0, n_types): a zero one-hot row
    y_cont = R.f32(r.standard_normal((B, ycd)))
    keep = R.f32(r.random(B))
    cd = float(F32(0.1))
    keep[1], keep[2] = cd, 0.01  # equal to cond_drop exactly: kept; below: dropped
    for ku in (None, keep):
        A = Arena()
        out = A.new(B * (n_types + ycd))
        yc, yv = idev(y_cat), dev(y_cont)
        kd = dev(ku) if ku is not None else None
        chk(L().tcx_vae_yvec(P(yc), P(yv), P(kd), cd, B, n_types, ycd, P(out), st()))
        A.check()
        ref = R.ref_vae_yvec(y_cat, y_cont, ku, cd, n_types)
        gate(f"vae_yvec keep_u={'given' if ku is not None else 'NULL'}", R.gate_exact(cpu(out, ref.shape), ref))
    assert ref[1].any() and not ref[2].any() and not ref[3, :n_types].any()


# ------------------------------------------------------------------------------------ data-path kernels
@pytest.mark.parametrize("E", (2, 3, 7, 128))
def test_cond_inputs(E):
    """odd E leaves the last column 0; E = 2 has half - 1 = 0 (no division by zero)"""
    n_types, ycd = 4, 4
    t = np.array([0.0, 1e-3, 1.0, 0.37], dtype=F32)
    y_cat = np.array([-1, 0, n_types, n_types + 3], dtype=np.int64)
    y_cont = R.f32(R.rng(3).standard_normal((4, ycd)))
    A = Arena()
    te, yv, yc = A.new(4 * E), A.new(4 * ycd), A.new(4, torch.int64)
    td, ycd_, yvd = dev(t), idev(y_cat), dev(y_cont)
    chk(L().tcx_cond_inputs(P(td), P(ycd_), P(yvd), 4, E, n_types, ycd, P(te), P(yv), P(yc), st()))
    A.check()
    rte, ryv, ryc = R.ref_cond_inputs(t, y_cat, y_cont, E, n_types)
    gte, gyv = cpu(te, (4, E)), cpu(yv, (4, ycd))
    gate(f"cond_inputs E={E} te", R.gate_abs(gte, rte, 1e-6))
    gate(f"cond_inputs E={E} yv", R.gate_abs(gyv, ryv, 1e-6))
    assert (gyv[:, [0, 3]] == y_cont[:, [0, 3]]).all()
    assert E % 2 == 0 or (gte[:, -1] == 0).all()
    assert cpu(yc).tolist() == ryc.tolist() == [0, 0, n_types, n_types]


@pytest.mark.parametrize("E", (2, 7, 64))
def test_prior_temb(E):
    t = np.array([0, 999, 17], dtype=np.int64)
    fr = R.prior_freqs(E)
    A = Arena()
    te = A.new(3 * E)
    td, fd = idev(t), dev(fr)
    chk(L().tcx_prior_temb(P(td), P(fd), 3, E, P(te), st()))
    A.check()
    got = cpu(te, (3, E))
    gate(f"prior_temb E={E}", R.gate_abs(got, R.ref_prior_temb(t, fr, E), 1e-6))
    assert E % 2 == 0 or (got[:, -1] == 0).all()


@pytest.mark.parametrize("HW", (1, 257))
@pytest.mark.parametrize("t_power", (1.0, 2.0, 0.5))
def test_qsample_vp(t_power, HW):
    """u = 0 gives a = 1, s = sqrt(1e-8).  x_t: 1e-5 |ref| + 1e-9; at HW = 257 with t_power 1 and 2 the
    float32-reference floor (module docstring)."""
    r = R.rng(5 + HW)
    u = np.array([0.0, 0.3, 1.0], dtype=F32)
    x0, eps = R.f32(r.random((3, HW))), R.f32(r.standard_normal((3, HW)))
    bmin, c2 = float(F32(0.1)), float(F32(14.95))
    A = Arena()
    t_out, x_t = A.new(3), A.new(3 * HW)
    x0d, ed, ud = dev(x0), dev(eps), dev(u)
    chk(L().tcx_qsample_vp(P(x0d), P(ed), P(ud), t_power, bmin, c2, 3, HW, P(t_out), P(x_t), st()))
    A.check()
    rt, rx = R.ref_qsample_vp(x0, eps, u, t_power, bmin, c2)
    _, r32 = R.ref_qsample_vp(x0, eps, u, t_power, bmin, c2, dt=F32)
    gate(f"qsample_vp p={t_power} HW={HW} t", R.gate_rel(cpu(t_out), rt, 1e-5, 1e-9))
    got = cpu(x_t, (3, HW))
    gate(f"qsample_vp p={t_power} HW={HW} x_t", R.gate_rel(got, rx, 1e-5, 1e-9, ref32=r32))
    u0 = (2 * x0[0].astype(F64) - 1) + np.sqrt(float(F32(1e-8))) * eps[0].astype(F64)
    gate("qsample_vp u=0 row", R.gate_rel(got[0], u0, 1e-5, 1e-9, ref32=r32[0]))


def test_cond_drop():
    B, ycd, n_types = 5, 3, 4
    rr = R.rng(17)
    y_cat = np.array([0, 1, 2, 3, 1], dtype=np.int64)
    y_cont = R.f32(rr.standard_normal((B, ycd)))
    p = float(F32(0.1))
    rv = R.f32([0.5, p, 0.05, 0.0, 0.99])  # r == p exactly: not dropped
    for r_ in (None, rv):
        A = Arena()
        oc, ov = A.new(B, torch.int64), A.new(B * ycd)
        ycd_, yvd = idev(y_cat), dev(y_cont)
        rd = dev(r_) if r_ is not None else None
        chk(L().tcx_cond_drop(P(ycd_), P(yvd), P(rd), p, B, ycd, n_types, P(oc), P(ov), st()))
        A.check()
        rc, ro = R.ref_cond_drop(y_cat, y_cont, r_, p, n_types)
        gate("cond_drop cat", R.gate_exact(cpu(oc), rc))
        gate("cond_drop cont", R.gate_exact(cpu(ov, (B, ycd)), ro))
    assert rc.tolist() == [0, 1, n_types, n_types, 1]


def schedule(T):
    ab = np.cumprod(1.0 - np.linspace(1e-4, 0.02, T))
    return R.f32(np.sqrt(ab)), R.f32(np.sqrt(1.0 - ab))


@pytest.mark.parametrize("Z", (1, 33))
def test_prior_qsample_and_q_sample(Z):
    """u = 1 clamps to T - 1; t_out is exact (u*u*T formed in fp32, then truncated)."""
    T = 1000
    sab, s1 = schedule(T)
    rr = R.rng(19 + Z)
    u = np.array([0.0, 0.5, 1.0, 0.7310586], dtype=F32)
    B = u.size
    z0, eps = R.f32(rr.standard_normal((B, Z))), R.f32(rr.standard_normal((B, Z)))
    A = Arena()
    t_out, z_t, z_t2 = A.new(B, torch.int64), A.new(B * Z), A.new(B * Z)
    zd, ed, ud, sd, s1d = dev(z0), dev(eps), dev(u), dev(sab), dev(s1)
    chk(L().tcx_prior_qsample(P(zd), P(ed), P(ud), P(sd), P(s1d), T, B, Z, P(t_out), P(z_t), st()))
    rt, rz = R.ref_prior_qsample(z0, eps, u, sab, s1, T)
    assert rt[:3].tolist() == [0, 250, T - 1]
    gate(f"prior_qsample Z={Z} t", R.gate_exact(cpu(t_out), rt))
    r32 = R.ref_q_sample(z0, rt, eps, sab, s1, dt=F32)
    gate(f"prior_qsample Z={Z} z_t", R.gate_rel(cpu(z_t, (B, Z)), rz, 1e-5, 1e-9, ref32=r32))
    t2 = np.array([0, T - 1, 5, 5], dtype=np.int64)
    td = idev(t2)
    chk(L().tcx_q_sample(P(zd), P(td), P(ed), P(sd), P(s1d), B, Z, P(z_t2), st()))
    A.check()
    gate(f"q_sample Z={Z}", R.gate_rel(cpu(z_t2, (B, Z)), R.ref_q_sample(z0, t2, eps, sab, s1), 1e-5, 1e-9,
                                       ref32=R.ref_q_sample(z0, t2, eps, sab, s1, dt=F32)))


def test_ddim_step():
    """z0 = (z - sqrt(1-abar_t) eps) / (sqrt(abar_t) + 1e-8); last: z0, else sqrt(abar_prev) z0 + sqrt(1-abar_prev) eps"""
    rr = R.rng(23)
    n = 257
    z, eps = R.f32(rr.standard_normal(n)), R.f32(rr.standard_normal(n))
    at, ap = float(F32(0.4)), float(F32(0.7))
    for last in (0, 1):
        def ref(dt):
            zz, ee = z.astype(dt), eps.astype(dt)
            z0 = (zz - np.sqrt(dt(1) - dt(at)) * ee) / (np.sqrt(dt(at)) + dt(F32(1e-8)))
            return z0 if last else np.sqrt(dt(ap)) * z0 + np.sqrt(dt(1) - dt(ap)) * ee
        A = Arena()
        zd = A.new(n, init=z)
        ed = dev(eps)
        chk(L().tcx_ddim_step(P(zd), P(ed), n, at, ap, last, st()))
        A.check()
        gate(f"ddim_step last={last}", R.gate_rel(cpu(zd), ref(F64), 1e-5, 1e-9, ref32=ref(F32)))


def test_u8_gather():
    N, npix = 4, 37
    x = R.rng(29).integers(0, 256, (N, npix)).astype(np.uint8)
    x[0, 0], x[0, 1], x[3, -1] = 0, 255, 255
    idx = np.array([3, 0, 0, 2, 3], dtype=np.int64)
    A = Arena()
    out = A.new(idx.size * npix)
    xd, ix = torch.from_numpy(x).cuda(), idev(idx)
    chk(L().tcx_u8_gather(P(xd), P(ix), idx.size, npix, P(out), st()))
    A.check()
    got = cpu(out, (idx.size, npix))
    gate("u8_gather (1 ulp)", R.gate_rel(got, x[idx].astype(F64) / 255.0, 2.0 ** -23))
    assert got[1, 0] == 0.0 and got[1, 1] == 1.0 and got[0, -1] == 1.0


@pytest.mark.parametrize("beta", (0.0, 1.0))
@pytest.mark.parametrize("rows,cols", [(3, 5), (4, 1), (300, 7)])
def test_copy2d(rows, cols, beta):
    """ld > cols on both sides; columns outside the window keep their values"""
    lds, ldd, c0 = cols + 3, cols + 2, 1
    rr = R.rng(31)
    src, dst0 = R.f32(rr.standard_normal((rows, lds))), R.f32(rr.standard_normal((rows, ldd)))
    A = Arena()
    sd = dev(src)
    dd = A.new(rows * ldd, init=dst0)
    chk(L().tcx_copy2d(P(sd) + 4 * 2, lds, P(dd) + 4 * c0, ldd, rows, cols, beta, st()))
    A.check()
    ref = dst0.copy()
    win = src[:, 2:2 + cols]
    ref[:, c0:c0 + cols] = (dst0[:, c0:c0 + cols] + win) if beta else win
    gate(f"copy2d {rows}x{cols} beta={beta}", R.gate_exact(cpu(dd, (rows, ldd)), ref))


@pytest.mark.parametrize("shape", [(2, 3, 5), (1, 1, 7), (2, 64, 1)], ids=str)
def test_transpose_bhc(shape):
    B, Rr, C = shape
    x = R.f32(R.rng(37).standard_normal(shape))
    A = Arena()
    y, back = A.new(x.size), A.new(x.size)
    xd = dev(x)
    chk(L().tcx_transpose_bhc(P(xd), P(y), B, Rr, C, st()))
    chk(L().tcx_transpose_bhc(P(y), P(back), B, C, Rr, st()))
    A.check()
    gate(f"transpose_bhc {shape}", R.gate_exact(cpu(y, (B, C, Rr)), x.transpose(0, 2, 1)))
    gate(f"transpose_bhc {shape} round trip", R.gate_exact(cpu(back, shape), x))


@pytest.mark.parametrize("B,C0,nm,ks", [(1, 4, 1, 3), (3, 32, 16, 3)])
def test_first_conv_bias_and_bwd(B, C0, nm, ks):
    """1e-5 |ref| + 1e-9; bias_b at (3, 32, 16, 3) takes the float32-reference floor (module docstring)"""
    rr = R.rng(41 + B)
    maps, w = R.f32(rr.standard_normal((B, nm))), R.f32(rr.standard_normal((C0, 1 + nm, ks, ks)))
    bias, S = R.f32(rr.standard_normal(C0)), R.f32(rr.standard_normal((B, C0)))
    dwx = R.f32(rr.standard_normal((C0, ks, ks)))
    md, wd, bd, Sd, dwxd = dev(maps), dev(w), dev(bias), dev(S), dev(dwx)
    for bz in (bias, None):
        A = Arena()
        out = A.new(B * C0)
        chk(L().tcx_first_conv_bias(P(md), P(wd), P(bd) if bz is not None else None, B, C0, nm, ks, P(out), st()))
        A.check()
        gate(f"first_conv_bias bias={'given' if bz is not None else 'NULL'}",
             R.gate_rel(cpu(out, (B, C0)), R.ref_first_conv_bias(maps, w, bz), 1e-5, 1e-9,
                        ref32=R.ref_first_conv_bias(maps, w, bz, dt=F32)))
    ref = R.ref_first_conv_bwd(S, maps, w, dwx)
    r32 = R.ref_first_conv_bwd(S, maps, w, dwx, dt=F32)
    for null in (None, "dmaps", "dw", "db"):
        A = Arena()
        outs = dict(dmaps=A.new(B * nm), dw=A.new(w.size), db=A.new(C0))
        if null:
            outs[null] = None
        chk(L().tcx_first_conv_bwd(P(Sd), P(md), P(wd), P(dwxd) if null != "dw" else None, B, C0, nm, ks,
                                   P(outs["dmaps"]), P(outs["dw"]), P(outs["db"]), st()))
        A.check()
        for k, name in enumerate(("dmaps", "dw", "db")):
            if outs[name] is not None:
                gate(f"first_conv_bwd NULL={null} {name}",
                     R.gate_rel(cpu(outs[name], ref[k].shape), ref[k], 1e-5, 1e-9, ref32=r32[k]))
    buf = torch.zeros(64, device="cuda")
    assert L().tcx_first_conv_bwd(P(buf), P(buf), P(buf), None, 1, 4, 1, 3, None, P(buf), None, st()) != 0  # dw without dwx
