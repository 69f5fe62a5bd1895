"""References, inputs, gates, mutants and case tables for the fp32 GEMM and conv weight-gradient
kernels of csrc/gemm.hip (no GPU import).

References are written from the header comments of include/tcx.h and evaluated in float64 on the
float32-rounded inputs the kernel receives:

  C[z](m, n) = alpha * sum_k A[z](m, k) B[z](k, n) + beta * C0[z](m, n) + bias[n],
      X[z](i, j) = X[off + (z / bdiv) * hi + (z % bdiv) * lo + i * s_i + j * s_j]
  dW[co][ci][ky][kx] = beta * dW0 + sum_{b,oy,ox} dY[b,oy,ox,co] * x[b, oy*s - p + ky, ox*s - p + kx, ci],
      circular or zero padding, ci < C1 from x1, the rest from x2
  y = act(x1 W1^T + x2 W2^T + b + resid)                                   (tcx_linear_ws)

Every operand is described by element strides into a flat buffer, so transposed, strided, sliced and
broadcast layouts are all the same code; the buffer ends at the last element the call may touch, so the
canary of the GPU test starts right behind a ragged tail.

Per-element gate: the fp32 MFMA is bitwise an fmaf chain, so any fp32 summation of n products is
within about n * 2^-24 * sum|terms| of the exact sum:
  GEMM   |got - ref| <= (K + nsplit + 4) * 2^-24 * S,  S = |alpha| sum_k |a||b| + |beta||C0| + |bias|
  wgrad  |got - ref| <= (n + nsplit + 4) * 2^-24 * (sum |dY||x| + |beta||dW0|),  n = Bt*Ho*Wo pixels
  linear 1.1 * the GEMM bound with n = K1 + K2 (1.1: Lipschitz constant of SiLU) + 4 * 2^-24 * |ref|
(+4: the alpha multiply, the beta fma, the bias add, second-order terms; unsplit nsplit = 0).  A
non-finite output is an infinite error; where S = 0 the result must be exact.

Aggregate gate for reductions longer than 300 terms (the per-element bound grows with n and would
admit operands truncated to 10 mantissa bits at K = 1056): RMS error against float64 <= 4 x the RMS
error of the float32 fma chain in plain k (pixel) order, evaluated here on the CPU.

Mutants are named wrong variants, evaluated in float64, that the gates must reject
(tests/test_gemm_ref_cpu.py).  The plan arithmetic of gemm.hip (gemm_split_plan, wgrad_plan,
linear_plan, the load-mode predicate, thin_wgrad_plan's refusals) is restated here so that each case's
claim about the branch it reaches is checked on the CPU and pinned on the GPU by the workspace sizes.
"""
import zlib

import numpy as np

import train_ops_ref as T
from train_ops_ref import F32, F64, U24, _diff, _worst, f32, ok  # noqa: F401

PATF = float(np.frombuffer(b"\x7b" * 4, dtype=F32)[0])  # what an unwritten output element holds
LONG = 300                                               # reductions longer than this also take the RMS gate


def cdiv(a, b):
    return (a + b - 1) // b


def seed_of(name):
    return zlib.crc32(name.encode())


# ------------------------------------------------------------------------------------ plans (gemm.hip)
def gemm_nt(N):
    return 1 if N <= 32 else (2 if N <= 64 else 3)


def gemm_split_plan(M, N, K, batch):
    """(nsplit, kcs) of gemm_split_plan"""
    tiles = cdiv(M, 128) * cdiv(N, 32 * gemm_nt(N)) * batch
    nch = cdiv(K, 32)
    if tiles >= 256 or nch < 8:
        return 1, nch
    s = min(cdiv(512, tiles), 16)
    s = min(s, nch // 4)
    if s < 2:
        return 1, nch
    kcs = cdiv(nch, s)
    return cdiv(nch, kcs), kcs


def split_chunks(K, nsplit, kcs):
    """32-chunks per split"""
    nch = cdiv(K, 32)
    return [min(kcs, nch - s * kcs) for s in range(nsplit)]


def gemm_workspace(M, N, K, batch):
    if min(M, N, K, batch) <= 0:
        return 0
    ns, _ = gemm_split_plan(M, N, K, batch)
    return ns * batch * M * N * 4 if ns > 1 else 0


def load_mode(K, ext, s_k, s_o, hi, lo, addr_bytes):
    """gemm_impl's predicate for one operand: s_k the stride along k, s_o along m (or n), ext = M (or N)"""
    z = hi % 4 == 0 and lo % 4 == 0 and addr_bytes % 16 == 0
    if K == 0:
        return 2
    if s_k == 1 and K % 4 == 0 and s_o % 4 == 0 and z:
        return 0
    if s_o == 1 and ext % 4 == 0 and s_k % 4 == 0 and z:
        return 1
    return 2


def wgrad_plan(M, K, Cout):
    """(nt, nsplit, cps) of wgrad_plan"""
    nt = 1 if Cout <= 32 else (2 if Cout <= 64 else 3)
    tiles = cdiv(K, 128) * cdiv(Cout, 32 * nt)
    nch = cdiv(max(M, 1), 32)
    ns = max(1, cdiv(2048, tiles))
    ns = min(ns, max(1, nch // 8), 256)
    cps = cdiv(nch, ns)
    return nt, cdiv(nch, cps), cps


def wgrad_workspace(Bt, Ho, Wo, Cin, Cout, ks):
    K = ks * ks * Cin
    return wgrad_plan(Bt * Ho * Wo, K, Cout)[1] * K * Cout * 4 + 256


def linear_plan(M, N, K1, K2):
    """(s1, k1cs, s2, k2cs) of linear_plan"""
    tiles = cdiv(M, 128) * cdiv(N, 96)

    def one(K):
        nch = cdiv(K, 32)
        s = max(1, min(min(cdiv(512, tiles), 16), nch // 2))
        kcs = cdiv(nch, s)
        return cdiv(nch, kcs), kcs

    return one(K1) + (one(K2) if K2 > 0 else (0, 0))


def linear_wants_split(M, N, K1, K2):
    return cdiv(M, 128) * cdiv(N, 96) < 128 and K1 % 4 == 0 and K2 % 4 == 0 and K1 + K2 >= 256


def thin_takes(c, x1_shift=0):
    """tcx_conv_wgrad hands the shape to thin.hip (thin_wgrad_plan and the conditions around its call)"""
    B, H, W, C1, C2, Cout, ks, stride, pad, circ = c
    if C2 != 0 or pad != 1 or x1_shift % 16:
        return False
    C = Cout if C1 == 1 else C1
    if circ and W < 2:   # refused at the call: the thin kernel's look-ahead would wrap twice
        return False
    return stride == 1 and ks == 3 and (C1 == 1 or Cout == 1) and C % 4 == 0 and C // 4 <= 512 and B > 0


# ------------------------------------------------------------------------------------ GEMM cases
class G:
    """One tcx_gemm call.  A = (s_m, s_k, hi, lo, off), B = (s_k, s_n, hi, lo, off), C = (s_m, s_n, hi, lo, off)
    in floats; shift_a / shift_b move the buffer's base by bytes; split: through tcx_gemm_ws as well."""

    def __init__(self, name, M, N, K, A, B, C=None, alpha=0.5, beta=2.0, bias=True, batch=1, bdiv=1, shift_a=0,
                 shift_b=0, modes=None, nsplit=1, chunks=None):
        self.name, self.M, self.N, self.K = name, M, N, K
        self.A, self.B = tuple(A), tuple(B)
        self.C = tuple(C) if C else (N, 1, M * N, 0, 0) if bdiv == 1 else (N, 1, bdiv * M * N, M * N, 0)
        self.alpha, self.beta, self.bias, self.batch, self.bdiv = alpha, beta, bias, batch, bdiv
        self.shift_a, self.shift_b = shift_a, shift_b
        self.modes, self.nsplit, self.chunks = modes, nsplit, chunks  # the table's claims

    def __repr__(self):
        return self.name

    def idx(self, op, swap_z=False, swap_s=False):
        """flat indices [batch][rows][cols] of operand 'A' (m, k), 'B' (k, n) or 'C' (m, n)"""
        s0, s1, hi, lo, off = getattr(self, op)
        r, c = {"A": (self.M, self.K), "B": (self.K, self.N), "C": (self.M, self.N)}[op]
        if swap_s:
            s0, s1 = s1, s0
        z = np.arange(self.batch)
        zh, zl = (z % self.bdiv, z // self.bdiv) if swap_z else (z // self.bdiv, z % self.bdiv)
        return (off + zh * hi + zl * lo)[:, None, None] + (np.arange(r) * s0)[None, :, None] \
            + (np.arange(c) * s1)[None, None, :]

    def size(self, op):
        i = self.idx(op)
        return int(i.max()) + 1 if i.size else 0

    def expect_modes(self):
        a, b = self.A, self.B
        la = load_mode(self.K, self.M, a[1], a[0], a[2], a[3], self.shift_a + 4 * a[4])
        lb = load_mode(self.K, self.N, b[0], b[1], b[2], b[3], self.shift_b + 4 * b[4])
        return la, lb

    def inputs(self):
        r = T.rng(seed_of(self.name))
        g = lambda n: f32(r.standard_normal(n))
        return dict(A=g(self.size("A")), B=g(self.size("B")), C=g(self.size("C")),
                    bias=g(self.N) if self.bias else None)


def opA(M, K, mode):
    return {0: (K, 1), 1: (1, M), 2: (K + 1, 1)}[mode] + (0, 0, 0)


def opB(K, N, mode):
    return {0: (1, K), 1: (N, 1), 2: (1, K + 1)}[mode] + (0, 0, 0)


def _modes():
    out = []
    for N in (28, 60, 100):
        for la in range(3):
            for lb in range(3):
                out.append(G(f"modes N={N} la={la} lb={lb}", 132, N, 68, opA(132, 68, la), opB(68, N, lb),
                             modes=(la, lb)))
    return out


def _batched(M, K, bdiv, gap=4):
    lo = M * K + gap
    return bdiv * lo + 2 * gap, lo


def _scalar():
    M, N, K = 132, 60, 68
    o = []
    # A scalar for one reason each, B n-contiguous (mode 1); then B scalar, A m-contiguous
    o.append(G("scalar A stride-2 view", M, N, K, (2 * K, 2, 0, 0, 0), opB(K, N, 1), modes=(2, 1)))
    o.append(G("scalar A K=67", M, N, 67, (68, 1, 0, 0, 0), opB(67, N, 1), modes=(2, 1)))
    o.append(G("scalar A M=131 transposed", 131, N, K, (1, 132, 0, 0, 0), opB(K, N, 1), modes=(2, 1)))
    o.append(G("scalar A base+4B", M, N, K, opA(M, K, 0), opB(K, N, 1), shift_a=4, modes=(2, 1)))
    o.append(G("scalar A transposed base+4B", M, N, K, opA(M, K, 1), opB(K, N, 1), shift_a=4, modes=(2, 1)))
    o.append(G("scalar A sa_hi%4", M, N, K, (K, 1, 2 * M * K + 1, M * K, 0), (N, 1, 2 * K * N, K * N, 0), batch=4,
               bdiv=2, modes=(2, 1)))
    o.append(G("scalar A sa_lo%4", M, N, K, (K, 1, 2 * M * K + 4, M * K + 1, 0), (N, 1, 2 * K * N, K * N, 0), batch=4,
               bdiv=2, modes=(2, 1)))
    o.append(G("scalar B stride-2 view", M, N, K, opA(M, K, 1), (2, 2 * K, 0, 0, 0), modes=(1, 2)))
    o.append(G("scalar B K=67", M, N, 67, opA(M, 67, 1), (1, 68, 0, 0, 0), modes=(1, 2)))
    o.append(G("scalar B N=59 transposed", M, 59, K, opA(M, K, 1), (60, 1, 0, 0, 0), modes=(1, 2)))
    o.append(G("scalar B base+4B", M, N, K, opA(M, K, 1), opB(K, N, 0), shift_b=4, modes=(1, 2)))
    o.append(G("scalar B transposed base+4B", M, N, K, opA(M, K, 1), opB(K, N, 1), shift_b=4, modes=(1, 2)))
    o.append(G("scalar B sb_hi%4", M, N, K, (1, M, 2 * M * K, M * K, 0), (1, K, 2 * K * N + 1, K * N, 0), batch=4,
               bdiv=2, modes=(1, 2)))
    o.append(G("scalar B sb_lo%4", M, N, K, (1, M, 2 * M * K, M * K, 0), (1, K, 2 * K * N + 4, K * N + 1, 0), batch=4,
               bdiv=2, modes=(1, 2)))
    return o


def _edges():
    o = []
    for M in (1, 127, 128, 129):
        o.append(G(f"edge M={M}", M, 40, 36, opA(M, 36, 0), opB(36, 40, 0)))
    for N in (1, 31, 32, 33, 63, 64, 65, 95, 96, 97):
        o.append(G(f"edge N={N}", 36, N, 36, opA(36, 36, 0), opB(36, N, 0)))
    for K in (0, 1, 3, 4, 31, 32, 33, 64):
        o.append(G(f"edge K={K}", 36, 40, K, opA(36, K, 0), opB(K, 40, 0)))
    o.append(G("edge K=0 no bias beta=0", 36, 40, 0, opA(36, 0, 0), opB(0, 40, 0), beta=0.0, bias=False))
    o.append(G("edge beta=0 over NaN", 36, 40, 36, opA(36, 36, 0), opB(36, 40, 0), beta=0.0))
    o.append(G("edge bias=NULL", 36, 40, 36, opA(36, 36, 0), opB(36, 40, 0), bias=False))
    return o


def _attention(d):
    """the five products of AttentionFn (functional.py), B = 2 images, N = 16 tokens, 4 heads"""
    Bi, N, h = 2, 16, 4
    C = h * d
    C3, z = 3 * C, Bi * h
    S_hl, q_hl, o_hl = (h * N * N, N * N), (N * C3, d), (N * C, d)
    kw = dict(batch=z, bdiv=h, beta=0.0, bias=False)
    sc = 1.0 / np.sqrt(d)
    S, qkv, o = (lambda s0, s1, off=0, hl=hl: (s0, s1) + hl + (off,) for hl in (S_hl, q_hl, o_hl))
    return [
        G(f"attn d={d} S=QK^T", N, N, d, qkv(C3, 1), qkv(1, C3, C), S(N, 1), alpha=sc, **kw),
        G(f"attn d={d} O=PV", N, d, N, S(N, 1), qkv(C3, 1, 2 * C), o(C, 1), alpha=1.0, **kw),
        G(f"attn d={d} dP=dO V^T", N, N, d, o(C, 1), qkv(1, C3, 2 * C), S(N, 1), alpha=1.0,
          **kw),
        G(f"attn d={d} dQ=dS K", N, d, N, S(N, 1), qkv(C3, 1, C), qkv(C3, 1), alpha=sc, **kw),
        G(f"attn d={d} dK=dS^T Q", N, d, N, S(1, N), qkv(C3, 1), qkv(C3, 1, C), alpha=sc, **kw),
        G(f"attn d={d} dV=P^T dO", N, d, N, S(1, N), o(C, 1), qkv(C3, 1, 2 * C), alpha=1.0,
          **kw),
    ]


def _batch():
    M, N, K = 36, 40, 36
    o = []
    for bdiv in (1, 3, 6):
        ah, al = _batched(M, K, bdiv)
        bh, bl = _batched(K, N, bdiv, 8)
        ch, cl = _batched(M, N, bdiv, 12)
        o.append(G(f"batch=6 bdiv={bdiv}", M, N, K, (K, 1, ah, al, 0), (1, K, bh, bl, 0), (N, 1, ch, cl, 0), batch=6,
                   bdiv=bdiv))
    o.append(G("batch=6 B broadcast", M, N, K, (K, 1, 3 * M * K, M * K, 0), (1, K, 0, 0, 0), batch=6, bdiv=3))
    o.append(G("C transposed", M, N, K, opA(M, K, 0), opB(K, N, 0), (1, M, M * N, 0, 0)))
    return o + _attention(3) + _attention(8)


def _split():
    o = [G("split (36,40,256)", 36, 40, 256, opA(36, 256, 0), opB(256, 40, 0), modes=(0, 0), nsplit=2, chunks=[4, 4]),
         G("split (36,40,260) transposed", 36, 40, 260, opA(36, 260, 1), opB(260, 40, 1), modes=(1, 1), nsplit=2,
           chunks=[5, 4]),
         G("split (132,100,544)x3 ld+1 strided C", 132, 100, 544, (545, 1, 132 * 545 + 3, 0, 0),
           (1, 545, 100 * 545 + 1, 0, 0), (2 * 100 + 3, 2, 132 * 203 + 5, 0, 0), batch=3, modes=(2, 2), nsplit=4,
           chunks=[5, 5, 5, 2]),
         G("split (36,28,1056)x2 bdiv=2", 36, 28, 1056, (1056, 1, 0, 36 * 1056, 0), (1, 1056, 0, 28 * 1056, 0),
           (28, 1, 0, 36 * 28, 0), batch=2, bdiv=2, modes=(0, 0), nsplit=7, chunks=[5] * 6 + [3]),
         G("split (8,200,2048)", 8, 200, 2048, opA(8, 2048, 0), opB(2048, 200, 1), modes=(0, 1), nsplit=16,
           chunks=[4] * 16)]
    return o


GEMM_MODES = _modes()
GEMM_SCALAR = _scalar()
GEMM_EDGES = _edges()
GEMM_BATCH = _batch()
GEMM_SPLIT = _split()
GEMM_NOSPLIT = [G("nosplit K=224", 36, 40, 224, opA(36, 224, 0), opB(224, 40, 0)),
                G("nosplit 256 tiles", 4, 4, 256, (256, 1, 4 * 256, 0, 0), (1, 256, 4 * 256, 0, 0), batch=256)]
GEMM_ALL = GEMM_MODES + GEMM_SCALAR + GEMM_EDGES + GEMM_BATCH + GEMM_SPLIT + GEMM_NOSPLIT

GEMM_MUTANTS = ["drop_last_k", "drop_last_chunk", "drop_split", "skip_last_row", "skip_last_col", "bias_by_row",
                "beta_ignored", "beta_on_partials", "alpha_twice", "bdiv_swapped", "a_strides_swapped", "trunc10"]


def trunc10(a):
    """operand mantissas truncated to 10 bits (what a TF32-style product would read)"""
    return (f32(a).view(np.uint32) & np.uint32(0xFFFFE000)).view(F32)


def gemm_applies(c, mut):
    ns = c.nsplit
    if mut in ("drop_last_k", "drop_last_chunk", "trunc10"):
        return c.K > 0
    if mut == "drop_split":
        return ns > 1
    if mut == "bias_by_row":
        return c.bias and c.M * c.N > 1 and c.N > 1
    if mut == "beta_ignored":
        return c.beta != 0
    if mut == "beta_on_partials":
        return c.beta != 0 and ns > 1
    if mut == "alpha_twice":
        return ns > 1 and c.alpha not in (0.0, 1.0)
    if mut == "bdiv_swapped":
        return c.K > 0 and any(not np.array_equal(c.idx(o), c.idx(o, swap_z=True)) for o in "ABC")
    if mut == "a_strides_swapped":
        return c.K > 0 and not np.array_equal(c.idx("A"), c.idx("A", swap_s=True))
    return True


def ref_gemm(c, inp, mutant=None):
    """float64: (C elements [batch][M][N], S of the gate); C0 = the elements' previous contents"""
    sw = mutant == "bdiv_swapped"
    ia = c.idx("A", swap_z=sw, swap_s=mutant == "a_strides_swapped")
    ib, ic = c.idx("B", swap_z=sw), c.idx("C", swap_z=sw)
    A = inp["A"][ia % max(inp["A"].size, 1)] if ia.size else np.zeros(ia.shape, F32)
    B = inp["B"][ib % max(inp["B"].size, 1)] if ib.size else np.zeros(ib.shape, F32)
    C0 = inp["C"][ic % inp["C"].size].astype(F64)
    if mutant == "trunc10":
        A, B = trunc10(A), trunc10(B)
    A, B = A.astype(F64), B.astype(F64)
    keep = np.ones(c.K, bool)
    if mutant == "drop_last_k":
        keep[-1] = False
    elif mutant == "drop_last_chunk":
        keep[32 * ((c.K - 1) // 32):] = False
    elif mutant == "drop_split":
        k0 = 32 * c.chunks[0]
        keep[k0:k0 + 32 * c.chunks[1]] = False
    acc = np.einsum("zmk,zkn->zmn", A[:, :, keep], B[:, keep, :])
    S = abs(c.alpha) * np.einsum("zmk,zkn->zmn", np.abs(A), np.abs(B))
    alpha = c.alpha * c.alpha if mutant == "alpha_twice" else c.alpha
    beta = {"beta_ignored": 0.0, "beta_on_partials": c.beta * c.nsplit}.get(mutant, c.beta)
    out = alpha * acc
    if beta != 0:
        out = out + beta * C0
    if c.beta != 0:
        S = S + abs(c.beta) * np.abs(C0)
    if c.bias:
        b = inp["bias"].astype(F64)
        out = out + (b[np.arange(c.M) % c.N][None, :, None] if mutant == "bias_by_row" else b[None, None, :])
        S = S + np.abs(b)[None, None, :]
    if mutant == "skip_last_row":
        out[:, -1, :] = PATF
    if mutant == "skip_last_col":
        out[:, :, -1] = PATF
    return out, S


def f32_gemm(c, inp):
    """the reference as a float32 fma chain in plain k order (each fma: exact product, one rounding)"""
    A = inp["A"][c.idx("A")] if c.K else np.zeros((c.batch, c.M, 0), F32)
    B = inp["B"][c.idx("B")] if c.K else np.zeros((c.batch, 0, c.N), F32)
    acc = np.zeros((c.batch, c.M, c.N), F32)
    for k in range(c.K):
        acc = (acc.astype(F64) + A[:, :, k, None].astype(F64) * B[:, k, None, :].astype(F64)).astype(F32)
    o = (F32(c.alpha) * acc).astype(F32)
    if c.beta != 0:
        o = (o.astype(F64) + F64(F32(c.beta)) * inp["C"][c.idx("C")].astype(F64)).astype(F32)
    if c.bias:
        o = (o + inp["bias"][None, None, :]).astype(F32)
    return o


def gate_sum(got, ref, S, n, nsplit=0, scale=1.0, extra=0.0):
    return _worst(_diff(got, ref), scale * (n + nsplit + 4) * U24 * np.asarray(S, F64) + extra)


def rms(got, ref):
    d = _diff(got, ref)
    return float(np.sqrt(np.mean(np.where(np.isfinite(d), d, np.inf) ** 2))) if d.size else 0.0


def gate_rms(got, ref, ref32):
    return rms(got, ref), 4.0 * rms(ref32, ref)


def gemm_gates(c, got, ref, S, nsplit=0, ref32=None):
    """[(name, (err, bound))]: the per-element gate, and for K > 300 the RMS gate"""
    g = [("elem", gate_sum(got, ref, S, c.K, nsplit))]
    if c.K > LONG:
        g.append(("rms", gate_rms(got, ref, ref32 if ref32 is not None else f32_gemm(c, c.inputs()))))
    return g


# ------------------------------------------------------------------------------------ tcx_linear_ws
LINEAR_SHAPES = [(65, 40, 260, 132), (65, 40, 260, 0)]
LINEAR_CASES = [(s, act, rb) for s in LINEAR_SHAPES for act in range(4) for rb in (True, False)]


def linear_inputs(M, N, K1, K2):
    r = T.rng(seed_of(f"linear {M} {N} {K1} {K2}"))
    g = lambda *s: f32(r.standard_normal(s))
    sc = 1.0 / np.sqrt(K1 + K2)
    return dict(x1=g(M, K1), x2=g(M, K2) if K2 else None, w=f32(g(N, K1 + K2) * sc), b=g(N), resid=g(M, N))


def act_np(v, act, dt):
    v = v.astype(dt)
    one = dt(1)
    if act == 1:
        return np.maximum(v, dt(0))
    if act == 2:
        return (one / (one + np.exp(-v))).astype(dt)
    if act == 3:
        return (v / (one + np.exp(-v))).astype(dt)
    return v


def ref_linear(inp, act, rb, mutant=None):
    """float64 (y, S): S = sum |x||w| + |b| + |resid|"""
    x = inp["x1"] if inp["x2"] is None else np.concatenate([inp["x1"], inp["x2"]], 1)
    if mutant == "x2_from_x1" and inp["x2"] is not None:
        x = np.concatenate([inp["x1"], inp["x1"][:, :inp["x2"].shape[1]]], 1)
    x, w = x.astype(F64), inp["w"].astype(F64)
    if mutant == "trunc10":
        x, w = trunc10(x).astype(F64), trunc10(w).astype(F64)
    if mutant == "drop_last_k":
        x = x[:, :-1]
        w = w[:, :-1]
    pre, S = x @ w.T, np.abs(x) @ np.abs(w).T
    if rb and mutant != "no_bias":
        pre, S = pre + inp["b"].astype(F64)[None], S + np.abs(inp["b"].astype(F64))[None]
    if rb and mutant != "no_resid":
        pre, S = pre + inp["resid"].astype(F64), S + np.abs(inp["resid"].astype(F64))
    return act_np(pre, 0 if mutant == "no_act" else act, F64), S


def f32_linear(inp, act, rb):
    x = inp["x1"] if inp["x2"] is None else np.concatenate([inp["x1"], inp["x2"]], 1)
    w = inp["w"]
    acc = np.zeros((x.shape[0], w.shape[0]), F32)
    for k in range(x.shape[1]):
        acc = (acc.astype(F64) + x[:, k, None].astype(F64) * w[None, :, k].astype(F64)).astype(F32)
    if rb:
        acc = ((acc + inp["b"][None]).astype(F32) + inp["resid"]).astype(F32)
    return act_np(acc, act, F32)


def gate_linear(got, ref, S, n, nsplit, ref32=None):
    """1.1 x the GEMM bound + 4 * 2^-24 |ref|; where the float32 evaluation itself misses that, 4 x its
    error (train_ops_ref._f32_floor; T.FALLBACK then holds that error)"""
    ref = np.asarray(ref, F64)
    b = 1.1 * (n + nsplit + 4) * U24 * np.asarray(S, F64) + 4 * U24 * np.abs(ref)
    return _worst(_diff(got, ref), np.maximum(b, T._f32_floor(ref32, ref, b)))


# ------------------------------------------------------------------------------------ conv weight gradient
class Wc:
    """One tcx_conv_wgrad call: shape = (B, H, W, C1, C2, Cout, ks, stride, pad, circular)"""

    def __init__(self, shape, beta=0.0, shift_x=0, shift_dy=0, nan_dw=False, inst=None, splits=None, tag=""):
        self.shape, self.beta, self.shift_x, self.shift_dy, self.nan_dw = tuple(shape), beta, shift_x, shift_dy, nan_dw
        self.inst, self.splits, self.tag = inst, splits, tag  # inst, splits: the table's claims

    def __repr__(self):
        return f"{self.shape} beta={self.beta}" + (f" x1+{self.shift_x}B" if self.shift_x else "") \
            + (f" dy+{self.shift_dy}B" if self.shift_dy else "") + (" NaN dw" if self.nan_dw else "") + self.tag

    def dims(self):
        B, H, W, C1, C2, Cout, ks, s, p, circ = self.shape
        Ho, Wo = (H + 2 * p - ks) // s + 1, (W + 2 * p - ks) // s + 1
        return Ho, Wo, B * Ho * Wo, ks * ks * (C1 + C2)

    def expect_inst(self):
        """<NT, ASC, BSC> of k_wgrad, or 'thin'"""
        B, H, W, C1, C2, Cout, ks, s, p, circ = self.shape
        Ho, Wo, M, K = self.dims()
        if thin_takes(self.shape, self.shift_x) and self.shift_dy % 16 == 0 and (Ho, Wo) == (H, W):
            return "thin"
        asc = C1 % 4 != 0 or C2 % 4 != 0 or self.shift_x % 16 != 0
        return wgrad_plan(M, K, Cout)[0], asc, Cout % 4 != 0 or self.shift_dy % 16 != 0

    def expect_splits(self):
        Ho, Wo, M, K = self.dims()
        _, ns, cps = wgrad_plan(M, K, self.shape[5])
        nch = cdiv(max(M, 1), 32)
        return [min(cps, nch - s * cps) for s in range(ns)]

    def inputs(self):
        B, H, W, C1, C2, Cout, ks, s, p, circ = self.shape
        Ho, Wo, M, K = self.dims()
        r = T.rng(seed_of(repr(self.shape)))
        g = lambda *sh: f32(r.standard_normal(sh))
        return dict(x1=g(B, H, W, C1), x2=g(B, H, W, C2) if C2 else None, dy=f32(g(B, Ho, Wo, Cout) * 0.1),
                    dw0=g(Cout, C1 + C2, ks, ks))


def _wgrad_inst():
    o = []
    for Cout, nt in ((20, 1), (21, 1), (36, 2), (37, 2), (100, 3), (101, 3)):
        for C1, C2 in ((12, 4), (6, 0)):
            o.append(Wc((1, 9, 7, C1, C2, Cout, 3, 1, 1, 1), inst=(nt, C1 % 4 != 0, Cout % 4 != 0), splits=[2]))
    o.append(Wc((1, 9, 7, 12, 4, 20, 3, 1, 1, 1), shift_x=4, inst=(1, True, False), splits=[2]))
    o.append(Wc((1, 9, 7, 12, 4, 36, 3, 1, 1, 1), shift_dy=4, inst=(2, False, True), splits=[2]))
    o.append(Wc((1, 9, 7, 12, 4, 100, 3, 1, 1, 1), shift_x=4, shift_dy=4, inst=(3, True, True), splits=[2]))
    return o


WGRAD_INST = _wgrad_inst()
WGRAD_GEOM = [Wc(s, inst=(1, False, False)) for s in [
    (2, 5, 6, 8, 0, 20, 1, 1, 0, 0),    # 1x1
    (2, 5, 6, 8, 0, 20, 3, 1, 0, 0),    # valid
    (2, 7, 6, 8, 0, 20, 3, 2, 1, 1),    # stride 2, odd H
    (2, 7, 6, 8, 0, 20, 3, 2, 1, 0),
    (2, 10, 6, 8, 0, 20, 4, 2, 1, 0),   # the 4x4 / stride-2 downsample, zero
    (2, 10, 6, 8, 0, 20, 4, 2, 1, 1),   # ... and circular
    (2, 6, 5, 8, 0, 20, 5, 1, 2, 1),    # pad 2: the wrap reaches two rows / columns across
    (3, 1, 1, 8, 0, 20, 3, 1, 1, 1),    # all nine taps read the one pixel
    (2, 2, 3, 8, 0, 20, 3, 1, 1, 1),
    (2, 2, 3, 8, 0, 20, 3, 1, 1, 0),
]]
WGRAD_SPLIT = [Wc((2, 16, 16, 8, 0, 32, 3, 1, 1, 1), inst=(1, False, False), splits=[8, 8]),
               Wc((1, 17, 32, 8, 0, 32, 3, 1, 1, 1), inst=(1, False, False), splits=[9, 8]),
               Wc((2, 16, 41, 8, 0, 32, 3, 1, 1, 1), inst=(1, False, False), splits=[9, 9, 9, 9, 5])]
_BETA_SHAPE = (1, 9, 7, 12, 4, 20, 3, 1, 1, 1)
WGRAD_BETA = [Wc(_BETA_SHAPE, beta=b, inst=(1, False, False)) for b in (0.0, 1.0, -0.5)] \
    + [Wc(_BETA_SHAPE, nan_dw=True, inst=(1, False, False)), Wc((2, 16, 16, 8, 0, 32, 3, 1, 1, 1), beta=-0.5,
                                                                 inst=(1, False, False), splits=[8, 8])]
_THIN_SHAPE = (2, 6, 5, 1, 0, 32, 3, 1, 1, 1)
WGRAD_THIN_EDGE = [Wc((2, 6, 5, 1, 0, 6, 3, 1, 1, 1), inst=(1, True, True), tag=" Cout%4"),
                   Wc((2, 6, 6, 1, 0, 8, 4, 2, 1, 1), inst=(1, True, False), tag=" 4x4 s2"),
                   Wc((2, 6, 5, 16, 0, 1, 3, 1, 0, 0), inst=(1, False, True), tag=" Cout=1 pad 0"),
                   Wc(_THIN_SHAPE, shift_x=4, inst=(1, True, False), tag=" declined"),
                   Wc((2, 3, 1, 1, 0, 32, 3, 1, 1, 1), inst=(1, True, False), tag=" W=1 circular"),
                   Wc(_THIN_SHAPE, inst="thin", tag=" taken")]
WGRAD_ALL = WGRAD_INST + WGRAD_GEOM + WGRAD_SPLIT + WGRAD_BETA + WGRAD_THIN_EDGE
# (H = W, ks, pad, stride, circular) that both weight-gradient entry points refuse
WGRAD_BAD_GEOMETRY = [(1, 4, 1, 2, 1), (1, 4, 1, 2, 0), (1, 5, 2, 1, 1), (0, 3, 1, 1, 1)]

WGRAD_MUTANTS = ["kykx_transposed", "stride_ignored", "zero_for_wrap", "wrap_for_zero", "src2_from_src1",
                 "drop_last_chunk", "beta_dropped", "layout_co_ky_kx_ci"]


def wgrad_applies(c, mut):
    B, H, W, C1, C2, Cout, ks, s, p, circ = c.shape
    return {"kykx_transposed": ks > 1 and (H, W) != (1, 1), "stride_ignored": s > 1, "zero_for_wrap": p > 0 and circ,
            "wrap_for_zero": p > 0 and not circ, "src2_from_src1": C2 > 0, "drop_last_chunk": B > 0,
            "beta_dropped": c.beta != 0, "layout_co_ky_kx_ci": ks > 1 and C1 + C2 > 1}[mut]


def im2col(x, ks, stride, pad, circular, Ho, Wo):
    """[B*Ho*Wo][ks*ks*C] with k = (ky*ks + kx)*C + c (restated from tests/test_gpu_wgrad.py)"""
    B, H, W, C = x.shape
    cols = np.zeros((B, Ho, Wo, ks, ks, C), x.dtype)
    for ky in range(ks):
        for kx in range(ks):
            ys, xs = np.arange(Ho) * stride - pad + ky, np.arange(Wo) * stride - pad + kx
            if circular:
                cols[:, :, :, ky, kx, :] = x[:, ys % H][:, :, xs % W]
            else:
                vy, vx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
                sub = x[:, np.clip(ys, 0, H - 1)][:, :, np.clip(xs, 0, W - 1)]
                cols[:, :, :, ky, kx, :] = sub * vy[None, :, None, None] * vx[None, None, :, None]
    return cols.reshape(B * Ho * Wo, ks * ks * C)


def _wgrad_operands(c, inp, mutant=None):
    B, H, W, C1, C2, Cout, ks, s, p, circ = c.shape
    Ho, Wo, M, K = c.dims()
    x2 = inp["x2"]
    if mutant == "src2_from_src1":
        x2 = inp["x1"][..., :C2]
    x = inp["x1"] if x2 is None else np.concatenate([inp["x1"], x2], 3)
    if mutant in ("zero_for_wrap", "wrap_for_zero"):
        circ = not circ
    cols = im2col(x, ks, 1 if mutant == "stride_ignored" else s, p, circ, Ho, Wo)
    return cols, inp["dy"].reshape(M, Cout)


def _to_dw(kc, c):
    B, H, W, C1, C2, Cout, ks, s, p, circ = c.shape
    return kc.reshape(ks, ks, C1 + C2, Cout).transpose(3, 2, 0, 1)


def ref_wgrad(c, inp, mutant=None):
    """float64 (dw [Cout][Cin][ks][ks], S of the gate)"""
    cols, dy = _wgrad_operands(c, inp, mutant)
    cols, dy = cols.astype(F64), dy.astype(F64)
    M = cols.shape[0]
    m1 = 32 * ((M - 1) // 32) if mutant == "drop_last_chunk" else M
    dw = _to_dw(cols[:m1].T @ dy[:m1], c)
    S = _to_dw(np.abs(cols).T @ np.abs(dy), c)
    if c.beta != 0:
        S = S + abs(c.beta) * np.abs(inp["dw0"].astype(F64))
        if mutant != "beta_dropped":
            dw = dw + c.beta * inp["dw0"].astype(F64)
    if mutant == "kykx_transposed":
        dw = dw.transpose(0, 1, 3, 2)
    if mutant == "layout_co_ky_kx_ci":
        dw = np.ascontiguousarray(dw.transpose(0, 2, 3, 1)).reshape(dw.shape)
    return np.ascontiguousarray(dw), S


def f32_wgrad(c, inp):
    """the reference as a float32 fma chain in pixel order"""
    cols, dy = _wgrad_operands(c, inp)
    acc = np.zeros((cols.shape[1], dy.shape[1]), F32)
    for m in range(cols.shape[0]):
        acc = (acc.astype(F64) + cols[m, :, None].astype(F64) * dy[m, None, :].astype(F64)).astype(F32)
    dw = _to_dw(acc, c)
    if c.beta != 0:
        dw = (dw.astype(F64) + F64(F32(c.beta)) * inp["dw0"].astype(F64)).astype(F32)
    return np.ascontiguousarray(dw)


def wgrad_gates(c, got, ref, S, ref32=None):
    Ho, Wo, M, K = c.dims()
    ns = len(c.expect_splits())
    g = [("elem", gate_sum(got, ref, S, M, ns))]
    if M > LONG:
        g.append(("rms", gate_rms(got, ref, ref32 if ref32 is not None else f32_wgrad(c, c.inputs()))))
    return g


def all_ok(gates):
    return all(ok(eb) for _, eb in gates)
