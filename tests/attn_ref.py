"""Reference, codecs, restated dispatch, inputs, gates, emulations and mutants for the attention kernels of
csrc/attention.hip and csrc/attention_split.hip (no GPU import).  tests/test_attn_ref_cpu.py proves the gates
on the CPU (every emulation inside, every mutant outside); tests/test_gpu_attn.py runs the same cases, inputs
and gates through the C ABI.

The reference is float64 numpy on the values the kernel receives: every input is made representable in the
entry's storage format before the reference sees it (`representable`).  Every gate returns (measured error,
bound) at the element where error - bound is largest, as train_ops_ref does; `ok` / `FALLBACK` are its.

Storage formats (csrc/h2.hpp), restated here independent of the GPU writers:
  f32   plain float32
  h2    [..][C/8][2][8] f16: 8 hi halves then 8 lo halves per 8-channel group, hi = f16(v), lo = f16(v - hi)
  bf16  the same records with bf16 halves; a bf16 product reads the hi halves only, so the value a bf16
        record stands for as an INPUT is its hi half; as an OUTPUT both halves are written
  b2    plain [..][C] bf16 (the records' hi halves)
"""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np

import train_ops_ref as T
from train_ops_ref import F32, F64, U24, ok  # noqa: F401

U = U24                      # float32 unit roundoff 2^-24
LOG2E = 1.4426950408889634
DIMS = (8, 16, 24, 32, 48, 64)     # head dims of k_attention / k_attention_mfma
DIMS_LONG = (16, 32, 48, 64)       # of k_attention_flash / k_attention_split
ENTRIES = ("attention", "attention_h2", "split", "split_bf16", "split_b2")
FMT_IN = {"attention": "f32", "attention_h2": "f32", "split": "h2", "split_bf16": "bf16", "split_b2": "b2"}
FMT_OUT = {"attention": "f32", "attention_h2": "h2", "split": "h2", "split_bf16": "bf16", "split_b2": "b2"}


# ------------------------------------------------------------------------------------ codecs
def bf16_bits(x):
    """float -> uint16 bf16 bit patterns, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return ((u + (((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF))) >> np.uint32(16)).astype(np.uint16)


def bf16_val(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(F32)


def bf16(x):
    """round to bf16 and back to float32"""
    return bf16_val(bf16_bits(x))


def f16(x):
    return np.asarray(x, dtype=F32).astype(np.float16).astype(F32)


def _split(x, fmt):
    """(hi, lo) as uint16 bit patterns of the float32 values x"""
    x = np.ascontiguousarray(x, dtype=F32)
    if fmt == "h2":
        hi = x.astype(np.float16)
        lo = (x - hi.astype(F32)).astype(np.float16)
        return hi.view(np.uint16), lo.view(np.uint16)
    hi = bf16_bits(x)
    return hi, bf16_bits(x - bf16_val(hi))


def _halves(u, fmt):
    u = np.asarray(u, dtype=np.uint16)
    return u.view(np.float16).astype(F64) if fmt == "h2" else bf16_val(u).astype(F64)


def encode(x, fmt):
    """values [.., C] -> the storage: f32 float32 [.., C]; h2 / bf16 uint16 [.., C/8, 2, 8]; b2 uint16 [.., C]"""
    if fmt == "f32":
        return np.ascontiguousarray(x, dtype=F32)
    if fmt == "b2":
        return bf16_bits(x)
    assert x.shape[-1] % 8 == 0
    hi, lo = _split(x, fmt)
    g = x.shape[:-1] + (x.shape[-1] // 8, 8)
    return np.ascontiguousarray(np.stack([hi.reshape(g), lo.reshape(g)], axis=-2))


def decode(u, fmt, lo=True):
    """storage -> float64 values [.., C]; records: hi + lo, or the hi halves alone (lo=False)"""
    if fmt == "f32":
        return np.asarray(u, dtype=F64)
    if fmt == "b2":
        return _halves(u, "bf16")
    h = _halves(u[..., 0, :], fmt)
    v = h + _halves(u[..., 1, :], fmt) if lo else h
    return v.reshape(u.shape[:-3] + (u.shape[-3] * 8,))


def representable(x, fmt):
    """the values the encoded tensor stands for as a kernel INPUT (bf16 records: the hi halves)"""
    return decode(encode(x, fmt), fmt, lo=(fmt == "h2"))


def nbytes(n_elem, fmt):
    return n_elem * (2 if fmt == "b2" else 4)


# ------------------------------------------------------------------------------------ dispatch, restated
def branch(entry, N, D, Bt=1, heads=1):
    """the host code of tcx_attention / tcx_attention_h2 (attention.hip) and attention_split (attention_split.hip)"""
    if heads <= 0 or heads > 65535 or Bt < 0 or Bt > 65535 or N <= 0:
        return "refused"
    if entry == "attention":
        if not (N <= 256 or N % 256 == 0):
            return "refused"
        if N > 256:
            return "flash" if D in DIMS_LONG else "unsupported"
        if D not in DIMS:
            return "unsupported"
        return "mfma" if N % 32 == 0 else "valu"
    if entry == "attention_h2":
        if (D * heads) % 8 or not ((N <= 256 and N % 32 == 0) or N % 256 == 0):
            return "refused"
        if N > 256:
            return "flash" if D in DIMS_LONG else "unsupported"
        return "mfma" if D in DIMS else "unsupported"
    assert entry in ("split", "split_bf16", "split_b2"), entry
    if N % 256:
        return "refused"
    if D not in DIMS_LONG:
        return "unsupported"
    return "split_pf2" if entry != "split" and N >= 512 else "split"


def instantiation(entry, N, D):
    """the kernel template instance a served call launches"""
    b = branch(entry, N, D)
    if b == "valu":
        return f"k_attention<{D}>"
    if b == "mfma":
        return f"k_attention_mfma<{D}>"
    if b == "flash":
        return f"k_attention_flash<{D}>"
    fmt = {"split": 0, "split_bf16": 1, "split_b2": 2}[entry]
    return f"k_attention_split<{D}, {fmt}, {int(b == 'split_pf2')}>"


ALL_INSTANTIATIONS = ([f"k_attention<{d}>" for d in DIMS] + [f"k_attention_mfma<{d}>" for d in DIMS] +
                      [f"k_attention_flash<{d}>" for d in DIMS_LONG] +
                      [f"k_attention_split<{d}, 0, 0>" for d in DIMS_LONG] +
                      [f"k_attention_split<{d}, {f}, {p}>" for d in DIMS_LONG for f in (1, 2) for p in (0, 1)])
assert len(ALL_INSTANTIATIONS) == 36


# ------------------------------------------------------------------------------------ float64 reference
Ref = namedtuple("Ref", "o P A sabs sig vmax")


def heads_of(qkv, heads, interleaved=False):
    """[Bt, N, 3C] -> q, k, v as [Bt, heads, N, d]: channels q | k | v, head h owns h*d .. h*d+d"""
    Bt, N, C3 = qkv.shape
    C = C3 // 3
    d = C // heads

    def sp(a):
        if interleaved:
            return a.reshape(Bt, N, d, heads).transpose(0, 3, 1, 2)
        return a.reshape(Bt, N, heads, d).transpose(0, 2, 1, 3)
    return sp(qkv[..., :C]), sp(qkv[..., C:2 * C]), sp(qkv[..., 2 * C:])


def merge(o):
    """[Bt, heads, N, d] -> [Bt, N, C]"""
    Bt, h, N, d = o.shape
    return np.ascontiguousarray(o.transpose(0, 2, 1, 3)).reshape(Bt, N, h * d)


def sdpa64(qkv, heads):
    """out [Bt, N, C] = softmax(q k^T / sqrt(d)) v in float64, with what the gates need:
    P [Bt, heads, N, N]; A[q, c] = sum_j P |v|; sabs[q, c] = max_j sum_c |q_c k_c| / sqrt(d) of the row's head;
    sig[q, c] = sqrt(sum_j P (v - o)^2); vmax[q, c] = max_j |v[j, c]|"""
    qkv = np.asarray(qkv, dtype=F64)
    q, k, v = heads_of(qkv, heads)
    d = q.shape[-1]
    scale = 1.0 / math.sqrt(d)
    s = q @ k.transpose(0, 1, 3, 2) * scale
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    o = p @ v
    sig = np.sqrt(np.maximum(p @ (v * v) - o * o, 0.0))
    sabs = (np.abs(q) @ np.abs(k).transpose(0, 1, 3, 2)).max(-1, keepdims=True) * scale
    vmax = np.broadcast_to(np.abs(v).max(2, keepdims=True), v.shape)
    return Ref(merge(o), p, merge(p @ np.abs(v)), merge(np.broadcast_to(sabs, o.shape)), merge(sig), merge(vmax))


# ------------------------------------------------------------------------------------ cases and inputs
class Case(namedtuple("Case", "entry branch N D heads Bt family arg")):
    """one call: `branch` is the dispatch branch the case claims (checked on the CPU)"""
    __slots__ = ()

    def __repr__(self):
        a = "" if self.arg is None else f"({self.arg:g})"
        return f"{self.entry}-{self.branch}-N{self.N}-D{self.D}-h{self.heads}-B{self.Bt}-{self.family}{a}"

    @property
    def C(self):
        return self.D * self.heads

    @property
    def fmt_in(self):
        return FMT_IN[self.entry]

    @property
    def fmt_out(self):
        return FMT_OUT[self.entry]

    @property
    def ones(self):
        """bf16 forms at D = 16 / 48: l is the MFMA's own sum of the rounded P (the ONES row)"""
        return self.entry in ("split_bf16", "split_b2") and self.D % 32 != 0

    @property
    def ntile(self):
        return self.N // 128 if self.branch in ("flash", "split", "split_pf2") else 1


def onehot_perm(N, b=0, h=0):
    """pi(i) = (m i + s) mod N, m the first integer >= 0.618 N coprime to N: neighbouring queries look at keys
    0.6 N apart, so pi crosses 32-key sub-tiles, 128-key tiles and 256-query blocks; s differs per (image, head)"""
    m = max(1, int(0.618 * N))
    while math.gcd(m, N) != 1:
        m += 1
    return (m * np.arange(N) + 1 + 7 * b + 3 * h) % N


def onehot_codes(N, d):
    """+-1 codes of the key index: bit (c mod nb) of j on dim c, nb = max(8, bits of N - 1) <= d, spread
    over the head dim, so two keys differ on at least d // nb dims; returns (codes [N, d], amplitude a) with
    a^2 * 2 * (d // nb) / sqrt(d) >= 40: the matching key leads every other by 40 natural-log units"""
    nb = max(8, int(N - 1).bit_length())
    assert nb <= d, (N, d)
    bit = (np.arange(N)[:, None] >> (np.arange(d) % nb)[None, :]) & 1
    need = 20.5 * math.sqrt(d) / (d // nb)
    a = math.ceil(math.sqrt(need) * 4) / 4     # a multiple of 1/4 below 16: exact in bf16 and f16
    return (2.0 * bit - 1.0), a


def onehot_v(N, C, fmt):
    """v[j, c] names (j, c): distinct over j at a fixed c and over c at a fixed j, exact in the format.
    f32 / h2: (512 j + c + 1) 2^-12, 20 significant bits, the h2 lo half normal.
    bf16 / b2: sign * (1 + m / 128) * 2^e, m = (j + 37 c) mod 128 (37 odd: distinct over c mod 128),
    e = j // 128 - 4 + 8 (c // 256), sign = (-1)^(c // 128)."""
    j, c = np.arange(N)[:, None], np.arange(C)[None, :]
    if fmt in ("f32", "h2"):
        assert N <= 2048 and C <= 511
        return (512.0 * j + c + 1.0) * 2.0 ** -12
    assert N <= 1024 and C <= 512
    m = (j + 37 * c) % 128
    return np.where((c // 128) % 2 == 1, -1.0, 1.0) * (1.0 + m / 128.0) * 2.0 ** (j // 128 - 4 + 8 * (c // 256))


ALPHA = 4.0   # q's component along the steering dim 0 of rising / falling / threshold


def steer(N, d, rise_log2):
    """k's dim-0 value per 128-key tile so that ALPHA * k0 / sqrt(d) * log2(e) = rise_log2[tile]"""
    t = np.arange(N) // 128
    return np.asarray(rise_log2, dtype=F64)[t] * math.log(2.0) * math.sqrt(d) / ALPHA


def make_inputs(c):
    """qkv [Bt, N, 3C] float64, representable in the entry's input format; deterministic from the case"""
    N, d, H, Bt, C = c.N, c.D, c.heads, c.Bt, c.C
    seed = (ENTRIES.index(c.entry) * 7919 + N * 31 + d * 17 + H * 5 + Bt) * 13 + len(c.family)
    g = T.rng(seed)
    q = g.standard_normal((Bt, H, N, d))
    k = g.standard_normal((Bt, H, N, d))
    v = g.standard_normal((Bt, H, N, d))
    nt = max(1, N // 128)
    if c.family == "gauss":
        q, k, v = q * c.arg, k * c.arg, v * c.arg
    elif c.family == "onehot":
        codes, a = onehot_codes(N, d)
        vv = onehot_v(N, C, c.fmt_in)
        for b in range(Bt):
            for h in range(H):
                q[b, h] = a * codes[onehot_perm(N, b, h)]
                k[b, h] = a * codes
                v[b, h] = vv[:, h * d:(h + 1) * d]
    elif c.family == "uniform":
        k[:] = k[:, :, :1, :]
    elif c.family == "constv":
        v[:] = v[:, :, :1, :]
    elif c.family in ("rising", "falling"):
        sgn = 1.0 if c.family == "rising" else -1.0
        q *= 0.5
        k *= 0.5
        q[..., 0] = ALPHA
        k[..., 0] = steer(N, d, sgn * c.arg * np.arange(nt))
    elif c.family == "threshold":
        q *= 0.02
        k *= 0.02
        q[..., 0::2, 0] = ALPHA * 7.75 / 8    # 3.875: the maximum rises by 7.75 log2 units, under the threshold
        q[..., 1::2, 0] = ALPHA * 8.25 / 8    # 4.125: by 8.25, over it
        k[..., 0] = steer(N, d, [0.0] + [8.0] * (nt - 1))
    else:
        raise ValueError(c.family)
    qkv = np.concatenate([merge(q), merge(k), merge(v)], axis=-1)
    return representable(qkv, c.fmt_in)


@lru_cache(maxsize=None)
def _cached(c):
    qkv = make_inputs(c)
    qkv.setflags(write=False)
    return qkv, sdpa64(qkv, c.heads)


def inputs(c):
    return _cached(c)[0]


def reference(c):
    return _cached(c)[1]


# ------------------------------------------------------------------------------------ gates
# Score error E_q (natural-log units), fp32 forms: the d-term dot product accumulates in fp32 (d roundings,
# each at most u of the running sum of |q_c k_c|), then one multiply by the scale and one subtraction of the
# maximum: E_q <= (d + 2) u max_j sum_c |q_c k_c| scale = (d + 2) u sabs.
#
# A relative error e_j on every p_j moves o = sum p_j v_j / sum p_j by at most
# sum p |e| |v| + |o| sum p |e| <= 2 max|e| A, A = sum_j P |v| >= |o|; hence the trailing 2 A.
# e_j is 2 E_q (the score's and the row maximum's) plus c1 u, c1 term by term:
#   2            expf / v_exp_f32 within 1 ulp = 2 u
#   N - 1        the adds of the N-term sum l
#   N            the N fused multiply-adds of sum_j p_j v_j
#   2            1 / l within 1 ulp
#   1            o * (1 / l)
#   0            the fp32 store
#   3 (nt - 1)   key-tiled forms, per further tile: alpha = exp (2 u) and one multiply of O and of l (1 u)
def c1(c):
    return 2 + (c.N - 1) + c.N + 2 + 1 + 3 * (c.ntile - 1)


def e_q(c, ref):
    e = (c.D + 2) * U * ref.sabs
    if c.entry == "split":
        # f16x3: q k = hi hi + hi lo + lo hi; the dropped lo lo and the two split residuals are each below
        # 2^-22 of |q k|: 3 * 2^-22 of sum |q k| scale
        e = e + 3 * 2.0 ** -22 * ref.sabs
    return e


def out_rounding(c, o, lo=False):
    """the output format's own rounding of the value o"""
    o = np.abs(o)
    if c.fmt_out == "f32":
        return 0.0 * o
    if c.fmt_out == "h2":
        # hi + lo carry 22 bits: 2^-22 |o|; the lo half is an f16 subnormal (spacing 2^-24) below 2^-14: 2^-25
        return 2.0 ** -22 * o + 2.0 ** -25
    if lo:
        # bf16 record, both halves: lo = bf16(o - hi) with |o - hi| <= 2^-9 |o|, rounded at 2^-9: 2^-18 |o|,
        # granted as 2^-17
        return 2.0 ** -17 * o
    return 2.0 ** -9 * o      # bf16, 8 significant bits, round to nearest even


def bound(c, ref, lo=False):
    """the per-element bound [Bt, N, C] of a case, from the roundings of its form"""
    o, A = np.abs(ref.o), ref.A
    if c.family == "onehot":
        # the matching key leads by >= 40; with the score error below 1 every other p is below e^-39, so the
        # output is v[pi(i)] up to N e^-39 max|v| (in o and in l), the roundings of l = 1 + tiny, 1 / l and
        # o / l (4 u) and the output format
        return out_rounding(c, o, lo) + 4 * U * o + 2 * c.N * math.exp(-39.0) * ref.vmax
    b = (2 * e_q(c, ref) + c1(c) * U) * 2 * A + out_rounding(c, o, lo)
    if c.entry == "split":
        # P 2^10 is split into f16 hi + lo: 2^-22 relative, and v p = hi hi + hi lo + lo hi drops 2^-22 more with
        # the split of v's own 2^-22: 3 * 2^-22 on 2 A.  Below the f16 normal range (p 2^10 < 2^-14) hi and lo
        # are subnormals, each within 2^-25 absolute: N terms of 2^-24 2^-10 max|v| against l >= 1
        b = b + 3 * 2.0 ** -22 * 2 * A + c.N * 2.0 ** -34 * ref.vmax
    elif c.entry in ("split_bf16", "split_b2"):
        if c.ones:
            # D = 16, 48: l is the sum of the same rounded P, so the output is a convex combination with the
            # weights p (1 + e_j), |e| <= 2^-9: its error is sum p e (v - o) / sum p (1 + e), at most
            # 2^-9 sum p |v - o| / (1 - 2^-9) <= 2 * 2^-9 sig (Cauchy-Schwarz: sum p |v - o| <= sig, where
            # sum p |v - o| <= A + |o| is the issue's (A - |o|)-like term); a constant V leaves the output
            # rounding alone
            b = b + 2 * 2.0 ** -9 * ref.sig
        else:
            # D = 32, 64: l sums the unrounded p, so sum p e v / l stays: 2^-9 A, stated as 2^-9 * 2 A
            b = b + 2.0 ** -9 * 2 * A
    return b


def needs_emul(c, lo=False):
    """The cases that are gated with their CPU emulation at hand (the 4 x fallback of train_ops_ref._f32_floor):
    the bf16 forms' hi halves.  Their output term is stated as 2^-9 |o|, but round-to-nearest bf16 (8
    significant bits) errs by up to 2^-8 |o| just above a power of two, so the bit-exact emulation itself
    misses the stated gate on a few gauss(3) cases (test_attn_ref_cpu.py lists them); everywhere else the
    emulation is inside and the stated gate stands unchanged."""
    return c.entry in ("split_bf16", "split_b2") and not lo


def gate(c, got, ref, emul=None, lo=False):
    """(err, bound) of an output against the float64 reference; `emul` (the form's CPU emulation) raises the
    bound to 4 x the emulation's error where the emulation itself misses it (train_ops_ref._f32_floor)"""
    b = bound(c, ref, lo)
    fl = T._f32_floor(emul, ref.o, b)
    return T._worst(T._diff(got, ref.o), np.maximum(b, fl))


# ------------------------------------------------------------------------------------ CPU emulations
def _emulate_bf16(c, q, k, v, defer, l_rounded):
    """k_attention_split<D, 1 | 2> as the kernel runs it: 128-key tiles, the running maximum deferred (it moves
    only when a tile's maximum passes it by more than `defer` log2 units of p; 0: the exact running maximum),
    p = exp2(s scale2 - m scale2 + 10) rounded to bf16 for the MFMA, O and l rescaled when the maximum moves.
    `l_rounded`: l sums the rounded p (the ONES row at D = 16 / 48; the VALU sum at D = 32 / 64 since the fix
    recorded in DESIGN.md); False is the D = 32 / 64 kernel before it, l from the unrounded p."""
    scale2 = F32(F32(1.0 / math.sqrt(c.D)) * F32(LOG2E))
    m = np.full(q.shape[:3] + (1,), -np.inf, F32)
    l = np.zeros_like(m)
    o = np.zeros(q.shape, F32)
    for t in range(0, c.N, 128):
        s = q @ k[:, :, t:t + 128].transpose(0, 1, 3, 2)
        mt = s.max(-1, keepdims=True)
        mn = np.where((mt - m) * scale2 > F32(defer), mt, m).astype(F32)
        alpha = np.exp2(((m - mn) * scale2).astype(F32)).astype(F32)
        mb = (-mn.astype(F64) * scale2 + 10.0).astype(F32)                       # fmaf(-mn, scale2, 10)
        p = np.exp2((s.astype(F64) * scale2 + mb).astype(F32)).astype(F32)       # exp2(fmaf(s, scale2, mb))
        pb = bf16(p)
        o = (o * alpha + pb @ v[:, :, t:t + 128]).astype(F32)
        l = (l * alpha + (pb if l_rounded else p).sum(-1, keepdims=True, dtype=F32)).astype(F32)
        m = mn
    return o, l


def emulate(c, qkv, lo=False, defer=8.0, l_rounded=True):
    """the form's arithmetic on the CPU: a float32 chain with an exact softmax (tcx_attention, tcx_attention_h2);
    the f16x3 form with the three hi / lo products and P 2^10 split into f16 hi + lo, exact softmax; the bf16
    forms key-tiled with the deferred maximum (_emulate_bf16).  Output rounded as the entry stores it."""
    q, k, v = (a.astype(F32) for a in heads_of(qkv, c.heads))
    scale = F32(1.0 / math.sqrt(c.D))
    kt = k.transpose(0, 1, 3, 2)
    if c.entry in ("split_bf16", "split_b2"):
        o, l = _emulate_bf16(c, q, k, v, defer, l_rounded)
    else:
        if c.entry == "split":
            qh, kh, vh = f16(q), f16(k), f16(v)
            ql, kl, vl = f16(q - qh), f16(k - kh), f16(v - vh)
            s = (qh @ kl.transpose(0, 1, 3, 2) + ql @ kh.transpose(0, 1, 3, 2)) + qh @ kh.transpose(0, 1, 3, 2)
        else:
            s = q @ kt
        s2 = s * F32(scale * F32(LOG2E))
        p = np.exp2(s2 - s2.max(-1, keepdims=True)).astype(F32)
        if c.entry == "split":
            p = p * F32(1024.0)
            ph = f16(p)
            pl = f16(p - ph)
            o = (pl @ vh + ph @ vl) + ph @ vh
        else:
            o = p @ v
        l = p.sum(-1, keepdims=True, dtype=F32)
    y = merge((o * (F32(1.0) / l)).astype(F32))
    if c.fmt_out == "f32":
        return y.astype(F64)
    return decode(encode(y, c.fmt_out), c.fmt_out, lo=(lo or c.fmt_out == "h2"))


# ------------------------------------------------------------------------------------ mutants
MUTANTS = ("scale_C", "heads_interleaved", "kv_swapped", "keys_swapped_in_subtile", "v_slot_groups_swapped",
           "last_tile_dropped", "last_subtile_not_in_l", "no_rescale_O", "no_rescale_l", "max_per_tile",
           "p_bf16_l_unrounded", "last_ragged_row_unwritten", "quad_ownership_rotated", "v_lo_ignored",
           "out_quads_swapped")
PATTERN = float(np.frombuffer(b"\x7b\x7b\x7b\x7b", dtype=F32)[0])   # what an unwritten output element holds


def applies(m, c):
    """the cases a mutant can be told from the truth on (its error exists there at all)"""
    tiled = c.branch in ("flash", "split", "split_pf2")
    return {"scale_C": c.heads > 1, "heads_interleaved": c.heads > 1, "keys_swapped_in_subtile": c.N >= 3,
            "v_slot_groups_swapped": c.N >= 16, "last_tile_dropped": tiled, "last_subtile_not_in_l": c.N >= 64,
            "no_rescale_O": tiled, "no_rescale_l": tiled, "max_per_tile": tiled,
            "p_bf16_l_unrounded": c.entry in ("split_bf16", "split_b2") and c.D == 16,
            "last_ragged_row_unwritten": c.branch == "valu", "quad_ownership_rotated": c.N >= 4,
            "v_lo_ignored": c.entry == "split"}.get(m, True)


def _online(s, v, m):
    """key-tiled online softmax over 128-key tiles, float64, with one of the three rescale mutants"""
    n = s.shape[-2]
    mx = np.full(s.shape[:-1] + (1,), -np.inf)
    l = np.zeros_like(mx)
    o = np.zeros(s.shape[:-1] + (v.shape[-1],))
    for t in range(0, s.shape[-1], 128):
        st = s[..., t:t + 128]
        mt = st.max(-1, keepdims=True)
        mn = mt if m == "max_per_tile" else np.maximum(mx, mt)
        al = np.ones_like(mn) if m == "max_per_tile" else np.exp(mx - mn)
        p = np.exp(st - mn)
        o = o * (1.0 if m == "no_rescale_O" else al) + p @ v[..., t:t + 128, :]
        l = l * (1.0 if m == "no_rescale_l" else al) + p.sum(-1, keepdims=True)
        mx = mn
    assert n == s.shape[-2]
    return o / l


def mutant(c, qkv, m):
    """a wrong float64 attention, [Bt, N, C]"""
    N, d = c.N, c.D
    q, k, v = heads_of(qkv, c.heads, interleaved=(m == "heads_interleaved"))
    if m == "kv_swapped":
        k, v = v, k
    scale = 1.0 / math.sqrt(c.C if m == "scale_C" else d)
    s = q @ k.transpose(0, 1, 3, 2) * scale
    if m == "v_lo_ignored":
        v = f16(v).astype(F64)
    if m in ("no_rescale_O", "no_rescale_l", "max_per_tile"):
        o = _online(s, v, m)
    else:
        if m == "last_tile_dropped":
            s, v = s[..., :N - 128], v[..., :N - 128, :]
        p = np.exp(s - s.max(-1, keepdims=True))
        l = p.sum(-1, keepdims=True)
        if m == "last_subtile_not_in_l":
            l = p[..., :N - 32].sum(-1, keepdims=True)
        if m == "p_bf16_l_unrounded":
            p = bf16(p * 1024.0).astype(F64) / 1024.0
        vv = v.copy()
        if m == "keys_swapped_in_subtile":
            vv[..., [1, 2], :] = v[..., [2, 1], :]
        if m == "v_slot_groups_swapped":
            vv[..., 0:8, :], vv[..., 8:16, :] = v[..., 8:16, :], v[..., 0:8, :]
        if m == "quad_ownership_rotated":
            n4 = N // 4 * 4
            vv[..., :n4, :] = np.roll(v[..., :n4, :].reshape(v.shape[:2] + (n4 // 4, 4, d)), 1, axis=3).reshape(
                v.shape[:2] + (n4, d))
        o = p @ vv / l
    if m == "heads_interleaved":
        Bt, H = o.shape[:2]
        y = np.ascontiguousarray(o.transpose(0, 2, 3, 1)).reshape(Bt, N, c.C)
    else:
        y = merge(o)
    if m == "last_ragged_row_unwritten":
        y[:, N - 1, :] = PATTERN
    if m == "out_quads_swapped":
        y = y.reshape(y.shape[:2] + (c.C // 8, 2, 4))[..., ::-1, :].reshape(y.shape)
    return y


# ------------------------------------------------------------------------------------ the case lists
def _mk(entry, N, D, heads, Bt, family, arg=None):
    return Case(entry, branch(entry, N, D, Bt, heads), N, D, heads, Bt, family, arg)


def _cycle(seq, i):
    return seq[i % len(seq)]


STRUCT = (("onehot", None), ("uniform", None), ("constv", None))
STEER = (("rising", 3.0), ("rising", 12.0), ("falling", 30.0), ("threshold", None), ("gauss", 3.0))
VALU_N = (1, 2, 3, 4, 5, 31, 33, 63, 65, 100, 144, 255)
MFMA_N = (32, 64, 96, 160, 224, 256)
HB_VALU = ((1, 1), (3, 2), (3, 1), (1, 2))            # (heads, Bt)
HB_MFMA = ((1, 1), (2, 3), (5, 2), (2, 1), (5, 1), (1, 3))
HB_FLASH = ((1, 1), (2, 2), (3, 1), (1, 3))
# (Bt, heads) of the split forms at N = 256: 1, 3, 9, 15 and 17 workgroups (xcd_remap: below 8, 8 + 1, two
# counts that are no multiple of 8, 2 * 8 + 1)
WG_SPLIT = ((1, 1), (1, 3), (3, 3), (3, 5), (17, 1))


def _groups():
    g = {}
    i = 0
    valu = []
    for N in VALU_N:
        for D in DIMS:
            h, b = _cycle(HB_VALU, i)
            i += 1
            valu.append(_mk("attention", N, D, h, b, "gauss", 1.0 if i % 2 else 3.0))
    for D in DIMS:   # N = 100: two query blocks, the second ragged; 3 heads
        valu += [_mk("attention", 100, D, 3, 2, f, a) for f, a in STRUCT]
    g["valu"] = valu
    mf = []
    for N in MFMA_N:
        for D in DIMS:
            h, b = _cycle(HB_MFMA, i)
            i += 1
            mf.append(_mk("attention", N, D, h, b, "gauss", 1.0 if i % 2 else 3.0))
    for j, D in enumerate(DIMS):
        mf += [_mk("attention", _cycle((96, 256, 160), j), D, 2, 2, f, a) for f, a in STRUCT]
    g["mfma"] = mf
    fl = []
    for N in (512, 768):
        for D in DIMS_LONG:
            h, b = _cycle(HB_FLASH, i)
            i += 1
            fl.append(_mk("attention", N, D, h, b, "gauss", 1.0 if i % 2 else 3.0))
    for D in DIMS_LONG:
        fl += [_mk("attention", 512, D, 2, 1, f, a) for f, a in STRUCT]
    for D, N in ((16, 768), (48, 1280)):
        fl += [_mk("attention", N, D, 1, 1, f, a) for f, a in STEER[:4]]
    g["flash"] = fl
    h2 = [_mk("attention_h2", _cycle(MFMA_N, j), D, _cycle((1, 2, 4), j) if D % 8 == 0 else 2, 2, "gauss", 1.0)
          for j, D in enumerate(DIMS)]
    h2 += [_mk("attention_h2", _cycle((512, 768), j), D, 2, 1, "gauss", 3.0) for j, D in enumerate(DIMS_LONG)]
    h2 += [_mk("attention_h2", 64, 8, 2, 1, "onehot"), _mk("attention_h2", 512, 32, 1, 1, "onehot"),
           _mk("attention_h2", 512, 64, 1, 1, "constv")]
    g["h2"] = h2
    for e in ("split", "split_bf16", "split_b2"):
        sp = []
        for N in (256, 512):
            for D in DIMS_LONG:
                h, b = _cycle(HB_FLASH, i)
                i += 1
                sp.append(_mk(e, N, D, h, b, "gauss", 1.0 if i % 2 else 3.0))
        sp += [_mk(e, 768, D, 1, 2, "gauss", 1.0) for D in (16, 48)]
        sp += [_mk(e, 256, _cycle(DIMS_LONG, j), h, b, "gauss", 3.0) for j, (b, h) in enumerate(WG_SPLIT)]
        for D in DIMS_LONG:
            for N in ((256,) if e == "split" else (256, 512)):
                sp += [_mk(e, N, D, 2, 1, f, a) for f, a in STRUCT]
        for D, N in ((16, 768), (64, 1280)):
            sp += [_mk(e, N, D, 1, 1, f, a) for f, a in STEER]
        g[e] = sp
    return g


GROUPS = _groups()
ALL_CASES = [c for cs in GROUPS.values() for c in cs]

# the knob-parity children of test_gpu_attn.py: fixed short lists
KNOB_CASES = {
    "TCX_ATTN_XCD": [_mk(e, 256, 16, h, b, "gauss", 3.0) for e in ("split", "split_bf16", "split_b2")
                     for b, h in ((3, 3), (17, 1))],
    "TCX_ATTN_PF2": [_mk(e, N, D, 2, 1, "gauss", 1.0) for e in ("split_bf16", "split_b2")
                     for N, D in ((512, 16), (768, 48), (512, 32), (768, 64))],
    "TCX_ATTN_DEFER": [_mk(e, 768, D, 1, 1, f, a) for e in ("split_bf16", "split_b2") for D in (16, 64)
                       for f, a in (("rising", 3.0), ("threshold", None), ("gauss", 3.0))],
}
