"""References, inputs, gates, mutants and case tables for the fp32 forward convolution: k_conv of
csrc/conv.hip behind tcx_conv2d / tcx_conv_transpose2x / tcx_convT2x / tcx_linear, the epilogues of
csrc/conv_common.hpp, the one-channel forwards of csrc/thin.hip and the three weight packers (no GPU
import).

The float64 reference is index arithmetic on NHWC arrays, written from include/tcx.h:

  src_s[b] = x_s[b % bmod]  (bmod = 0: x_s[b]);  GroupNorm+SiLU prologue silu(x * scale[b][c] + shift[b][c])
  on the sources that have tables;  in = concat(src_1, src_2) along the channels;  bilinear x2
  (align_corners = False, source index clamped) when upsampling;  the result padded by `pad` on every side,
  circular (index mod n, in upsampled coordinates) or with zeros;
  y[b, oy, ox, co] = act(sum_{ky,kx,ci} in_pad[b, oy*s + ky, ox*s + kx, ci] * w[co][ci][ky][kx]
                         + bias[co] + bias_b[b][co] + resid[b, oy, ox, co])
  gn[b][g][co] = (sum, sum of squares) of y over the pixels 128 g .. 128 g + 127 of image b

ConvTranspose2d(4, 2, 1) is evaluated as its four sub-pixel 2x2 convs (output row 2a + r reads input rows
a - (1 - r) + d with kernel row r + 1 - 2 (d - (1 - r))); the data gradient of a stride-1 conv as a conv over
dY with pad' = ks - 1 - pad and the weight w'[r][co][ky][kx] = w[co][ci_lo + r][ks-1-ky][ks-1-kx].
tests/test_conv_ref_cpu.py compares every kind with torch's float64 operators.

Gates.  Plain sums (act 0 / 1, no prologue, no upsample): gemm_ref's |got - ref| <= (n + 4) 2^-24 S with
n = ks*ks*Cin + (bias, bias_b, resid present) and S = sum |in||w| + |bias| + |bias_b| + |resid|; for n > 300
also gemm_ref's RMS gate.  Sigmoid / SiLU: gemm_ref.gate_linear (1.1 x that bound + 4 * 2^-24 |ref|).  The
upsample rounds each bilinear tap three times: n + 3, S over the bilinear taps of |x|.  The prologue rounds
z = x*scale + shift once (2^-24 |z|, carried through silu' <= 1.1) and silu(z) a few times: n + 8 with
S over |w| (|silu z| + |z|).  Where the float32 evaluation of this file itself misses such a gate the case
takes 4 x that evaluation's error (train_ops_ref._f32_floor); plain sums never do (asserted on the CPU).
Every prologue case also takes the RMS gate, whatever its n.

The dispatch of conv.hip / thin.hip is restated below (dispatch, epilogue, thin_takes) so that the claim
each case makes about the branch it reaches is checked on the CPU.
"""
import numpy as np

import train_ops_ref as T
from gemm_ref import (F32, F64, LONG, PATF, U24, _diff, _worst, act_np, cdiv, f32, gate_rms, gate_sum,  # noqa: F401
                      ok, seed_of)

BM, BK, MAXTAP, PRO_MAXC = 128, 32, 16, 384


def rup(v, a=32):
    return cdiv(v, a) * a


# ------------------------------------------------------------------------------------ cases
class Cv:
    """One call.  kind: conv (tcx_conv2d) | convT (tcx_conv_transpose2x; entry 'convT2x' for the zero-padded
    alias) | linear (tcx_linear: Bt rows, C1 + C2 columns) | dgrad (tcx_pack_conv_dgrad_weight + tcx_conv2d).
    pro: bit 0 / 1 = source 1 / 2 has prologue tables.  shift_*: bytes added to that operand's base.
    inst / epi: the table's claims (dispatch(), epilogue())."""

    def __init__(self, name, Bt, H, W, C1, Cout, C2=0, ks=3, stride=1, pad=1, circ=1, bmod=0, ups=0, act=0,
                 bias=True, bias_b=False, resid=False, gn=False, pro=0, cout_pad=None, kpad=None, kind="conv",
                 shift_x=0, shift_y=0, shift_r=0, shift_bb=0, entry=None, fwd=None, kwide=0, inst=None, epi=None):
        self.name, self.kind, self.Bt, self.H, self.W, self.C1, self.C2, self.Cout = name, kind, Bt, H, W, C1, C2, Cout
        self.ks, self.stride, self.pad, self.circ, self.bmod, self.ups, self.act = ks, stride, pad, circ, bmod, ups, act
        self.bias, self.bias_b, self.resid, self.gn, self.pro = bias, bias_b, resid, gn, pro
        self.shift_x, self.shift_y, self.shift_r, self.shift_bb = shift_x, shift_y, shift_r, shift_bb
        self.entry, self.fwd, self.kwide = entry, fwd, kwide
        if kind == "convT":
            self.ks, self.stride, self.pad = 2, 1, 1
        self.Cin = C1 + C2
        self.K = self.ks * self.ks * self.Cin
        self.cout_pad = cout_pad if cout_pad else rup(Cout)
        self.kpad = kpad if kpad else rup(self.K)
        self.inst, self.epi = inst, epi

    def __repr__(self):
        return self.name

    def dims(self):
        """Hi, Wi, Ho, Wo (of one k_conv launch), M"""
        Hi, Wi = (2 * self.H, 2 * self.W) if self.ups else (self.H, self.W)
        if self.kind == "convT":
            Ho, Wo = Hi, Wi
        else:
            Ho, Wo = (Hi + 2 * self.pad - self.ks) // self.stride + 1, (Wi + 2 * self.pad - self.ks) // self.stride + 1
        return Hi, Wi, Ho, Wo, self.Bt * Ho * Wo

    def out_shape(self):
        Hi, Wi, Ho, Wo, M = self.dims()
        return (self.Bt, 2 * Ho, 2 * Wo, self.Cout) if self.kind == "convT" else (self.Bt, Ho, Wo, self.Cout)

    def nterms(self):
        return self.K + int(self.bias) + int(self.bias_b) + int(self.resid)

    def plain(self):
        return self.act < 2 and not self.pro and not self.ups

    def inputs(self):
        r = T.rng(seed_of(self.name))
        g = lambda *s: f32(r.standard_normal(s))
        u = lambda lo, hi, *s: f32(r.uniform(lo, hi, s))
        bs = self.bmod if self.bmod else self.Bt
        o = dict(x1=g(bs, self.H, self.W, self.C1), x2=g(bs, self.H, self.W, self.C2) if self.C2 else None)
        sc = 1.0 / np.sqrt(self.K)
        if self.kind == "convT":
            o["w"] = f32(g(self.Cin, self.Cout, 4, 4) * sc)
        elif self.kind == "dgrad":
            cof, cif, ci_lo, n_ci = self.fwd  # forward conv: Cout_f = C1 here, n_ci = Cout here
            o["w"] = f32(g(cof, cif, self.ks, self.ks) * sc)
        elif self.kind == "linear" and self.kwide:
            o["w"] = f32(g(self.Cout, self.kwide) * sc)  # the columns past K are another projection's
        else:
            o["w"] = f32(g(self.Cout, self.Cin, self.ks, self.ks) * sc)
        o["bias"] = g(self.Cout) if self.bias else None
        o["bias_b"] = g(self.Bt, self.Cout) if self.bias_b else None
        o["resid"] = g(*self.out_shape()) if self.resid else None
        # silu's argument x*scale + shift spans about [-20, 20] for x ~ N(0, 1)
        for i, C in ((1, self.C1), (2, self.C2)):
            has = self.pro >> (i - 1) & 1
            o[f"sc{i}"] = u(0.5, 6.0, self.Bt, C) if has else None
            o[f"sh{i}"] = u(-4.0, 4.0, self.Bt, C) if has else None
        return o


# ------------------------------------------------------------------------------------ dispatch (conv.hip, thin.hip)
def thin_takes(c):
    """thin_conv_takes and the conditions around its call in tcx_conv2d: 'cin1', 'cout1' or None"""
    Hi, Wi, Ho, Wo, M = c.dims()
    if c.kind not in ("conv", "dgrad") or c.ups or c.gn or c.pro or c.bmod or c.C2 or c.stride != 1:
        return None
    if c.ks < 1 or c.ks > 7 or c.Bt <= 0 or c.Bt * Ho >= 2 ** 31:
        return None
    cin1_lds = (c.ks * c.ks * c.Cout + c.Cout + c.ks * (Wo + c.ks - 1)) * 4
    if (c.C1 == 1 and c.Cout % 4 == 0 and c.ks * c.ks * c.Cout <= 8192 and Wo + c.ks - 1 <= 4096
            and cin1_lds <= 48 * 1024 and c.shift_y % 16 == 0 and (not c.resid or c.shift_r % 16 == 0)
            and (not c.bias_b or c.shift_bb % 16 == 0)):
        return "cin1"
    cout1_lds = (c.ks * c.ks * c.C1 + c.ks * c.W * ((c.C1 // 4) | 1)) * 4
    if c.Cout == 1 and c.C1 % 4 == 0 and cout1_lds <= 48 * 1024 and c.shift_x % 16 == 0:
        return "cout1"
    return None


def conv_mode(c):
    """tcx_conv2d's (tcx_linear's, the transposed conv's) mode choice: 0 float4, 1 scalar, 2 upsample"""
    vec_ok = c.C1 % 4 == 0 and c.C2 % 4 == 0 and c.shift_x % 16 == 0
    return 2 if c.ups else (0 if vec_ok else 1)


def launch_uni(c, mode):
    """launch_nt's `uni`: the chunk-uniform MODE 3 (extents below 2 GiB here; tcx_linear passes none)"""
    return (mode == 0 and c.Cin % BK == 0 and c.C1 % BK == 0 and c.C2 in (0, c.C1) and c.ks * c.ks <= MAXTAP
            and c.kpad == c.K and not c.ups and c.kind != "linear")


def launch_nt(cout_pad):
    return 3 if cout_pad % 96 == 0 else (2 if cout_pad % 64 == 0 else 1)


def dispatch(c):
    """'cin1' | 'cout1' | (NT, MODE, CIRC, PRO) of k_conv"""
    t = thin_takes(c)
    if t:
        return t
    mode = conv_mode(c)
    if c.pro or launch_uni(c, mode):
        mode = 3
    return launch_nt(c.cout_pad), mode, bool(c.circ), bool(c.pro)


def epilogue(c):
    """conv_epi_fast and conv_epi_store_fast: 'general' | 'cols' | 'quad' | 'quad_act' (k_conv launches only)"""
    Hi, Wi, Ho, Wo, M = c.dims()
    BN = 32 * launch_nt(c.cout_pad)
    fast = (c.kind != "convT" and not c.bias_b and M % 128 == 0 and (Ho * Wo) % 128 == 0 and c.Cout % BN == 0
            and M * c.Cout < 2 ** 29)
    if not fast:
        return "general"
    return "cols" if c.resid else ("quad" if c.act == 0 else "quad_act")


# ------------------------------------------------------------------------------------ the reference
def _silu(z, dt):
    return (z / (dt(1) + np.exp(-z))).astype(dt)


def _fma(a, b, c, dt):
    """a*b + c with one rounding (float32: through float64, whose product of two float32 is exact)"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(dt)


def _axis(n_src, ups, lo, hi, circ, mutant):
    """Per padded coordinate e in [-lo, n + hi): (i0, i1, l0, l1), source rows and their weights (float32
    exact).  No upsample: l0 = 1 inside / 0 in the zero padding, l1 = 0."""
    n = 2 * n_src if ups else n_src
    e = np.arange(-lo, n + hi)
    valid = np.ones(e.size, bool)
    if circ:
        if mutant == "wrap_off_by_one":
            d = np.clip(np.where(e < 0, e + n - 1, np.where(e >= n, e - n + 1, e)), 0, n - 1)
        else:
            d = e % n
    else:
        valid = (e >= 0) & (e < n)
        d = np.clip(e, 0, n - 1)
    if not ups:
        return d, d, valid.astype(F64), np.zeros(e.size)
    if mutant == "ups_wrap_source":   # the pad wrapped after mapping to source coordinates
        s = 0.5 * (e + 0.5) - 0.5
        i0 = np.floor(s).astype(int)
        return i0 % n_src, (i0 + 1) % n_src, 1.0 - (s - i0), s - i0
    if mutant == "ups_align_corners":
        s = d * (n_src - 1) / max(n - 1, 1)
    else:
        s = np.maximum(0.5 * (d + 0.5) - 0.5, 0.0)
    i0 = s.astype(int)
    i1 = i0 + (i0 < n_src - 1)
    return i0, i1, 1.0 - (s - i0), s - i0


def _sources(c, inp, dt, mutant):
    """[Bt, H, W, Cin] after bmod aliasing, prologue and concat, and the |.| array of the gate"""
    b = np.arange(c.Bt)
    bs = (np.minimum(b, c.bmod - 1) if mutant == "bmod_ignored" else b % c.bmod) if c.bmod else b
    tabs = {1: (inp["sc1"], inp["sh1"]), 2: (inp["sc2"], inp["sh2"])}
    if mutant == "pro_wrong_source":
        tabs = {1: tabs[2], 2: tabs[1]}
    outs, mags = [], []
    for i, x in ((1, inp["x1"]), (2, inp["x2"])):
        if x is None:
            continue
        a = x[bs].astype(dt)
        mag = np.abs(a).astype(F64)
        sc, sh = tabs[i]
        if sc is not None:
            if mutant == "pro_image0":
                sc, sh = np.repeat(sc[:1], c.Bt, 0), np.repeat(sh[:1], c.Bt, 0)
            z = _fma(a, sc[:, None, None, :].astype(dt), np.broadcast_to(sh[:, None, None, :], a.shape).astype(dt), dt)
            a = _silu(z, dt)
            mag = np.abs(a).astype(F64) + np.abs(z).astype(F64)
        outs.append(a)
        mags.append(mag)
    return np.concatenate(outs, 3), np.concatenate(mags, 3)


def _padded(a, c, dt, mutant, lo=None, hi=None):
    """the effective input on padded coordinates [Bt, Hi + lo_y + hi_y, Wi + lo_x + hi_x, Cin]; lo / hi: (y, x)"""
    lo = lo if lo is not None else (c.pad, c.pad)
    hi = hi if hi is not None else (c.pad, c.pad)
    if mutant == "pad_far_side":
        lo, hi = tuple(c.ks - 1 - p for p in lo), tuple(h + c.ks + c.pad for h in hi)
    y0, y1, ly0, ly1 = _axis(c.H, c.ups, lo[0], hi[0], c.circ, mutant)
    x0, x1, lx0, lx1 = _axis(c.W, c.ups, lo[1], hi[1], c.circ, mutant)
    ly0, ly1 = (v.astype(dt)[None, :, None, None] for v in (ly0, ly1))
    lx0, lx1 = (v.astype(dt)[None, None, :, None] for v in (lx0, lx1))
    g = lambda iy, ix: a[:, iy][:, :, ix]
    if not c.ups:
        return (g(y0, x0) * (ly0 * lx0)).astype(dt)
    r0 = _fma(np.broadcast_to(lx1, g(y0, x1).shape), g(y0, x1), (lx0 * g(y0, x0)).astype(dt), dt)
    r1 = _fma(np.broadcast_to(lx1, g(y1, x1).shape), g(y1, x1), (lx0 * g(y1, x0)).astype(dt), dt)
    return _fma(np.broadcast_to(ly1, r1.shape), r1, (ly0 * r0).astype(dt), dt)


def eff_weight(c, inp, mutant=None, phase=None):
    """[Cout][Cin][ks][ks] of the conv that the call (or one phase of the transposed conv) computes"""
    w = inp["w"]
    if c.kind == "convT":
        ry, rx = phase
        if mutant == "phases_swapped" and ry != rx:
            ry, rx = rx, ry
        o = np.zeros((c.Cout, c.Cin, 2, 2), w.dtype)
        for dy in range(2):
            for dx in range(2):
                ky, kx = ry + 1 - 2 * (dy - (1 - ry)), rx + 1 - 2 * (dx - (1 - rx))
                o[:, :, dy, dx] = w[:, :, ky, kx].T
        return o
    if c.kind == "dgrad":
        cof, cif, ci_lo, n_ci = c.fwd
        sel = w[:, 0:n_ci] if mutant == "ci_lo_ignored" else w[:, ci_lo:ci_lo + n_ci]
        o = sel.transpose(1, 0, 2, 3)
        return np.ascontiguousarray(o if mutant == "dgrad_no_flip" else o[:, :, ::-1, ::-1])
    if c.kind == "linear":
        return w[:, :c.K].reshape(c.Cout, c.K, 1, 1)
    return w


def _cols(ap, c, Ho, Wo):
    """im2col of the padded input: [Bt, Ho, Wo, ks*ks, Cin]"""
    s = c.stride
    return np.stack([ap[:, ky:ky + (Ho - 1) * s + 1:s, kx:kx + (Wo - 1) * s + 1:s]
                     for ky in range(c.ks) for kx in range(c.ks)], 3)


def _sum(cols, w, dt, mutant, c):
    """[Bt, Ho, Wo, Cout]: float64 matmul, or the float32 fma chain in k order"""
    Bt, Ho, Wo, T_, Cin = cols.shape
    wk = w.transpose(0, 3, 2, 1) if mutant == "taps_transposed" else w.transpose(0, 2, 3, 1)
    wk = np.ascontiguousarray(wk).reshape(w.shape[0], -1)   # [Cout][(ky*ks + kx)*Cin + ci]
    A = cols.reshape(-1, T_ * Cin)
    if mutant == "drop_last_chunk":
        wk = wk.copy()
        wk[:, BK * ((A.shape[1] - 1) // BK):] = 0
    if dt is F64:
        acc = A.astype(F64) @ wk.astype(F64).T
    else:
        acc = np.zeros((A.shape[0], wk.shape[0]), F32)
        for k in range(A.shape[1]):
            acc = (acc.astype(F64) + A[:, k, None].astype(F64) * wk[None, :, k].astype(F64)).astype(F32)
    return acc.reshape(Bt, Ho, Wo, wk.shape[0])


def evaluate(c, inp, mutant=None, dt=F64):
    """dict(y [out_shape], S (float64 gate sums, same shape), gn [Bt][nsplit][Cout][2] or None).  dt = F32: the
    float32 evaluation (sequential k order, every step rounded)."""
    Hi, Wi, Ho, Wo, M = c.dims()
    a, mag = _sources(c, inp, dt, mutant)
    phases = [(ry, rx) for ry in range(2) for rx in range(2)] if c.kind == "convT" else [None]
    y = np.full(c.out_shape(), PATF, dt) if mutant == "subpixel_offset_dropped" else np.zeros(c.out_shape(), dt)
    S = np.zeros(c.out_shape(), F64)
    for ph in phases:
        lo = hi = None
        if ph:
            lo, hi = (1 - ph[0], 1 - ph[1]), (ph[0], ph[1])
        w = eff_weight(c, inp, mutant, ph)
        cols = _cols(_padded(a, c, dt, mutant, lo, hi), c, Ho, Wo)
        acc = _sum(cols, w, dt, mutant, c)
        sm = _sum(_cols(_padded(mag, c, F64, None, lo, hi), c, Ho, Wo), np.abs(w), F64, None, c)
        if ph:
            oy, ox = (0, 0) if mutant == "subpixel_offset_dropped" else ph
            y[:, oy::2, ox::2][:, :Ho, :Wo] = acc
            S[:, ph[0]::2, ph[1]::2] = sm
        else:
            y, S = acc, sm
    if mutant == "window_tail":
        # the chunk past K: x continues into the next row (the canary after the last), w into the next projection
        n = min(rup(c.K), c.kwide) - c.K
        flat = np.concatenate([inp["x1"].reshape(-1).astype(F64), np.full(BK, PATF, F64)])
        nxt = np.stack([flat[(m + 1) * c.K:(m + 1) * c.K + n] for m in range(c.Bt)])
        y = y + (nxt @ inp["w"][:, c.K:c.K + n].astype(F64).T).reshape(y.shape)
    for key in ("bias", "bias_b", "resid"):
        v = inp[key]
        if v is None:
            continue
        if key == "bias":
            v = v[None, None, None, :]
        elif key == "bias_b":
            if mutant == "bias_b_first_image":   # the image of the 128-pixel tile's first pixel, for the whole tile
                m = np.arange(M).reshape(c.Bt, Ho, Wo)
                v = v[(m // BM * BM) // (Ho * Wo)]
            else:
                v = v[:, None, None, :]
        y = (y + v.astype(dt)).astype(dt)
        S = S + np.abs(v.astype(F64))
    y = act_np(y, c.act, dt)
    gn = None
    if c.gn:
        v = y.astype(F64).reshape(c.Bt, (Ho * Wo) // BM, BM, c.Cout)
        gn = np.stack([v.sum(2), (v * v).sum(2)], -1)
        if mutant == "gn_neighbour_group":
            gn = np.roll(gn, 1, 1)
    return dict(y=y, S=S, gn=gn)


def flat_output(c, res, mutant=None, tail=256):
    """the output buffer as the call leaves it, with `tail` canary floats behind it"""
    y = np.asarray(res["y"], F64).reshape(-1, c.Cout)
    buf = np.concatenate([y.reshape(-1), np.full(tail, PATF, F64)])
    if mutant == "rows_ge_M_stored":      # the tile's rows past M, computed from pixel 0's gather
        buf[y.size:y.size + c.Cout] = y[0] if y.size else 0.0
    if mutant == "chan_ge_Cout_stored":   # column Cout of pixel m is column 0 of pixel m + 1
        buf[c.Cout::c.Cout] = 0.0
    return buf


# ------------------------------------------------------------------------------------ gates
def elem_bound(c, ref, ref32=None):
    """the per-element bound (array); T.FALLBACK holds the float32 evaluation's error where its floor was used"""
    n, S, yr = c.nterms(), ref["S"], ref["y"]
    T.FALLBACK = None
    if c.plain():   # no fallback in this class
        return (n + 4) * U24 * S
    n += (3 if c.ups else 0) + (8 if c.pro else 0)
    b = 1.1 * (n + 4) * U24 * S + 4 * U24 * np.abs(yr)
    return np.maximum(b, T._f32_floor(ref32, yr, b))


def needs32(c):
    """the case's gates use the float32 evaluation (fallback of the non-plain classes, the RMS gate's yardstick)"""
    return not c.plain() or c.nterms() > LONG


def gates(c, got, ref, ref32=None):
    """[(name, (err, bound))] for an output `got` of out_shape against evaluate()'s float64 result; ref32: the
    float32 evaluation's y (required where needs32).  The RMS gate also covers every prologue case: the
    per-element bound there carries |z| up to 20 and alone would admit operands truncated to 10 bits."""
    assert ref32 is not None or not needs32(c)
    g = [("elem", _worst(_diff(got, ref["y"]), elem_bound(c, ref, ref32)))]
    if c.nterms() > LONG or c.pro:
        g.append(("rms", gate_rms(got, ref["y"], ref32)))
    return g


def verdict(c, buf, ref, ref32=None):
    """gates of a flat output buffer with canary floats behind it (flat_output)"""
    n = int(np.prod(c.out_shape()))
    return gates(c, buf[:n].reshape(c.out_shape()), ref, ref32) + \
        [("canary", (float(np.count_nonzero(buf[n:] != PATF)), 0.0))]


def gn_gates(c, part, got_y, ref, bound):
    """the partials against the float64 sums of the GPU's own outputs (20 * 2^-24 * sum |v|: the 16 fp32 adds of
    the quad form plus slack; likewise the squares), and against the reference within 128 x the output gate"""
    Hi, Wi, Ho, Wo, M = c.dims()
    v = np.asarray(got_y, F64).reshape(c.Bt, (Ho * Wo) // BM, BM, c.Cout)
    own = np.stack([v.sum(2), (v * v).sum(2)], -1)
    bnd = 20 * U24 * np.stack([np.abs(v).sum(2), (v * v).sum(2)], -1)
    gmax = np.broadcast_to(bound, ref["y"].shape).reshape(v.shape).max(2)   # the output gate of the group's worst element
    return [("gn own", _worst(_diff(part, own), bnd)),
            ("gn ref", _worst(_diff(part[..., 0], ref["gn"][..., 0]), 128 * gmax))]


def all_ok(gs):
    return all(ok(eb) for _, eb in gs)


# ------------------------------------------------------------------------------------ packers (reference layouts)
def pack_conv(w, cout_pad, kpad):
    Cout, Cin, ks, _ = w.shape
    o = np.zeros((cout_pad, kpad), F32)
    o[:Cout, :ks * ks * Cin] = w.transpose(0, 2, 3, 1).reshape(Cout, -1)
    return o


def pack_convT(w, cout_pad, kpad):
    Cin, Cout = w.shape[:2]
    c = Cv("pack", 1, 1, 1, Cin, Cout, kind="convT")
    return np.stack([pack_conv(eff_weight(c, dict(w=w), None, (ph >> 1, ph & 1)), cout_pad, kpad) for ph in range(4)])


def pack_dgrad(w, ci_lo, n_ci, cout_pad, kpad):
    Cout, Cin, ks, _ = w.shape
    c = Cv("pack", 1, 1, 1, Cout, n_ci, ks=ks, kind="dgrad", fwd=(Cout, Cin, ci_lo, n_ci))
    return pack_conv(eff_weight(c, dict(w=w)), cout_pad, kpad)


def pack_case(c, inp):
    """the packed weight the case's call reads"""
    if c.kind == "convT":
        return pack_convT(inp["w"], c.cout_pad, c.kpad)
    if c.kind == "linear":
        o = np.zeros((c.cout_pad, c.kpad), F32)
        wd = inp["w"].reshape(c.Cout, -1)
        o[:c.Cout, :wd.shape[1]] = wd
        return o
    return pack_conv(eff_weight(c, inp), c.cout_pad, c.kpad)


# ------------------------------------------------------------------------------------ case tables
def _inst():
    """a. the 24 fp32 k_conv<NT, MODE, CIRC, PRO>: cout_pad 32 / 64 / 96 over Cout = 20"""
    o = []
    for nt in (1, 2, 3):
        cp = 32 * nt
        for circ in (1, 0):
            z = "circ" if circ else "zero"
            o.append(Cv(f"a NT{nt} MODE0 {z} C1=12", 2, 5, 7, 12, 20, circ=circ, cout_pad=cp, inst=(nt, 0, bool(circ), False)))
            c1 = (3, 6, 1)[nt - 1]   # Cin = 1: stride 2 keeps it off thin.hip
            o.append(Cv(f"a NT{nt} MODE1 {z} C1={c1}", 2, 5, 7, c1, 20, circ=circ, cout_pad=cp, stride=2 if c1 == 1 else 1,
                        inst=(nt, 1, bool(circ), False)))
            c2 = 32 if nt == 2 else 0
            o.append(Cv(f"a NT{nt} MODE3 {z} C1=32 C2={c2}", 2, 5, 7, 32, 20, C2=c2, circ=circ, cout_pad=cp,
                        inst=(nt, 3, bool(circ), False)))
            o.append(Cv(f"a NT{nt} MODE3->0 {z} kpad>K C2={c2}", 2, 5, 7, 32, 20, C2=c2, circ=circ, cout_pad=cp,
                        kpad=9 * (32 + c2) + 32, inst=(nt, 0, bool(circ), False)))
        o.append(Cv(f"a NT{nt} MODE0 circ C1=32 C2=8", 2, 5, 7, 32, 20, C2=8, cout_pad=cp, inst=(nt, 0, True, False)))
        o.append(Cv(f"a NT{nt} MODE2 circ", 2, 3, 5, 8, 20, ups=1, cout_pad=cp, inst=(nt, 2, True, False)))
        o.append(Cv(f"a NT{nt} MODE3 PRO", 3, 8, 16, 32, 20, pro=1, cout_pad=cp, inst=(nt, 3, True, True)))
    return o


def _edges():
    """b. tile edges: M, Ho*Wo, Cout, kpad"""
    o = [Cv("b M=0", 0, 5, 7, 12, 20), Cv("b M=1", 1, 1, 1, 12, 20), Cv("b M=127", 1, 1, 127, 12, 20),
         Cv("b M=128", 1, 8, 16, 12, 20), Cv("b M=129", 3, 1, 43, 12, 20), Cv("b M=257", 1, 1, 257, 12, 20),
         Cv("b HoWo=1 Bt=5", 5, 1, 1, 12, 20, bias_b=True, resid=True),
         Cv("b HoWo=35 Bt=4 bias_b resid", 4, 5, 7, 12, 20, bias_b=True, resid=True, epi="general"),
         Cv("b HoWo=35 Bt=5 bias_b resid MODE3", 5, 5, 7, 32, 40, bias_b=True, resid=True, act=1, epi="general"),
         Cv("b HoWo=128 Bt=2 bias_b", 2, 8, 16, 12, 32, bias_b=True, epi="general"),
         Cv("b HoWo=256", 1, 16, 16, 12, 32, epi="quad")]
    for co in (1, 31, 32, 33, 95, 96, 97, 193):
        o.append(Cv(f"b Cout={co}", 1, 8, 16, 12, co, C2=4, epi="quad" if co in (32, 96) else "general"))
    o += [Cv("b K=4 kpad=32", 2, 5, 7, 4, 20, ks=1, pad=0), Cv("b K=28 kpad=32", 2, 5, 7, 28, 20, ks=1, pad=0),
          Cv("b K=36 kpad=64", 2, 5, 7, 4, 20), Cv("b K=32 kpad=K", 2, 5, 7, 32, 20, ks=1, pad=0, inst=(1, 3, True, False))]
    return o


def _geometry():
    """c. ks 1..5, stride 1..3, pad 0 .. ks - 1 on 7 x 5 (W < H), both paddings, MODE 0 / 1; one- and two-pixel
    images with pad == H"""
    o = []
    for ks in range(1, 6):
        for circ in (1, 0):
            for pad in sorted({0, ks // 2, ks - 1}):
                s = (ks + pad) % 3 + 1
                for c1 in (4, 3):
                    o.append(Cv(f"c ks={ks} s={s} pad={pad} {'circ' if circ else 'zero'} C1={c1}", 2, 7, 5, c1, 20, ks=ks,
                                stride=s, pad=pad, circ=circ, inst=(1, 0 if c1 == 4 else 1, bool(circ), False)))
    for H, W, ks, pad in ((1, 1, 3, 1), (2, 1, 3, 1), (1, 2, 3, 1), (2, 2, 5, 2), (2, 3, 5, 2), (2, 2, 4, 2)):
        for c1 in (4, 3):
            o.append(Cv(f"c tiny {H}x{W} ks={ks} pad={pad} circ C1={c1}", 3, H, W, c1, 20, ks=ks, pad=pad))
    o.append(Cv("c tiny 2x2 ks=4 pad=2 circ MODE3", 3, 2, 2, 32, 20, ks=4, pad=2, inst=(1, 3, True, False)))
    o.append(Cv("c tiny 1x2 ks=3 pad=3 zero", 3, 1, 2, 4, 20, ks=3, pad=3, circ=0))
    return o


def _sources_cases():
    """d. two sources, bmod with Bt % bmod != 0, a misaligned x1"""
    o = [Cv("d two sources MODE0 C1=8 C2=12", 2, 5, 7, 8, 20, C2=12, inst=(1, 0, True, False)),
         Cv("d two sources MODE3 zero", 2, 5, 7, 32, 20, C2=32, circ=0, inst=(1, 3, False, False)),
         Cv("d x1+4B MODE1", 2, 5, 7, 12, 20, shift_x=4, inst=(1, 1, True, False))]
    for bmod, Bt in ((1, 2), (2, 3), (3, 4)):
        for c1, mode in ((12, 0), (3, 1), (32, 3)):
            o.append(Cv(f"d bmod={bmod} Bt={Bt} MODE{mode}", Bt, 5, 7, c1, 20, bmod=bmod, bias_b=True, resid=True,
                        circ=bmod != 2, inst=(1, mode, bmod != 2, False)))
    o.append(Cv("d bmod=2 Bt=5 Cin=1", 5, 5, 7, 1, 20, bmod=2, bias_b=True, resid=True, inst=(1, 1, True, False)))
    return o


def _upsample():
    """e. MODE 2"""
    o = []
    for i, (H, W) in enumerate(((1, 1), (1, 2), (2, 3), (3, 5), (5, 2), (2, 1))):
        ks = (3, 1)[i % 2]
        c2 = (0, 4)[i // 2 % 2]
        cp = (32, 64, 96)[i % 3]
        o.append(Cv(f"e up {H}x{W} ks={ks} C2={c2} cp={cp} act={i % 4}", 3, H, W, 8, 20, C2=c2, ks=ks, pad=ks // 2, ups=1,
                    cout_pad=cp, act=i % 4, resid=i % 2 == 0, inst=(cp // 32, 2, True, False)))
    o.append(Cv("e up 8x8 quad_act", 1, 8, 8, 8, 32, ups=1, act=1, inst=(1, 2, True, False), epi="quad_act"))
    o.append(Cv("e up 4x4 s2 ks=4", 2, 4, 4, 8, 20, ups=1, ks=4, stride=2, pad=1, inst=(1, 2, True, False)))
    return o


def _prologue():
    """f. MODE 3 with the GroupNorm+SiLU prologue; one image per tile"""
    o = []
    for c1, c2, pro in ((32, 0, 1), (96, 0, 1), (384, 0, 1), (32, 32, 1), (32, 32, 2), (32, 32, 3), (96, 96, 3)):
        o.append(Cv(f"f pro C1={c1} C2={c2} tables={pro}", 3, 8, 16, c1, 20, C2=c2, pro=pro, inst=(1, 3, True, True)))
    o.append(Cv("f pro 4x4 s2 C1=32 tables=1", 3, 16, 32, 32, 20, ks=4, stride=2, pad=1, pro=1, inst=(1, 3, True, True)))
    o.append(Cv("f pro 4x4 s2 C1=C2=32 tables=3 gn", 3, 16, 32, 32, 64, C2=32, ks=4, stride=2, pad=1, pro=3, gn=True,
                act=0, inst=(2, 3, True, True), epi="quad"))
    return o


def _epilogues():
    """g. general (Cout % BN), general (bias_b), cols, quad / quad_act: each with and without GN partials"""
    o = []
    for form, kw in (("general", dict(Cout=20)), ("general", dict(Cout=32, bias_b=True)), ("cols", dict(Cout=32, resid=True)),
                     ("quad", dict(Cout=32))):
        for act in range(4):
            for gn in (False, True):
                kw2 = dict(kw)
                co = kw2.pop("Cout")
                epi = "quad_act" if form == "quad" and act else form
                o.append(Cv(f"g {form}{' bias_b' if kw.get('bias_b') else ''} Cout={co} act={act} gn={int(gn)}", 2, 8, 16, 12,
                            co, act=act, gn=gn, epi=epi, **kw2))
    o.append(Cv("g quad NT3 Cout=96 gn", 2, 8, 16, 32, 96, gn=True, epi="quad", inst=(3, 3, True, False)))
    o.append(Cv("g cols NT2 Cout=64 act=3 gn", 2, 8, 16, 12, 64, gn=True, act=3, resid=True, epi="cols"))
    o.append(Cv("g quad HoWo=256 gn (two groups per image)", 2, 16, 16, 12, 32, gn=True, epi="quad"))
    o.append(Cv("g general HoWo=256 Cout=20 act=1 gn", 2, 16, 16, 12, 20, gn=True, act=1, epi="general"))
    return o


def _transposed():
    """h. both entries, zero and circular, M % 128 != 0"""
    o = []
    shapes = ((1, 1), (1, 3), (5, 5), (3, 7), (8, 16))
    cins, couts = (3, 4, 32, 36), (1, 20, 33, 96)
    i = 0
    for hw in shapes:
        for ci, co in ((ci, co) for ci in cins for co in couts):
            act, circ = (i + i // 16) % 4, (i // 2 + i // 8) % 2
            entry = "convT2x" if (not circ and i % 3 == 0) else "transpose2x"
            mode = 3 if ci == 32 else (0 if ci % 4 == 0 else 1)
            o.append(Cv(f"h {entry} {hw[0]}x{hw[1]} Cin={ci} Cout={co} act={act} {'circ' if circ else 'zero'}"
                        f"{'' if i % 5 else ' nobias'}", 3 if hw != (8, 16) else 2, hw[0], hw[1], ci, co, kind="convT",
                        circ=circ, act=act, bias=i % 5 != 0, entry=entry, epi="general",
                        inst=(launch_nt(rup(co)), mode, bool(circ), False)))
            i += 1
    return o


def _dgrad():
    """i. the data gradient through the dgrad pack and tcx_conv2d with pad' = ks - 1 - pad.  fwd = (Cout, Cin,
    ci_lo, n_ci) of the forward conv; here C1 = Cout_f (dY's channels) and Cout = n_ci"""
    o = []
    for ks, pad, circ, cif, ci_lo, n_ci in ((3, 1, 1, 12, 0, 12), (3, 0, 0, 12, 5, 7), (3, 2, 0, 12, 0, 5), (5, 2, 1, 12, 4, 8),
                                            (5, 1, 0, 12, 5, 4), (5, 0, 0, 12, 8, 4), (1, 0, 0, 12, 5, 7), (3, 1, 1, 9, 5, 4)):
        Ho, Wo = 7 + 2 * pad - ks + 1, 6 + 2 * pad - ks + 1   # the forward conv of a 7 x 6 image: dY's size
        o.append(Cv(f"i dgrad ks={ks} pad={pad} {'circ' if circ else 'zero'} Cin={cif} ci_lo={ci_lo} n_ci={n_ci}", 2, Ho, Wo,
                    8, n_ci, ks=ks, pad=ks - 1 - pad, circ=circ, bias=False, kind="dgrad", fwd=(8, cif, ci_lo, n_ci)))
    return o


def _linear():
    """j. tcx_linear: rows Bt, K1 = C1, K2 = C2, N = Cout"""
    kw = dict(kind="linear", ks=1, pad=0, circ=0)
    o = [Cv(f"j linear M={M} N=33", M, 1, 1, 36, 33, act=M % 4, resid=M > 1, **kw) for M in (0, 1, 7, 129)]
    o += [Cv("j linear K=30 scalar N=1", 7, 1, 1, 30, 1, inst=(1, 1, False, False), **kw),
          Cv("j linear K=7 scalar N=97 act=2", 7, 1, 1, 7, 97, act=2, cout_pad=192, inst=(3, 1, False, False), **kw),
          Cv("j linear two sources N=97 act=3", 7, 1, 1, 36, 97, C2=28, act=3, resid=True, cout_pad=192,
             inst=(3, 0, False, False), **kw),
          Cv("j linear two sources K=64 N=33", 129, 1, 1, 32, 33, C2=32, act=1, inst=(2, 0, False, False), **kw),
          Cv("j linear window K=36 of 100", 7, 1, 1, 36, 33, kwide=100, kpad=128, resid=True, **kw),
          Cv("j linear window K=20 of 64 act=3", 129, 1, 1, 20, 33, kwide=64, kpad=64, act=3, **kw)]
    return o


def _thin():
    """k. thin.hip: both sides of every condition of thin_conv_takes; the accepted side at ks / pad / W / act"""
    o = []
    T_, D = "cin1", (1, 1, False, False)
    o += [Cv("k cin1 ks=7 taken", 2, 7, 9, 1, 8, ks=7, pad=3, inst="cin1"),
          Cv("k cin1 ks=8 declined", 2, 7, 9, 1, 8, ks=8, pad=3, inst=(1, 1, True, False)),
          Cv("k cin1 ks=7 Cout=164 taken", 1, 1, 9, 1, 164, ks=7, pad=3, circ=0, inst="cin1"),
          Cv("k cin1 ks=7 Cout=168 declined (ks*ks*Cout)", 1, 1, 9, 1, 168, ks=7, pad=3, circ=0, inst=(3, 1, False, False)),
          Cv("k cin1 Cout=6 declined", 2, 5, 7, 1, 6, inst=(1, 1, True, False)),
          Cv("k cin1 y+4B declined", 2, 5, 7, 1, 8, shift_y=4, inst=(1, 1, True, False)),
          Cv("k cin1 resid+4B declined", 2, 5, 7, 1, 8, resid=True, shift_r=4, inst=(1, 1, True, False)),
          Cv("k cin1 bias_b+4B declined", 2, 5, 7, 1, 8, bias_b=True, shift_bb=4, inst=(1, 1, True, False)),
          Cv("k cin1 x+4B taken", 2, 5, 7, 1, 8, shift_x=4, inst="cin1"),
          Cv("k cin1 LDS 48 KB taken", 1, 1, 578, 1, 164, ks=7, pad=3, circ=0, inst="cin1"),
          Cv("k cin1 LDS 48 KB declined", 1, 1, 579, 1, 164, ks=7, pad=3, circ=0, inst=(3, 1, False, False)),
          Cv("k cin1 row 4096 taken", 1, 1, 4096, 1, 4, ks=1, pad=0, inst="cin1"),
          Cv("k cin1 row 4097 declined", 1, 1, 4097, 1, 4, ks=1, pad=0, inst=(1, 1, True, False)),
          Cv("k cin1 stride 2 declined", 2, 5, 7, 1, 8, stride=2, inst=(1, 1, True, False)),
          Cv("k cout1 x+4B declined", 2, 5, 7, 8, 1, shift_x=4, inst=(1, 1, True, False)),
          Cv("k cout1 Cin=6 declined", 2, 5, 7, 6, 1, inst=(1, 1, True, False)),
          Cv("k cout1 LDS 48 KB taken", 1, 2, 42, 100, 1, ks=7, pad=3, circ=0, inst="cout1"),
          Cv("k cout1 LDS 48 KB declined", 1, 2, 43, 100, 1, ks=7, pad=3, circ=0, inst=(1, 0, False, False)),
          Cv("k cout1 ks=8 declined", 2, 7, 9, 4, 1, ks=8, pad=3, inst=(1, 0, True, False)),
          Cv("k cin1 2112 rows", 33, 64, 5, 1, 4, inst="cin1"),
          Cv("k cout1 2112 rows bias_b", 33, 64, 5, 4, 1, bias_b=True, inst="cout1")]
    i = 0
    for ks in (1, 2, 3, 4, 7):
        for pad in sorted({0, 1, ks - 1}):
            for circ in (1, 0):
                W = (1, 5, 65, 130)[i % 4]
                if W + 2 * pad < ks or (circ and pad > W):
                    W = 65
                act = i % 4
                wide = (4, 100)[i // 2 % 2]
                z = "circ" if circ else "zero"
                H = max(3, ks - 2 * pad, pad)
                o.append(Cv(f"k cin1 ks={ks} pad={pad} {z} W={W} Cout={wide} act={act}", 2, H, W, 1, wide,
                            ks=ks, pad=pad, circ=circ, act=act, bias_b=i % 3 == 0, resid=i % 2 == 0, inst="cin1"))
                W1 = min(W, (12288 - ks * ks * wide) // (ks * ((wide // 4) | 1)))   # cout1_lds <= 48 KB
                o.append(Cv(f"k cout1 ks={ks} pad={pad} {z} W={W1} Cin={wide} act={act}", 2, H, W1, wide, 1,
                            ks=ks, pad=pad, circ=circ, act=act, bias_b=i % 3 == 0, resid=i % 2 == 0, inst="cout1"))
                i += 1
    return o


GROUPS = {"a": _inst(), "b": _edges(), "c": _geometry(), "d": _sources_cases(), "e": _upsample(), "f": _prologue(),
          "g": _epilogues(), "h": _transposed(), "i": _dgrad(), "j": _linear(), "k": _thin()}
ALL = [c for g in GROUPS.values() for c in g]
assert len({c.name for c in ALL}) == len(ALL)

# (H, W, ks, stride, pad, circular, upsample) that tcx_conv2d refuses, and the words its message holds
BAD_GEOMETRY = [((2, 2, 3, 2, 0, 1, 0), "larger than the padded input"), ((2, 2, 3, 2, 0, 0, 0), "larger than the padded input"),
                ((5, 1, 5, 2, 1, 0, 0), "larger than the padded input"), ((2, 5, 5, 1, 3, 1, 0), "wraps more than once"),
                ((5, 2, 5, 1, 3, 1, 0), "wraps more than once"), ((1, 1, 3, 1, 3, 1, 1), "wraps more than once"),
                ((4, 4, 3, 1, 1, 0, 1), "upsample needs")]

# ------------------------------------------------------------------------------------ mutants
MUTANTS = ["wrap_off_by_one", "pad_far_side", "taps_transposed", "dgrad_no_flip", "ci_lo_ignored", "bmod_ignored",
           "bias_b_first_image", "subpixel_offset_dropped", "phases_swapped", "ups_align_corners", "ups_wrap_source",
           "drop_last_chunk", "window_tail", "pro_image0", "pro_wrong_source", "gn_neighbour_group", "rows_ge_M_stored",
           "chan_ge_Cout_stored"]


def applies(c, mut):
    """the case names the mutated branch"""
    Hi, Wi, Ho, Wo, M = c.dims()
    if M == 0:
        return False
    return {
        "wrap_off_by_one": c.circ and c.kind != "linear" and (c.pad > 0 or c.kind == "convT") and min(Hi, Wi) > 1,
        "pad_far_side": c.kind in ("conv", "dgrad") and c.ks - 1 - c.pad != c.pad and Hi * Wi > 1,
        "taps_transposed": c.kind in ("conv", "dgrad") and c.ks > 1 and Hi * Wi > 1,
        "dgrad_no_flip": c.kind == "dgrad" and c.ks > 1,
        "ci_lo_ignored": c.kind == "dgrad" and c.fwd[2] > 0,
        "bmod_ignored": c.bmod > 0 and c.Bt > c.bmod and c.bmod > 1,
        "bias_b_first_image": c.bias_b and c.Bt > 1 and (Ho * Wo) % BM != 0 and c.kind == "conv" and not thin_takes(c),
        "subpixel_offset_dropped": c.kind == "convT",
        "phases_swapped": c.kind == "convT",
        "ups_align_corners": c.ups and c.H * c.W > 1,
        "ups_wrap_source": c.ups and c.H * c.W > 1,
        "drop_last_chunk": True,
        "window_tail": c.kind == "linear" and c.kwide > 0,
        "pro_image0": c.pro and c.Bt > 1,
        "pro_wrong_source": c.pro and c.C2 > 0,
        "gn_neighbour_group": c.gn and (Ho * Wo) // BM > 1,
        "rows_ge_M_stored": M % BM != 0,
        "chan_ge_Cout_stored": c.Cout % 32 != 0,
    }[mut]
