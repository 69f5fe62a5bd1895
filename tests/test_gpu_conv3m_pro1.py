"""GPU: the GroupNorm+SiLU-prologue 3x3 conv on 16x16x32 MFMAs (csrc/conv3m.hip, k_conv3m PRO 1) through
tcx_conv2d_h2_pro, in its two forms: with the halo DMA offsets reloaded from an LDS table and the
transform's arithmetic kept scalar (the default), and the form before it (TCX_CONV3M_PRO1_TAB=0), which
recomputes each offset at its issue.  Only addresses, register placement and the scalar / packed form of
IEEE operations differ, so the two must agree bit for bit.

Shapes are the smallest around k_conv3m's tile (256 pixels: 4 / 8 / 16 rows of 64 / 32 / 16): half a tile
high (the dispatcher hands those to another kernel: asked through the kernel's own debug stamps, which only
k_conv3m writes, and skipped), one tile high (every halo row wraps onto the tile itself, the worst case
for a precomputed offset) and two tiles high; Cin = 32, 64, 96, 192 is 1, 2, 3, 6 trips of the tap loop;
Cout one and two column tiles; Bt = 3 puts three images' tiles on one table layout.  Sources hold exact
zeros and values whose scale * x + shift lies in [-100, -80] (e^-t near and past the fp32 range: silu -> -0).

Each case: (a) both forms bit-equal, output and GroupNorm partials; (b) the output within the h2 conv gate
(test_gpu_ops.close: 2e-5 of the output scale) of conv_ref's float64 evaluation; (c) the 0x7b canaries
around the output and the partials intact; (d) a second run bit-equal; (e) the range flag raised by one
source value that leaves the f16 range after the transform, and not without it.

The library reads the knob once, so each form runs every case in one child process of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 1024  # canary bytes on each side
CANARY = 0x7B

SHAPES = [(64, 2), (64, 4), (64, 8), (32, 4), (32, 8), (32, 16), (16, 8), (16, 16), (16, 32)]
CASES = [(W, H, Cin, Cout, Bt) for W, H in SHAPES for Cin in (32, 64, 96, 192) for Cout in (96, 192) for Bt in (1, 3)]


def case_id(c):
    return "W%d-H%d-Cin%d-Cout%d-Bt%d" % c


def inputs(case):
    """x [Bt][H][W][Cin], w [Cout][Cin][3][3], bias [Cout], scale / shift [Bt][Cin] (float32), and the flat index
    of the source value the range-flag run replaces"""
    W, H, Cin, Cout, Bt = case
    g = np.random.default_rng(1000 + CASES.index(case))
    x = (g.standard_normal((Bt, H, W, Cin)) * 2.0).astype(np.float32)
    sc = g.uniform(0.5, 2.0, (Bt, Cin)).astype(np.float32)
    sh = g.standard_normal((Bt, Cin)).astype(np.float32)
    # exact zeros and t = scale * x + shift in [-100, -80], at the tile's corners (the wrapped halo) and inside
    px = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2), (H - 1, W // 3)]
    for b in range(Bt):
        for n, (yy, xx) in enumerate(px):
            cs = np.arange(n % 4, Cin, 4)
            t = -80.0 - 20.0 * ((cs + n) % 5) / 4.0
            x[b, yy, xx, cs] = ((t - sh[b, cs]) / sc[b, cs]).astype(np.float32)
            x[b, yy, xx, (cs + 1) % Cin] = 0.0
    w = (g.standard_normal((Cout, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    bias = g.standard_normal(Cout).astype(np.float32)
    big = np.ravel_multi_index((Bt - 1, H - 1, W - 2, Cin - 3), x.shape)
    return x, w, bias, sc, sh, int(big)


# ------------------------------------------------------------------------------------ child: one form, all cases
def child(out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "vae-diffusion-toy-crystals_amd")]
    import torch

    from test_gpu_h2 import pack_frag, pack_h2
    from test_gpu_ops import L, chk, dev, st
    from toycrystals_amd._lib import TcxError

    def padded(nbytes):
        buf = torch.full((PAD + nbytes + PAD,), CANARY, dtype=torch.uint8, device="cuda")
        return buf, buf.data_ptr() + PAD

    out = {}
    stamps = torch.zeros(8, dtype=torch.int64, device="cuda")
    for i, case in enumerate(CASES):
        W, H, Cin, Cout, Bt = case
        x, w, bias, sc, sh, big = inputs(case)
        wh, ws, cpad, kpad = pack_h2(w)
        wf = pack_frag(wh, cpad, kpad, Cin)
        xd, bd, scd, shd = dev(x), dev(bias), dev(sc), dev(sh)
        ny, ng = Bt * H * W * Cout * 4, Bt * max(1, H * W // 128) * Cout * 2 * 8
        ovf = torch.zeros(1, dtype=torch.int32, device="cuda")

        def run(src):
            ybuf, yp = padded(ny)
            gbuf, gp = padded(ng)
            ovf.zero_()
            chk(L().tcx_conv2d_h2_pro(src.data_ptr(), None, Bt, 0, H, W, Cin, 0, wh.data_ptr(),
                                      wf.data_ptr() if wf is not None else None, ws.data_ptr(), bd.data_ptr(), None, None,
                                      yp, 0, Cout, cpad, kpad, 3, 1, 1, 1, 0, gp, scd.data_ptr(), shd.data_ptr(), None,
                                      None, 0, ovf.data_ptr(), st()))
            torch.cuda.synchronize()
            return ybuf.cpu().numpy(), gbuf.cpu().numpy(), int(ovf.item())

        # which kernel the dispatcher chose: only k_conv3m writes the debug stamps
        stamps.zero_()
        chk(L().tcx_debug_conv_stamps(stamps.data_ptr(), 1))
        try:
            run(xd)
        except TcxError as e:
            # only the dispatcher's own refusal of the shape (no kernel of the prologue path covers it) counts as
            # "another kernel"; a launch or LDS-attribute error of the form under test fails the file
            if "the GroupNorm+SiLU prologue needs" not in str(e):
                raise
            stamps.zero_()
        finally:
            chk(L().tcx_debug_conv_stamps(None, 0))
        is3m = bool(stamps.cpu().numpy().any())
        if not is3m:
            out[f"{i}_m"] = np.zeros(5, np.int64)
            continue
        y1, g1, o1 = run(xd)
        y2, g2, o2 = run(xd)
        xb = x.copy()
        b, c = big // (H * W * Cin), big % Cin
        xb.reshape(-1)[big] = (1.0e5 - sh[b, c]) / sc[b, c]  # silu(1e5) leaves the f16 range
        _, _, o3 = run(dev(xb))
        out[f"{i}_y"], out[f"{i}_g"] = y1, g1
        out[f"{i}_m"] = np.array([is3m, o1, o2, o3, np.array_equal(y1, y2) and np.array_equal(g1, g2)], np.int64)
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def forms(tmp_path_factory):
    """{knob: npz of every case's output buffer, partials buffer and flags}"""
    d = tmp_path_factory.mktemp("conv3m_pro1")
    res = {}
    for knob in ("1", "0"):
        path = str(d / f"form_{knob}.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True,
                           timeout=600, env=dict(os.environ, TCX_CONV3M_PRO1_TAB=knob))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        res[knob] = np.load(path)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_pro1_forms(forms, case):
    import conv_ref as R
    from test_gpu_ops import close

    i = CASES.index(case)
    W, H, Cin, Cout, Bt = case
    new, old = forms["1"], forms["0"]
    is3m, o1, o2, o3, same = (int(v) for v in new[f"{i}_m"])
    if not is3m:
        # k_conv3m takes whole 256-pixel tiles of one image (conv3m_takes): only the half-tile shapes may skip
        assert (H * W) % 256 != 0, "k_conv3m did not run a shape it covers"
        assert not int(old[f"{i}_m"][0])
        pytest.skip("the dispatcher gives this shape to another kernel")
    assert int(old[f"{i}_m"][0]), "the knob's form left k_conv3m"
    ny = Bt * H * W * Cout * 4
    ybuf, gbuf = new[f"{i}_y"], new[f"{i}_g"]
    # (c) canaries
    for buf, n in ((ybuf, ny), (gbuf, gbuf.size - 2 * PAD)):
        assert buf.size == n + 2 * PAD
        assert (buf[:PAD] == CANARY).all() and (buf[PAD + n:] == CANARY).all()
    # (a) the two forms, bit for bit
    assert np.array_equal(ybuf, old[f"{i}_y"]), "outputs differ between the forms"
    assert np.array_equal(gbuf, old[f"{i}_g"]), "GroupNorm partials differ between the forms"
    # (d) a second run
    assert same and int(old[f"{i}_m"][4])
    # (e) the range flag
    assert (o1, o2, o3) == (0, 0, 1), (o1, o2, o3)
    assert tuple(int(v) for v in old[f"{i}_m"][1:4]) == (0, 0, 1)
    # (b) float64
    x, w, bias, sc, sh, _ = inputs(case)
    c = R.Cv(case_id(case), Bt, H, W, Cin, Cout, pro=1, gn=True)
    ref = R.evaluate(c, dict(x1=x, x2=None, w=w, bias=bias, bias_b=None, resid=None, sc1=sc, sh1=sh, sc2=None, sh2=None))
    got = ybuf[PAD:PAD + ny].view(np.float32).reshape(Bt, H, W, Cout).astype(np.float64)
    assert np.isfinite(got).all()
    err = close(got, ref["y"])
    part = gbuf[PAD:gbuf.size - PAD].view(np.float64).reshape(Bt, H * W // 128, Cout, 2)
    print(f"{case_id(case)}: max err {err:.3e} of scale {max(1.0, float(np.abs(ref['y']).max())):.2f}")
    # the partials of a 128-pixel group against float64: every output is within e = 2e-5 of the scale (the gate
    # above), so the sum is within 128 e and the sum of squares within 128 e (2 scale + e), plus the kernel's own
    # fp32 per-lane sums (conv_ref.gn_gates: 20 * 2^-24 of sum |y| and of sum y^2)
    scale = max(1.0, float(np.abs(ref["y"]).max()))
    e = 2e-5 * scale
    v = np.abs(ref["y"]).reshape(Bt, H * W // 128, 128, Cout)
    b0 = 128 * e + 20 * 2.0 ** -24 * v.sum(2)
    b1 = 128 * e * (2 * scale + e) + 20 * 2.0 ** -24 * (v * v).sum(2)
    d0, d1 = np.abs(part[..., 0] - ref["gn"][..., 0]), np.abs(part[..., 1] - ref["gn"][..., 1])
    print(f"  partials: sum err {float(d0.max()):.3e} (bound {float(b0.min()):.3e}), squares err {float(d1.max()):.3e} "
          f"(bound {float(b1.min()):.3e})")
    assert (d0 <= b0).all() and (d1 <= b1).all()


if __name__ == "__main__":
    child(sys.argv[1])
