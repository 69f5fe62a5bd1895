"""GPU: the fused attention block of the split-precision evaluator (csrc/attn_block.hip: the qkv 1x1 conv
computed inside the attention workgroup, then the proj launch) against float64 and against the three
launches it replaces (qkv conv, k_attention_split, proj conv; TCX_ATTN_BLOCK=0).

The fused kernel forms the same products in the same order per output element as the three launches (the
qkv GEMM's chunk order and hi*lo, lo*hi, hi*hi order, the attention loop unchanged), so this pull request
claims the "same order kept" outcome: bit-identical block outputs and whole forwards."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from oracle import nn_np

from test_gpu_h2 import from_h2, pack_h2, to_h2
from test_gpu_ops import L, chk, dev, st

pytestmark = pytest.mark.gpu

N, C, HEADS = 256, 192, 4


def _weights(rng, co, ci):
    """Packed h2 weights of a 1x1 conv, its bias, and the float64 values the pack represents."""
    w = rng.standard_normal((co, ci, 1, 1)) / np.sqrt(ci)
    b = rng.standard_normal(co) * 0.1
    wh, ws, cpad, kpad = pack_h2(w)
    assert kpad == ci
    wd = from_h2(wh).double().cpu().numpy()[:co, :ci] * float(ws[0].item())
    return wh, ws, cpad, dev(b), wd, b.astype(np.float32).astype(np.float64)


def _conv1x1(x, wh, ws, b, cpad, co, Bt, resid, y, out_h2, ovf):
    chk(L().tcx_conv2d_h2_pro(x.data_ptr(), None, Bt, 0, 16, 16, C, 0, wh.data_ptr(), None, ws.data_ptr(), b.data_ptr(),
                              None, resid.data_ptr() if resid is not None else None, y.data_ptr(), int(out_h2), co,
                              cpad, C, 1, 1, 0, 1, 0, None, None, None, None, None, 0, ovf.data_ptr(), st()))


@pytest.mark.parametrize("Bt,amp", [(1, 1.0), (3, 1.0), (1, 3.0), (3, 3.0)])
def test_block_vs_float64_and_three_launches(Bt, amp):
    """a + proj(attention(qkv(x))) on h2-representable records x (amp 3: peaked softmax rows), a random fp32
    residual and random packed weights, against float64 numpy on the values the h2 inputs represent; the
    three launches on the same inputs give e3 against the same reference.  Gate: err_fused <= 2 e3 + 2e-7 of
    the scale (what test_attention_split_vs_oracle grants a reordered accumulation); and, the order being
    kept, the two outputs are bit-equal."""
    rng = np.random.default_rng(1000 * Bt + int(amp))
    xh = to_h2(dev(rng.standard_normal((Bt, N, C)) * amp))
    xd = from_h2(xh).double().cpu().numpy()
    resid = dev(rng.standard_normal((Bt, N, C)))
    qwh, qws, qcp, qb, qw64, qb64 = _weights(rng, 3 * C, C)
    pwh, pws, pcp, pb, pw64, pb64 = _weights(rng, C, C)
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")

    # float64 reference
    qkv = xd @ qw64.T + qb64
    d = C // HEADS
    sp = lambda a: a.reshape(Bt, N, HEADS, d).transpose(0, 2, 1, 3)  # noqa: E731
    o = nn_np.sdpa(sp(qkv[..., :C]), sp(qkv[..., C:2 * C]), sp(qkv[..., 2 * C:])).transpose(0, 2, 1, 3).reshape(Bt, N, C)
    ref = resid.double().cpu().numpy() + o @ pw64.T + pb64

    # fused: qkv + attention in one kernel, then proj + residual in place
    a_f = resid.clone()
    oh = torch.empty((Bt, N, C), device="cuda")
    chk(L().tcx_attn_block_h2(xh.data_ptr(), a_f.data_ptr(), oh.data_ptr(), qwh.data_ptr(), qws.data_ptr(),
                              qb.data_ptr(), qcp, pwh.data_ptr(), pws.data_ptr(), pb.data_ptr(), pcp, Bt, N, C, HEADS,
                              ovf.data_ptr(), st()))
    # the three launches
    a_3 = resid.clone()
    qkv_h = torch.empty((Bt, N, 3 * C), device="cuda")
    o3 = torch.empty((Bt, N, C), device="cuda")
    _conv1x1(xh, qwh, qws, qb, qcp, 3 * C, Bt, None, qkv_h, True, ovf)
    chk(L().tcx_attention_split(qkv_h.data_ptr(), o3.data_ptr(), Bt, N, C, HEADS, st()))
    _conv1x1(o3, pwh, pws, pb, pcp, C, Bt, a_3, a_3, False, ovf)
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0

    got_f, got_3 = a_f.double().cpu().numpy(), a_3.double().cpu().numpy()
    scale = max(1.0, float(np.abs(ref).max()))
    e_f, e_3 = float(np.abs(got_f - ref).max()), float(np.abs(got_3 - ref).max())
    print(f"attention block Bt {Bt} amp {amp}: fused err {e_f:.3e}  three-launch err {e_3:.3e}  (scale {scale:.2f})")
    assert e_3 <= 2e-5 * scale
    assert e_f <= 2 * e_3 + 2e-7 * scale, (e_f, e_3)
    # the records as bit patterns (a hi / lo pair read as one fp32 can be a NaN)
    assert torch.equal(oh.view(torch.int32), o3.view(torch.int32)), "attention output records differ"
    assert np.array_equal(got_f, got_3)


CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests", sys.argv[1] + "/vae-diffusion-toy-crystals_amd"]
from toycrystals_amd import _lib
from test_gpu_models import cu, unet
prec, base, B, H = sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
g = np.random.default_rng(11)
x = g.standard_normal((B, 1, H, H)).astype(np.float32)
t = g.uniform(0.05, 0.95, B).astype(np.float32)
y = (np.arange(B) % 4).astype(np.int64)
yc = g.uniform(-1, 1, (B, 4)).astype(np.float32)
m = unet(base)
_lib.set_conv_precision(prec)
with torch.no_grad():
    e = m(cu(x), cu(t), cu(y), cu(yc)).cpu().numpy()
np.save(sys.argv[2], e)
"""


def _forward(tmp_path, knob, prec, base, B, H):
    """One forward in a child process (the library reads TCX_ATTN_BLOCK once)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / f"e_{knob}.npy")
    r = subprocess.run([sys.executable, "-c", CHILD, root, path, prec, str(base), str(B), str(H)],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, TCX_ATTN_BLOCK=knob))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(path)


def test_forward_knob_on_vs_off_bit_identical(tmp_path):
    """unet(96), B = 3, 64x64, f16x3: the bottleneck is N = 256, C = 192, 4 heads, so TCX_ATTN_BLOCK=1 runs
    k_attn_block; the whole forward is bit-identical to the three launches."""
    a = _forward(tmp_path, "1", "f16x3", 96, 3, 64)
    b = _forward(tmp_path, "0", "f16x3", 96, 3, 64)
    print(f"knob on vs off: max |diff| {float(np.abs(a - b).max()):.3e} of scale {float(np.abs(b).max()):.3f}")
    assert np.isfinite(a).all()
    assert np.array_equal(a, b)


@pytest.mark.parametrize("prec,base,H", [("f16x3", 32, 64), ("f16x3", 96, 32), ("bf16", 96, 64)])
def test_other_shapes_and_formats_keep_the_three_launches(tmp_path, prec, base, H):
    """C2 = 64 (unet(32)), N = 64 (32x32) and the bf16 records never reach the fused kernel: the forward is
    bit-identical with the knob at 1 and 0."""
    a = _forward(tmp_path, "1", prec, base, 3, H)
    b = _forward(tmp_path, "0", prec, base, 3, H)
    assert np.isfinite(a).all()
    assert np.array_equal(a, b)


def test_range_flag_from_fused_kernel_falls_back_to_fp32():
    """As test_gpu_h2.test_unet_range_fallback_to_fp32 with qkv.weight scaled by 1e5: q, k, v leave the f16
    range inside k_attn_block, which raises the flag; the evaluator warns and returns the fp32 result."""
    from toycrystals_amd import _lib
    from toycrystals_amd.models.sde_score_model import CondUNetTiny
    torch.manual_seed(0)
    m = CondUNetTiny(4, 4, 96).cuda().eval()
    with torch.no_grad():
        m.attn.qkv.weight.mul_(1e5)
    x = torch.randn(2, 1, 64, 64, device="cuda")
    t = torch.full((2,), 0.3, device="cuda")
    yc = torch.tensor([0, 1], device="cuda")
    yv = torch.zeros(2, 4, device="cuda")
    old = _lib.conv_precision()
    _lib.set_conv_precision("f16x3")
    try:
        with warnings.catch_warnings(record=True) as rec, torch.no_grad():
            warnings.simplefilter("always")
            e = m(x, t, yc, yv)
        assert any("f16 range" in str(r.message) for r in rec)
        _lib.set_conv_precision("fp32")
        with torch.no_grad():
            e32 = m(x, t, yc, yv)
    finally:
        _lib.set_conv_precision(old)
    assert torch.equal(e, e32)
