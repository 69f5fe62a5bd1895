"""GPU: the decode-free forms of three memory passes against the forms they replace, bit for bit, in one process
through tcx_debug_pass_forms (bit 0 the first conv's record kernel, bit 1 the banded x2 upsample, bit 2 the
register head's reduction; a set bit selects the older form).  Both forms evaluate the same expressions on
the same values, so nothing but equality is accepted: records, range flag and eps.

The upsample goes through the C ABI with its output between runs of 0x7b bytes; every call runs twice (a
form that depended on what the first call left behind would differ).  The first conv and the head have no
entry of their own and run inside a CondUNetTiny forward with classifier-free guidance."""
import warnings

import numpy as np
import pytest
import torch

from test_gpu_ops import L, chk, dev, st

pytestmark = pytest.mark.gpu

PAD = 4096  # canary bytes either side of an output


@pytest.fixture(autouse=True)
def _new_forms_afterwards():
    from toycrystals_amd import _lib
    prec = _lib.conv_precision()
    _lib.set_conv_precision("f16x3")
    yield
    _lib.set_conv_precision(prec)
    L().tcx_debug_pass_forms(0)


def _upsample(mask, x, sc, sh, shape):
    """(record bytes, range flag) of tcx_upsample2x_h2 under `mask`, run twice; the canaries are checked."""
    Bt, H, W, C = shape
    n = Bt * 2 * H * 2 * W * C * 4
    out = []
    prev = L().tcx_debug_pass_forms(mask)
    try:
        for _ in range(2):
            buf = torch.full((n + 2 * PAD,), 0x7B, dtype=torch.uint8, device="cuda")
            ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
            chk(L().tcx_upsample2x_h2(x.data_ptr(), buf.data_ptr() + PAD, Bt, H, W, C,
                                      sc.data_ptr() if sc is not None else None,
                                      sh.data_ptr() if sh is not None else None, ovf.data_ptr(), st()))
            b = buf.cpu().numpy()
            assert np.all(b[:PAD] == 0x7B) and np.all(b[PAD + n:] == 0x7B), "canary"
            out.append((b[PAD:PAD + n].copy(), int(ovf.item())))
    finally:
        L().tcx_debug_pass_forms(prev)
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    return out[0]


# (2, 6, 16, 192): 3 bands per image; (1, 2, 385, 8): W C = 3080, beside the band limit of 3072 — k_upsample2x_g8
UP_SHAPES = [(2, 2, 2, 8), (3, 4, 2, 16), (2, 6, 16, 192), (2, 16, 16, 192), (2, 32, 32, 96), (1, 2, 385, 8)]


@pytest.mark.parametrize("tables", [False, True])
@pytest.mark.parametrize("shape", UP_SHAPES)
def test_upsample_forms_bit_for_bit(shape, tables):
    Bt, H, W, C = shape
    rng = np.random.default_rng(11)
    x = dev(rng.standard_normal(shape) * 2.0)
    sc = dev(rng.uniform(0.5, 1.5, (Bt, C))) if tables else None
    sh = dev(rng.standard_normal((Bt, C))) if tables else None
    new, fnew = _upsample(0, x, sc, sh, shape)
    old, fold = _upsample(7, x, sc, sh, shape)
    assert fnew == 0 and fold == 0
    assert np.array_equal(new, old)
    # one value beyond the f16 range, in the first and in the last band: the same flag, the same bytes
    for pos in ((0, 0, 0, 0), (Bt - 1, H - 1, W - 1, C - 1)):
        xs = x.clone()
        xs[pos] = 3.0e5 if not tables else 3.0e5 / float(sc[pos[0], pos[3]])
        new, fnew = _upsample(0, xs, sc, sh, shape)
        old, fold = _upsample(7, xs, sc, sh, shape)
        assert fnew == 1 and fold == 1, (pos, fnew, fold)
        assert np.array_equal(new, old)


def _eps(model, mask, args):
    """(eps, range flag, warned) of a CFG forward under `mask`, run twice."""
    from toycrystals_amd.models.sde_score_model import predict_eps_cfg
    out = []
    prev = L().tcx_debug_pass_forms(mask)
    try:
        for _ in range(2):
            with warnings.catch_warnings(record=True) as rec, torch.no_grad():
                warnings.simplefilter("always")
                e = predict_eps_cfg(model, *args, 1.5).cpu().numpy()
            out.append((e, int(model.tcx_pack().ovf[0].item()), any("f16 range" in str(r.message) for r in rec)))
    finally:
        L().tcx_debug_pass_forms(prev)
    assert np.array_equal(out[0][0], out[1][0], equal_nan=True) and out[0][1:] == out[1][1:]
    return out[0]


# base 96 at 64^2: k_conv_first_rec96 and k_head8r<3>; base 32 at 32^2: the run-time record kernel and
# k_head8r<1>; base 16 at 16^2: the fallback head (fp32 convs: base_ch % 32 != 0)
@pytest.mark.parametrize("base,hw,B", [(96, 64, 2), (32, 32, 3), (16, 16, 3)])
def test_unet_forward_forms_bit_for_bit(base, hw, B):
    from toycrystals_amd.models.sde_score_model import CondUNetTiny
    torch.manual_seed(base)
    m = CondUNetTiny(4, 4, base).cuda().eval()
    g = torch.Generator().manual_seed(3)
    args = (torch.randn(B, 1, hw, hw, generator=g).cuda(), torch.linspace(0.2, 0.8, B).cuda(),
            (torch.arange(B) % 4).cuda(), torch.randn(B, 4, generator=g).cuda())
    new = _eps(m, 0, args)
    old = _eps(m, 7, args)
    assert np.isfinite(new[0]).all() and float(np.abs(new[0]).max()) > 0
    assert new[1] == 0 and old[1] == 0 and not new[2] and not old[2]
    assert np.array_equal(new[0], old[0])
    # a GroupNorm_0 gain that takes the first conv's records beyond the f16 range: the same flag (and the
    # same fp32 recomputation) under both forms
    with torch.no_grad():
        m.down1.net[1].weight.mul_(1.0e6)
    new = _eps(m, 0, args)
    old = _eps(m, 7, args)
    split = base % 32 == 0
    assert new[1] == old[1] == (1 if split else 0) and new[2] == old[2] == split
    assert np.array_equal(new[0], old[0], equal_nan=True)
