"""The instruction mix of k_conv3m's tap loop, read from the compiler's assembly (tools/loop_valu_mix.py):
what runs beside the 648 MFMAs of one trip (9 tap pairs) is what the GroupNorm-prologue form costs over
the h2-source one.  Static: compiles conv3m.hip to gfx950 assembly with the Makefile's flags (about half
a minute, once per session), no GPU.

The GroupNorm-prologue form with the LDS offset table (PRO 1, VT) must keep its loop free of packed-f32
VALU (v_pk_*_f32 beside MFMAs cost more than two scalar ops, and the compiler packs two values across the
schedule's fences when it can) and of 32-bit integer multiplies (the halo DMA offsets come from the LDS
table), within 256 VGPRs with no scratch at two workgroups per CU.  Its VALU bound is the arithmetic that
must remain per trip (64 values at 64-px rows, 48 at 32 / 16: exp, rcp, add, fma, multiply, residual, two
converts and a half max each, plus table reads: about 610 / 510) plus 20 % for unit addressing, the DMA
issue and the range flag.  Every other form keeps the count it had when the table was added."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vae-diffusion-toy-crystals_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import loop_valu_mix as lvm  # noqa: E402


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    return re.search(r"^CXXFLAGS := (.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()


@pytest.fixture(scope="session")
def mix(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("conv3m_asm") / "conv3m.s"
    subprocess.run([hipcc, *_makefile_flags(), "--cuda-device-only", "-S", "conv3m.hip", "-o", str(out)],
                   cwd=CSRC, check=True, capture_output=True, timeout=600)
    res = {}
    for sym, (cnt, rsrc) in lvm.analyse(str(out), "k_conv3mILi").items():
        m = re.search(r"k_conv3mILi(\d+)ELb([01])ELi(\d)ELb([01])E", sym)
        assert m, sym
        res[(int(m.group(1)), bool(int(m.group(2))), int(m.group(3)), bool(int(m.group(4))))] = (cnt, rsrc)
    return res


def test_tool_counts_a_loop(tmp_path):
    """the innermost loop with the most MFMAs is the one counted; the outer loop's and the function's other
    instructions are not"""
    f = tmp_path / "k.s"
    f.write_text("\t.type\t_ZN3tcx1kEv,@function\n_ZN3tcx1kEv:\n"
                 "\tv_mul_lo_u32 v1, v2, v3\n"
                 ".LBB0_1:\n\tv_pk_fma_f32 v[0:1], v[2:3], v[4:5], v[6:7]\n"
                 ".LBB0_2:\n"
                 "\tv_mfma_f32_16x16x32_f16 v[0:3], v[4:7], v[8:11], v[0:3]\n"
                 "\tv_mfma_f32_16x16x32_f16 v[0:3], v[4:7], v[8:11], v[0:3]\n"
                 "\tv_exp_f32_e32 v1, v1\n\tv_cndmask_b32_e32 v1, v2, v3, vcc\n\tv_readlane_b32 s0, v1, 3\n"
                 "\tds_read_b32 v1, v2\n\ts_add_i32 s0, s0, 1\n"
                 "\ts_cbranch_scc1 .LBB0_2\n"
                 "\tv_mul_hi_u32 v1, v2, v3\n\ts_cbranch_scc1 .LBB0_1\n"
                 ".Lfunc_end0:\n; NumVgprs: 12\n; ScratchSize: 0\n; Occupancy: 8\n")
    (cnt, rsrc), = lvm.analyse(str(f)).values()
    assert cnt == {"mfma": 2, "valu": 3, "pk_f32": 0, "imul32": 0, "lane": 1, "cndmask": 1, "trans": 1}
    assert rsrc["NumVgprs"] == 12 and rsrc["ScratchSize"] == 0 and rsrc["Occupancy"] == 8


def test_every_form_is_compiled(mix):
    for w in (16, 32, 64):
        assert {(w, True, 0, False), (w, False, 0, False), (w, True, 1, True), (w, True, 2, False),
                (w, True, 3, False)} <= set(mix)
    for cnt, _ in mix.values():
        assert cnt["mfma"] == 648  # 9 tap pairs x 72


@pytest.mark.parametrize("w,bound", [(64, 750), (32, 620), (16, 620)])
def test_pro1_table_form_loop(mix, w, bound):
    cnt, rsrc = mix[(w, True, 1, True)]
    print(w, cnt, rsrc)
    assert cnt["pk_f32"] == 0
    assert cnt["imul32"] == 0
    assert rsrc["ScratchSize"] == 0
    assert rsrc["Occupancy"] == 2
    assert rsrc["NumVgprs"] <= 256
    assert cnt["valu"] <= bound


def test_other_forms_keep_their_loops(mix):
    """loop VALU per trip no higher than before the table: 8 for the h2-source forms, 72 / 64 with a
    chunk-major second source (PRO 2), and the knob's PRO 1 form without the table as it was"""
    before = {0: {64: 8, 32: 8, 16: 8}, 3: {64: 8, 32: 8, 16: 8}, 2: {64: 72, 32: 64, 16: 64},
              1: {64: 1118, 32: 910, 16: 911}}
    for (w, fast, pro, vt), (cnt, rsrc) in mix.items():
        if vt:
            continue
        print(w, fast, pro, cnt, rsrc)
        assert cnt["valu"] <= before[pro][w], (w, fast, pro)
        assert rsrc["ScratchSize"] == 0 and rsrc["Occupancy"] == 2, (w, fast, pro)
