"""The instruction mix of the record loops of three memory passes of the 64^2 U-Net, read from the compiler's
assembly (tools/pass_valu_mix.py): the first conv's record kernel, the banded x2 upsample's output phase and
the register head.  They move 32-48 B per record and were bound by VALU issue, not by HBM: 313 VALU per
record in k_conv_first_rec's loop, 220 in k_upsample2x_band<4, true>'s, 222 per 8-pixel pass in k_head8r<3>,
half of it index decode (divisions, integer multiplies, address forming, ds_bpermute shuffles).  Static:
compiles unet_first.hip, unet_head.hip and norm.hip to gfx950 assembly with the Makefile's flags (a minute or
two, once per session), no GPU.

Bounds.  First conv: the arithmetic of a record is about 160 VALU (72 fma, 8 x (fma, mul, exp2, add, rcp,
mul), ~30 for the f16 split, the range flag); at 183 the modelled VALU time equals the 74 us the 403 MB
write takes at the GroupNorm-apply pass's rate, and 200 leaves a margin of 17.  Upsample: the lerp and the
split of a record need about 95; 130.  Head: no more than the 222 per pass it had with the shuffles.  A unit
(record, or pass of the head) is two global stores in all three kernels."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vae-diffusion-toy-crystals_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pass_valu_mix as pvm  # noqa: E402

FIRST = r"k_conv_first_rec96"
UPS = (r"k_upsample2x_bandILi4ELb1ELi16ELi192EE", r"k_upsample2x_bandILi4ELb1ELi32ELi96EE")
HEAD = r"k_head8rILi3ELb0ELb0EE"  # k_head8r<3, false, false>: fp32 source, DPP reduction


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
def asm(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    d = tmp_path_factory.mktemp("pass_asm")
    procs = {n: subprocess.Popen([hipcc, *_makefile_flags(), "--cuda-device-only", "-S", n + ".hip", "-o",
                                  str(d / (n + ".s"))], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for n in ("unet_first", "unet_head", "norm")}
    for n, p in procs.items():
        out, _ = p.communicate(timeout=900)
        assert p.returncode == 0, out.decode(errors="replace")[-2000:]
    return {n: str(d / (n + ".s")) for n in procs}


def _one(path, pattern):
    res = pvm.analyse(path, pattern)
    assert len(res) == 1, (pattern, list(res))
    (cnt, rsrc, looped), = res.values()
    print(pattern, cnt, rsrc, "loop" if looped else "whole kernel")
    return cnt, rsrc, looped


def test_tool_counts_the_store_loop(tmp_path):
    """the innermost loop with the most global stores is counted; a side block that rejoins the body with an
    s_branch is no loop; a kernel without a store loop is counted whole"""
    f = tmp_path / "k.s"
    f.write_text("\t.type\t_ZN3tcx1kEv,@function\n_ZN3tcx1kEv:\n"
                 "\tv_mul_lo_u32 v1, v2, v3\n"
                 ".LBB0_1:\n\tv_add_u32_e32 v1, v2, v3\n\ts_cbranch_scc1 .LBB0_1\n"
                 "\ts_branch .LBB0_3\n"
                 ".LBB0_2:\n\tv_fma_f32 v1, v2, v3, v4\n\tv_mul_hi_u32 v1, v2, v3\n\tv_rcp_f32_e32 v1, v1\n"
                 "\tglobal_store_dwordx4 v[0:1], v[2:5], off\n"
                 ".LBB0_3:\n\tds_read_b128 v[0:3], v4\n\tds_bpermute_b32 v1, v2, v3\n\tv_mul_u32_u24_e32 v1, v2, v3\n"
                 "\tglobal_store_dwordx4 v[0:1], v[2:5], off offset:16\n\ts_add_i32 s0, s0, 1\n"
                 "\ts_cbranch_scc1 .LBB0_2\n"
                 "\tv_mov_b32_e32 v1, v2\n\tglobal_store_dword v[0:1], v2, off\n\ts_branch .LBB0_2\n"
                 ".Lfunc_end0:\n; NumVgprs: 12\n; ScratchSize: 0\n; Occupancy: 8\n"
                 "\t.type\t_ZN3tcx1jEv,@function\n_ZN3tcx1jEv:\n"
                 "\tv_mov_b32_e32 v1, v2\n\tglobal_store_dword v[0:1], v2, off\n\ts_endpgm\n"
                 ".Lfunc_end1:\n; NumVgprs: 3\n; ScratchSize: 8\n")
    res = pvm.analyse(str(f))
    cnt, rsrc, looped = res["_ZN3tcx1kEv"]
    assert looped
    assert cnt == {"valu": 4, "imul32": 1, "trans": 1, "lds": 2, "bpermute": 1, "stores": 2}
    assert rsrc["NumVgprs"] == 12 and rsrc["ScratchSize"] == 0
    cnt, rsrc, looped = res["_ZN3tcx1jEv"]
    assert not looped and cnt["valu"] == 1 and cnt["stores"] == 1 and rsrc["ScratchSize"] == 8


def test_first_conv_record_loop(asm):
    cnt, rsrc, looped = _one(asm["unet_first"], FIRST)
    assert looped and cnt["stores"] == 2  # one record per trip
    assert cnt["imul32"] == 0
    assert rsrc["ScratchSize"] == 0
    assert rsrc["NumVgprs"] <= 100
    assert cnt["valu"] <= 200


@pytest.mark.parametrize("sym", UPS)
def test_upsample_record_loop(asm, sym):
    cnt, rsrc, looped = _one(asm["norm"], sym)
    assert looped and cnt["stores"] == 8  # a column's four records per trip
    assert cnt["imul32"] == 0
    assert rsrc["ScratchSize"] == 0
    assert cnt["lds"] == 16  # each staged row's horizontal pair is read once
    assert cnt["valu"] / 4 <= 130


def test_head_passes(asm):
    cnt, rsrc, looped = _one(asm["unet_head"], HEAD)
    assert not looped and cnt["stores"] == 16  # the 8 passes are unrolled: the whole kernel, two stores per pass
    assert cnt["bpermute"] == 0
    assert rsrc["ScratchSize"] == 0
    assert cnt["valu"] / 8 <= 222
