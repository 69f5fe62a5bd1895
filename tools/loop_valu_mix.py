#!/usr/bin/env python3
"""Instruction mix of a kernel's main MFMA loop, from the compiler's assembly.

For every function of a `.s` file (hipcc -S --cuda-device-only) whose symbol matches a pattern, find
the innermost loop (a label and a later branch back to it) that holds the most v_mfma instructions and
count, over one trip of it: MFMAs, VALU instructions (every v_* that is not an MFMA), packed-f32 VALU
(v_pk_*_f32), 32-bit integer multiplies (v_mul_lo_u32 / v_mul_hi_u32 / _i32), lane moves
(v_readlane / v_writelane: SGPRs spilled to VGPR lanes), v_cndmask and transcendentals (v_exp, v_log,
v_rcp, v_rsq, v_sqrt, v_sin, v_cos), with the function's NumVgprs / ScratchSize / Occupancy comment
lines.  Blocks only some waves execute (role branches inside the loop) count in full.

usage: loop_valu_mix.py file.s [symbol-regex]        (default pattern: every function with an MFMA loop)
"""
import re
import shutil
import subprocess
import sys

CLASSES = ("mfma", "valu", "pk_f32", "imul32", "lane", "cndmask", "trans")
_TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")
_LABEL = re.compile(r"^([.\w$]+):")
_BRANCH = re.compile(r"^\s+s_c?branch\w*\s+([.\w$]+)")
_INSN = re.compile(r"^\s+([a-z]\w+)")


def classify(op: str):
    """Classes of one mnemonic (a tuple of names from CLASSES)."""
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return ("mfma",)
    if not op.startswith("v_"):
        return ()
    out = ["valu"]
    if op.startswith("v_pk_") and op.endswith("_f32"):
        out.append("pk_f32")
    if re.match(r"v_mul_(lo|hi)_[ui]32", op):
        out.append("imul32")
    if op.startswith("v_readlane") or op.startswith("v_writelane"):
        out.append("lane")
    if op.startswith("v_cndmask"):
        out.append("cndmask")
    if op.startswith(_TRANS):
        out.append("trans")
    return tuple(out)


def functions(lines):
    """(symbol, first line, end line) of every function, and its trailing resource comments."""
    out = []
    i = 0
    while i < len(lines):
        m = re.match(r"^\s+\.type\s+([\w$.]+),@function", lines[i])
        if m:
            sym = m.group(1)
            j = i
            while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
                j += 1
            res = {}
            for k in range(j, min(j + 80, len(lines))):
                r = re.match(r"^;\s*(NumVgprs|NumAgprs|ScratchSize|Occupancy|NumSgprs|LDSByteSize):\s*(\d+)", lines[k])
                if r and r.group(1) not in res:
                    res[r.group(1)] = int(r.group(2))
            out.append((sym, i, j, res))
            i = j
        i += 1
    return out


def main_loop(lines, lo, hi):
    """(first, last) line of the innermost loop of lines[lo:hi] with the most MFMAs, or None."""
    labels = {}
    best = None
    for n in range(lo, hi):
        m = _LABEL.match(lines[n])
        if m:
            labels[m.group(1)] = n
            continue
        b = _BRANCH.match(lines[n])
        if b and b.group(1) in labels:  # a branch back
            a = labels[b.group(1)]
            nm = sum(1 for t in range(a, n) if (i := _INSN.match(lines[t])) and classify(i.group(1)) == ("mfma",))
            key = (nm, -(n - a))
            if nm > 0 and (best is None or key > best[0]):
                best = (key, a, n)
    return None if best is None else (best[1], best[2])


def loop_mix(lines, a, b):
    cnt = dict.fromkeys(CLASSES, 0)
    for t in range(a, b + 1):
        i = _INSN.match(lines[t])
        if i:
            for c in classify(i.group(1)):
                cnt[c] += 1
    return cnt


def analyse(path, pattern=None):
    """{symbol: (counts dict, resources dict)} of every matching function with an MFMA loop."""
    lines = open(path).read().splitlines()
    rx = re.compile(pattern) if pattern else None
    out = {}
    for sym, lo, hi, res in functions(lines):
        if rx and not rx.search(sym):
            continue
        lp = main_loop(lines, lo, hi)
        if lp:
            out[sym] = (loop_mix(lines, *lp), res)
    return out


def demangle(sym):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt:
        return sym
    try:
        return subprocess.run([filt, sym], capture_output=True, text=True, timeout=10).stdout.strip() or sym
    except (OSError, subprocess.SubprocessError):
        return sym


def main() -> int:
    if len(sys.argv) < 2:
        print(__doc__)
        return 2
    res = analyse(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else None)
    print(f"{'MFMA':>5} {'VALU':>5} {'pk_f32':>6} {'imul32':>6} {'lane':>5} {'cndmask':>7} {'trans':>5} "
          f"{'VGPR':>5} {'scratch':>7} {'occ':>3}  main loop of")
    for sym, (c, r) in res.items():
        name = re.sub(r"tcx::\(anonymous namespace\)::|void |\(tcx::ConvParams\)", "", demangle(sym))
        print(f"{c['mfma']:5d} {c['valu']:5d} {c['pk_f32']:6d} {c['imul32']:6d} {c['lane']:5d} {c['cndmask']:7d} "
              f"{c['trans']:5d} {r.get('NumVgprs', -1):5d} {r.get('ScratchSize', -1):7d} {r.get('Occupancy', -1):3d}  {name}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
