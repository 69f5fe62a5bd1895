#!/usr/bin/env python3
"""Instruction mix of the record loop of a non-MFMA pass kernel, from the compiler's assembly.

The memory passes of the U-Net (first conv, upsample, head, GroupNorm apply) move 32-64 B per record and
are bound by VALU issue, not by HBM, when the index decode around the arithmetic is large.  For every
function of a `.s` file (hipcc -S --cuda-device-only) whose symbol matches a pattern, this finds the record
loop — the innermost loop (a label and a later branch back to it) that holds the most global stores; a
kernel whose passes are fully unrolled has none and is counted whole — and reports over one trip of it:
VALU instructions, 32-bit integer multiplies (v_mul_lo / v_mul_hi / v_mad_u32_u24 and kin do not count:
only the quarter-rate v_mul_{lo,hi}_{u,i}32 and v_mad_{u,i}64_{u,i}32), transcendentals, LDS operations
(ds_*, ds_bpermute among them, also listed alone), global stores, and the function's VGPRs and scratch.
Blocks only some lanes or waves execute (uniform branches inside the loop) count in full, so a loop with
two alternative bodies counts both.

--per N divides the per-trip counts by N records (or passes) per trip.

usage: pass_valu_mix.py file.s [symbol-regex] [--per N]
"""
import re
import sys

import loop_valu_mix as lvm

COLUMNS = ("valu", "imul32", "trans", "lds", "bpermute", "stores")
_STORE = re.compile(r"^(global|buffer|flat)_store_")
_IMUL = re.compile(r"^v_(mul_(lo|hi)_[ui]32|mad_[ui]64_[ui]32)")
_CBRANCH = re.compile(r"^\s+s_cbranch\w*\s+([.\w$]+)")
_TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")


def classify(op: str):
    out = []
    if op.startswith("v_"):
        out.append("valu")
        if _IMUL.match(op):
            out.append("imul32")
        if op.startswith(_TRANS):
            out.append("trans")
    elif op.startswith("ds_"):
        out.append("lds")
        if op.startswith("ds_bpermute") or op.startswith("ds_permute"):
            out.append("bpermute")
    elif _STORE.match(op):
        out.append("stores")
    return out


def _count(lines, a, b):
    cnt = dict.fromkeys(COLUMNS, 0)
    for t in range(a, b + 1):
        i = lvm._INSN.match(lines[t])
        if i:
            for c in classify(i.group(1)):
                cnt[c] += 1
    return cnt


def record_loop(lines, lo, hi):
    """(first, last) line of the innermost loop of lines[lo:hi] with the most global stores, or None."""
    labels = {}
    best = None
    for n in range(lo, hi):
        m = lvm._LABEL.match(lines[n])
        if m:
            labels[m.group(1)] = n
            continue
        b = _CBRANCH.match(lines[n])  # a loop's latch; an s_branch back is a side block rejoining the body
        if b and b.group(1) in labels:
            a = labels[b.group(1)]
            ns = _count(lines, a, n)["stores"]
            key = (ns, -(n - a))
            if ns > 0 and (best is None or key > best[0]):
                best = (key, a, n)
    return None if best is None else (best[1], best[2])


def analyse(path, pattern=None):
    """{symbol: (counts per trip, resources, looped)}: looped is False where the whole function was counted."""
    lines = open(path).read().splitlines()
    rx = re.compile(pattern) if pattern else None
    out = {}
    for sym, lo, hi, res in lvm.functions(lines):
        if rx and not rx.search(sym):
            continue
        lp = record_loop(lines, lo, hi)
        a, b = lp if lp else (lo, hi)
        out[sym] = (_count(lines, a, b), res, lp is not None)
    return out


def main() -> int:
    args = [a for a in sys.argv[1:]]
    per = 1
    if "--per" in args:
        k = args.index("--per")
        per = int(args[k + 1])
        del args[k:k + 2]
    if not args:
        print(__doc__)
        return 2
    res = analyse(args[0], args[1] if len(args) > 1 else None)
    print(f"{'VALU':>7} {'imul32':>6} {'trans':>6} {'LDS':>5} {'bperm':>5} {'stores':>6} {'VGPR':>5} {'scratch':>7}  "
          f"record loop of (per {per})")
    for sym, (c, r, looped) in res.items():
        name = re.sub(r"tcx::\(anonymous namespace\)::|void ", "", lvm.demangle(sym))
        name = re.sub(r"\(.*$", "", name) + ("" if looped else "  [no loop: whole kernel]")
        print(f"{c['valu'] / per:7.1f} {c['imul32'] / per:6.1f} {c['trans'] / per:6.1f} {c['lds'] / per:5.1f} "
              f"{c['bpermute'] / per:5.1f} {c['stores'] / per:6.1f} {r.get('NumVgprs', -1):5d} "
              f"{r.get('ScratchSize', -1):7d}  {name}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
