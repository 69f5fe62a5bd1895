#!/usr/bin/env python3
"""Timing of k_attention_split_wide (csrc/attention_split_wide.hip) at Bt = 128 rows (B = 64 with CFG), 4 heads,
d = 96 and 128, N = 256 and 576:
  the three formats (fmt 0 h2 records, 1 bf16 records, 2 two-byte bf16) with the fraction of the 2.5 PFLOP/s
  f16 / bf16 MFMA rate of the products the kernel EXECUTES (S and PV, 2 N^2 d flop each, three f16 products per
  product at fmt 0, one bf16 product at fmt 1 / 2; padding rows of the last tiles not counted), and
  tcx_attention_wide(out_h2 = 1) (fp32 qkv, fp32 MFMA) on the same shapes beside them;
  one CFG evaluation of CondUNetTiny(4, 4, 192) (d = 96), B = 64, at 64x64 and at 96x96: f16x3 with
  TCX_ATTN_SPLIT_WIDE=1 (h2 qkv + k_attention_split_wide) and =0 (fp32 qkv + tcx_attention_wide(out_h2 = 1)),
  alternating pairs, and bf16 once.  The library reads its environment once, so every end-to-end figure comes
  from a fresh child process (`--eval PREC SIZE`).
µs per launch: HIP events around REPS back-to-back launches on the stream, after a warm-up.
PART=kernels runs the kernel part alone."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-diffusion-toy-crystals_amd"))
import torch
from toycrystals_amd import _lib
from toycrystals_amd._lib import lib, check

REPS = int(os.environ.get("REPS", "50"))
PAIRS = int(os.environ.get("PAIRS", "3"))
Bt, heads = 128, 4
PEAK = 2.5e15


def timed(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def evaluation(prec, size):
    """ms per CFG evaluation of the base-192 net at size x size, B = 64: three windows of five"""
    from toycrystals_amd.models.sde_score_model import CondUNetTiny, predict_eps_cfg
    torch.manual_seed(0)
    m = CondUNetTiny(4, 4, 192).cuda().eval()
    B = 64
    x = torch.randn(B, 1, size, size, device="cuda")
    t = torch.full((B,), 0.42, device="cuda")
    y_cat = (torch.arange(B) % 4).cuda()
    y_cont = torch.rand(B, 4, device="cuda")
    _lib.set_conv_precision(prec)
    ts = [timed(lambda: predict_eps_cfg(m, x, t, y_cat, y_cont, 1.5), 5) / 1e3 for _ in range(3)]
    assert _lib.used_conv_precision() == prec, _lib.used_conv_precision()
    print(f"EVAL {prec} {min(ts):.3f} ms (windows {' '.join(f'{v:.2f}' for v in ts)})", flush=True)


def child(prec, size, **env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--eval", prec, str(size)], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [s for s in r.stdout.splitlines() if s.startswith("EVAL")][-1]
    return float(line.split()[2]), line


def stored(qkv, fmt, L, st):
    """[Bt, N, 3C] fp32 -> h2 records / bf16 records (the library's writers), or two-byte bf16"""
    if fmt == 2:
        return qkv.to(torch.bfloat16)
    out = torch.empty_like(qkv)
    if fmt == 1:
        C3 = qkv.shape[2]
        one, zero = torch.ones(Bt, C3, device="cuda"), torch.zeros(Bt, C3, device="cuda")
        check(L.tcx_gn_apply_tab_bf16(qkv.data_ptr(), out.data_ptr(), Bt, qkv.shape[1], C3, one.data_ptr(),
                                      zero.data_ptr(), 0, st))
    else:
        check(L.tcx_f32_to_h2(qkv.data_ptr(), out.data_ptr(), qkv.numel(), None, st))
    return out


def kernels():
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    for d in (96, 128):
        for N in (256, 576):
            C = d * heads
            qkv = torch.randn(Bt, N, 3 * C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(N + d))
            out = torch.empty(Bt, N, C, device="cuda")
            flop = 2 * 2.0 * Bt * heads * N * N * d
            old = lambda: check(L.tcx_attention_wide(qkv.data_ptr(), out.data_ptr(), 1, Bt, N, C, heads, None, st))
            ts = [timed(old) for _ in range(3)]
            print(f"d={d} N={N} tcx_attention_wide(out_h2 = 1): {' '.join(f'{t:.1f}' for t in ts)} us", flush=True)
            for fmt in (0, 1, 2):
                x = stored(qkv, fmt, L, st)
                new = lambda: check(L.tcx_attention_split_wide(x.data_ptr(), out.data_ptr(), fmt, Bt, N, C, heads, st))
                ts = [timed(new) for _ in range(3)]
                k = 3 if fmt == 0 else 1
                print(f"d={d} N={N} split_wide fmt {fmt}: {' '.join(f'{t:.1f}' for t in ts)} us  "
                      f"({k * flop / min(ts) / 1e6:.1f} TFLOP/s executed, {k * flop / (min(ts) * 1e-6) / PEAK:.3f} of the "
                      f"f16 / bf16 MFMA rate)", flush=True)


def main():
    kernels()
    if os.environ.get("PART") == "kernels":
        return
    torch.cuda.empty_cache()
    for size in (64, 96):
        for i in range(PAIRS):
            a, b = child("f16x3", size, TCX_ATTN_SPLIT_WIDE="1")[0], child("f16x3", size, TCX_ATTN_SPLIT_WIDE="0")[0]
            print(f"{size}x{size} base_ch 192 f16x3 pair {i + 1}: TCX_ATTN_SPLIT_WIDE=1 {a:.3f} ms, =0 {b:.3f} ms, "
                  f"ratio {a / b:.4f}", flush=True)
        print(f"{size}x{size} base_ch 192 bf16: " + child("bf16", size)[1], flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--eval":
        evaluation(sys.argv[2], int(sys.argv[3]))
    else:
        main()
