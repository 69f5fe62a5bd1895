#!/usr/bin/env python3
"""Timing of the wide-head attention (tcx_attention_wide, tcx_attention_wide_fwd_lse, tcx_attention_wide_bwd:
csrc/attention_wide.hip, csrc/attention_wide_bwd.hip) at Bt = 128, 4 heads, d = 96 and 128, N = 256 and 576:
  forward (LSE form) and backward (dq + dkv launches) on their own, with the fraction of the 157.3 TFLOP/s
  fp32-MFMA rate of the products the kernels EXECUTE (2 N^2 d flop each: forward S and PV = 2; dq S, dP, dQ = 3;
  dkv S, dP, dK, dV = 4; padding rows of the last tiles not counted).  The dq / dkv split of the backward comes
  from a kernel trace of PART=kernels (the C entry launches both);
  one diffusion_loss_eps forward + backward of CondUNetTiny(4, 4, 192) at 64x64, B = 32, in a fresh child
  process per variant, TCX_ATTN_FUSED=1 (the wide pair) and =0 (the GEMM chain: the only route before these
  kernels) alternating, three pairs.
µs per call: HIP events around REPS back-to-back calls on the stream, after a warm-up.
PART=kernels runs the kernel part alone (for a kernel trace); `--step` is the child of the second part."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-diffusion-toy-crystals_amd"))
import torch
from toycrystals_amd._lib import lib, check

REPS = int(os.environ.get("REPS", "50"))
Bt, heads = 128, 4
PEAK = 157.3e12


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


def step_child():
    from toycrystals_amd import functional as TF
    from toycrystals_amd.models.sde_score_model import CondUNetTiny, VPSDE, diffusion_loss_eps
    torch.manual_seed(0)
    B = 32
    model = CondUNetTiny(4, 4, 192).cuda().train()
    x0 = torch.rand(B, 1, 64, 64, device="cuda")
    y_cat = (torch.arange(B, device="cuda") % 4).to(torch.int64)
    y_cont = torch.rand(B, 4, device="cuda")

    def step():
        model.zero_grad(set_to_none=True)
        diffusion_loss_eps(model, VPSDE(0.1, 30.0), x0, y_cat, y_cont, p_uncond=0.1).backward()

    ms = timed(step, 10, 3) / 1e3
    print(f"TCX_ATTN_FUSED={os.environ.get('TCX_ATTN_FUSED', '1')} (fused switch {TF._ATTN_FUSED}): {ms:.2f} ms per "
          f"forward + backward, peak memory {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB")


def main():
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    for d in (96, 128):
        for N in (256, 576):
            C = d * heads
            g = torch.Generator(device="cuda").manual_seed(N + d)
            qkv = torch.randn(Bt, N, 3 * C, device="cuda", generator=g)
            dout = torch.randn(Bt, N, C, device="cuda", generator=g)
            out, dqkv = torch.empty(Bt, N, C, device="cuda"), torch.empty(Bt, N, 3 * C, device="cuda")
            lse, ws = torch.empty(Bt, heads, N, device="cuda"), torch.empty(Bt, heads, N, device="cuda")
            nb = Bt * heads * N * 4
            assert L.tcx_attention_wide_bwd_workspace(Bt, N, C, heads) == nb
            p = [t.data_ptr() for t in (qkv, out, dout, lse, dqkv, ws)]
            fwd = lambda: check(L.tcx_attention_wide_fwd_lse(p[0], p[1], p[3], Bt, N, C, heads, st))
            bwd = lambda: check(L.tcx_attention_wide_bwd(p[0], p[1], p[2], p[3], p[4], Bt, N, C, heads, p[5], nb, st))
            flop = 2.0 * Bt * heads * N * N * d
            for name, fn, k in (("fwd_lse", fwd, 2), ("bwd (dq + dkv)", bwd, 7)):
                ts = [timed(fn) for _ in range(3)]
                print(f"wide d={d} N={N} {name}: {' '.join(f'{t:.1f}' for t in ts)} us  "
                      f"({k * flop / min(ts) / 1e6:.1f} TFLOP/s executed, {k * flop / (min(ts) * 1e-6) / PEAK:.3f} of the "
                      f"fp32-MFMA rate)", flush=True)
    if os.environ.get("PART") == "kernels":
        return
    torch.cuda.empty_cache()
    for i in range(3):
        for v in ("1", "0"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step"], env=dict(os.environ, TCX_ATTN_FUSED=v),
                               capture_output=True, text=True, timeout=300)
            print(f"64x64 base_ch 192 B=32 step pair {i + 1}: " + (r.stdout.strip().splitlines() or [r.stderr[-400:]])[-1],
                  flush=True)


if __name__ == "__main__":
    step_child() if "--step" in sys.argv else main()
