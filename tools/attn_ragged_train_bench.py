#!/usr/bin/env python3
"""Timing of the any-N training attention (tcx_attention_ragged_fwd_lse, tcx_attention_ragged_bwd:
csrc/attention_ragged.hip, csrc/attention_ragged_bwd.hip) at the base-96 bottleneck's training shape,
Bt = 128, C = 192, 4 heads (d = 48):
  N = 576 (96x96): forward and backward (dq + dkv launches) on their own;
  N = 512: alternating pairs beside tcx_attention_fwd_lse + tcx_attention_bwd, the only size both serve
           (information only: AttentionFn routes no shape of the existing set to the new entries);
  one diffusion_loss_eps forward + backward of CondUNetTiny(4, 4, 96) at 96x96, B = 128, in a fresh child
  process per variant, TCX_ATTN_FUSED=1 and =0 (the GEMM chain: the only route before these kernels)
  alternating, three pairs.
µs per call: HIP events around REPS back-to-back calls on the stream, after a warm-up.
PART=kernels runs the N = 576 part alone (for a kernel trace); `--step` is the child of the third part."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-diffusion-toy-crystals_amd"))
import torch
from toycrystals_amd._lib import lib, check

REPS = int(os.environ.get("REPS", "50"))
Bt, C, heads = 128, 192, 4


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
    B = 128
    model = CondUNetTiny(4, 4, 96).cuda().train()
    x0 = torch.rand(B, 1, 96, 96, device="cuda")
    y_cat = (torch.arange(B, device="cuda") % 4).to(torch.int64)
    y_cont = torch.rand(B, 4, device="cuda")

    def step():
        model.zero_grad(set_to_none=True)
        diffusion_loss_eps(model, VPSDE(0.1, 30.0), x0, y_cat, y_cont, p_uncond=0.1).backward()

    ms = timed(step, 5, 2) / 1e3
    print(f"TCX_ATTN_FUSED={os.environ.get('TCX_ATTN_FUSED', '1')} (fused switch {TF._ATTN_FUSED}): {ms:.2f} ms per "
          f"forward + backward, peak memory {torch.cuda.max_memory_allocated() / 2**30:.2f} GiB")
    return ms


def main():
    L = lib()
    st = torch.cuda.current_stream().cuda_stream

    def bufs(N):
        g = torch.Generator(device="cuda").manual_seed(N)
        t = dict(qkv=torch.randn(Bt, N, 3 * C, device="cuda", generator=g),
                 dout=torch.randn(Bt, N, C, device="cuda", generator=g))
        for k in ("out", "out2"):
            t[k] = torch.empty(Bt, N, C, device="cuda")
        for k in ("dqkv", "dqkv2"):
            t[k] = torch.empty(Bt, N, 3 * C, device="cuda")
        for k in ("lse", "lse2", "ws"):
            t[k] = torch.empty(Bt, heads, N, device="cuda")
        return {k: v.data_ptr() for k, v in t.items()}, t

    def ragged(p, N):
        assert L.tcx_attention_ragged_bwd_workspace(Bt, N, C, heads) == Bt * heads * N * 4
        fwd = lambda: check(L.tcx_attention_ragged_fwd_lse(p["qkv"], p["out"], p["lse"], Bt, N, C, heads, st))
        bwd = lambda: check(L.tcx_attention_ragged_bwd(p["qkv"], p["out"], p["dout"], p["lse"], p["dqkv"], Bt, N, C, heads,
                                                       p["ws"], Bt * heads * N * 4, st))
        return fwd, bwd

    p, keep = bufs(576)
    fwd, bwd = ragged(p, 576)
    d = C // heads
    # algorithmic products of 2 N^2 d flop each: 2 forward (S, PV), 5 backward (S, dP, dQ, dK, dV; the kernels
    # execute 7, S and dP once per launch)
    flop = 2.0 * Bt * heads * 576 * 576 * d
    for name, fn, k in (("fwd_lse", fwd, 2), ("bwd (dq + dkv)", bwd, 5)):
        ts = [timed(fn) for _ in range(3)]
        print(f"ragged N=576 {name}: {' '.join(f'{t:.1f}' for t in ts)} us  ({k * flop / min(ts) / 1e6:.1f} TFLOP/s algorithmic)")
    if os.environ.get("PART") == "kernels":
        return

    p, keep = bufs(512)
    fwd, bwd = ragged(p, 512)
    ffwd = lambda: check(L.tcx_attention_fwd_lse(p["qkv"], p["out2"], p["lse2"], Bt, 512, C, heads, st))
    fbwd = lambda: check(L.tcx_attention_bwd(p["qkv"], p["out2"], p["dout"], p["lse2"], p["dqkv2"], Bt, 512, C, heads,
                                             p["ws"], Bt * heads * 512 * 4, st))
    for _ in range(4):
        a, b, c, e = timed(fwd), timed(ffwd), timed(bwd), timed(fbwd)
        print(f"N=512 pair: fwd ragged {a:.1f} us, flash {b:.1f} us ({a / b:.3f});  bwd ragged {c:.1f} us, "
              f"tcx_attention_bwd {e:.1f} us ({c / e:.3f});  fwd + bwd {(a + c) / (b + e):.3f}")
    print(f"N=512 max |ragged - fused| out {float((keep['out'] - keep['out2']).abs().max()):.3e}, "
          f"dqkv {float((keep['dqkv'] - keep['dqkv2']).abs().max()):.3e} (dqkv absmax {float(keep['dqkv2'].abs().max()):.3f})")
    del keep
    torch.cuda.empty_cache()

    for i in range(3):
        for v in ("1", "0"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step"], env=dict(os.environ, TCX_ATTN_FUSED=v),
                               capture_output=True, text=True, timeout=600)
            print(f"96x96 B=128 step pair {i + 1}: " + (r.stdout.strip().splitlines() or [r.stderr[-400:]])[-1], flush=True)


if __name__ == "__main__":
    step_child() if "--step" in sys.argv else main()
