#!/usr/bin/env python3
"""Timing of k_attention_split_ragged (csrc/attention_split_ragged.hip) at the base-96 bottleneck's shape, Bt = 256
rows (B = 128 with CFG), C = 192, 4 heads (d = 48):
  N = 576 (96x96): fmt 0 (h2) beside tcx_attention_ragged(out_h2 = 1), alternating pairs in this process;
  N = 512: fmt 0 and fmt 1 beside k_attention_split, the same arithmetic with no tails (information only);
  one evaluation of the base-96 net at 96x96, B = 128, CFG 1.5, one lane: f16x3 with the split route on and
  with TCX_ATTN_SPLIT=0 (fp32-MFMA attention), alternating pairs, and bf16 once.  The library reads its
  environment once, so every end-to-end figure comes from a fresh child process (`--eval PREC`).
µs per launch: HIP events around REPS back-to-back launches on the stream, after a warm-up."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-diffusion-toy-crystals_amd"))
import torch
from toycrystals_amd import _lib
from toycrystals_amd._lib import lib, check

L = lib()
st = torch.cuda.current_stream().cuda_stream
REPS = int(os.environ.get("REPS", "50"))
PAIRS = int(os.environ.get("PAIRS", "3"))
Bt, C, heads = 256, 192, 4


def timed(fn, reps=REPS):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def evaluation(prec):
    """ms per evaluation of the base-96 net at 96x96, B = 128, CFG: three windows of five"""
    from toycrystals_amd.models.sde_score_model import CondUNetTiny, predict_eps_cfg
    torch.manual_seed(0)
    m = CondUNetTiny(4, 4, 96).cuda().eval()
    B = 128
    x = torch.randn(B, 1, 96, 96, device="cuda")
    t = torch.full((B,), 0.42, device="cuda")
    y_cat = (torch.arange(B) % 4).cuda()
    y_cont = torch.rand(B, 4, device="cuda")
    _lib.set_conv_precision(prec)
    ts = [timed(lambda: predict_eps_cfg(m, x, t, y_cat, y_cont, 1.5), 5) / 1e3 for _ in range(3)]
    assert _lib.used_conv_precision() == prec, _lib.used_conv_precision()
    print(f"EVAL {prec} {min(ts):.3f} ms (windows {' '.join(f'{v:.2f}' for v in ts)})", flush=True)


def child(prec, **env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--eval", prec], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [s for s in r.stdout.splitlines() if s.startswith("EVAL")][-1]
    return float(line.split()[2]), line


def records(qkv, bf):
    """[Bt, N, 3C] fp32 -> h2 records (the library's writers), or bf16 records"""
    out = torch.empty_like(qkv)
    if bf:
        one, zero = torch.ones(Bt, 3 * C, device="cuda"), torch.zeros(Bt, 3 * C, device="cuda")
        check(L.tcx_gn_apply_tab_bf16(qkv.data_ptr(), out.data_ptr(), Bt, qkv.shape[1], 3 * C, one.data_ptr(),
                                      zero.data_ptr(), 0, st))
    else:
        check(L.tcx_f32_to_h2(qkv.data_ptr(), out.data_ptr(), qkv.numel(), None, st))
    return out


def main():
    g = torch.Generator(device="cuda").manual_seed(576)
    qkv = torch.randn(Bt, 576, 3 * C, device="cuda", generator=g)
    qh = records(qkv, False)
    o_new, o_old = torch.empty(Bt, 576, C, device="cuda"), torch.empty(Bt, 576, C, device="cuda")
    new = lambda: check(L.tcx_attention_split_ragged(qh.data_ptr(), o_new.data_ptr(), 0, Bt, 576, C, heads, st))
    old = lambda: check(L.tcx_attention_ragged(qkv.data_ptr(), o_old.data_ptr(), 1, Bt, 576, C, heads, None, st))
    flop = 4.0 * Bt * heads * 576 * 576 * (C // heads)
    for _ in range(PAIRS):
        a, b = timed(new), timed(old)
        print(f"N=576 pair: split_ragged fmt 0 {a:.1f} us ({flop / a / 1e6:.1f} TFLOP/s algorithmic), "
              f"ragged fp32 -> h2 {b:.1f} us, new / old {a / b:.3f}")
    def back(t):   # h2 records -> fp32
        f = torch.empty_like(t)
        check(L.tcx_h2_to_f32(t.data_ptr(), f.data_ptr(), t.numel(), st))
        return f
    print(f"N=576 max |split_ragged - ragged| {float((back(o_new) - back(o_old)).abs().max()):.3e}")
    qb = records(qkv, True)
    nb = lambda: check(L.tcx_attention_split_ragged(qb.data_ptr(), o_new.data_ptr(), 1, Bt, 576, C, heads, st))
    print(f"N=576 split_ragged fmt 1 (bf16 records): {' '.join(f'{timed(nb):.1f}' for _ in range(3))} us")

    qkv = torch.randn(Bt, 512, 3 * C, device="cuda", generator=g)
    o_new, o_old = torch.empty(Bt, 512, C, device="cuda"), torch.empty(Bt, 512, C, device="cuda")
    for fmt, ref in ((0, L.tcx_attention_split), (1, L.tcx_attention_split_bf16)):
        q = records(qkv, bool(fmt))
        new = lambda: check(L.tcx_attention_split_ragged(q.data_ptr(), o_new.data_ptr(), fmt, Bt, 512, C, heads, st))
        old = lambda: check(ref(q.data_ptr(), o_old.data_ptr(), Bt, 512, C, heads, st))
        for _ in range(PAIRS):
            a, b = timed(new), timed(old)
            print(f"N=512 fmt {fmt} pair: split_ragged {a:.1f} us, k_attention_split {b:.1f} us, ratio {a / b:.3f}")

    for i in range(PAIRS):
        (a, la), (b, lb) = child("f16x3"), child("f16x3", TCX_ATTN_SPLIT="0")
        print(f"96x96 f16x3 pair {i}: split route {a:.3f} ms, TCX_ATTN_SPLIT=0 {b:.3f} ms, ratio {a / b:.4f}")
    print("96x96 bf16: " + child("bf16")[1])


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--eval":
        evaluation(sys.argv[2])
    else:
        main()
