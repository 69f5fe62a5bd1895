#!/usr/bin/env python3
"""Timing of k_attention_ragged (csrc/attention_ragged.hip) at the base-96 bottleneck's shape, Bt = 256 rows
(B = 128 with CFG), C = 192, 4 heads (d = 48):
  N = 576 (96x96): its own time, fp32 and h2 output;
  N = 512: alternating A/B pairs beside k_attention_flash (tcx_attention), the only size both serve;
  one evaluation of the base-96 net at 96x96, B = 128, CFG 1.5, one lane, per precision.
µs per launch: HIP events around REPS back-to-back launches on the stream, after a warm-up."""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-diffusion-toy-crystals_amd"))
import torch
from toycrystals_amd import _lib
from toycrystals_amd._lib import lib, check

L = lib()
st = torch.cuda.current_stream().cuda_stream
REPS = int(os.environ.get("REPS", "50"))
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


def bufs(N):
    g = torch.Generator(device="cuda").manual_seed(N)
    return torch.randn(Bt, N, 3 * C, device="cuda", generator=g), torch.empty(Bt, N, C, device="cuda")


def ragged(qkv, out, N, h2=0):
    return lambda: check(L.tcx_attention_ragged(qkv.data_ptr(), out.data_ptr(), h2, Bt, N, C, heads, None, st))


qkv, out = bufs(576)
flop = 4.0 * Bt * heads * 576 * 576 * (C // heads)
t576 = {}
for h2 in (0, 1):
    ts = [timed(ragged(qkv, out, 576, h2)) for _ in range(3)]
    print(f"ragged N=576 out_h2={h2}: {' '.join(f'{t:.1f}' for t in ts)} us  ({flop / min(ts) / 1e6:.1f} TFLOP/s algorithmic)")
    t576[h2] = min(ts)

qkv, out = bufs(512)
out2 = torch.empty_like(out)
flash = lambda: check(L.tcx_attention(qkv.data_ptr(), out2.data_ptr(), Bt, 512, C, heads, st))
pairs = [(timed(ragged(qkv, out, 512)), timed(flash)) for _ in range(4)]
for a, b in pairs:
    print(f"N=512 pair: ragged {a:.1f} us, flash {b:.1f} us, ragged / flash {a / b:.3f}")
print(f"N=512 max |ragged - flash| {float((out - out2).abs().max()):.3e} (output absmax {float(out2.abs().max()):.3f})")

from toycrystals_amd.models.sde_score_model import CondUNetTiny, predict_eps_cfg
torch.manual_seed(0)
m = CondUNetTiny(4, 4, 96).cuda().eval()
B = 128
x = torch.randn(B, 1, 96, 96, device="cuda")
t = torch.full((B,), 0.42, device="cuda")
y_cat = (torch.arange(B) % 4).cuda()
y_cont = torch.rand(B, 4, device="cuda")
for prec in ("f16x3", "fp32"):
    _lib.set_conv_precision(prec)
    ts = [timed(lambda: predict_eps_cfg(m, x, t, y_cat, y_cont, 1.5), 5) for _ in range(3)]
    print(f"base-96 evaluation at 96x96, B=128, CFG, {prec}: {' '.join(f'{v / 1e3:.2f}' for v in ts)} ms; "
          f"attention (N=576 above) {100 * t576[prec == 'f16x3'] / min(ts):.1f} % of it")
