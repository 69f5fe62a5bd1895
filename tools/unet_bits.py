#!/usr/bin/env python3
"""Fingerprint of the U-Net evaluator and the samplers: for a fixed list of small cases, one line per run with
the case name, the return code and the SHA-256 of the output bytes (on a non-zero code: tcx_last_error()
instead).  The package is imported from the tree the script lies in, so the same script run in two trees
compares two builds of libtcx: equal files mean bit-identical results and identical refusals.

    python tools/unet_bits.py [OUT]      (OUT: also write the lines there)

The cases are the smallest shapes that reach each branch of the first-conv and head dispatches and each
tensor format; weights are CondUNetTiny's random init at seed 0, inputs are seeded."""
import hashlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vae-diffusion-toy-crystals_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from toycrystals_amd import _lib  # noqa: E402
from toycrystals_amd.models.sde_score_model import (CondUNetTiny, VPSDE, predict_eps_cfg,  # noqa: E402
                                                    sample_probability_flow_ode, sample_reverse_sde_euler_maruyama)

# (base_ch, H, W, precision, batches): what the shape reaches
CASES = [
    (8, 16, 16, "fp32", (3, 2)),     # first conv through tcx_conv2d, k_head
    (16, 16, 16, "fp32", (3, 2)),    # k_conv_first<0>, k_head
    (32, 32, 32, "f16x3", (3, 2)),   # k_conv_first_rec, k_head8r<1>
    (32, 32, 96, "f16x3", (3, 2)),   # k_conv_first<2> (LDS tile form), fp32-record attention
    (64, 32, 32, "f16x3", (3, 2)),   # k_head8r<2>
    (128, 32, 32, "f16x3", (3, 2)),  # k_head8<4>
    (96, 64, 64, "fp32", (3, 2)),    # k_conv_first_rec96, k_attn_block, chunk-major skips in f16x3;
    (96, 64, 64, "f16x3", (3, 2)),   # the same shape in fp32 and in bf16 records (fmt 1)
    (96, 64, 64, "bf16", (3, 2)),
    (96, 256, 256, "bf16", (1, 1)),  # fmt 2 (b2), FR_PX_WIDE, k_head8r<3, true>
]


def _line(name, fn):
    try:
        out = fn()
        torch.cuda.synchronize()
        return f"{name} 0 {hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()}"
    except _lib.TcxError as e:
        m = re.search(r"\(rc=(-?\d+)\): (.*)", str(e), re.S)
        return f"{name} {m.group(1)} {m.group(2)}" if m else f"{name} ? {e}"


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    dev = torch.device("cuda", 0)
    sde = VPSDE(0.1, 20.0)
    L = _lib.lib()
    lines = []
    for base, H, W, prec, batches in CASES:
        _lib.set_conv_precision(prec)
        torch.manual_seed(0)
        model = CondUNetTiny(4, 4, base).to(dev).eval()
        for B, guidance in zip(batches, (1.5, 0.0)):
            g = torch.Generator().manual_seed(1)
            x = torch.randn(B, 1, H, W, generator=g).to(dev)
            t = torch.linspace(0.2, 0.8, B).to(dev)
            y_cat = (torch.arange(B) % 4).to(dev)
            y_cont = torch.randn(B, 4, generator=g).to(dev)
            shape = (B, 1, H, W)
            name = f"c{base}_{H}x{W}_{prec}_B{B}_g{guidance}"
            runs = [("eval", 1, lambda: predict_eps_cfg(model, x, t, y_cat, y_cont, guidance))]
            for lanes in (1, 2):
                runs.append((f"sde3_L{lanes}", lanes, lambda: sample_reverse_sde_euler_maruyama(
                    model, sde, y_cat, y_cont, shape, n_steps=3, guidance_scale=guidance, t_end=0.005, seed=7)))
            for lanes in (1, 2):
                runs.append((f"ode2_L{lanes}", lanes, lambda: sample_probability_flow_ode(
                    model, sde, y_cat, y_cont, shape, n_steps=2, guidance_scale=guidance, t_end=0.005, seed=7)))
            runs.append(("sde3_x0hat", 1, lambda: sample_reverse_sde_euler_maruyama(
                model, sde, y_cat, y_cont, shape, n_steps=3, guidance_scale=guidance, t_end=0.005, seed=7,
                return_x0_hat=True)))
            for what, lanes, fn in runs:
                prev = L.tcx_set_sample_lanes(lanes)
                try:
                    with torch.no_grad():
                        lines.append(_line(f"{name}_{what}", fn))
                finally:
                    L.tcx_set_sample_lanes(prev)
                print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
