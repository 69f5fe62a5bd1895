#!/usr/bin/env python3
"""Convergence and cost of the score model's deterministic samplers on the MI355X: the Heun PF-ODE
(sample_probability_flow_ode, two U-Net evaluations per step) against DPM-Solver++(2M)
(sample_dpm_solver_pp, one per step) and its first-order form.

Error: the trained base-96 model (tests/golden/trained96_ema.npz) with the settings of
tests/golden/ode96_trained_50.npz (its conditions and x_T seed, CFG 1.5, t_end 0.005, beta 0.1 - 30),
B = 4; max-abs of x0_hat relative to max(1, |x0_hat|max) against a 400-step order-2 run of the same
sampler on the same device (the project's x0_hat metric).
Time: each configuration at B = 128, CFG 1.5, 4 sampling lanes, Philox x_T; one warm-up call, then the
median of REPS calls, host clock around a call that ends in a device synchronise.

usage (GPU box): python tools/dpmpp_convergence.py [--out profiles/dpmpp_convergence.txt] [--reps 3]
"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vae-diffusion-toy-crystals_amd")]
GOLDEN = os.path.join(ROOT, "tests", "golden")

from toycrystals_amd import _lib  # noqa: E402
from toycrystals_amd.models.sde_score_model import (CondUNetTiny, VPSDE, sample_dpm_solver_pp,  # noqa: E402
                                                    sample_probability_flow_ode)

# (label, sampler, steps, keywords)
CONFIGS = ([("Heun", sample_probability_flow_ode, n, {}) for n in (12, 25, 50)]
           + [("DPM-Solver++(2M)", sample_dpm_solver_pp, n, dict(order=2)) for n in (10, 20, 24, 30, 50)]
           + [("DPM-Solver++ order 1", sample_dpm_solver_pp, n, dict(order=1)) for n in (20, 50)])


def evaluations(fn, n):
    return 2 * n + 1 if fn is sample_probability_flow_ode else n + 1


def rel_err(a, ref):
    return float((a - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpmpp_convergence.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-steps", type=int, default=400)
    ap.add_argument("--time-batch", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: this tool measures on the MI355X only")
    g = dict(np.load(os.path.join(GOLDEN, "ode96_trained_50.npz")))
    torch.manual_seed(0)
    model = CondUNetTiny(4, 4, 96)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, "trained96_ema.npz")).items()})
    model = model.cuda().eval()
    sde = VPSDE(float(g["beta_min"]), float(g["beta_max"]))
    cfg, t_end, B = float(g["cfg"]), float(g["t_end"]), int(g["B"])
    torch.manual_seed(int(g["noise_seed"]))
    x_T = torch.randn((B, 1, 64, 64)).cuda()
    y_cat, y_cont = torch.from_numpy(g["y_cat"]).cuda(), torch.from_numpy(g["y_cont"]).cuda()

    def x0_hat(fn, n, kw):
        return fn(model, sde, y_cat, y_cont, (B, 1, 64, 64), n_steps=n, guidance_scale=cfg, t_end=t_end,
                  x_init=x_T.clone(), return_x0_hat=True, **kw)

    ref = x0_hat(sample_dpm_solver_pp, args.ref_steps, dict(order=2))
    errs = [rel_err(x0_hat(fn, n, kw), ref) for _, fn, n, kw in CONFIGS]
    precision = _lib.used_conv_precision()

    Bt = args.time_batch
    yc = (torch.arange(Bt) % 4).cuda()
    yv = torch.zeros(Bt, 4)
    yv[:, 1] = torch.linspace(0.0, math.pi / 3, Bt)
    yv = yv.cuda()

    def timed(fn, n, kw):
        t0 = time.perf_counter()
        fn(model, sde, yc, yv, (Bt, 1, 64, 64), n_steps=n, guidance_scale=cfg, t_end=t_end, seed=7, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    times = []
    prev = _lib.lib().tcx_set_sample_lanes(4)
    try:
        for _, fn, n, kw in CONFIGS:
            timed(fn, n, kw)  # warm-up: workspace growth, code objects
            times.append(statistics.median(timed(fn, n, kw) for _ in range(args.reps)))
    finally:
        _lib.lib().tcx_set_sample_lanes(prev)

    lines = [f"# tools/dpmpp_convergence.py on {torch.cuda.get_device_name(0)}, conv precision {precision}",
             f"# error: trained96_ema, settings of ode96_trained_50, B = {B}: x0_hat max-abs / max(1, |x0_hat|max) vs a "
             f"{args.ref_steps}-step order-2 DPM-Solver++ run",
             f"# time: B = {Bt}, CFG {cfg:g}, 4 lanes, median of {args.reps} calls after one warm-up",
             f"{'sampler (quadratic grid)':<24} {'steps':>5} {'U-Net evals':>11} {'error':>10} {'time s':>8} {'images/s':>9} "
             f"{'ms/eval':>8}"]
    for (label, fn, n, kw), e, t in zip(CONFIGS, errs, times):
        ev = evaluations(fn, n)
        lines.append(f"{label:<24} {n:>5} {ev:>11} {e:>10.4g} {t:>8.3f} {Bt / t:>9.1f} {1e3 * t / ev:>8.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
