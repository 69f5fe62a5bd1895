#!/usr/bin/env python3
"""The DPM-Solver++(2M) fixture tests/golden/dpmpp96_trained_20.npz: the float64 restatement
(tests/dpmpp_ref.py over oracle/score_model_torch.py in float64) on the trained base-96 model
(trained96_ema.npz) with the settings of ode96_trained_50.npz (its conditions, x_T seed, CFG 1.5,
t_end 0.005, beta 0.1 - 30), B = 4, 20 steps, order 2, lower-order final step.  There is no reference
implementation of this sampler to record, so the fixture is the float64 solution of the stated
update; it reads nothing outside this repository.  About a minute on 8 cores.

    python tests/golden/make_dpmpp_golden.py      # writes tests/golden/dpmpp96_trained_20.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vae-diffusion-toy-crystals_amd"), os.path.join(ROOT, "tests")]

import dpmpp_ref as R  # noqa: E402

STEPS, ORDER, LOWER_ORDER_FINAL = 20, 2, True


def main():
    torch.set_num_threads(8)
    g = dict(np.load(os.path.join(HERE, "ode96_trained_50.npz")))
    sd = dict(np.load(os.path.join(HERE, "trained96_ema.npz")))
    B = int(g["B"])
    beta_min, beta_max, cfg, t_end = float(g["beta_min"]), float(g["beta_max"]), float(g["cfg"]), float(g["t_end"])
    torch.manual_seed(int(g["noise_seed"]))
    x_T = torch.randn((B, 1, 64, 64)).numpy()  # the x_T of ode96_trained_50 (tests/test_gpu_models.py)
    eps = R.torch_eps(sd, g["y_cat"], g["y_cont"], cfg, torch.float64)
    x0 = R.sample(eps, x_T, R.grid(STEPS, t_end), beta_min, beta_max, ORDER, LOWER_ORDER_FINAL)
    out = R.to_image(x0)
    unsat = float(np.mean((out > 0.0) & (out < 1.0)))
    print(f"|x0_hat|max {np.abs(x0).max():.4g}, unsaturated {100 * unsat:.1f} %")
    np.savez_compressed(os.path.join(HERE, "dpmpp96_trained_20.npz"), y_cat=g["y_cat"], y_cont=g["y_cont"],
                        out=out.astype(np.float32), x0_unclamped=x0.astype(np.float32), steps=np.int64(STEPS),
                        order=np.int64(ORDER), lower_order_final=np.int64(LOWER_ORDER_FINAL), cfg=np.float64(cfg),
                        t_end=np.float64(t_end), beta_min=np.float64(beta_min), beta_max=np.float64(beta_max),
                        base_ch=np.int64(96), noise_seed=g["noise_seed"], B=np.int64(B))


if __name__ == "__main__":
    main()
