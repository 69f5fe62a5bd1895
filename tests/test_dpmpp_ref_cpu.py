"""CPU: the DPM-Solver++(2M) reference (tests/dpmpp_ref.py), the coefficient table of the package
(dpmpp_table) and what the GPU parity gates of tests/test_gpu_dpmpp.py can and cannot see.

Gates: 1e-4 max-abs on the clamped image, 1e-4 relative to max(1, |x0_hat|max) on x0_hat.

For every GPU parity case an fp32 evaluation of the trajectory (fp32 network, fp32 table, fp32 update)
must sit at <= 0.5 of both gates against the float64 reference, so the device has room for its own
summation order.  Measured here: <= 0.007 of the x0_hat gate on the untrained cases, whose pixels are all
saturated (dpmpp_ref.X_T_SEEDS: image error 0).  The trained fixture, which is set and not picked, sits
at 0.44 / 0.50 and is held to the gates themselves.

Mutants (dpmpp_ref.MUTANTS) against the same gates.  A mutant that changes no arithmetic of a case
(dpmpp_ref.mutant_is_live: n_steps = 0 has no step at all, order 1 has no history term, ...) IS the
right solver there and must reproduce the reference bit for bit.  Where it is live:
  * history_sign, sigma_next_in_x0 and second_order_step0 change a data prediction by its own size
    (a flipped sign, sigma_{i+1} / sigma_i - 1 of the eps term, 1.5x the first prediction): they must
    fail the gates in EVERY case where they are live;
  * r_inverted, history_stale and no_lower_order_final change the update by a multiple of
    x0_i - x0_{i-1} that vanishes with |r - 1/r| or with h: on the untrained cases, whose |x0_hat|max
    of ~8e3 (1/alpha(1) = 2e3) makes the relative gate ~0.8 absolute, r_inverted falls to 0.75 of the
    gate (n = 2) and no_lower_order_final stays at 0.2 - 0.7 of it (printed): not all can be seen.
    They must fail on the trained fixture, the trajectory the sampler is for (measured: >= 13x).
Every mutant is thereby failed by at least one GPU parity case.
"""
import os

import numpy as np
import pytest
import torch

import dpmpp_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GATE = 1e-4
ALWAYS_VISIBLE = ("history_sign", "sigma_next_in_x0", "second_order_step0")


def gate_ratios(x0, ref):
    """(x0_hat gate, image gate) as fractions of the 1e-4 gates."""
    return R.rel_err(x0, ref) / GATE, float(np.abs(R.to_image(x0) - R.to_image(ref)).max()) / GATE


# ---------------------------------------------------------------- the table

@pytest.mark.parametrize("n", [0, 1, 2, 3, 5, 20, 50])
@pytest.mark.parametrize("order,lof", [(2, True), (2, False), (1, True)])
def test_dpmpp_table_equals_float64_coefficients(n, order, lof):
    """dpmpp_table is the float64 coefficients of the fp32 grid rounded once: equal to the reference's to fp32
    rounding (1 ulp: torch's and numpy's float64 exp / expm1 / log may differ in the last float64 bit, which
    moves an fp32 rounding only on a tie), on the grid the step table carries."""
    from toycrystals_amd.models.sde_score_model import VPSDE, dpmpp_table, step_table
    sde = VPSDE(R.BETA_MIN, R.BETA_MAX)
    tab = dpmpp_table(sde, n, R.T_END, order, lof).numpy()
    ts = R.grid(n, R.T_END)
    assert np.array_equal(step_table(sde, n, R.T_END)[:, 0].numpy(), ts)
    ref = R.coefficients(ts, R.BETA_MIN, R.BETA_MAX, order, lof)
    assert tab.shape == (n, R.N_COEF) and tab.dtype == np.float32
    ref32 = ref.astype(np.float32)
    assert np.all(np.abs(tab - ref32) <= np.spacing(np.abs(ref32)))
    for i in range(n):
        first = R.is_first_order(i, n, order, lof)
        assert (tab[i, 4] == 1.0 and tab[i, 5] == 0.0) == first
        assert np.isclose(float(tab[i, 4]) + float(tab[i, 5]), 1.0, atol=2e-7)  # D is an affine combination


def test_dpmpp_table_refuses_other_orders():
    from toycrystals_amd.models.sde_score_model import VPSDE, dpmpp_table
    for order in (0, 3):
        with pytest.raises(ValueError, match="order"):
            dpmpp_table(VPSDE(), 4, 1e-3, order=order)
        with pytest.raises(ValueError, match="order"):
            R.coefficients(R.grid(4, 1e-3), 0.1, 20.0, order=order)


def test_first_step_coefficients_in_closed_form():
    """Independent of expm1 / lambda bookkeeping: -alpha_1 expm1(-h_0) = alpha_1 - (sigma_1 / sigma_0) alpha_0,
    the DDIM identity of a first-order data-prediction step."""
    ts = R.grid(5, R.T_END)
    c = R.coefficients(ts, R.BETA_MIN, R.BETA_MAX)
    alpha, sigma, _ = R.schedule(ts, R.BETA_MIN, R.BETA_MAX)
    assert np.allclose(c[:, 3], alpha[1:] - (sigma[1:] / sigma[:-1]) * alpha[:-1], rtol=1e-12, atol=0)
    assert np.allclose(alpha ** 2 + sigma ** 2, 1.0, rtol=0, atol=1e-15)


# ---------------------------------------------------------------- the solver on a small net

def _small_case(n, order=2, lof=True, g=1.5):
    return (16, 3, 16, 16, g, n, order, lof)


def test_single_step_equals_closed_form():
    for order, lof in ((2, True), (2, False), (1, True)):
        c = _small_case(1, order, lof)
        sd, y_cat, y_cont, x_T, ts = R.case_setup(c)
        eps = R.torch_eps(sd, y_cat, y_cont, c[4], torch.float64)
        want = R.closed_form_single_step(eps, x_T, ts, R.BETA_MIN, R.BETA_MAX)
        assert R.rel_err(R.case_reference(c), want) < 1e-13


@pytest.mark.parametrize("n", [2, 3, 5])
def test_order1_equals_first_order_formula(n):
    c = _small_case(n, order=1)
    sd, y_cat, y_cont, x_T, ts = R.case_setup(c)
    eps = R.torch_eps(sd, y_cat, y_cont, c[4], torch.float64)
    want = R.first_order_every_step(eps, x_T, ts, R.BETA_MIN, R.BETA_MAX)
    assert R.rel_err(R.case_reference(c), want) < 1e-13
    assert np.array_equal(R.case_reference(c), R.case_reference(_small_case(n, order=1, lof=False)))
    assert not np.array_equal(R.case_reference(_small_case(n, order=2, lof=False)), want)  # the history term acts


def test_numpy_and_torch_networks_agree():
    """The reference takes either restatement of the network: the numpy oracle and the torch one give the
    same float64 trajectory (3 steps, the first second-order step) up to the timestep embedding, which the
    torch restatement evaluates in fp32 before its float64 layers (a 6e-8 relative change of their input)."""
    c = _small_case(3)
    sd, y_cat, y_cont, x_T, ts = R.case_setup(c)
    x0 = R.sample(R.numpy_eps(sd, y_cat, y_cont, c[4], np.float64), x_T, ts, R.BETA_MIN, R.BETA_MAX, c[6], c[7])
    assert R.rel_err(x0, R.case_reference(c)) < 1e-6


# ---------------------------------------------------------------- every GPU parity case

@pytest.mark.parametrize("case", R.PARITY_CASES, ids=R.case_id)
def test_parity_case_fp32_headroom_and_mutants(case):
    base, B, H, W, g, n, order, lof = case
    sd, y_cat, y_cont, x_T, ts = R.case_setup(case)
    ref = R.case_reference(case)
    x32 = R.sample_fp32(R.torch_eps(sd, y_cat, y_cont, g, torch.float32), x_T, ts, R.BETA_MIN, R.BETA_MAX, order, lof)
    rx, ri = gate_ratios(x32, ref)
    out = R.to_image(ref)
    print(f"{R.case_id(case)}: fp32 vs float64 at {rx:.4f} (x0_hat) / {ri:.4f} (image) of the gates; |x0|max "
          f"{np.abs(ref).max():.4g}, unsaturated {100 * np.mean((out > 0) & (out < 1)):.1f} %")
    assert x32.dtype == np.float32
    assert rx <= 0.5 and ri <= 0.5
    eps64 = R.torch_eps(sd, y_cat, y_cont, g, torch.float64)
    for mut in R.MUTANTS:
        if n == 0 and mut != R.MUTANTS[0]:
            continue  # no step: every mutant is the projection alone (one of them shows it)
        xm = R.sample(eps64, x_T, ts, R.BETA_MIN, R.BETA_MAX, order, lof, mutant=mut)
        if not R.mutant_is_live(mut, n, order, lof):
            assert np.array_equal(xm, ref), mut
            continue
        mx, mi = gate_ratios(xm, ref)
        print(f"  {mut}: {mx:.3g} (x0_hat) / {mi:.3g} (image) of the gates")
        assert not np.array_equal(xm, ref), mut
        if mut in ALWAYS_VISIBLE:
            assert max(mx, mi) > 1.0, mut


def test_every_mutant_is_live_in_a_parity_case():
    for mut in R.MUTANTS:
        assert any(R.mutant_is_live(mut, c[5], c[6], c[7]) for c in R.PARITY_CASES), mut
    assert not any(R.mutant_is_live(mut, 0, 2, True) for mut in R.MUTANTS)


def test_trained_fixture_fp32_headroom_and_every_mutant_fails():
    """The trained fixture (20 steps, order 2, lower-order final step: every mutant is live).  The fp32
    evaluation and the mutants run in fp32 on the fixture's first two images against the stored float64
    solution.  This case is set, not picked: the fp32 evaluation must hold the gates themselves.  Measured
    0.44 (x0_hat) / 0.50 (image) of the gates, of which the fp32 network alone gives 0.37 / 0.42 and the fp32
    update alone 0.15 / 0.18 (float64 network); the weakest mutant, no_lower_order_final, is at 13x the gate."""
    g = dict(np.load(os.path.join(GOLDEN, "dpmpp96_trained_20.npz")))
    sd = dict(np.load(os.path.join(GOLDEN, "trained96_ema.npz")))
    n, order, lof = int(g["steps"]), int(g["order"]), bool(g["lower_order_final"])
    assert all(R.mutant_is_live(m, n, order, lof) for m in R.MUTANTS)
    torch.manual_seed(int(g["noise_seed"]))
    rows = slice(0, 2)
    x_T = torch.randn((int(g["B"]), 1, 64, 64)).numpy()[rows]
    ref = g["x0_unclamped"][rows].astype(np.float64)
    assert np.abs(R.to_image(ref) - g["out"][rows]).max() < 1e-7
    ts = R.grid(n, float(g["t_end"]))
    eps = R.torch_eps(sd, g["y_cat"][rows], g["y_cont"][rows], float(g["cfg"]), torch.float32)
    beta = (float(g["beta_min"]), float(g["beta_max"]))
    rx, ri = gate_ratios(R.sample_fp32(eps, x_T, ts, *beta, order, lof), ref)
    print(f"dpmpp96_trained_20: fp32 vs float64 at {rx:.3f} (x0_hat) / {ri:.3f} (image) of the gates")
    assert rx < 1.0 and ri < 1.0
    for mut in R.MUTANTS:
        mx, mi = gate_ratios(R.sample_fp32(eps, x_T, ts, *beta, order, lof, mutant=mut), ref)
        print(f"  {mut}: {mx:.3g} (x0_hat) / {mi:.3g} (image) of the gates")
        assert max(mx, mi) > 1.0, mut
