"""The f16x3 arithmetic contract (tests/f16x3_ref.py) INSIDE the adaptive Dormand-Prince solve, on the CPU: what csrc/ode_dp5_f16x3w.hip
is allowed to differ from f64 by, without a GPU.

The 32-bit frame problem of test_cnf_dopri5 runs its two hidden layers on f16x3_ref.linear (test_cnf_solve_kernels.F patched as
test_f16x3_emulation._PatchedF patches the oracle's).  Its FREE run stands in for the kernel: the attempts it chooses and the decisions
it takes are replayed in f64 (test_cnf_dopri5.replay), and the checks are those of the GPU test:

  * state within X_TOL max(1, |x|max) of the replay (X_TOL = 1e-5: the suite's number for the bf16x6 kernel, unchanged);
  * every accepted attempt has s64 <= 1 + delta, every rejected one s64 >= 1 - delta, s64 = sqrt(ratio) of the f64 replay, with
    delta = 4 x the larger of the worst |s_f16x3 - s64| and the worst |s_f32 - s64| over the same attempts;
  * attempts that decide nothing (s64 inside 1 +- delta) are at most 10 % of all attempts.

Control: the same run on the FIRST f16 product alone (2^-12 relative per product) must miss the state bound on the stress weights, so
that the test is able to fail.

Measured with exactly these inputs: 103 attempts, none undecided, the nearest s64 to 1 at 1.021; worst |s_f16x3 - s64| 1.96e-4 (plain
f32: 6.1e-5); worst state error 3.1e-5 against a bound of 8.7e-5, on the seeded weights at most 6.4e-7; 62-74 evaluations per stress
frame in reverse, 20 per seeded frame."""
import math

import pytest
import torch

import test_cnf_solve_kernels as K
from test_cnf_solve_kernels import base_samples, rnd
from test_cnf_dopri5 import X_TOL, CpuWeights, check_decisions, frame_problem, measure_delta, replay
from test_cnf_dopri5_f16x3 import PatchedF

BT, TOL = 2, 1e-5
RUNS = ((128, True), (129, True), (257, True), (200, False))        # (n, reverse)


def emulate(W, monkeypatch, first_only=False):
    """Every frame of RUNS -> (bad, stats, figures): the checks above on the free run of the patched 32-bit problem."""
    bad, stats = [], dict(attempts=0, undecided=0)
    fig = dict(worst_h3=0.0, worst_f32=0.0, worst_state=0.0, worst_state_over_bound=0.0, nearest=float("inf"), nfe=[])
    for n, reverse in RUNS:
        c, y = rnd(2000 + n, BT, 1600, scale=0.5), base_samples(2001 + n, BT, n)
        hyper = W.hyper(c)
        t0, t1 = (W.t_end, 0.0) if reverse else (0.0, W.t_end)
        for b in range(BT):
            p64 = frame_problem(W, y, hyper, b, reverse, None, None, None)
            p32 = frame_problem(W, y, hyper, b, reverse, None, None, None, torch.float32)
            with monkeypatch.context() as m:
                m.setattr(K, "F", PatchedF(first_only))
                free = replay(*p32, t0, t1, TOL, TOL)
                wh3, s64s, r64 = measure_delta(p32, p64, t0, t1, TOL, TOL, free["dts"], free["accepted"])
            w32, _, _ = measure_delta(p32, p64, t0, t1, TOL, TOL, free["dts"], free["accepted"])
            tag = "n%d %s frame %d" % (n, "rev" if reverse else "fwd", b)
            check_decisions(tag, r64, dict(accepted=free["accepted"]), 4 * max(wh3, w32), bad, stats, controller_too=False)
            err = float((free["out"][0].double() - r64["out"][0]).abs().max())
            bound = X_TOL * max(1.0, float(r64["out"][0].abs().max()))
            if not err <= bound:
                bad.append("%s: state %.3e from the f64 replay, bound %.3e" % (tag, err, bound))
            fig["worst_h3"], fig["worst_f32"] = max(fig["worst_h3"], wh3), max(fig["worst_f32"], w32)
            fig["worst_state_over_bound"] = max(fig["worst_state_over_bound"], err / bound)
            fig["worst_state"] = max(fig["worst_state"], err)
            fig["nearest"] = min([fig["nearest"]] + s64s, key=lambda s: abs(s - 1.0))
            fig["nfe"].append(free["nfe"])
    return bad, stats, fig


@pytest.fixture(scope="module")
def cpu_weights(seeded_sd, stress_sd):
    return {"seeded": CpuWeights(seeded_sd), "stress": CpuWeights(stress_sd)}


@pytest.mark.parametrize("which", ["seeded", "stress"])
def test_f16x3_free_run_against_its_f64_replay(which, cpu_weights, monkeypatch):
    bad, stats, fig = emulate(cpu_weights[which], monkeypatch)
    print("%s: %d attempts, %d undecided, nearest s64 %.4f, worst |s_f16x3 - s64| %.3e, |s_f32 - s64| %.3e, state %.3e (%.0f %% of its bound), nfe %s"
          % (which, stats["attempts"], stats["undecided"], fig["nearest"], fig["worst_h3"], fig["worst_f32"], fig["worst_state"],
             100 * fig["worst_state_over_bound"], fig["nfe"]))
    assert stats["attempts"] >= 3 * len(RUNS) * BT
    assert stats["undecided"] <= 0.1 * stats["attempts"], "attempts that decide nothing: %d of %d" % (stats["undecided"], stats["attempts"])
    assert not bad, "\n".join(bad)


def test_first_product_alone_misses_the_state_bound(cpu_weights, monkeypatch):
    """The control: one f16 plane per operand on the stress weights is outside X_TOL of its own f64 replay."""
    bad, _, fig = emulate(cpu_weights["stress"], monkeypatch, first_only=True)
    print("first product only: worst state %.3e = %.1f x its bound" % (fig["worst_state"], fig["worst_state_over_bound"]))
    assert any("state" in b for b in bad), "the first-product-only run passes the state bound: the bound cannot fail"
    assert math.isfinite(fig["worst_state"])
