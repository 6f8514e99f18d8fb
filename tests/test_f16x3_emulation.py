"""The f16x3 arithmetic contract (tests/f16x3_ref.py) inside the point-CNF solve, on the CPU: oracle.model.odenet with its two
512 x 512 hidden layers multiplied on three f16 products, against the same solve in f64.

Bound: 5e-6 on the sampled state -- half the suite's flat 1e-5, the share the bf16x6 kernels are held to against the f32-MFMA image
(test_cnf_solve_kernels.IMG_TOL).  The first-product-only control (one f16 plane per operand: 2^-12 relative per product) must miss
the full 1e-5, so that the test is able to fail."""
import pytest
import torch
import torch.nn.functional as F

import f16x3_ref
from oracle import model as O

BOUND, CONTROL_FLOOR = 5e-6, 1e-5
FRAMES, POINTS, STEPS = 10, 64, 8


class _PatchedF:
    """torch.nn.functional with linear() on (512, 512) weights replaced; everything else passes through."""

    def __init__(self, first_only):
        self.first_only = first_only

    def __getattr__(self, name):
        return getattr(F, name)

    def linear(self, x, w, b=None):
        if tuple(w.shape) == (512, 512) and x.dtype == torch.float32:
            return f16x3_ref.linear(x, w, b, first_only=self.first_only)
        return F.linear(x, w, b)


def _solve(sd, y, c):
    return O.point_cnf(sd, y, c, None, True, "rk4", STEPS)


@pytest.fixture(scope="module")
def inputs():
    g = torch.Generator().manual_seed(7)
    return torch.randn(FRAMES, POINTS, 3, generator=g), torch.randn(FRAMES, 1600, generator=g)


def test_split_is_exact_to_two_planes_and_flushes_subnormals():
    x = torch.tensor([1.0, 3.14159274, 1e-3, 65000.0, 2.0 ** -14, 2.0 ** -15, 1.5 * 2.0 ** -14 + 2.0 ** -26, -7.123456e2, 0.0])
    p1, p2 = f16x3_ref.split(x)
    for p in (p1, p2):
        assert bool((p.half().float() == p).all())                                   # f16 values
        assert bool(((p == 0) | (p.abs() >= f16x3_ref.F16_MIN_NORMAL)).all())        # no subnormal survives
    big = x.abs() >= 2.0 ** -3          # both planes normal from here: the split is good to 2^-22 relative
    assert bool(((x - p1 - p2).abs()[big] <= x.abs()[big] * 2.0 ** -22).all())
    assert float(p1[5]) == 0.0 and float(p2[5]) == 0.0                               # 2^-15: flushed in both planes


def test_weight_shift_puts_the_maximum_below_f16_max():
    for m in (1.0, 0.999, 0.03, 2.0 ** 9, 2.0 ** 15 - 1, 1e-20):
        s = f16x3_ref.weight_shift(torch.tensor([m, -m / 3]))
        assert 2.0 ** 14 <= m * 2.0 ** s < 2.0 ** 15, (m, s)
    assert f16x3_ref.weight_shift(torch.zeros(4)) == 0


def test_weight_shift_is_clamped_so_the_unscale_factor_stays_normal():
    """max |w| below 2^-86: the shift stops at MAX_SHIFT, 2^-(4 + s) is a normal f32 number, and the layer's (negligible) product is
    still the product, not zero times a flushed factor; an f32-subnormal maximum takes shift 0."""
    assert f16x3_ref.weight_shift(torch.tensor([2.0 ** -86])) == f16x3_ref.MAX_SHIFT == 100
    assert f16x3_ref.weight_shift(torch.tensor([2.0 ** -87])) == 100
    assert f16x3_ref.weight_shift(torch.tensor([2.0 ** -120])) == 100
    assert f16x3_ref.weight_shift(torch.tensor([2.0 ** -130])) == 0
    assert float(torch.tensor(2.0 ** -(f16x3_ref.ACT_SHIFT + f16x3_ref.MAX_SHIFT), dtype=torch.float32)) >= 2.0 ** -126
    w = torch.full((4, 8), 2.0 ** -90)
    out = f16x3_ref.linear(torch.ones(2, 8), w)
    assert bool((out == 8 * 2.0 ** -90).all())


@pytest.mark.parametrize("which", ["seeded", "stress"])
def test_three_f16_products_solve_matches_f64(which, seeded_sd, stress_sd, inputs, monkeypatch):
    sd = seeded_sd if which == "seeded" else stress_sd
    y, c = inputs
    want = _solve({k: v.double() for k, v in sd.items()}, y.double(), c.double())
    monkeypatch.setattr(O, "F", _PatchedF(first_only=False))
    got = _solve(sd, y, c)
    monkeypatch.setattr(O, "F", _PatchedF(first_only=True))
    control = _solve(sd, y, c)
    err, cerr = float((got.double() - want).abs().max()), float((control.double() - want).abs().max())
    print("f16x3 emulation, %s weights, S = %d: max |x - x_f64| = %.3e (bound %.1e), first product only %.3e" % (which, STEPS, err, BOUND, cerr))
    assert err <= BOUND, err
    assert cerr > CONTROL_FLOOR, cerr
