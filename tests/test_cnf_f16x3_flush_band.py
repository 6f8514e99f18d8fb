"""The f16x3 point-CNF kernel (csrc/ode_f16x3w.hip) on launches whose hidden activations SIT IN THE FLUSH BAND, against the output
bits recorded from its parent: the kernel that flushed an f16-subnormal plane value by comparing the f32 value with 2^-14 - 2^-25 and
selecting 0 in front of the conversion.  The kernel now converts first and zeroes the halves of the plane word whose exponent field is
0 (f16x3_common.h: xh_flush_word); tests/test_f16x3_flush_word.py shows on the CPU that the two give the same words, this file that the
kernel still puts out the parent's bits where the flush matters -- the launches of test_cnf_f16x3_planes.py were not built to have
activations down there.

The hyper rows are edited (band(), below) so that, in both hidden layers that are split (layer 0's output in layer 1's producers, layer
1's output in pass 0 of layer 2):
  * units 0..63 have their gate shut (gate column -30: sigmoid 1e-13) and a bias that sweeps -17.2 .. -9.3 over the units, i.e.
    X = 16 softplus(x) from 2^-20 to 2^-10 through the threshold 2^-14, the same for every point and moving with the stage time;
    units 64..95 sweep the same range with the gate half open, so that X also varies from point to point;
  * units 96..159 get a bias of -5.6 .. -2.6 (gate untouched): X in 2^-4 .. 1, whose f16 remainder is of either sign and up to
    2^-12 in magnitude, i.e. on both sides of +-2^-14 (the second plane's flush);
  * in frame 1 every other unit of the two layers is dead (gate -30, bias -40: X = 0 exactly), so that the band's products are
    not rounded away under 400 ordinary ones; frame 0 keeps them.
Shapes: one workgroup (n = 128) and a second one with 96 invalid columns (n = 160), two frames, one and three RK4 steps (stage 2 reuses
the tables stage 1 built, on more than one step), both directions, and a per-frame step table with two different counts.

tests/golden/cnf_h3w_flush_band_bits.npz holds what `python tools/record_cnf_h3w_bits.py --band` wrote on a build of the parent commit
(these are the kernel's own outputs, not the oracle's).  On the recording box the matrix pipe honours f16 subnormals: a build with the
flush of plane 1 switched off differed from the fixture in 5 of the 5 launches below, one with the flush of plane 2 off in 5 of 5
("the wave's instruction stream"), so the launches do reach the band."""
import os

import numpy as np
import pytest
import torch

from test_cnf_f16x3 import launch_h3
from test_cnf_f16x3_planes import bits
from test_cnf_solve_kernels import Weights, base_samples, dev, rnd, weights  # noqa: F401

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cnf_h3w_flush_band_bits.npz")
LDH, H, BOFF = 3078, 512, 3 * 512 + 3

CASES = (dict(n=128, steps=1, reverse=True, w="seeded"),
         dict(n=160, steps=3, reverse=False, w="stress"),
         dict(n=160, steps=1, reverse=False, w="seeded"),
         dict(n=128, steps=3, reverse=True, w="stress"),
         dict(n=160, steps=(3, 1), reverse=True, w="seeded"))      # a step count per frame
case_id = lambda c: "n%d-s%s-%s-%s" % (c["n"], "".join(map(str, c["steps"])) + "tab" if isinstance(c["steps"], tuple) else c["steps"],
                                        "rev" if c["reverse"] else "fwd", c["w"])


def band(hy):
    """The edit of the (2, LDH) hyper rows described in the module docstring, in place."""
    sweep = torch.linspace(-17.2, -9.3, 64)
    for l in (0, 1):
        g, b = l * H, BOFF + l * H
        for f in (0, 1):
            if f == 1:
                hy[f, g:g + H] = -30.0
                hy[f, b:b + H] = -40.0
                hy[f, g + 96:g + 160] = 0.5
            hy[f, g:g + 64] = -30.0
            hy[f, b:b + 64] = sweep + 0.05 * f
            hy[f, g + 64:g + 96] = 0.0
            hy[f, b + 64:b + 96] = sweep[::2] + 0.03 * f
            hy[f, b + 96:b + 160] = torch.linspace(-5.6, -2.6, 64) + 0.02 * f
    return hy


def run_case(W, c):
    """The launch of one case on the weight set W -> output bits."""
    from caspr_amd import ops
    ctx, y = rnd(5600 + c["n"], 2, 1600), base_samples(5601 + c["n"], 2, c["n"])
    steps = torch.tensor(c["steps"], dtype=torch.int32, device="cuda:0") if isinstance(c["steps"], tuple) else c["steps"]
    out = launch_h3(W, y, band(W.hyper(ctx, LDH)), steps, c["reverse"])
    ops.check_deferred_errors()
    return bits(out)


@pytest.fixture(scope="module")
def parent():
    return np.load(FIXTURE, allow_pickle=False)


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_flush_band_bits_of_the_parent_kernel(dev, weights, parent, case):
    got, want = run_case(weights[case["w"]], case), parent[case_id(case)]
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.isfinite(got.view(np.float32)).all()
    bad = int((got != want).sum())
    print("%s: %d of %d words differ from the parent's" % (case_id(case), bad, got.size))
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(want)), "%d of %d output words differ from the parent kernel's" % (bad, got.size)
