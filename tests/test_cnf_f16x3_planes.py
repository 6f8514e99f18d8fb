"""The f16x3 point-CNF kernel (csrc/ode_f16x3w.hip) against the recorded output BITS of its parent: the kernel that kept the f32
activations of hidden layer 1 in the accumulator file and split them again in each of layer 2's passes 1-3.  Keeping the two f16 planes
there instead is the same function of the same values, multiplied and summed in the same order, so every output bit must stay.

tests/golden/cnf_h3w_parent_bits.npz holds what tools/record_cnf_h3w_bits.py wrote on a build of the parent commit: the launches of
CASES below (the smallest at which the change can go wrong: one full workgroup and one step; a ragged second workgroup with two steps,
i.e. frame indexing and the stage-to-stage carry of the ring and of the first fragments; both directions; every MovingBatchNorm
arrangement used; both weight sets), and one launch whose layer-1 hyper bias of unit 7 trips the range guard on frame 1 (bias 5000, as
test_cnf_f16x3.test_range_guard: far past the limit) and on frame 2 (bias 4095, the limit itself: the gated product decides, and on
the recorded build it took all 130 points over): the NaN points, the untouched points of frame 0 and the status word.

A DELIBERATE change of the kernel's arithmetic re-records the fixture with the tool (python tools/record_cnf_h3w_bits.py on the GPU box)
and says so in its commit; anything else that moves a bit here is a bug."""
import os

import numpy as np
import pytest
import torch

from test_cnf_f16x3 import launch_h3
from test_cnf_solve_kernels import Weights, base_samples, dev, mbn_pair, rnd, weights  # noqa: F401

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cnf_h3w_parent_bits.npz")
LDH = 3078

CASES = (dict(n=128, BT=1, steps=1, reverse=True, mbn="none", w="seeded"),
         dict(n=129, BT=2, steps=2, reverse=True, mbn="both", w="stress"),
         dict(n=257, BT=2, steps=1, reverse=False, mbn="in", w="stress"),
         dict(n=384, BT=3, steps=3, reverse=True, mbn="both", w="seeded"))
case_id = lambda c: "n%d-bt%d-s%d-%s-mbn_%s-%s" % (c["n"], c["BT"], c["steps"], "rev" if c["reverse"] else "fwd", c["mbn"], c["w"])


def bits(x):
    """The raw bits of an f32 GPU tensor as an int32 numpy array."""
    return x.detach().contiguous().view(torch.int32).cpu().numpy()


def run_case(W, c):
    """The launch of one case on the weight set W -> output bits."""
    from caspr_amd import ops
    ctx, y = rnd(5000 + c["n"], c["BT"], 1600), base_samples(5001 + c["n"], c["BT"], c["n"])
    mi, mo = mbn_pair(c["reverse"], c["mbn"])
    out = launch_h3(W, y, W.hyper(ctx, LDH), c["steps"], c["reverse"], mi, mo)
    ops.check_deferred_errors()
    return bits(out)


def run_guard(W):
    """The launch that trips the range guard -> (output bits, status word)."""
    from caspr_amd import lib as _lib
    from caspr_amd import ops
    BT, n, steps = 3, 130, 2
    ctx, y = rnd(5400, BT, 1600), base_samples(5401, BT, n)
    hot = W.hyper(ctx, LDH)
    col = (3 * 512 + 3) + 512 + 7       # the hyper BIAS column of layer 1, unit 7
    hot[1, col] = 5000.0
    hot[2, col] = 4095.0
    ops.check_deferred_errors()
    out = launch_h3(W, y, hot, steps, True)
    torch.cuda.synchronize()
    word = int(ops._cnf_h3.words[(0, torch.cuda.current_stream().cuda_stream)][0].cpu()[0])
    with pytest.raises(_lib.CasprHipError):
        ops.check_deferred_errors()
    return bits(out), word


@pytest.fixture(scope="module")
def parent():
    return np.load(FIXTURE, allow_pickle=False)


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_bits_of_the_parent_kernel(dev, weights, parent, case):
    got, want = run_case(weights[case["w"]], case), parent[case_id(case)]
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = int((got != want).sum())
    print("%s: %d of %d words differ from the parent's" % (case_id(case), bad, got.size))
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(want)), "%d of %d output words differ from the parent kernel's" % (bad, got.size)


def test_range_guard_bits_of_the_parent_kernel(dev, weights, parent):
    got, word = run_guard(weights["seeded"])
    want = parent["guard"]
    nan = np.isnan(got.view(np.float32))
    print("guard: NaN points per frame %s, status word %d" % (nan.all(axis=2).sum(axis=1).tolist(), word))
    assert nan[1].all() and not nan[0].any(), "the case no longer trips the guard where it was built to"
    assert word == int(parent["guard_status"]) and word != 0
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(want)), "%d of %d output words differ from the parent kernel's" % (int((got != want).sum()), got.size)
