"""The device base sampler: csrc/base_sample.hip, ops.base_samples, CaSPR(base_sampler="device").

The kernel is held to the numpy f64 restatement in tests/base_sample_ref.py: the Philox words, the chosen candidate of the
truncated mode and the contour assignment exactly, the values within VALUE_TOL (below), the fused log-density bit for bit to
what torch computes on the kernel's own y.  The model-level tests check that a batch split into shards draws the same samples,
that no host generator moves, and the draw numbering."""
import copy
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import base_sample_ref as R  # noqa: E402

SEED = 0x123456789ABCDEF0
DRAW = 2
FRAME_IDS = [0, 7, 2 ** 33 + 1]
SHAPES = (65, 1)          # n = 65: one full 64-lane workgroup and a ragged one per frame; n = 1: a single lane
TRUNC = 0.5               # P(none of four candidates inside) = (1 - erf(0.5 / sqrt 2))^4 = 14.5 %: the fallback is exercised
RADII = [0.1, 0.45, 0.9]
# Bound on |y_device - y_restatement|, from the number formats.  Every argument of logf / log1pf / sincospif is exact in f32 (the
# kernel's header), so the error of a normal y = r c comes from the functions and the roundings alone: logf / log1pf within 1 ulp
# and a correctly rounded sqrtf give r within 1 ulp, sincospif gives c within 1 ulp of 1, the product adds half an ulp: 2.5 ulp of r,
# asserted as 4 ulp of the largest r a 24-bit uniform can give, sqrt(-2 ln 2^-25) = 5.89: 4 x 2^-23 x 5.89 = 2.81e-6.  (A contour
# point is a few ulp of a radius <= 0.9.)  The same evaluation order with correctly rounded f32 functions is 3.8e-7 from the
# restatement over 36,864 values; a difference above 1e-5 would be a bug in any case.
VALUE_TOL = 4.0 * 2.0 ** -23 * math.sqrt(2.0 * 25.0 * math.log(2.0))


# ---------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """The Random123 known-answer vectors of philox4x32_10 (kat_vectors): all-zero, all-ones and the pi-digits counter / key."""
    def run(ctr, key):
        return [int(v) for v in R.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))]
    assert run([0] * 4, [0] * 2) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert run([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert run([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0]) == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_surface_without_gpu():
    """The constructor argument is validated, the draw number survives a deepcopy, the C symbol is declared, bound and built,
    and the op refuses host tensors (no CPU fallback)."""
    from caspr_amd import lib, ops
    from caspr_amd.csrc import build
    from caspr_amd.models import CaSPR
    with pytest.raises(ValueError):
        CaSPR(base_sampler="bogus")
    assert CaSPR().base_sampler == "host"
    m = CaSPR(base_sampler="device", base_seed=3)
    m.seed_base(9, draw=5)
    c = copy.deepcopy(m)
    assert (c.base_sampler, c.base_seed, c._base_draw) == ("device", 9, 5) and isinstance(c._base_draw, int)
    hdr = open(os.path.join(ROOT, "include", "caspr_hip.h")).read()
    assert re.search(r"\bint caspr_base_sample_f32\(", hdr) and "caspr_base_sample_f32" in lib.SIGNATURES
    assert len(lib.SIGNATURES["caspr_base_sample_f32"][1]) == 12 and "base_sample.hip" in build.SOURCES
    assert build.EXTRA["base_sample.hip"] == ["-ffp-contract=off"]
    with pytest.raises(ValueError):
        ops.base_samples(2, 4, 0, 0, torch.zeros(2, dtype=torch.int64))


def test_restatement_exercises_the_truncation_fallback():
    """What test_values relies on, checked on the restatement alone: in its truncated draws some elements have no candidate inside
    (the fallback to candidate 0), and at most 0.1 % of the elements have a candidate within VALUE_TOL of the bound (those are
    excluded from the comparison: a candidate that close may fall on either side in f32)."""
    for n in SHAPES:
        _, _, cand = R.truncated(SEED, DRAW, FRAME_IDS, n, TRUNC)
        assert int((~(np.abs(cand) < TRUNC).any(axis=-1)).sum()) >= 1
        near = (np.abs(np.abs(cand) - TRUNC) <= VALUE_TOL).any(axis=-1)
        assert near.mean() <= 1e-3
    assert [int(v) for v in np.bincount(R.contour_index(7, 3))] == [2, 2, 3]
    assert [int(v) for v in np.bincount(R.contour_index(65, 3))] == [21, 21, 23]
    assert [int(v) for v in np.bincount(R.contour_index(1, 3), minlength=3)] == [0, 0, 1]


# ---------------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from caspr_amd import ops as _ops
    return _ops


def _model(dev, sd, **kw):
    from caspr_amd.models import CaSPR
    m = CaSPR(**kw)
    m.load_state_dict(sd)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def dmodel(dev, seeded_sd):
    return _model(dev, seeded_sd, base_sampler="device", base_seed=11)


@pytest.fixture(scope="module")
def hmodel(dev, seeded_sd):
    return _model(dev, seeded_sd)


@pytest.fixture(scope="module")
def batch(dev):
    from caspr_amd.utils.synthetic import dense_sequences
    x, sp = dense_sequences(4, 2, 256)
    return x.to(dev), sp[0, :, 0, 3].to(dev)


def _ids(dev, ids):
    return torch.tensor(list(ids), dtype=torch.int64, device=dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SHAPES)
def test_raw_words_bit_exact(dev, ops, n):
    _, _, raw = ops.base_samples(3, n, SEED, DRAW, _ids(dev, FRAME_IDS), raw=True)
    want = R.words(SEED, DRAW, FRAME_IDS, n)
    assert np.array_equal(raw.cpu().numpy().view(np.uint32), want)
    # the words of block 0 do not depend on the mode
    for kw in ({"trunc_std": TRUNC}, {"radii": RADII}):
        assert np.array_equal(ops.base_samples(3, n, SEED, DRAW, _ids(dev, FRAME_IDS), raw=True, **kw)[2].cpu().numpy().view(np.uint32), want)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,n", [(m, n) for m in ("gaussian", "truncated", "contours") for n in SHAPES] + [("contours", 7)])
def test_values(dev, ops, mode, n):
    """y against the f64 restatement within VALUE_TOL; the truncated mode's chosen candidate and the contour assignment exactly."""
    ids = _ids(dev, FRAME_IDS)
    if mode == "gaussian":
        y = ops.base_samples(3, n, SEED, DRAW, ids)[0].cpu().double().numpy()
        want, keep = R.gaussian(SEED, DRAW, FRAME_IDS, n), None
    elif mode == "truncated":
        y = ops.base_samples(3, n, SEED, DRAW, ids, trunc_std=TRUNC)[0].cpu().double().numpy()
        want, chosen, cand = R.truncated(SEED, DRAW, FRAME_IDS, n, TRUNC)
        keep = ~(np.abs(np.abs(cand) - TRUNC) <= VALUE_TOL).any(axis=-1)
        assert (~keep).mean() <= 1e-3
        got_chosen = np.abs(cand - y[..., None]).argmin(axis=-1)          # the candidate the device picked
        assert np.array_equal(got_chosen[keep], chosen[keep])
        assert (np.abs(y) < TRUNC)[keep & (np.abs(cand) < TRUNC).any(axis=-1)].all()
    else:
        y = ops.base_samples(3, n, SEED, DRAW, ids, radii=RADII)[0].cpu().double().numpy()
        want, idx = R.contours(SEED, DRAW, FRAME_IDS, n, RADII)
        keep = None
        r32 = np.asarray(RADII, dtype=np.float32).astype(np.float64)
        got_idx = np.abs(np.linalg.norm(y, axis=-1)[..., None] - r32).argmin(axis=-1)   # the contour each point landed on
        assert np.array_equal(got_idx, np.broadcast_to(idx, got_idx.shape))
    diff = np.abs(y - want)
    if keep is not None:
        diff = diff[keep]
    print("base_sample %s n=%d: max |y - restatement| = %.3e (max |y| %.2f)" % (mode, n, diff.max(), np.abs(want).max()))
    assert diff.max() <= VALUE_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("n", SHAPES + (7,))
def test_logp_bit_exact(dev, ops, n):
    """The fused log-density equals standard_normal_logprob(y).sum(2) evaluated by torch on the kernel's own y, bit for bit."""
    from caspr_amd.models.utils import standard_normal_logprob
    for kw in ({}, {"trunc_std": TRUNC}, {"radii": RADII}):
        y, logp = ops.base_samples(3, n, SEED, DRAW, _ids(dev, FRAME_IDS), **kw)
        want = standard_normal_logprob(y).view(3, n, -1).sum(2)
        assert np.array_equal(_bits(logp), _bits(want)), kw


@pytest.mark.gpu
def test_launch_invariance(dev, ops):
    for kw in ({}, {"trunc_std": TRUNC}, {"radii": RADII}):
        whole = ops.base_samples(4, 65, SEED, DRAW, _ids(dev, [5, 6, 7, 8]), **kw)
        a = ops.base_samples(2, 65, SEED, DRAW, _ids(dev, [5, 6]), **kw)
        b = ops.base_samples(2, 65, SEED, DRAW, _ids(dev, [7, 8]), **kw)
        for w, pa, pb in zip(whole, a, b):
            assert np.array_equal(_bits(w), _bits(torch.cat([pa, pb], dim=0)))


@pytest.mark.gpu
def test_reconstruct_shard_invariance(dev, dmodel, batch):
    """A B = 4 batch against its two B = 2 halves with their global sequence ids: y and logp_y bitwise; x within the project's
    flat 1e-5 (the encoder and the flow pick launch shapes by batch size, so bitwise equality of x is not promised)."""
    x, ts = batch
    dmodel.seed_base(11)
    y, lp, px, _ = dmodel.reconstruct(x, num_points=64, timestamps=ts)
    halves = []
    for lo in (0, 2):
        dmodel.seed_base(11)
        halves.append(dmodel.reconstruct(x[lo:lo + 2], num_points=64, timestamps=ts, sequence_ids=[lo, lo + 1]))
    hy, hlp, hx = (torch.cat([h[i] for h in halves], dim=0) for i in range(3))
    assert np.array_equal(_bits(y), _bits(hy)) and np.array_equal(_bits(lp), _bits(hlp))
    dx = float((px - hx).abs().max())
    print("reconstruct shard invariance: max |x_whole - x_halves| = %.3e, bitwise %s" % (dx, np.array_equal(_bits(px), _bits(hx))))
    assert dx <= 1e-5
    # without the global ids the second half draws the first half's samples: the ids are what carries the invariance
    dmodel.seed_base(11)
    y_local = dmodel.reconstruct(x[2:4], num_points=64, timestamps=ts)[0]
    assert np.array_equal(_bits(y_local), _bits(y[0:2])) and not np.array_equal(_bits(y_local), _bits(y[2:4]))


@pytest.mark.gpu
def test_constant_in_time(dev, dmodel, batch):
    x, ts = batch
    dmodel.seed_base(11)
    y, lp, _, _ = dmodel.reconstruct(x, num_points=64, timestamps=ts, constant_in_time=True)
    assert np.array_equal(_bits(y[:, 0]), _bits(y[:, 1])) and np.array_equal(_bits(lp[:, 0]), _bits(lp[:, 1]))
    for b in range(1, 4):
        assert not np.array_equal(_bits(y[0]), _bits(y[b]))
    dmodel.seed_base(11)
    y_t = dmodel.reconstruct(x, num_points=64, timestamps=ts)[0]
    assert not np.array_equal(_bits(y_t[:, 0]), _bits(y[:, 0]))      # the per-sequence ids are apart from the per-frame ids
    dmodel.seed_base(11)
    h = dmodel.reconstruct(x[2:4], num_points=64, timestamps=ts, constant_in_time=True, sequence_ids=[2, 3])[0]
    assert np.array_equal(_bits(h), _bits(y[2:4]))


@pytest.mark.gpu
def test_host_generators_untouched(dev, dmodel, hmodel, batch):
    x, ts = batch
    for kw in ({}, {"truncate_std": 2.0}, {"sample_contours": RADII}):
        t0, n0 = torch.get_rng_state(), np.random.get_state()
        dmodel.reconstruct(x[:1], num_points=64, timestamps=ts, **kw)
        torch.cuda.synchronize()
        n1 = np.random.get_state()
        assert torch.equal(t0, torch.get_rng_state()), kw
        assert n0[0] == n1[0] and np.array_equal(n0[1], n1[1]) and n0[2:] == n1[2:], kw
    # control: the host sampler does advance torch's generator, so the comparison above can see a draw
    t0 = torch.get_rng_state()
    hmodel.reconstruct(x[:1], num_points=64, timestamps=ts)
    assert not torch.equal(t0, torch.get_rng_state())


@pytest.mark.gpu
def test_draw_numbering(dev, seeded_sd):
    m = _model(dev, seeded_sd, base_sampler="device", base_seed=11, check_tol=None)
    z = torch.from_numpy(np.random.default_rng(3).normal(0, 0.1, (1, 2, m.cnf_args.zdim)).astype(np.float32)).to(dev)
    with torch.no_grad():
        a1, a2 = m.decode(z, num_points=64)[0], m.decode(z, num_points=64)[0]
        assert not np.array_equal(_bits(a1), _bits(a2))
        m.seed_base(11)
        b1 = m.decode(z, num_points=64)[0]
        c = copy.deepcopy(m)                                  # carries the draw number: its next decode is draw 1
        b2, c2 = m.decode(z, num_points=64)[0], c.decode(z, num_points=64)[0]
        assert np.array_equal(_bits(a1), _bits(b1)) and np.array_equal(_bits(a2), _bits(b2)) and np.array_equal(_bits(a2), _bits(c2))
        m.seed_base(11, draw=1)
        assert np.array_equal(_bits(m.decode(z, num_points=64)[0]), _bits(a2))
        m.seed_base(12)
        assert not np.array_equal(_bits(m.decode(z, num_points=64)[0]), _bits(a1))
        # a given y draws nothing and consumes no draw number
        before = m._base_draw
        m.decode(z, num_points=64, y=a1)
        assert m._base_draw == before


@pytest.mark.gpu
def test_distribution(dev, ops):
    """Derived bounds (5 sigma of the sampling distribution of each statistic), fixed seeds."""
    y = ops.base_samples(8, 32768, 1, 0, _ids(dev, range(8)))[0].double()
    N = y.numel()
    assert N == 786432
    assert abs(float(y.mean())) < 5.0 / math.sqrt(N)
    assert abs(float(y.var(unbiased=False)) - 1.0) < 5.0 * math.sqrt(2.0 / N)
    p = math.erfc(3.0 / math.sqrt(2.0))
    assert abs(float((y.abs() > 3.0).double().mean()) - p) < 5.0 * math.sqrt(p * (1.0 - p) / N)
    n = 4096
    c = ops.base_samples(8, n, 1, 0, _ids(dev, range(8)), radii=RADII)[0].double().cpu().numpy()
    idx = R.contour_index(n, len(RADII))
    for k, r in enumerate(np.asarray(RADII, dtype=np.float32)):
        pts = c[:, idx == k].reshape(-1, 3)
        assert np.abs(np.linalg.norm(pts, axis=1) - float(r)).max() <= 4.0 * float(np.spacing(r))
        # a component of a direction with a sign-symmetric, axis-symmetric law has variance 1 / 3
        assert np.abs(pts.mean(axis=0)).max() < 5.0 * float(r) / math.sqrt(3.0 * pts.shape[0])


@pytest.mark.gpu
def test_host_sampler_unchanged(dev, hmodel, batch):
    from caspr_amd.models.utils import sample_gaussian
    x, ts = batch
    torch.manual_seed(0)
    y = hmodel.reconstruct(x[:1], num_points=64, timestamps=ts)[0]
    torch.manual_seed(0)
    want = sample_gaussian((2, 64, 3)).view(1, 2, 64, 3)
    assert np.array_equal(_bits(y), _bits(want))
