"""The adaptive Dormand-Prince solve of the point CNF on the f16x3 evaluation (ops.cnf_dopri5 with the pack_cnf_h3 packs,
csrc/ode_dp5_f16x3w.hip, include/caspr_hip.h: caspr_cnf_dopri5_h3_f32; opt-in: ops.CNF_DP5_SPLIT = "f16x3").

The method is test_cnf_dopri5's, whose helpers are imported: the kernel is checked against ITS OWN traced attempts replayed in f64
(state within X_TOL = 1e-5 of the tensor maximum -- the suite's number for the bf16x6 kernel, unchanged; accept / reject against
s64 = sqrt(ratio) of the replay; the controller formulas on the traced numbers).  delta, the band in which an attempt decides nothing,
is measured WITHOUT the kernel: 4 x the larger of |s - s64| of the same attempts replayed in 32-bit arithmetic with the two hidden
layers on the f16x3 restatement (tests/f16x3_ref.py) and in plain f32.

Figures land in test_hip_parity's JSON report under "cnf_dopri5_f16x3:" keys.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import f16x3_ref
import test_cnf_solve_kernels as K
from test_hip_parity import REPORT, record
from test_cnf_solve_kernels import Weights, base_samples, mbn_f64, mbn_pair, rnd, LIVE
from test_cnf_dopri5 import X_TOL, check_decisions, frame_problem, measure_delta, same_bits, traced

KERNEL = "cnf_dp5_h3w_kernel"


class PatchedF:
    """torch.nn.functional with linear() on (512, 512) f32 weights on three f16 products (as test_f16x3_emulation._PatchedF patches the
    oracle's); everything else, and every f64 call, passes through."""

    def __init__(self, first_only=False):
        self.first_only = first_only

    def __getattr__(self, name):
        return getattr(F, name)

    def linear(self, x, w, b=None):
        if tuple(w.shape) == (512, 512) and x.dtype == torch.float32:
            return f16x3_ref.linear(x, w, b, first_only=self.first_only)
        return F.linear(x, w, b)


def report(key, **kw):
    REPORT["cnf_dopri5_f16x3:" + key] = kw
    record("cnf_dopri5_f16x3:%s:recorded" % key, 0, 0, 0)


def measure_delta_h3(monkeypatch, p32, p64, t0, t1, tol, dts, decisions):
    """-> (the larger of the worst |s_f16x3 - s64| and the worst |s_f32 - s64| over the given attempts, the f64 replay)."""
    w32, _, r64 = measure_delta(p32, p64, t0, t1, tol, tol, dts, decisions)
    with monkeypatch.context() as m:
        m.setattr(K, "F", PatchedF())
        wh3, _, _ = measure_delta(p32, p64, t0, t1, tol, tol, dts, decisions)
    return max(w32, wh3), r64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights(dev, seeded_sd, stress_sd):
    from caspr_amd import ops
    out = {"seeded": Weights(seeded_sd, dev), "stress": Weights(stress_sd, dev)}
    for W in out.values():
        W.w1h, W.w2h = ops.pack_cnf_h3(W.dev["w1"]), ops.pack_cnf_h3(W.dev["w2"])
    return out


def solve(W, y, hyper, rtol, atol, reverse, mbn_in=None, mbn_out=None, e=None, logp=None, max_attempts=1000, packs=True, tcol=None):
    """One ops.cnf_dopri5 call with the trace -> (x, logp | None, info, kernel name) on the CPU; packs: hand over the f16x3 packs."""
    from caspr_amd import ops
    g = lambda v: None if v is None else v.to("cuda:0").contiguous()
    D = W.dev
    res = ops.cnf_dopri5(g(y), g(hyper), D["tcol"] if tcol is None else g(tcol), D["w0"], D["b0"], D["b1"], D["b2"], D["w3"], D["b3"], W.w1x, W.w2x, W.t_end, rtol, atol,
                         reverse, g(mbn_in), g(mbn_out), e=g(e), logp=g(logp), max_attempts=max_attempts, return_trace=True,
                         w1h=W.w1h if packs else None, w2h=W.w2h if packs else None)
    torch.cuda.synchronize()
    info = {k: v.cpu() for k, v in res[-1].items() if torch.is_tensor(v)}
    assert ("kernel" in res[-1]) == ("finished" in res[-1]) == packs          # the two items of a call that hands the packs over
    return res[0].cpu(), (res[1].cpu() if e is not None else None), info, res[-1].get("kernel")


def same_info(a, b, idx=None):
    """Every item of trace b is, bit for bit, the item of trace a (its rows idx)."""
    return all(same_bits((a[k] if idx is None else a[k][idx]).float(), b[k].float()) for k in b)


# ---------------------------------------------------------------------------------------------
# route matrix
# ---------------------------------------------------------------------------------------------
N_EDGES = (128, 129, 255, 256, 257, 1000)       # one workgroup exactly; one point over; one short of two; two; two and a point; eight, the last partial
MBNS = ("both", "in", "out", "none")
LDHS = (3078, 3091, 3080)


def _cases():
    """Every n five times; direction, MBN, ldh and the weight set cycle along the list so that every n sees both directions, three of
    the MBN sets, every ldh and both weight sets; BT is 17 twice, else 1 or 3 (1 at n = 1000: the CPU replay is the cost of a case)."""
    out = []
    for r in range(5):
        for i, n in enumerate(N_EDGES):
            j = 6 * r + i
            BT = 17 if (r, n) in ((1, 129), (3, 256)) else (1 if (n == 1000 or j % 2 == 0) else 3)
            out.append(dict(n=n, BT=BT, reverse=(r + i) % 2 == 0, mbn=MBNS[(j // 2) % 4], ldh=LDHS[(r + i) % 3], w="seeded" if (3 * r + i) % 4 == 3 else "stress"))
    return out


CASES = _cases()
MATRIX = dict(attempts=0, undecided=0, worst_s_diff=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["n%d-bt%d-%s-mbn_%s-ldh%d-%s" % (c["n"], c["BT"], "rev" if c["reverse"] else "fwd", c["mbn"], c["ldh"], c["w"])
                                             for c in CASES])
def test_route_matrix(dev, weights, case, monkeypatch):
    """State and decisions of every frame against the f64 replay of the kernel's own attempts; the launch twice, bit for bit."""
    W = weights[case["w"]]
    BT, n, reverse, tol = case["BT"], case["n"], case["reverse"], 1e-5
    seed = 2000 + n
    c, y = rnd(seed, BT, 1600, scale=0.5), base_samples(seed + 1, BT, n)
    hyper = W.hyper(c, case["ldh"])
    mi, mo = mbn_pair(reverse, case["mbn"])
    x, _, info, kernel = solve(W, y, hyper, tol, tol, reverse, mi, mo)
    x2, _, info2, _ = solve(W, y, hyper, tol, tol, reverse, mi, mo)
    bad = []
    if kernel != KERNEL:
        bad.append("the call ran %s" % kernel)
    if not (same_bits(x, x2) and same_info(info, info2)):
        bad.append("two launches differ in their bits")
    if not bool((info["finished"] == 1).all()):
        bad.append("finished flags %s" % info["finished"].tolist())
    t0, t1 = (W.t_end, 0.0) if reverse else (0.0, W.t_end)
    stats = dict(attempts=0, undecided=0)
    frames = range(BT) if BT <= 5 else (0, 7, BT - 1)          # (17 frames: three of them replayed; all of them launched)
    for b in frames:
        got = traced(info, b)
        if got["nfe"] != 2 + 6 * len(got["dts"]):
            bad.append("frame %d: %d evaluations counted for %d attempts" % (b, got["nfe"], len(got["dts"])))
        p64 = frame_problem(W, y, hyper, b, reverse, mi, None, None)
        p32 = frame_problem(W, y, hyper, b, reverse, mi, None, None, torch.float32)
        worst, r64 = measure_delta_h3(monkeypatch, p32, p64, t0, t1, tol, got["dts"], got["accepted"])
        MATRIX["worst_s_diff"] = max(MATRIX["worst_s_diff"], worst)
        delta = 4 * worst
        print("frame %d: %d attempts, %d rejected, |s32 - s64| max %.3e, s64 %s" % (b, len(got["dts"]), got["accepted"].count(False), worst,
                                                                                      ["%.4f" % math.sqrt(max(r)) for r in r64["ratios"]]))
        check_decisions("frame %d" % b, r64, got, delta, bad, stats)
        ox = r64["out"][0]
        if mo is not None:
            ox, _ = mbn_f64(mo.double(), ox, None, reverse)
        scale = max(1.0, float(ox.abs().max()))
        err = float((x[b:b + 1].double() - ox).abs().max())
        REPORT["cnf_dopri5_f16x3:matrix:n%d-bt%d-%s:frame%d:x" % (n, BT, "rev" if reverse else "fwd", b)] = {
            "max_abs_err": err, "bound": X_TOL * scale, "attempts": len(got["dts"]), "kernel": kernel}
        print("  x: max abs err %.3e, bound %.3e" % (err, X_TOL * scale))
        if not (bool(torch.isfinite(x[b]).all()) and err <= X_TOL * scale):
            bad.append("frame %d x: max abs err %.3e > %.1e x %.3g" % (b, err, X_TOL, scale))
    MATRIX["attempts"] += stats["attempts"]
    MATRIX["undecided"] += stats["undecided"]
    report("matrix:totals", attempts=MATRIX["attempts"], undecided=MATRIX["undecided"], worst_s32_minus_s64=MATRIX["worst_s_diff"],
           delta=4 * MATRIX["worst_s_diff"])
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_undecided_attempts_over_the_matrix():
    """Attempts whose s64 lies inside 1 +- delta decide nothing: at most 10 % of the attempts of the matrix cases that ran (all of
    them in a full run; the cases feed MATRIX, this test, which follows them in the file, is the one place that judges the total)."""
    assert MATRIX["undecided"] <= 0.1 * MATRIX["attempts"], "attempts that decide nothing: %d of %d" % (MATRIX["undecided"], MATRIX["attempts"])


@pytest.mark.gpu
def test_a_frame_does_not_depend_on_its_batch(dev, weights):
    """Output, trace and counters of a frame: alone, inside a batch, under a permutation of the frames, on a second stream."""
    W = weights["stress"]
    BT, n = 6, 150
    c, y = rnd(41, BT, 1600, scale=0.5), base_samples(42, BT, n)
    hyper = W.hyper(c, 3080)
    mi, mo = mbn_pair(True, "both")
    x, _, info, kernel = solve(W, y, hyper, 1e-5, 1e-5, True, mi, mo)
    assert kernel == KERNEL
    perm = torch.tensor([4, 2, 5, 0, 3, 1])
    xp, _, infop, _ = solve(W, y[perm], hyper[perm], 1e-5, 1e-5, True, mi, mo)
    with torch.cuda.stream(torch.cuda.Stream()):
        xs, _, infos, _ = solve(W, y, hyper, 1e-5, 1e-5, True, mi, mo)
    bad = []
    if not same_info(info, infos):
        bad.append("second stream: the trace differs")
    if not same_info(info, infop, perm):
        bad.append("permutation: the trace differs")
    if not (same_bits(x, xs) and same_bits(x[perm], xp)):
        bad.append("outputs differ under a permutation / on a second stream")
    for b in (0, 3, 5):
        i = torch.tensor([b])
        x1, _, info1, _ = solve(W, y[i], hyper[i], 1e-5, 1e-5, True, mi, mo)
        if not (same_bits(x1, x[i]) and same_info(info, info1, i)):
            bad.append("frame %d alone differs from the frame inside the batch" % b)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_fallbacks_keep_their_bits(dev, weights):
    """n = 127 and a call with e / logp go where they go without the packs, bit for bit, and say so."""
    W = weights["stress"]
    BT = 2
    c = rnd(71, BT, 1600, scale=0.5)
    hyper = W.hyper(c, 3080)
    y = base_samples(72, BT, 127)
    a, b = solve(W, y, hyper, 1e-5, 1e-5, True), solve(W, y, hyper, 1e-5, 1e-5, True, packs=False)
    assert a[3] == "cnf_dp5_kernel<false>" and b[3] is None and same_bits(a[0], b[0]) and same_info(a[2], b[2]) and len(b[2]) == 9
    y = base_samples(73, BT, 130)
    e, lp0 = rnd(74, BT, 130, 3), rnd(75, BT, 130, 1)
    a, b = solve(W, y, hyper, 1e-5, 1e-5, False, e=e, logp=lp0), solve(W, y, hyper, 1e-5, 1e-5, False, e=e, logp=lp0, packs=False)
    assert a[3] == "cnf_dp5_kernel<true>" and b[3] is None and same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_info(a[2], b[2])


GUARD_SCALE = 4.0e4      # frame 1's base samples times this: see test_range_guard_retires_the_frame


def guard_inputs(W):
    BT, n = 3, 200
    c, y = rnd(81, BT, 1600, scale=0.5), base_samples(82, BT, n)
    y[1] *= GUARD_SCALE
    return c, y


def first_hidden_max(W, y_row, hyper_row, t, tcol=None):
    """max over points and units of the input layer's activation at time t, in f32 as the kernel computes it (unscaled)."""
    hy, tc = hyper_row[:LIVE], (W.cpu["tcol"] if tcol is None else tcol)
    gate = torch.sigmoid(hy[K._cols(0, False)] + t * tc[K._cols(0, False)])
    beta = hy[K._cols(0, True)] + t * tc[K._cols(0, True)]
    return float(F.softplus(F.linear(y_row, W.cpu["w0"], W.cpu["b0"]) * gate + beta).max())


@pytest.mark.gpu
def test_range_guard_retires_the_frame(dev, weights):
    """Frame 1 of three has its samples scaled until an input-layer activation passes 4095 (f16's range after the 2^4 prescale) at
    the start time -- checked on the CPU first.  The frame retires at once with NaN in all of its rows and finished = 3; the other
    two frames keep the bits of a run without it; the deferred channel raises and names the remedy."""
    from caspr_amd import ops
    from caspr_amd.lib import CasprHipError
    W = weights["seeded"]
    c, y = guard_inputs(W)
    hyper = W.hyper(c, 3080)
    assert first_hidden_max(W, y[1], hyper[1], W.t_end) > 4095.0 and all(first_hidden_max(W, y[b], hyper[b], W.t_end) < 100.0 for b in (0, 2))
    ops.check_deferred_errors()
    x, _, info, kernel = solve(W, y, hyper, 1e-5, 1e-5, True, max_attempts=40)
    assert kernel == KERNEL
    with pytest.raises(CasprHipError, match='cnf_dp5_split="bf16x6"'):
        ops.check_deferred_errors()
    ops.check_deferred_errors()                                    # reported once
    keep = torch.tensor([0, 2])
    xk, _, infok, _ = solve(W, y[keep], hyper[keep], 1e-5, 1e-5, True, max_attempts=40)
    ops.check_deferred_errors()
    assert bool(torch.isnan(x[1]).all()), "the retired frame's rows are not all NaN"
    assert info["finished"].tolist() == [1, 3, 1]
    assert int(info["accepted"][1] + info["rejected"][1]) <= 1 and int(info["nfe"][1]) <= 8, "the frame ran on after the guard tripped"
    assert same_bits(x[keep], xk) and same_info(info, infok, keep), "the other frames changed"
    assert bool(torch.isfinite(xk).all())


GUARD_UNIT, GUARD_SLOPE, GUARD_TIME = 7, -100.0, 0.2


@pytest.mark.gpu
def test_range_guard_retires_the_frame_in_the_middle_of_the_solve(dev, weights):
    """The guard after accepted steps.  Input-layer unit 7 has its gate shut (its activation is its hyper bias, the same for every point)
    and a bias that falls by 100 per unit of time in every frame; frame 1 starts it at 4095 + 100 x 0.2, so that frame's activation is
    below 4095 while t > 0.2 and at or above it from there on (the solve runs from t_end = 0.5 down to 0).  On the CPU (f32, no guard)
    that frame evaluates at t = 0.2912, 0.2547, 0.0717 in its THIRD attempt, after two accepted ones: the crossing lies inside a gap
    of 0.18.  The frame must retire there: NaN in all rows, finished = 3, the attempt that was running traced as rejected with a NaN
    ratio and counted, nothing after it; the other two frames keep the bits of a run without it; the deferred error names the remedy."""
    from caspr_amd import ops
    from caspr_amd.lib import CasprHipError
    W = weights["seeded"]
    assert abs(W.t_end - 0.5) < 1e-6
    BT, n = 3, 200
    tcol = W.cpu["tcol"].clone()
    tcol[GUARD_UNIT], tcol[K.BOFF + GUARD_UNIT] = 0.0, GUARD_SLOPE
    c, y = rnd(91, BT, 1600, scale=0.5), base_samples(92, BT, n)
    hyper = W.hyper(c, 3080)
    hyper[:, GUARD_UNIT] = -40.0
    hyper[:, K.BOFF + GUARD_UNIT] = 0.0
    hyper[1, K.BOFF + GUARD_UNIT] = 4095.0 - GUARD_TIME * GUARD_SLOPE
    assert first_hidden_max(W, y[1], hyper[1], GUARD_TIME + 0.05, tcol) < 4095.0 <= first_hidden_max(W, y[1], hyper[1], GUARD_TIME - 0.05, tcol)
    assert all(first_hidden_max(W, y[b], hyper[b], t, tcol) < 200.0 for b in (0, 2) for t in (0.5, 0.0, -0.6))
    ops.check_deferred_errors()
    x, _, info, kernel = solve(W, y, hyper, 1e-5, 1e-5, True, max_attempts=60, tcol=tcol)
    assert kernel == KERNEL
    with pytest.raises(CasprHipError, match='cnf_dp5_split="bf16x6"'):
        ops.check_deferred_errors()
    keep = torch.tensor([0, 2])
    xk, _, infok, _ = solve(W, y[keep], hyper[keep], 1e-5, 1e-5, True, max_attempts=60, tcol=tcol)
    ops.check_deferred_errors()
    acc, rej, nfe = int(info["accepted"][1]), int(info["rejected"][1]), int(info["nfe"][1])
    print("retired after %d accepted, %d rejected attempts, %d evaluations" % (acc, rej, nfe))
    assert info["finished"].tolist() == [1, 3, 1] and bool(torch.isnan(x[1]).all())
    assert acc >= 1 and rej >= 1 and nfe == 2 + 6 * (acc + rej), "not retired in the middle of the solve"
    rows = info["attempts"][1]
    last = rows[acc + rej - 1]
    assert bool(torch.isnan(last[2])) and float(last[4]) == 0.0 and float(last[0]) > GUARD_TIME - 0.05 and float(last[1]) > 0.0
    assert bool(torch.isfinite(rows[:acc + rej - 1]).all()) and bool((rows[acc + rej:] == 0).all()), "the trace goes on after the retirement"
    assert same_bits(x[keep], xk) and same_info(info, infok, keep) and bool(torch.isfinite(xk).all()), "the other frames changed"


@pytest.mark.gpu
def test_attempt_budget_and_bad_packs(dev, weights):
    """max_attempts = 2 on the stress weights: the error status of the other route, raised -- nothing hangs.  Bad packs raise."""
    from caspr_amd import ops
    from caspr_amd.lib import CasprHipError
    W = weights["stress"]
    BT, n = 2, 160
    c, y = rnd(51, BT, 1600, scale=0.5), base_samples(52, BT, n)
    hyper = W.hyper(c, 3080)
    with pytest.raises(CasprHipError, match="max_attempts"):
        solve(W, y, hyper, 1e-6, 1e-6, True, max_attempts=2)
    with pytest.raises(CasprHipError, match="max_attempts"):
        solve(W, y, hyper, 1e-6, 1e-6, True, max_attempts=2, packs=False)
    x, _, info, kernel = solve(W, y, hyper, 1e-5, 1e-5, True)            # the library is still usable afterwards
    assert kernel == KERNEL and bool(torch.isfinite(x).all()) and int((info["accepted"] + info["rejected"]).max()) > 2
    D = W.dev
    call = lambda **kw: ops.cnf_dopri5(y.to(dev), hyper.to(dev), D["tcol"], D["w0"], D["b0"], D["b1"], D["b2"], D["w3"], D["b3"], W.w1x, W.w2x,
                                       W.t_end, 1e-5, 1e-5, True, **kw)
    with pytest.raises(ValueError, match="pack_cnf_h3"):
        call(w1h=W.w1h[:-1], w2h=W.w2h)
    with pytest.raises(ValueError, match="pack_cnf_h3"):
        call(w1h=W.w1h, w2h=W.w2h.float())
    with pytest.raises(ValueError, match="pack_cnf_h3"):
        call(w1h=W.w1x, w2h=W.w2x)                                  # the bf16x6 packs in the wrong place


@pytest.mark.gpu
def test_model_surface(dev, seeded_sd, monkeypatch):
    """With ops.CNF_DP5_SPLIT = "f16x3", CaSPR(cnf_method="dopri5").reconstruct() runs the new kernel and get_nfe() is its trace's
    maximum; with the switch at its default the result is, bit for bit, ops.cnf_dopri5 on the bf16x6 route from the same y / z."""
    from caspr_amd import ops
    from caspr_amd.models import CaSPR
    from caspr_amd.utils.synthetic import dense_sequences
    assert ops.CNF_DP5_SPLIT == "bf16x6"
    m = CaSPR(cnf_method="dopri5", cnf_atol=1e-5, cnf_rtol=1e-5)
    m.load_state_dict(seeded_sd)
    m = m.to(dev).eval()
    blk = m.point_cnf.chain[1]
    x, sp = dense_sequences(1, 2, 256)
    y = rnd(61, 1, 2, 256, 3).to(dev)
    ts = sp[0, :, 0, 3].to(dev)
    with torch.no_grad():
        _, _, gx, _ = m.reconstruct(x.to(dev), num_points=256, timestamps=ts, y=y)
        ops.check_deferred_errors()
        assert blk.last_dp5_kernel == "cnf_dp5_kernel<false>"
        z0, _ = m.encode(x.to(dev))
        z = m.aggregate_and_solve_latent(z0, ts.view(1, -1))
        w = blk._weights()
        hyper = ops.conv1x1(w["hyp"], w["hyp_bias"], z.reshape(1, 2, -1).contiguous(), row_invariant=True)[0]
        w1x, w2x = blk._weights_x6()
        args = (y.view(2, 256, 3), hyper, w["tcol"], w["w0"], w["b0"], w["b1"], w["b2"], w["w3"], w["b3"], w1x, w2x, blk.end_time(), 1e-5, 1e-5, True,
                m.point_cnf.chain[2].kernel_params(), m.point_cnf.chain[0].kernel_params())
        want, info = ops.cnf_dopri5(*args, return_trace=True)
        assert "kernel" not in info and same_bits(gx.view(2, 256, 3).cpu(), want.cpu())
        monkeypatch.setattr(ops, "CNF_DP5_SPLIT", "f16x3")
        _, _, hx, _ = m.reconstruct(x.to(dev), num_points=256, timestamps=ts, y=y)
        ops.check_deferred_errors()
        assert blk.last_dp5_kernel == KERNEL
        nfe = blk.last_nfe_per_frame.cpu()
        assert int(m.get_nfe()[1]) == int(nfe.max()) and nfe.shape == (2,) and int(nfe.min()) >= 8
        w1h, w2h = blk._weights_h3()
        wanth, infoh = ops.cnf_dopri5(*args, return_trace=True, w1h=w1h, w2h=w2h)
        assert infoh["kernel"] == KERNEL and same_bits(hx.view(2, 256, 3).cpu(), wanth.cpu()) and infoh["nfe"].cpu().tolist() == nfe.tolist()
        err = float((hx - gx).abs().max())
        report("model_surface", max_abs_diff_to_bf16x6_route=err, nfe=nfe.tolist())
        monkeypatch.setattr(ops, "CNF_DP5_SPLIT", "f16x4")
        with pytest.raises(ValueError, match="CNF_DP5_SPLIT"):
            m.reconstruct(x.to(dev), num_points=256, timestamps=ts, y=y)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["seeded", "stress"])
def test_tolerance_is_honoured(dev, weights, which):
    """Tightening rtol = atol (1e-4, 1e-5, 1e-6) moves the result towards the converged f64 solution (RK4, 256 steps, f64), as far as
    an f32 output can show it: two distances are told apart only when they differ by more than one unit in the last place of the
    largest coordinate (test_cnf_dopri5.test_tolerance_is_honoured).  The bf16x6 route's distances are recorded beside them."""
    from test_cnf_solve_kernels import reference
    W = weights[which]
    BT, n = 3, 200
    c, y = rnd(31, BT, 1600, scale=0.5), base_samples(32, BT, n)
    hyper = W.hyper(c, 3080)
    conv, _ = reference(W, y, hyper, 256, True)
    dist, other = {}, {}
    for tol in (1e-4, 1e-5, 1e-6):
        x, _, info, kernel = solve(W, y, hyper, tol, tol, True)
        assert kernel == KERNEL
        dist[tol] = float((x.double() - conv).abs().max())
        other[tol] = float((solve(W, y, hyper, tol, tol, True, packs=False)[0].double() - conv).abs().max())
        print("%s tol %.0e: distance %.3e (bf16x6 route %.3e), nfe %s" % (which, tol, dist[tol], other[tol], info["nfe"].tolist()))
    ulp = 2.0 ** -23 * float(conv.abs().max())
    report("contract:%s" % which, distance_1e4=dist[1e-4], distance_1e5=dist[1e-5], distance_1e6=dist[1e-6], bf16x6_distance_1e4=other[1e-4],
           bf16x6_distance_1e5=other[1e-5], bf16x6_distance_1e6=other[1e-6], f32_ulp_at_absmax=ulp)
    assert dist[1e-4] + ulp >= dist[1e-5] and dist[1e-5] + ulp >= dist[1e-6] and dist[1e-4] + ulp >= dist[1e-6], (dist, ulp)
