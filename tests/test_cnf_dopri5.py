"""The adaptive Dormand-Prince solve of the point CNF (ops.cnf_dopri5, csrc/ode_dp5.hip, include/caspr_hip.h: caspr_cnf_dopri5_f32).

A free-running comparison cannot be the test: in f32 and f64 the oracle's own dopri5 chooses different step sequences on the stress
weights and ends 1e-3 .. 3e-3 apart, both valid at a LOCAL tolerance of 1e-5.  The kernel is therefore checked against ITS OWN step
sequence replayed in f64:

  * replay(): f64 Dormand-Prince attempts at GIVEN dt's (and, optionally, given decisions) on the C contract's ConcatSquash layers
    (test_cnf_solve_kernels.odenet_f64) -- pinned on the CPU to oracle.model.dopri5_solve: fed the oracle's dt's it reproduces the
    oracle's result, ratios and decisions to 1e-12;
  * state: per frame, the replay of the kernel's traced dt's and decisions is within the suite's bounds of the kernel's output
    (1e-5 of the tensor maximum on x, 1e-4 on logp: test_cnf_solve_kernels' numbers, same evaluation body);
  * decisions: with s = sqrt(ratio) of the f64 replay, accepted attempts have s <= 1 + delta, rejected ones s >= 1 - delta; the next
    traced dt is the controller formula on the traced ratio; the first dt the formula on the traced d0 / d1 / d2 / h0; d0, d1 match
    f64 to 1e-4 relative (d2 is a difference of two evaluations h0 apart and cancels in f32: not compared);
  * delta is measured WITHOUT the kernel: the same attempts replayed with the oracle arithmetic in f32 and f64, 4 x the largest
    |s32 - s64| over attempts with s64 in [0.5, 2] (the bf16x6 products are documented at 2.6e-6 from f64, a few times plain f32);
  * attempts whose s64 lies inside [1 - delta, 1 + delta] decide nothing: at most 10 % of the attempts of the matrix.

Every figure lands in test_hip_parity's JSON report under "cnf_dopri5:" keys.

Three one-line mutations of csrc/ode_dp5.hip, each of which makes this file fail (tried on the GPU: 25, 30 and 30 of the 32 route-matrix and
contract cases): DP_BETA's 44/45 -> 44/46; DP_SAFETY 0.9 -> 0.8; the slot-order sum starting at slot 1 instead of slot 0.
"""
import math

import numpy as np
import pytest
import torch

from oracle import model as O
from test_hip_parity import REPORT, record
from test_cnf_solve_kernels import (Weights, base_samples, block_params, hyper_of, mbn_f64, mbn_pair, odenet_f64, rnd, LIVE)

X_TOL, LP_TOL = 1e-5, 1e-4
SAFETY, IFACTOR, DFACTOR = 0.9, 10.0, 0.2


# ---------------------------------------------------------------------------------------------
# the replay
# ---------------------------------------------------------------------------------------------
def _rms(x):
    return float(x.norm() / (x.numel() ** 0.5))


def controller(dt, r):
    """torchdiffeq 0.0.1's step-size update on the larger ratio r (plain Python floats)."""
    if r == 0:
        return dt * IFACTOR
    dfac = 1.0 if r < 1 else DFACTOR
    return dt / max(1.0 / IFACTOR, min(math.sqrt(r) ** 0.2 / SAFETY, 1.0 / dfac))


def initial_step(d1, d2, h0):
    h1 = max(1e-6, h0 * 1e-3) if (d1 <= 1e-15 and d2 <= 1e-15) else (0.01 / max(d1, d2)) ** 0.2
    return min(100 * h0, h1)


def replay(func, y0, t0, t1, rtol, atol, dts=None, decisions=None):
    """Dormand-Prince 5(4) attempts on the tuple state y0 from t0 to t1 (t0 > t1: t and f negated, as upstream) in the dtype of y0.
    dts: the step of every attempt (None: the controller's own, starting from the selected initial step); decisions: accept / reject
    per attempt (None: by the ratios).  The run ends with the accepted attempt that reaches t1, interpolated there.
    -> dict(out, ratios [(r_x, r_logp)], accepted [bool], dts, next_dts (the controller's proposal after every attempt), d0, d1, d2,
    h0, dt0, nfe)."""
    sign = -1.0 if t0 > t1 else 1.0
    t, tend = sign * t0, sign * t1
    nfe = [0]

    def f(tt, ys):
        nfe[0] += 1
        return tuple(sign * o for o in func(sign * tt, ys))

    ys = tuple(y0)
    f0 = f(t, ys)
    scale = [atol + y.abs() * rtol for y in ys]
    d0 = max(_rms(y / s) for y, s in zip(ys, scale))
    d1 = max(_rms(k / s) for k, s in zip(f0, scale))
    h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * max(_rms(y / s) / max(_rms(k / s), 1e-300) for y, k, s in zip(ys, f0, scale))
    f1 = f(t + h0, tuple(y + h0 * k for y, k in zip(ys, f0)))
    d2 = max(_rms((b - a) / s) / h0 for a, b, s in zip(f0, f1, scale))
    dt0 = initial_step(d1, d2, h0)
    res = dict(ratios=[], accepted=[], dts=[], next_dts=[], d0=d0, d1=d1, d2=d2, h0=h0, dt0=dt0)
    dt, k = dt0, 0
    while True:
        if dts is not None:
            assert k < len(dts), "the given attempts end before t1 is reached"
            dt = float(dts[k])
        ks = [f0]
        for a, brow in zip(O._DP_ALPHA, O._DP_BETA):
            yi = tuple(y + dt * sum(b * kk[i] for b, kk in zip(brow, ks) if b != 0) for i, y in enumerate(ys))
            ks.append(f(t + a * dt, yi))
        ynew = tuple(y + dt * sum(c * kk[i] for c, kk in zip(O._DP_CSOL, ks) if c != 0) for i, y in enumerate(ys))
        err = tuple(dt * sum(c * kk[i] for c, kk in zip(O._DP_CERR, ks) if c != 0) for i in range(len(ys)))
        ratios = tuple(float(torch.mean((e / (atol + rtol * torch.max(a_.abs(), b_.abs()))) ** 2)) for a_, b_, e in zip(ys, ynew, err))
        accept = all(r <= 1 for r in ratios) if decisions is None else bool(decisions[k])
        res["ratios"].append(ratios)
        res["accepted"].append(accept)
        res["dts"].append(dt)
        res["next_dts"].append(controller(dt, max(ratios)))
        k += 1
        if accept:
            if t + dt >= tend:
                if t + dt == tend:
                    out = ynew
                else:
                    ymid = tuple(y + dt * sum(c * kk[i] for c, kk in zip(O._DP_CMID, ks) if c != 0) for i, y in enumerate(ys))
                    xx = (tend - t) / ((t + dt) - t)
                    out = []
                    for i in range(len(ys)):
                        fa, fb = f0[i], ks[-1][i]
                        A = 2 * dt * (fb - fa) - 8 * (ynew[i] + ys[i]) + 16 * ymid[i]
                        Bc = dt * (5 * fa - 3 * fb) + 18 * ys[i] + 14 * ynew[i] - 32 * ymid[i]
                        C = dt * (fb - 4 * fa) - 11 * ys[i] - 5 * ynew[i] + 16 * ymid[i]
                        out.append((((A * xx + Bc) * xx + C) * xx + dt * fa) * xx + ys[i])
                    out = tuple(out)
                res.update(out=out, nfe=nfe[0])
                return res
            t, ys, f0 = t + dt, ynew, ks[-1]
        dt = res["next_dts"][-1]


def frame_func(hyper_row, tcol, W, e=None):
    """The ODE function of ONE frame on the state (x (1,n,3), logp (1,n,1)) from the kernels' hyper row / tcol columns; with e the
    Hutchinson estimate -e^T J e by forward-mode autograd, without it a zero derivative of logp (oracle.cnf_block)."""
    hy = hyper_row[None, :LIVE]

    def func(t, ys):
        if e is None:
            return odenet_f64(t, ys[0], hy, tcol, W), torch.zeros_like(ys[1])
        dy, je = torch.func.jvp(lambda z: odenet_f64(t, z, hy, tcol, W), (ys[0],), (e,))
        return dy, -(je * e).sum(-1, keepdim=True)
    return func


def frame_problem(W, y, hyper, b, reverse, mbn_in, e, logp, dtype=torch.float64):
    """-> (func, (x0, lp0)) of frame b in `dtype`, after the MovingBatchNorm prologue."""
    d = lambda v: None if v is None else v.detach().cpu().to(dtype)
    Wd = {k: d(W.cpu[k]) for k in ("w0", "b0", "w1", "b1", "w2", "b2", "w3", "b3")}
    x = d(y[b:b + 1])
    lp = d(logp[b:b + 1]) if logp is not None else None
    if mbn_in is not None:
        x, lp = mbn_f64(d(mbn_in), x, lp, reverse)
    if lp is None:
        lp = torch.zeros(1, x.shape[1], 1, dtype=dtype)
    return frame_func(d(hyper[b]), d(W.cpu["tcol"]), Wd, None if e is None else d(e[b:b + 1])), (x, lp)


def oracle_run(func, y0, t0, t1, rtol, atol):
    """oracle.model.dopri5_solve with its evaluation times and ratios captured -> (out, times, ratios per attempt)."""
    times, means = [], []

    def spy(t, ys):
        times.append(float(t))
        return func(t, ys)
    torch.func.jvp(lambda z: 2.0 * z, (torch.zeros(1),), (torch.ones(1),))     # forward-mode AD loads its decompositions on first use: before the patch
    orig = torch.mean

    def mean(x, *a, **k):
        r = orig(x, *a, **k)
        if not a and not k:
            means.append(float(r))
        return r
    torch.mean = mean
    try:
        out = O.dopri5_solve(spy, y0, [t0, t1], rtol, atol)[-1]
    finally:
        torch.mean = orig
    return out, times, list(zip(means[0::2], means[1::2]))


def oracle_dts(times, ratios, t0, t1):
    """The dt of every attempt of an oracle run from its evaluation times: evaluation 2 + 6k + 4 (alpha = 1) is at t_k + dt_k."""
    sign = -1.0 if t0 > t1 else 1.0
    t, dts = sign * t0, []
    for k, r in enumerate(ratios):
        dts.append(sign * times[2 + 6 * k + 4] - t)
        if all(x <= 1 for x in r):
            t = sign * times[2 + 6 * k + 4]
    return dts


def measure_delta(prob32, prob64, t0, t1, rtol, atol, dts, decisions):
    """The same attempts in f32 and f64 oracle arithmetic -> (largest |s32 - s64| over attempts with s64 in [0.5, 2], s64 list, the
    f64 replay)."""
    r32 = replay(*prob32, t0, t1, rtol, atol, dts=dts, decisions=decisions)
    r64 = replay(*prob64, t0, t1, rtol, atol, dts=dts, decisions=decisions)
    worst, s64s = 0.0, []
    for a, b in zip(r32["ratios"], r64["ratios"]):
        s32, s64 = math.sqrt(max(a)), math.sqrt(max(b))
        s64s.append(s64)
        if 0.5 <= s64 <= 2.0:
            worst = max(worst, abs(s32 - s64))
    return worst, s64s, r64


def check_decisions(tag, r64, got, delta, bad, stats, controller_too=True):
    """The decision checks on one frame.  got: dict(dts, accepted, ratios (float32 pairs), d0, d1, d2, h0, dt0) as traced."""
    f32 = np.float32
    for k, (rat, acc) in enumerate(zip(r64["ratios"], got["accepted"])):
        s = math.sqrt(max(rat))
        stats["attempts"] += 1
        stats["undecided"] += int(1 - delta <= s <= 1 + delta)
        if acc and not s <= 1 + delta:
            bad.append("%s: attempt %d accepted at s64 = %.6f > 1 + %.2e" % (tag, k, s, delta))
        if not acc and not s >= 1 - delta:
            bad.append("%s: attempt %d rejected at s64 = %.6f < 1 - %.2e" % (tag, k, s, delta))
        if controller_too and k + 1 < len(got["dts"]):
            r = f32(max(got["ratios"][k]))
            if r == 0:
                want = f32(got["dts"][k]) * f32(IFACTOR)
            else:
                fac = max(f32(1.0 / IFACTOR), min(f32(np.power(np.sqrt(r), f32(0.2))) / f32(SAFETY), f32(1.0) if r < 1 else f32(1.0 / DFACTOR)))
                want = f32(got["dts"][k]) / fac
            if not abs(float(got["dts"][k + 1]) - float(want)) <= 1e-6 * abs(float(want)):
                bad.append("%s: dt after attempt %d is %.9g, the controller gives %.9g" % (tag, k, got["dts"][k + 1], want))
    if not controller_too:
        return
    d1, d2, h0 = f32(got["d1"]), f32(got["d2"]), f32(got["h0"])
    h1 = max(f32(1e-6), h0 * f32(1e-3)) if (d1 <= 1e-15 and d2 <= 1e-15) else f32(np.power(f32(0.01) / max(d1, d2), f32(0.2)))
    want = min(f32(100) * h0, h1)
    if not (abs(float(got["dt0"]) - float(want)) <= 1e-6 * float(want) and got["dt0"] == got["dts"][0]):
        bad.append("%s: first dt %.9g (trace row 0: %.9g), the formula gives %.9g" % (tag, got["dt0"], got["dts"][0], want))
    for nm in ("d0", "d1", "h0"):
        if not abs(got[nm] - r64[nm]) <= 1e-4 * abs(r64[nm]):
            bad.append("%s: %s = %.8g, f64 %.8g" % (tag, nm, got[nm], r64[nm]))


def report(key, **kw):
    REPORT["cnf_dopri5:" + key] = kw
    record("cnf_dopri5:%s:recorded" % key, 0, 0, 0)


# ---------------------------------------------------------------------------------------------
# 1. CPU: the replay is the oracle's solver; the checks run on the oracle's f32 run in place of the kernel
# ---------------------------------------------------------------------------------------------
class CpuWeights:
    def __init__(self, sd):
        P32 = block_params(sd, torch.float32)
        self.P64 = block_params(sd)
        self.cpu = {k: P32[k] for k in ("tcol", "w0", "b0", "w1", "b1", "w2", "b2", "w3", "b3")}
        self.t_end = float(np.float32(P32["t_end"]))

    def hyper(self, c, ldh=LIVE):
        out = torch.full((c.shape[0], ldh), float("nan"), dtype=torch.float32)
        out[:, :LIVE] = hyper_of(self.P64, c).float()
        return out


@pytest.mark.parametrize("which,reverse,div", [("seeded", True, False), ("stress", True, False), ("stress", False, True)])
def test_replay_is_the_oracle_solver(which, reverse, div, seeded_sd, stress_sd):
    """replay() fed the dt's of oracle.model.dopri5_solve reproduces its result, ratios and decisions to 1e-12 (f64); free-running it
    takes the same steps.  The f64 free run has no attempt near s = 1 on these seeds.  Then the GPU test's state and accept / reject
    checks run on the oracle's F32 free run in the kernel's place (the f32 oracle keeps dt in f64, so the controller check, which is
    about f32 arithmetic, has nothing to look at there)."""
    W = CpuWeights(seeded_sd if which == "seeded" else stress_sd)
    BT, n, tol = 2, 96, 1e-5
    c, y = rnd(11, BT, 1600, scale=0.5), rnd(12, BT, n, 3, scale=1.3)
    e, lp0 = (rnd(13, BT, n, 3), rnd(14, BT, n, 1)) if div else (None, None)
    hyper = W.hyper(c)
    t0, t1 = (W.t_end, 0.0) if reverse else (0.0, W.t_end)
    bad, stats = [], dict(attempts=0, undecided=0)
    for b in range(BT):
        p64 = frame_problem(W, y, hyper, b, reverse, None, e, lp0)
        out, times, ratios = oracle_run(*p64, t0, t1, tol, tol)
        dts = oracle_dts(times, ratios, t0, t1)
        r = replay(*p64, t0, t1, tol, tol, dts=dts)
        assert len(r["ratios"]) == len(ratios) and r["nfe"] == len(times) == 2 + 6 * len(ratios)
        assert r["accepted"] == [all(x <= 1 for x in rr) for rr in ratios]
        for i in range(2):
            assert float((r["out"][i] - out[i]).abs().max()) <= 1e-12 * max(1.0, float(out[i].abs().max()))
        for ra, rb in zip(r["ratios"], ratios):
            assert all(abs(u - v) <= 1e-12 * max(1.0, abs(v)) for u, v in zip(ra, rb)), (ra, rb)
        free = replay(*p64, t0, t1, tol, tol)
        assert free["accepted"] == r["accepted"] and all(abs(u - v) <= 1e-12 * v for u, v in zip(free["dts"], dts))
        s64 = [math.sqrt(max(rr)) for rr in ratios]
        assert not any(0.99 <= s <= 1.01 for s in s64), "an attempt of the f64 free run decides nothing: %s" % s64
        # the oracle's f32 run in the kernel's place
        p32 = frame_problem(W, y, hyper, b, reverse, None, e, lp0, torch.float32)
        out32, times32, ratios32 = oracle_run(*p32, t0, t1, tol, tol)
        dts32 = oracle_dts(times32, ratios32, t0, t1)
        acc32 = [all(x <= 1 for x in rr) for rr in ratios32]
        w, _, r64 = measure_delta(p32, p64, t0, t1, tol, tol, dts32, acc32)
        check_decisions("%s frame %d" % (which, b), r64, dict(accepted=acc32), 4 * w, bad, stats, controller_too=False)
        for i, tl in ((0, X_TOL), (1, LP_TOL)):
            err = float((out32[i].double() - r64["out"][i]).abs().max())
            if not err <= tl * max(1.0, float(r64["out"][i].abs().max())):
                bad.append("%s frame %d: f32 oracle vs its f64 replay, tensor %d: %.3e" % (which, b, i, err))
    assert stats["undecided"] <= 0.1 * stats["attempts"]
    assert not bad, "\n".join(bad)


def test_controller_formulas():
    """The two scalar formulas the decision checks apply, on hand-made numbers."""
    assert controller(0.1, 0.0) == 1.0
    assert abs(controller(0.1, 1e-20) - 1.0) < 1e-12                    # growth is capped at 10
    assert abs(controller(0.1, 4.0) - 0.1 / (2.0 ** 0.2 / 0.9)) < 1e-12
    assert abs(controller(0.1, 1e12) - 0.02) < 1e-12                    # shrink is capped at 0.2
    assert initial_step(2.0, 3.0, 1e-4) == 1e-2 and abs(initial_step(2.0, 3.0, 1.0) - (0.01 / 3.0) ** 0.2) < 1e-12


def test_abi_and_option_surface():
    """The header declares the two entry points, lib.py binds them, and the model takes the option without a GPU."""
    import os
    from caspr_amd import lib
    from caspr_amd.models import CaSPR
    from caspr_amd.models.flow import PointCNFArgs
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "caspr_hip.h")).read()
    for name in ("caspr_cnf_dopri5_ws_bytes", "caspr_cnf_dopri5_f32"):
        assert name + "(" in hdr and name in lib.SIGNATURES
    assert len(lib.SIGNATURES["caspr_cnf_dopri5_f32"][1]) == 31
    assert PointCNFArgs().method == "rk4" and PointCNFArgs(method="dopri5").method == "dopri5"
    m = CaSPR(cnf_method="dopri5", cnf_atol=1e-4, cnf_rtol=1e-6)
    blk = m.point_cnf.chain[1]
    assert (blk.method, blk.test_atol, blk.test_rtol) == ("dopri5", 1e-4, 1e-6)
    assert CaSPR().point_cnf.chain[1].method == "rk4" and sorted(CaSPR().state_dict()) == sorted(m.state_dict())
    with pytest.raises(ValueError):
        CaSPR(cnf_method="euler")


# ---------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights(dev, seeded_sd, stress_sd):
    return {"seeded": Weights(seeded_sd, dev), "stress": Weights(stress_sd, dev)}


def solve(W, y, hyper, rtol, atol, reverse, mbn_in=None, mbn_out=None, e=None, logp=None, max_attempts=1000):
    """One ops.cnf_dopri5 call with the trace -> (x, logp | None, info) on the CPU."""
    from caspr_amd import ops
    g = lambda v: None if v is None else v.to("cuda:0").contiguous()
    D = W.dev
    res = ops.cnf_dopri5(g(y), g(hyper), D["tcol"], D["w0"], D["b0"], D["b1"], D["b2"], D["w3"], D["b3"], W.w1x, W.w2x, W.t_end, rtol, atol,
                         reverse, g(mbn_in), g(mbn_out), e=g(e), logp=g(logp), max_attempts=max_attempts, return_trace=True)
    torch.cuda.synchronize()
    info = {k: v.cpu() for k, v in res[-1].items()}
    return res[0].cpu(), (res[1].cpu() if e is not None else None), info


def traced(info, b):
    """Frame b's attempts out of the trace, as check_decisions takes them."""
    k = int(info["accepted"][b]) + int(info["rejected"][b])
    rows = info["attempts"][b, :k].double().numpy()
    return dict(dts=[float(v) for v in rows[:, 1]], accepted=[bool(v) for v in rows[:, 4]], ratios=[(np.float32(r[2]), np.float32(r[3])) for r in rows],
                t=[float(v) for v in rows[:, 0]], d0=float(info["d0"][b]), d1=float(info["d1"][b]), d2=float(info["d2"][b]), h0=float(info["h0"][b]),
                dt0=float(info["dt0"][b]), nfe=int(info["nfe"][b]))


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


N_EDGES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 1000)
MBNS = ("both", "in", "out", "none")
LDHS = (3078, 3091, 3080)


def _cases():
    """Both variants see every n edge; (direction, MBN) cycle with period 8 along the list, ldh, BT and the weight set cycle too."""
    out = []
    for div in (False, True):
        for i, n in enumerate(N_EDGES):
            j = i + (3 if div else 0)
            BT = 17 if n == (65 if not div else 31) else (5 if (i % 2 and n < 257) else 1)
            out.append(dict(div=div, n=n, BT=BT, reverse=j % 2 == 0, mbn=MBNS[(j // 2) % 4], ldh=LDHS[i % 3], w="seeded" if i % 4 == 3 else "stress"))
    return out


CASES = _cases()
MATRIX = dict(attempts=0, undecided=0, worst_s_diff=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["%s-n%d-bt%d-%s-mbn_%s-ldh%d-%s" % ("div" if c["div"] else "nodiv", c["n"], c["BT"], "rev" if c["reverse"] else "fwd",
                                                                                   c["mbn"], c["ldh"], c["w"]) for c in CASES])
def test_route_matrix(dev, weights, case):
    """State and decisions of every frame against the f64 replay of the kernel's own attempts; the launch twice, bit for bit."""
    W = weights[case["w"]]
    BT, n, reverse, div, tol = case["BT"], case["n"], case["reverse"], case["div"], 1e-5
    seed = 2000 + n
    c, y = rnd(seed, BT, 1600, scale=0.5), base_samples(seed + 1, BT, n)
    e, lp0 = (rnd(seed + 2, BT, n, 3), rnd(seed + 3, BT, n, 1)) if div else (None, None)
    hyper = W.hyper(c, case["ldh"])
    mi, mo = mbn_pair(reverse, case["mbn"])
    x, lp, info = solve(W, y, hyper, tol, tol, reverse, mi, mo, e, lp0)
    x2, lp2, info2 = solve(W, y, hyper, tol, tol, reverse, mi, mo, e, lp0)
    bad = []
    if not (same_bits(x, x2) and (lp is None or same_bits(lp, lp2)) and all(same_bits(info[k].float(), info2[k].float()) for k in info)):
        bad.append("two launches differ in their bits")
    t0, t1 = (W.t_end, 0.0) if reverse else (0.0, W.t_end)
    stats = dict(attempts=0, undecided=0)
    frames = range(BT) if BT <= 5 else (0, 7, BT - 1)          # (17 frames: three of them replayed; all of them launched)
    for b in frames:
        got = traced(info, b)
        if got["nfe"] != 2 + 6 * len(got["dts"]):
            bad.append("frame %d: %d evaluations counted for %d attempts" % (b, got["nfe"], len(got["dts"])))
        p64 = frame_problem(W, y, hyper, b, reverse, mi, e, lp0)
        p32 = frame_problem(W, y, hyper, b, reverse, mi, e, lp0, torch.float32)
        worst, _, r64 = measure_delta(p32, p64, t0, t1, tol, tol, got["dts"], got["accepted"])
        MATRIX["worst_s_diff"] = max(MATRIX["worst_s_diff"], worst)
        delta = 4 * worst
        print("frame %d: %d attempts, %d rejected, |s32 - s64| max %.3e, s64 %s" % (b, len(got["dts"]), got["accepted"].count(False), worst,
                                                                                      ["%.4f" % math.sqrt(max(r)) for r in r64["ratios"]]))
        check_decisions("frame %d" % b, r64, got, delta, bad, stats)
        ox, olp = r64["out"]
        if mo is not None:
            ox, olp = mbn_f64(mo.double(), ox, olp, reverse)
        for nm, g_, w_, tl in (("x", x[b:b + 1], ox, X_TOL), ("logp", lp[b:b + 1] if div else None, olp, LP_TOL)):
            if g_ is None:
                continue
            scale = max(1.0, float(w_.abs().max()))
            err = float((g_.double() - w_).abs().max())
            key = "cnf_dopri5:matrix:%s-n%d-bt%d:frame%d:%s" % ("div" if div else "nodiv", n, BT, b, nm)
            REPORT[key] = {"max_abs_err": err, "bound": tl * scale, "attempts": len(got["dts"]), "kernel": "cnf_dp5_kernel<%s>" % str(div).lower()}
            print("  %s: max abs err %.3e, bound %.3e" % (nm, err, tl * scale))
            if not (bool(torch.isfinite(g_).all()) and err <= tl * scale):
                bad.append("frame %d %s: max abs err %.3e > %.1e x %.3g" % (b, nm, err, tl, scale))
    MATRIX["attempts"] += stats["attempts"]
    MATRIX["undecided"] += stats["undecided"]
    report("matrix:totals", attempts=MATRIX["attempts"], undecided=MATRIX["undecided"], worst_s32_minus_s64=MATRIX["worst_s_diff"],
           delta=4 * MATRIX["worst_s_diff"])
    assert MATRIX["undecided"] <= 0.1 * max(MATRIX["attempts"], 10), "attempts that decide nothing: %d of %d" % (MATRIX["undecided"], MATRIX["attempts"])
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["seeded", "stress"])
def test_tolerance_is_honoured(dev, weights, which):
    """Tightening rtol = atol (1e-4, 1e-5, 1e-6) moves the result towards the converged f64 solution (RK4, 256 steps, f64)
    monotonically; the distance at 1e-5 is recorded beside the f64 oracle's own (no bound on it).
    Monotone as far as an f32 output can show it: two distances are told apart only when they differ by more than one unit in the
    last place of the largest coordinate (2^-23 |x|max, 4.8e-7 at |x| = 5).  Measured on the seeded weights, where the solve is at the
    f32 floor already at 1e-4: 3.62e-7, 4.63e-7, 3.57e-7 (1e-4, 1e-5, 1e-6) -- differences of 1e-7, a fifth of that unit; on the
    stress weights the distances fall strictly."""
    from test_cnf_solve_kernels import reference
    W = weights[which]
    BT, n = 3, 200
    c, y = rnd(31, BT, 1600, scale=0.5), base_samples(32, BT, n)
    hyper = W.hyper(c, 3080)
    conv, _ = reference(W, y, hyper, 256, True)
    dist = {}
    for tol in (1e-4, 1e-5, 1e-6):
        x, _, info = solve(W, y, hyper, tol, tol, True)
        dist[tol] = float((x.double() - conv).abs().max())
        print("%s tol %.0e: distance %.3e, nfe %s" % (which, tol, dist[tol], info["nfe"].tolist()))
    own = 0.0
    for b in range(BT):
        p64 = frame_problem(W, y, hyper, b, True, None, None, None)
        out = O.dopri5_solve(p64[0], p64[1], [W.t_end, 0.0], 1e-5, 1e-5)[-1]
        own = max(own, float((out[0] - conv[b:b + 1]).abs().max()))
    report("contract:%s" % which, distance_1e4=dist[1e-4], distance_1e5=dist[1e-5], distance_1e6=dist[1e-6], f64_oracle_distance_1e5=own)
    ulp = 2.0 ** -23 * float(conv.abs().max())
    report("contract:%s:resolution" % which, f32_ulp_at_absmax=ulp)
    assert dist[1e-4] + ulp >= dist[1e-5] and dist[1e-5] + ulp >= dist[1e-6] and dist[1e-4] + ulp >= dist[1e-6], (dist, ulp)


@pytest.mark.gpu
@pytest.mark.parametrize("div", [False, True])
def test_a_frame_does_not_depend_on_its_batch(dev, weights, div):
    """Output, trace and counters of a frame: alone, inside a batch, under a permutation of the frames, on a second stream."""
    W = weights["stress"]
    BT, n = 6, 150
    c, y = rnd(41, BT, 1600, scale=0.5), base_samples(42, BT, n)
    e, lp0 = (rnd(43, BT, n, 3), rnd(44, BT, n, 1)) if div else (None, None)
    hyper = W.hyper(c, 3080)
    mi, mo = mbn_pair(not div, "both")
    sub = lambda v, idx: None if v is None else v[idx].contiguous()
    x, lp, info = solve(W, y, hyper, 1e-5, 1e-5, not div, mi, mo, e, lp0)
    perm = torch.tensor([4, 2, 5, 0, 3, 1])
    xp, lpp, infop = solve(W, y[perm], hyper[perm], 1e-5, 1e-5, not div, mi, mo, sub(e, perm), sub(lp0, perm))
    with torch.cuda.stream(torch.cuda.Stream()):
        xs, lps, infos = solve(W, y, hyper, 1e-5, 1e-5, not div, mi, mo, e, lp0)
    bad = []
    for k in info:
        if not same_bits(info[k].float(), infos[k].float()):
            bad.append("second stream: %s differs" % k)
        if not same_bits(info[k][perm].float(), infop[k].float()):
            bad.append("permutation: %s differs" % k)
    if not (same_bits(x, xs) and same_bits(x[perm], xp) and (not div or (same_bits(lp, lps) and same_bits(lp[perm], lpp)))):
        bad.append("outputs differ under a permutation / on a second stream")
    for b in (0, 3, 5):
        i = torch.tensor([b])
        x1, lp1, info1 = solve(W, y[i], hyper[i], 1e-5, 1e-5, not div, mi, mo, sub(e, i), sub(lp0, i))
        if not (same_bits(x1, x[i]) and (not div or same_bits(lp1, lp[i])) and all(same_bits(info1[k].float(), info[k][i].float()) for k in info)):
            bad.append("frame %d alone differs from the frame inside the batch" % b)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_attempt_budget_and_bad_arguments(dev, weights):
    """max_attempts = 3 on the stress weights: the error status, raised -- nothing hangs.  Bad arguments raise as in ops.cnf_rk4."""
    from caspr_amd import ops
    from caspr_amd.lib import CasprHipError
    W = weights["stress"]
    BT, n = 2, 100
    c, y = rnd(51, BT, 1600, scale=0.5), base_samples(52, BT, n)
    hyper = W.hyper(c, 3080)
    with pytest.raises(CasprHipError, match="max_attempts"):
        solve(W, y, hyper, 1e-6, 1e-6, True, max_attempts=3)
    x, _, info = solve(W, y, hyper, 1e-5, 1e-5, True)            # the library is still usable afterwards
    assert bool(torch.isfinite(x).all()) and int((info["accepted"] + info["rejected"]).max()) > 3
    D = W.dev
    yd, hd = y.to(dev), hyper.to(dev)
    call = lambda y_=yd, h_=hd, rtol=1e-5, atol=1e-5, **kw: ops.cnf_dopri5(y_, h_, D["tcol"], D["w0"], D["b0"], D["b1"], D["b2"], D["w3"], D["b3"], W.w1x, W.w2x,
                                                                        W.t_end, rtol, atol, True, **kw)
    with pytest.raises(ValueError):
        call(y_=yd[:, :, :2].contiguous())
    with pytest.raises(ValueError):
        call(h_=hd[:1])
    with pytest.raises(ValueError):
        call(e=torch.zeros_like(yd))
    with pytest.raises(ValueError):
        call(mbn_in=torch.zeros(11, device=dev))
    with pytest.raises(ValueError):
        call(rtol=0.0)
    with pytest.raises(ValueError):
        call(atol=float("nan"))
    with pytest.raises(ValueError):
        call(max_attempts=0)
    with pytest.raises(ValueError):
        ops.cnf_dopri5(yd, hd, D["tcol"], D["w0"], D["b0"], D["b1"], D["b2"], D["w3"], D["b3"], None, None, W.t_end, 1e-5, 1e-5, True)


@pytest.mark.gpu
def test_model_surface(dev, seeded_sd, monkeypatch):
    """CaSPR(cnf_method="dopri5") loads the same state_dict; reconstruct() is ops.cnf_dopri5 on the same y / z; get_nfe() is the trace's
    maximum; the guard launches no check solve for the block; with grad enabled the option raises."""
    import warnings
    from caspr_amd import ops
    from caspr_amd.models import CaSPR
    from caspr_amd.utils.synthetic import dense_sequences
    m = CaSPR(cnf_method="dopri5", cnf_atol=1e-5, cnf_rtol=1e-5)
    m.load_state_dict(seeded_sd)
    m = m.to(dev).eval()
    assert m.point_cnf.chain[1].method == "dopri5"
    x, sp = dense_sequences(1, 3, 1024)
    y = rnd(61, 1, 3, 200, 3).to(dev)
    ts = sp[0, :, 0, 3].to(dev)

    def no_rk4(*a, **k):
        raise AssertionError("a dopri5 block must not launch an RK4 (check) solve")
    monkeypatch.setattr(ops, "cnf_rk4", no_rk4)
    with torch.no_grad(), warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _, _, gx, _ = m.reconstruct(x.to(dev), num_points=200, timestamps=ts, y=y)
        ops.check_deferred_errors()
        torch.cuda.synchronize()
    assert not [w for w in caught if "point CNF" in str(w.message)], [str(w.message) for w in caught]
    blk = m.point_cnf.chain[1]
    nfe = blk.last_nfe_per_frame.cpu()
    assert int(m.get_nfe()[1]) == int(nfe.max()) and nfe.shape == (3,) and int(nfe.min()) >= 8
    with torch.no_grad():
        z0, _ = m.encode(x.to(dev))
        z = m.aggregate_and_solve_latent(z0, ts.view(1, -1))
        w = blk._weights()
        hyper = ops.conv1x1(w["hyp"], w["hyp_bias"], z.reshape(1, 3, -1).contiguous(), row_invariant=True)[0]
        w1x, w2x = blk._weights_x6()
        want, info = ops.cnf_dopri5(y.view(3, 200, 3), hyper, w["tcol"], w["w0"], w["b0"], w["b1"], w["b2"], w["w3"], w["b3"], w1x, w2x, blk.end_time(),
                                    1e-5, 1e-5, True, m.point_cnf.chain[2].kernel_params(), m.point_cnf.chain[0].kernel_params(), return_trace=True)
    assert same_bits(gx.view(3, 200, 3).cpu(), want.cpu()) and info["nfe"].cpu().tolist() == nfe.tolist()
    with pytest.raises(ValueError, match="dopri5"):
        m.point_cnf(y.view(3, 200, 3), z.reshape(3, -1), reverse=True)           # grad enabled
