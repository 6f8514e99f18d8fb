"""The adaptive Dormand-Prince solve of the latent ODE (ops.latent_dopri5, csrc/ode_latent_dp5.hip, include/caspr_hip.h:
caspr_latent_dopri5_f32): one launch, the step control on the device, error control per sequence.

A free-running comparison cannot be the test: on the stress weights at 1e-6 the oracle's own dopri5 takes different step sequences in
f32 and in f64 (evaluations [74,68,74,68,62,80] against [74,68,68,68,80,80] on six sequences).  As for the point CNF
(test_cnf_dopri5.py) the kernel is checked against ITS OWN traced attempts replayed in f64:

  * replay(): f64 Dormand-Prince attempts at GIVEN dt's (and, optionally, given decisions) on oracle.model.dynamics, with outputs at
    every requested stamp by the reference's rule (steps are not clipped: the 4th-order interpolant inside the step, y_new at its
    end, z0 at stamps equal to times[0]) -- pinned on the CPU to oracle.model.dopri5_solve: fed the oracle's dt's it reproduces the
    oracle's result at every stamp, ratios and decisions to 1e-12;
  * state: per sequence, every output stamp is within 1e-5 x max(1, |z|max) of the replay of the kernel's traced dt's and decisions
    (the bound the suite holds the latent RK4 kernels to against f64: stress_latent_rk4_*, latent_team_vs_oracle; same evaluation body);
  * decisions: with s = sqrt(ratio) of the f64 replay, accepted attempts have s <= 1 + delta, rejected ones s >= 1 - delta; the next
    traced dt is the controller formula on the traced ratio, the first dt the initial-step formula on the traced d1 / d2 / h0 (f32,
    1e-6 relative); d0, d1, h0 match f64 to 1e-4 relative;
  * delta is measured WITHOUT the kernel: the same attempts replayed with the oracle arithmetic in f32 and f64, 4 x the largest
    |s32 - s64| over attempts with s64 in [0.5, 2];
  * attempts whose s64 lies inside [1 - delta, 1 + delta] decide nothing: at most 10 % of the attempts of the matrix, which must also
    hold at least one rejected attempt.

  * a second matrix (WIDTHS) holds the same criterion at the other widths the kernel accepts -- (D, H) = (20, 512), (33, 256), (64, 64),
    (1, 64) on the nets of test_latent_widths.py -- with totals and a 10 % cap of its own; that its tolerance and horizon produce
    rejected attempts is checked on the CPU, on the oracle's f32 run.

Every figure lands in test_hip_parity's JSON report under "latent_dopri5:" keys.

Three one-line mutations of csrc/ode_latent_dp5.hip, each of which makes this file fail (tried on the GPU: each breaks 10 of the 20
route-matrix cases; eight of the others hold one stamp or all-equal stamps and make no attempt):
LDP_BETA's 44/45 -> 44/46; LDP_SAFETY 0.9 -> 0.8; the first mid-point weight of LDP_CMID halved by 3 instead of 2.
"""
import math
import os
import types

import numpy as np
import pytest
import torch

from oracle import model as O
from test_hip_parity import REPORT, record
from test_cnf_dopri5 import check_decisions, controller, initial_step, same_bits
from test_latent_widths import module, net

Z_TOL = 1e-5
PRE = "latent_ode.ode_func.dynamics_net"
BASE_STAMPS = [0.0, 0.0, 0.05, 0.1, 0.1, 0.35, 0.5, 0.8, 1.0]       # a stamp equal to times[0], a repeat, 0.05 / 0.1 inside the first steps
# (D, H) next to the models' (64, 512), on the nets of test_latent_widths.py (non-zero biases on all four layers): a ragged K chunk of
# layer 0 and RTD = 2 row tiles of the output layer; RTD = 3 and KCH = 16 < 32 chunks; seven of the eight waves without a row tile;
# one component, so that the `/ D` of the error norms divides by 1
WIDTHS = [(20, 512), (33, 256), (64, 64), (1, 64)]


def width_name(D, H):
    return "D%dH%d" % (D, H)


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def sequences(seed, B, D=64):
    """z0 = 0.5 .. 2.0 x randn, the scale cycling along the batch."""
    scales = torch.tensor([0.5, 0.8, 1.1, 1.4, 1.7, 2.0])[torch.arange(B) % 6]
    return rnd(seed, B, D) * scales[:, None]


def stamps(horizon, t_first=0.0, base=BASE_STAMPS):
    return torch.tensor([t_first + horizon * b for b in base], dtype=torch.float32)


def rel_of(times):
    """The solver's times: relative to times[0], in the f32 arithmetic of latent_ode_model.py:58, as Python floats."""
    return [float(v) for v in (times.float() - times.float()[0]).double()]


def dyn_sd(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items() if k.startswith(PRE)}


def problem(sd, z0row, dtype=torch.float64):
    """-> (f, z0) of ONE sequence in `dtype` (the dynamics are autonomous)."""
    w = dyn_sd(sd, dtype)
    return (lambda z: O.dynamics(w, z)), z0row.detach().cpu().reshape(1, -1).to(dtype)


# ---------------------------------------------------------------------------------------------
# the replay
# ---------------------------------------------------------------------------------------------
def _rms(x):
    return float(x.norm() / (x.numel() ** 0.5))


def replay(f, z0, rel, rtol, atol, dts=None, decisions=None):
    """Dormand-Prince 5(4) attempts on the one-tensor state z0 with outputs at every time of `rel` (ascending, rel[0] == 0, repeats
    allowed) in the dtype of z0.  dts: the step of every attempt (None: the controller's own, from the selected initial step);
    decisions: accept / reject per attempt (None: by the ratio).
    -> dict(out [per stamp], ratios [(r,)], accepted, dts, next_dts, t [attempt start], d0, d1, d2, h0, dt0, nfe)."""
    nfe = [0]

    def F(z):
        nfe[0] += 1
        return f(z)

    z, t = z0, rel[0]
    f0 = F(z)
    scale = atol + z.abs() * rtol
    d0, d1 = _rms(z / scale), _rms(f0 / scale)
    h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * (d0 / max(d1, 1e-300))
    f1 = F(z + h0 * f0)
    d2 = _rms((f1 - f0) / scale) / h0
    dt0 = initial_step(d1, d2, h0)
    res = dict(ratios=[], accepted=[], dts=[], next_dts=[], t=[], d0=d0, d1=d1, d2=d2, h0=h0, dt0=dt0)
    out, interp, t0s, t1s, dt, k = [z], None, t, t, dt0, 0
    for tn in rel[1:]:
        while tn > t1s:
            if dts is not None:
                assert k < len(dts), "the given attempts end at t = %.9g, before the stamp %.9g" % (t1s, tn)
                dt = float(dts[k])
            ks = [f0]
            for brow in O._DP_BETA:
                ks.append(F(z + dt * sum(b * kk for b, kk in zip(brow, ks) if b != 0)))
            znew = z + dt * sum(c * kk for c, kk in zip(O._DP_CSOL, ks) if c != 0)
            err = dt * sum(c * kk for c, kk in zip(O._DP_CERR, ks) if c != 0)
            r = float(torch.mean((err / (atol + rtol * torch.max(z.abs(), znew.abs()))) ** 2))
            accept = r <= 1 if decisions is None else bool(decisions[k])
            res["ratios"].append((r,))
            res["accepted"].append(accept)
            res["dts"].append(dt)
            res["t"].append(t)
            res["next_dts"].append(controller(dt, r))
            k += 1
            if accept:
                zmid = z + dt * sum(c * kk for c, kk in zip(O._DP_CMID, ks) if c != 0)
                fa, fb = f0, ks[-1]
                interp = (2 * dt * (fb - fa) - 8 * (znew + z) + 16 * zmid, dt * (5 * fa - 3 * fb) + 18 * z + 14 * znew - 32 * zmid,
                          dt * (fb - 4 * fa) - 11 * z - 5 * znew + 16 * zmid, dt * fa, z)
                t0s, t1s = t, t + dt
                t, z, f0 = t + dt, znew, ks[-1]
            dt = res["next_dts"][-1]
        if interp is None or tn == t1s:
            out.append(z)
        else:
            xx = (tn - t0s) / (t1s - t0s)
            A, Bc, C, D, E = interp
            out.append((((A * xx + Bc) * xx + C) * xx + D) * xx + E)
    res.update(out=out, nfe=nfe[0])
    return res


def oracle_run(f, z0, rel, rtol, atol):
    """oracle.model.dopri5_solve on the one-tensor state with its evaluation times, ratios and dt's captured -> (out per stamp, times,
    ratios, dts).  The dt's are the oracle's own to the bit: its initial step from the norms it computed (h0 is the time of its second
    evaluation, rel[0] being 0), then its controller formula on its ratios (differences of evaluation times would lose the last bits)."""
    times, means, norms = [], [], []

    def spy(t, ys):
        times.append(float(t))
        return (f(ys[0]),)
    orig = torch.mean

    def mean(x, *a, **k):
        r = orig(x, *a, **k)
        if not a and not k:
            means.append(float(r))
        return r
    orig_rms = O._rms

    def rms(x):
        norms.append(orig_rms(x))
        return norms[-1]
    torch.mean, O._rms = mean, rms
    try:
        out = O.dopri5_solve(spy, (z0,), rel, rtol, atol)
    finally:
        torch.mean, O._rms = orig, orig_rms
    h0 = times[1] - rel[0]
    dts = [initial_step(norms[1], norms[-1] / h0, h0)]           # _rms calls: d0, d1, (two for h0,) d2
    for m in means[:-1]:
        dts.append(controller(dts[-1], m))
    return [o[0] for o in out], times, [(m,) for m in means], dts[:len(means)]


def measure_delta(p32, p64, rel, rtol, atol, dts, decisions):
    """The same attempts in f32 and f64 oracle arithmetic -> (largest |s32 - s64| over attempts with s64 in [0.5, 2], the f64 replay)."""
    r32 = replay(*p32, rel, rtol, atol, dts=dts, decisions=decisions)
    r64 = replay(*p64, rel, rtol, atol, dts=dts, decisions=decisions)
    worst = 0.0
    for a, b in zip(r32["ratios"], r64["ratios"]):
        s32, s64 = math.sqrt(a[0]), math.sqrt(b[0])
        if 0.5 <= s64 <= 2.0:
            worst = max(worst, abs(s32 - s64))
    return worst, r64


def check_state(tag, got_rows, r64, bad, key=None):
    """Every output stamp of one sequence (Tu, D) against the f64 replay: 1e-5 x max(1, |z|max)."""
    want = torch.cat(r64["out"], 0)
    scale = max(1.0, float(want.abs().max()))
    err = float((got_rows.double() - want).abs().max()) if bool(torch.isfinite(got_rows).all()) else float("inf")
    if key is not None:
        REPORT[key] = {"max_abs_err": err, "bound": Z_TOL * scale, "attempts": len(r64["dts"]), "kernel": "latent_dp5_kernel"}
    print("  %s: max abs err %.3e, bound %.3e" % (tag, err, Z_TOL * scale))
    if not err <= Z_TOL * scale:
        bad.append("%s: max abs err over the stamps %.3e > %.1e x %.3g" % (tag, err, Z_TOL, scale))


def check_head(tag, r64, got, bad):
    """A solve without attempts (every stamp equals times[0]): the initial-step figures alone."""
    f32 = np.float32
    d1, d2, h0 = f32(got["d1"]), f32(got["d2"]), f32(got["h0"])
    h1 = max(f32(1e-6), h0 * f32(1e-3)) if (d1 <= 1e-15 and d2 <= 1e-15) else f32(np.power(f32(0.01) / max(d1, d2), f32(0.2)))
    want = min(f32(100) * h0, h1)
    if not abs(float(got["dt0"]) - float(want)) <= 1e-6 * float(want):
        bad.append("%s: first dt %.9g, the formula gives %.9g" % (tag, got["dt0"], want))
    for nm in ("d0", "d1", "h0"):
        if not abs(got[nm] - r64[nm]) <= 1e-4 * abs(r64[nm]):
            bad.append("%s: %s = %.8g, f64 %.8g" % (tag, nm, got[nm], r64[nm]))


def report(key, **kw):
    REPORT["latent_dopri5:" + key] = kw
    record("latent_dopri5:%s:recorded" % key, 0, 0, 0)


# ---------------------------------------------------------------------------------------------
# 1. CPU: the replay is the oracle's solver; the checks run on the oracle's f32 run in place of the kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,tol,horizon,t_first", [("seeded", 1e-3, 1.0, 0.0), ("seeded", 1e-6, 3.0, 0.25), ("stress", 1e-3, 3.0, 0.25),
                                                        ("stress", 1e-6, 1.0, 0.0)])
def test_replay_is_the_oracle_solver(which, tol, horizon, t_first, seeded_sd, stress_sd):
    """replay() fed the dt's of oracle.model.dopri5_solve reproduces its result at every stamp, ratios and decisions to 1e-12 (f64);
    free-running it takes the same steps.  The stamps hold a repeat, a stamp equal to times[0] and several stamps inside one accepted
    step.  Then the GPU test's state and accept / reject checks run on the oracle's F32 free run in the kernel's place (the f32 oracle
    keeps dt in f64, so the controller check, which is about f32 arithmetic, has nothing to look at there)."""
    sd = seeded_sd if which == "seeded" else stress_sd
    z0 = sequences(71, 6)
    rel = rel_of(stamps(horizon, t_first))
    assert rel[1] == 0.0 and rel[3] == rel[4]
    bad, stats, several = [], dict(attempts=0, undecided=0), False
    for b in range(6):
        p64, p32 = problem(sd, z0[b]), problem(sd, z0[b], torch.float32)
        out, times, ratios, dts = oracle_run(*p64, rel, tol, tol)
        assert all(abs(times[2 + 6 * k + 4] - (t_ + d_)) <= 1e-12 for k, (t_, d_) in enumerate(zip(replay(*p64, rel, tol, tol, dts=dts)["t"], dts)))
        r = replay(*p64, rel, tol, tol, dts=dts)
        assert len(r["ratios"]) == len(ratios) and r["nfe"] == len(times) == 2 + 6 * len(ratios)
        assert r["accepted"] == [x[0] <= 1 for x in ratios]
        assert len(r["out"]) == len(out) == len(rel)
        for i, (u, v) in enumerate(zip(r["out"], out)):
            assert float((u - v).abs().max()) <= 1e-12 * max(1.0, float(v.abs().max())), "stamp %d" % i
        assert bool((r["out"][1] == p64[1]).all()) and bool((r["out"][3] == r["out"][4]).all())
        for ra, rb in zip(r["ratios"], ratios):
            assert abs(ra[0] - rb[0]) <= 1e-12 * max(1.0, abs(rb[0])), (ra, rb)
        free = replay(*p64, rel, tol, tol)
        assert free["accepted"] == r["accepted"] and all(abs(u - v) <= 1e-12 * v for u, v in zip(free["dts"], dts))
        ends = [t + d for t, d, a in zip(r["t"], r["dts"], r["accepted"]) if a]
        several = several or any(sum(1 for x in set(rel) if lo < x < hi) >= 2 for lo, hi in zip([0.0] + ends[:-1], ends))
        # the oracle's f32 run in the kernel's place
        out32, times32, ratios32, dts32 = oracle_run(*p32, rel, tol, tol)
        acc32 = [x[0] <= 1 for x in ratios32]
        w, r64 = measure_delta(p32, p64, rel, tol, tol, dts32, acc32)
        check_decisions("%s sequence %d" % (which, b), r64, dict(accepted=acc32), 4 * w, bad, stats, controller_too=False)
        check_state("%s sequence %d (f32 oracle vs its f64 replay)" % (which, b), torch.cat(out32, 0), r64, bad)
    if tol == 1e-3:
        assert several, "no accepted step holds several stamps: the interpolant is not exercised"
    assert stats["undecided"] <= 0.1 * stats["attempts"]
    assert not bad, "\n".join(bad)


def test_abi_and_option_surface():
    """The header declares the entry point, lib.py binds it, and the model takes the option without a GPU."""
    from caspr_amd import lib
    from caspr_amd.csrc import build
    from caspr_amd.models import CaSPR
    from caspr_amd.models.latent_ode_model import LatentODE
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "caspr_hip.h")).read()
    assert "caspr_latent_dopri5_f32(" in hdr and "caspr_latent_dopri5_f32" in lib.SIGNATURES
    assert len(lib.SIGNATURES["caspr_latent_dopri5_f32"][1]) == 22 and "ode_latent_dp5.hip" in build.SOURCES
    m = CaSPR(latent_method="dopri5", latent_rtol=1e-4, latent_atol=1e-6)
    lat = m.latent_ode
    assert (lat.method, lat.rtol, lat.atol) == ("dopri5", 1e-4, 1e-6)
    d = CaSPR()
    assert (d.latent_ode.method, d.latent_ode.rtol, d.latent_ode.atol) == ("rk4", 1e-3, 1e-3) and LatentODE().method == "rk4"
    assert sorted(d.state_dict()) == sorted(m.state_dict())
    assert (lat.solver.method, lat.solver.rtol, lat.solver.atol) == ("dopri5", 1e-3, 1e-3)        # latent_ode_model.py:38,83
    with pytest.raises(ValueError):
        CaSPR(latent_method="euler")
    both = CaSPR(cnf_method="dopri5", latent_method="dopri5")
    assert both.point_cnf.chain[1].method == "dopri5" and both.latent_ode.method == "dopri5"


# ---------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev, seeded_sd, stress_sd):
    from caspr_amd.models import CaSPR
    out = {}
    for name, sd in (("seeded", seeded_sd), ("stress", stress_sd)):
        m = CaSPR(latent_method="dopri5")
        m.load_state_dict(sd)
        out[name] = (m.to(dev).eval(), sd)
    for D, H in WIDTHS:                               # the other widths the kernel accepts: LatentODE(input_size = D, hidden_size = H) alone
        out[width_name(D, H)] = (types.SimpleNamespace(latent_ode=module(D, H, dev, method="dopri5")), net(D, H))
    return out


def solve(model, z0, times, rtol, atol, max_attempts=1000):
    """One ops.latent_dopri5 call with the trace -> (out, info) on the CPU.  z0: a GPU tensor (possibly a strided view)."""
    from caspr_amd import ops
    out, info = ops.latent_dopri5(z0, times.to("cuda:0").float().contiguous(), rtol, atol, model.latent_ode._weights(), max_attempts=max_attempts,
                                  return_trace=True)
    torch.cuda.synchronize()
    return out.cpu(), {k: v.cpu() for k, v in info.items()}


def traced(info, b):
    """Sequence b's attempts out of the trace, as check_decisions takes them."""
    k = int(info["accepted"][b]) + int(info["rejected"][b])
    rows = info["attempts"][b, :k].double().numpy()
    return dict(dts=[float(v) for v in rows[:, 1]], accepted=[bool(v) for v in rows[:, 3]], ratios=[(np.float32(r[2]),) for r in rows],
                t=[float(v) for v in rows[:, 0]], d0=float(info["d0"][b]), d1=float(info["d1"][b]), d2=float(info["d2"][b]), h0=float(info["h0"][b]),
                dt0=float(info["dt0"][b]), nfe=int(info["nfe"][b]))


def same_info(a, b, idx_a=None, idx_b=None):
    pick = lambda v, i: v if i is None else v[i]
    return all(same_bits(pick(a[k], idx_a).float().contiguous(), pick(b[k], idx_b).float().contiguous()) for k in a)


def _cases():
    """B in {1, 5, 16, 17, 33} x Tu in {1, 2, 9, 40}; the weight set, tolerance, horizon, stamp pattern and z0 layout cycle along the
    list so that every value of each meets several of the others.  Ten of the twenty cases are stress weights at 1e-6: the ones that
    exercise the reject path."""
    out, i = [], 0
    for B in (1, 5, 16, 17, 33):
        for Tu in (1, 2, 9, 40):
            hard = i % 2 == 0
            out.append(dict(B=B, Tu=Tu, w="stress" if (hard or i % 4 == 1) else "seeded", tol=1e-6 if (hard or i % 4 == 3) else 1e-3,
                            horizon=(1.0, 3.0)[(i // 2) % 2], pattern=("plain", "repeats", "equal", "solve_at")[(i + i // 4) % 4],
                            strided=i % 3 != 0, t_first=(0.0, 0.25)[i % 2]))
            i += 1
    return out


CASES = _cases()
MATRIX = dict(attempts=0, undecided=0, rejected=0, worst_s_diff=0.0, cases=0)


def case_stamps(case, seed):
    """-> (sorted stamps (Tu',) f32, time tensor (B, T) or None).  plain: distinct ascending; repeats: every third stamp doubled and the
    first one repeated; equal: all stamps equal; solve_at: an unsorted (B, Tu) tensor of grid stamps (repeats across the batch)."""
    B, Tu, H, t0 = case["B"], case["Tu"], case["horizon"], case["t_first"]
    if case["pattern"] == "equal":
        return torch.full((Tu,), t0 + 0.5, dtype=torch.float32), None
    if case["pattern"] == "solve_at":
        g = torch.Generator().manual_seed(seed)
        tt = t0 + H * torch.randint(0, 21, (B, Tu), generator=g).float() / 20.0
        return torch.sort(tt.reshape(-1), stable=True)[0].contiguous(), tt
    t = t0 + H * torch.linspace(0.0, 1.0, Tu) ** 1.5 if Tu > 1 else torch.tensor([t0])
    if case["pattern"] == "repeats" and Tu > 1:
        idx = sorted(list(range(Tu)) + list(range(0, Tu, 3)))[:Tu]
        t = t[idx]
    return t.float().contiguous(), None


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=["b%d-tu%d-%s-%.0e-h%d-%s-%s" % (c["B"], c["Tu"], c["w"], c["tol"], c["horizon"], c["pattern"],
                                                                              "strided" if c["strided"] else "contig") for c in CASES])
def test_route_matrix(dev, models, case):
    """State and decisions of the replayed sequences against the f64 replay of the kernel's own attempts; the launch twice, bit for bit."""
    route_case(dev, models, case, MATRIX, len(CASES))


def route_case(dev, models, case, MATRIX, ncases):
    """One case of a route matrix (`MATRIX`: its running totals, `ncases` its length); D = case["D"] latent dims (64 where absent)."""
    model, sd = models[case["w"]]
    B, tol, D = case["B"], case["tol"], case.get("D", 64)
    seed = 3000 + 50 * B + case["Tu"]
    z0 = sequences(seed, B, D)
    if case["strided"]:
        wide = torch.full((B, 1600), float("nan"))
        wide[:, :D] = z0
        zg = wide.to(dev)[:, :D]                     # the encoder's layout: a column slice, row stride 1600
    else:
        zg = z0.to(dev).contiguous()
    times, tt = case_stamps(case, seed + 1)
    out, info = solve(model, zg, times, tol, tol)
    out2, info2 = solve(model, zg, times, tol, tol)
    bad = []
    if not (same_bits(out, out2) and same_info(info, info2)):
        bad.append("two launches differ in their bits")
    if tt is not None:
        lat = model.latent_ode
        prev = (lat.rtol, lat.atol)
        try:
            lat.rtol = lat.atol = tol
            with torch.no_grad():
                got = lat.solve_at(zg, tt.to(dev)).cpu()
        finally:
            lat.rtol, lat.atol = prev
        pos = torch.searchsorted(times, tt.reshape(-1)).view(tt.shape)           # any row of a repeated stamp: they are bit-identical
        if not same_bits(got, out[torch.arange(B).view(-1, 1).expand_as(pos), pos]):
            bad.append("solve_at differs from the op on the sorted stamps followed by the gather")
    rel = rel_of(times)
    eq = [i for i in range(1, len(rel)) if rel[i] == rel[i - 1]]
    if eq and not all(same_bits(out[:, i], out[:, i - 1]) for i in eq):
        bad.append("repeated stamps give different rows")
    if not same_bits(out[:, 0], z0):
        bad.append("the row of times[0] is not z0")
    stats = dict(attempts=0, undecided=0)
    picks = range(B) if B <= 5 else sorted({0, 7, 15, B - 1})       # (larger batches: four sequences replayed; all of them launched)
    nfe_all, att_all = info["nfe"].long(), (info["accepted"] + info["rejected"]).long()
    if not bool((nfe_all == 2 + 6 * att_all).all()):
        bad.append("evaluations != 2 + 6 x attempts: %s / %s" % (nfe_all.tolist(), att_all.tolist()))
    for b in picks:
        got = traced(info, b)
        p64, p32 = problem(sd, z0[b]), problem(sd, z0[b], torch.float32)
        tag = "sequence %d" % b
        try:
            worst, r64 = measure_delta(p32, p64, rel, tol, tol, got["dts"], got["accepted"])
        except AssertionError as e:
            bad.append("%s: %s" % (tag, e))
            continue
        if len(r64["dts"]) != len(got["dts"]):
            bad.append("%s: %d attempts traced, the stamps are reached after %d" % (tag, len(got["dts"]), len(r64["dts"])))
        MATRIX["worst_s_diff"] = max(MATRIX["worst_s_diff"], worst)
        MATRIX["rejected"] += got["accepted"].count(False)
        delta = 4 * worst
        print("%s: %d attempts, %d rejected, |s32 - s64| max %.3e, s64 %s" % (tag, len(got["dts"]), got["accepted"].count(False), worst,
                                                                             ["%.4f" % math.sqrt(r[0]) for r in r64["ratios"]]))
        if got["dts"]:
            check_decisions(tag, r64, got, delta, bad, stats)
            for k, (tk, tw) in enumerate(zip(got["t"], r64["t"])):
                if not abs(tk - tw) <= 1e-6 * max(1.0, abs(tw)):
                    bad.append("%s: attempt %d traced at t = %.9g, the accepted steps sum to %.9g" % (tag, k, tk, tw))
        else:
            check_head(tag, r64, got, bad)
        check_state(tag, out[b], r64, bad, key="latent_dopri5:matrix:b%d-tu%d-%s-%.0e:%s" % (B, case["Tu"], case["w"], tol, tag.replace(" ", "")))
    MATRIX["attempts"] += stats["attempts"]
    MATRIX["undecided"] += stats["undecided"]
    MATRIX["cases"] += 1
    report(MATRIX.get("key", "matrix:totals"), attempts=MATRIX["attempts"], undecided=MATRIX["undecided"], rejected=MATRIX["rejected"],
           worst_s32_minus_s64=MATRIX["worst_s_diff"], delta=4 * MATRIX["worst_s_diff"])
    assert MATRIX["undecided"] <= 0.1 * max(MATRIX["attempts"], 10), "attempts that decide nothing: %d of %d" % (MATRIX["undecided"], MATRIX["attempts"])
    if MATRIX["cases"] == ncases:
        assert MATRIX["rejected"] >= 1, "the matrix holds no rejected attempt: the reject path was not exercised"
    assert not bad, "\n".join(bad)


def _width_cases():
    """Per (D, H) of WIDTHS: five sequences at 1e-6 over a horizon of 3 (all replayed; strided z0, repeated stamps, times[0] = 0.25) and
    seventeen at 1e-3 through solve_at (two workgroups, the second with one column)."""
    out = []
    for D, H in WIDTHS:
        out.append(dict(D=D, H=H, w=width_name(D, H), B=5, Tu=9, tol=1e-6, horizon=3.0, pattern="repeats", strided=True, t_first=0.25))
        out.append(dict(D=D, H=H, w=width_name(D, H), B=17, Tu=2, tol=1e-3, horizon=1.0, pattern="solve_at", strided=False, t_first=0.0))
    return out


WIDTH_CASES = _width_cases()
WIDTH_MATRIX = dict(attempts=0, undecided=0, rejected=0, worst_s_diff=0.0, cases=0, key="matrix_widths:totals")
WIDTH_IDS = ["D%d-H%d-b%d-tu%d-%.0e-h%d-%s-%s" % (c["D"], c["H"], c["B"], c["Tu"], c["tol"], c["horizon"], c["pattern"], "strided" if c["strided"] else "contig")
             for c in WIDTH_CASES]


def test_width_cases_hold_a_rejected_attempt():
    """CPU: the oracle's f32 run on the width cases, in the kernel's place -- its attempts hold at least one rejection between them
    (tolerance and horizon were chosen for that), and the GPU test's state and accept / reject checks pass on it."""
    bad, stats, rejected = [], dict(attempts=0, undecided=0), 0
    for case in WIDTH_CASES:
        sd, B, tol = net(case["D"], case["H"]), case["B"], case["tol"]
        seed = 3000 + 50 * B + case["Tu"]
        z0 = sequences(seed, B, case["D"])
        rel = rel_of(case_stamps(case, seed + 1)[0])
        for b in (range(B) if B <= 5 else sorted({0, 7, 15, B - 1})):
            p64, p32 = problem(sd, z0[b]), problem(sd, z0[b], torch.float32)
            out32, _, ratios32, dts32 = oracle_run(*p32, rel, tol, tol)
            acc32 = [x[0] <= 1 for x in ratios32]
            rejected += acc32.count(False)
            w, r64 = measure_delta(p32, p64, rel, tol, tol, dts32, acc32)
            tag = "%s sequence %d" % (case["w"], b)
            print("%s: %d attempts, %d rejected, s64 %s" % (tag, len(acc32), acc32.count(False), ["%.4f" % math.sqrt(r[0]) for r in r64["ratios"]]))
            check_decisions(tag, r64, dict(accepted=acc32), 4 * w, bad, stats, controller_too=False)
            check_state(tag, torch.cat(out32, 0), r64, bad)
    assert rejected >= 1, "the width cases hold no rejected attempt"
    assert stats["undecided"] <= 0.1 * stats["attempts"]
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDTH_CASES, ids=WIDTH_IDS)
def test_route_matrix_widths(dev, models, case):
    """The route matrix's criterion at the other widths the kernel accepts (WIDTHS), with its own totals and its own 10 % cap."""
    route_case(dev, models, case, WIDTH_MATRIX, len(WIDTH_CASES))


@pytest.mark.gpu
def test_a_sequence_does_not_depend_on_its_batch(dev, models):
    """Output, trace and counters of a sequence: alone, inside batches of 6 / 17 / 33 (other columns, other workgroups), under a
    permutation, on a second stream, and next to a neighbour with a different step history (z0 scaled by 4)."""
    model, _ = models["stress"]
    tol = 1e-6
    z0 = sequences(81, 33)
    times = stamps(1.0, 0.25)
    zg = z0.to(dev)
    out, info = solve(model, zg, times, tol, tol)
    bad = []
    for n in (6, 17):
        o, i = solve(model, zg[:n].contiguous(), times, tol, tol)
        if not (same_bits(o, out[:n]) and same_info(i, info, None, slice(0, n))):
            bad.append("the first %d sequences alone differ from the same sequences inside the batch of 33" % n)
    perm = torch.randperm(33, generator=torch.Generator().manual_seed(5))
    o, i = solve(model, zg[perm].contiguous(), times, tol, tol)
    if not (same_bits(o, out[perm]) and same_info(i, info, None, perm)):
        bad.append("a permutation of the batch changes a sequence's bits")
    with torch.cuda.stream(torch.cuda.Stream()):
        o, i = solve(model, zg, times, tol, tol)
    if not (same_bits(o, out) and same_info(i, info)):
        bad.append("a second stream changes the bits")
    for b in (0, 15, 16, 32):
        o, i = solve(model, zg[b:b + 1].contiguous(), times, tol, tol)
        if not (same_bits(o, out[b:b + 1]) and same_info(i, info, None, slice(b, b + 1))):
            bad.append("sequence %d alone differs from the sequence inside the batch" % b)
    z4 = z0[:6].clone()
    z4[1::2] *= 4.0                                   # every other sequence: another scale, another step history
    o, i = solve(model, z4.to(dev), times, tol, tol)
    even = torch.tensor([0, 2, 4])
    if not (same_bits(o[even], out[even]) and same_info(i, info, even, even)):
        bad.append("a neighbour with a different step history changes a sequence's bits")
    att = (i["accepted"] + i["rejected"]).tolist()
    assert att[1] != att[0] or att[3] != att[2], "the scaled neighbours took the same number of attempts: nothing was shown (%s)" % att
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["seeded", "stress"])
def test_tolerance_is_honoured(dev, models, which):
    """Tightening rtol = atol (1e-3, 1e-5, 1e-6) moves the result towards the converged f64 solution (oracle.model.latent_solve in f64,
    RK4, 256 steps per interval) monotonically, as far as an f32 output can show it: two distances are told apart only when they differ
    by more than one unit in the last place of |z|max.  The distances and the f64 oracle's own at the same tolerances are recorded, no
    bound on them."""
    model, sd = models[which]
    z0 = sequences(91, 6)
    times = stamps(1.0)
    sd64 = dyn_sd(sd, torch.float64)
    conv = O.latent_solve(sd64, z0.double(), times.double(), "rk4", 256)
    rel = rel_of(times)
    dist, own = {}, {}
    for tol in (1e-3, 1e-5, 1e-6):
        out, info = solve(model, z0.to(dev), times, tol, tol)
        dist[tol] = float((out.double() - conv).abs().max())
        o = 0.0
        for b in range(6):
            p64 = problem(sd, z0[b])
            res = O.dopri5_solve(lambda t, ys: (p64[0](ys[0]),), (p64[1],), rel, tol, tol)
            o = max(o, float((torch.cat([r[0] for r in res], 0) - conv[b]).abs().max()))
        own[tol] = o
        print("%s tol %.0e: distance %.3e (f64 oracle %.3e), nfe %s" % (which, tol, dist[tol], o, info["nfe"].tolist()))
    ulp = 2.0 ** -23 * float(conv.abs().max())
    report("contract:%s" % which, distance_1e3=dist[1e-3], distance_1e5=dist[1e-5], distance_1e6=dist[1e-6], f64_oracle_distance_1e3=own[1e-3],
           f64_oracle_distance_1e5=own[1e-5], f64_oracle_distance_1e6=own[1e-6], f32_ulp_at_absmax=ulp)
    assert dist[1e-3] + ulp >= dist[1e-5] and dist[1e-5] + ulp >= dist[1e-6] and dist[1e-3] + ulp >= dist[1e-6], (dist, ulp)


@pytest.mark.gpu
def test_attempt_budget_and_bad_arguments(dev, models):
    """max_attempts = 3 on the stress weights at 1e-6: NaN in the unreached rows, the error status through the deferred channel,
    raised -- nothing hangs, the library is usable afterwards.  Bad arguments raise as in ops.latent_rk4 / ops.cnf_dopri5."""
    from caspr_amd import ops
    from caspr_amd.lib import CasprHipError
    model, _ = models["stress"]
    ops.check_deferred_errors()
    z0 = sequences(95, 5).to(dev)
    times = stamps(1.0)
    wts = model.latent_ode._weights()
    out, info = ops.latent_dopri5(z0, times.to(dev), 1e-6, 1e-6, wts, max_attempts=3, return_trace=True)
    with pytest.raises(CasprHipError, match="max_attempts"):
        ops.check_deferred_errors()
    torch.cuda.synchronize()
    out = out.cpu()
    assert (info["accepted"] + info["rejected"]).cpu().tolist() == [3] * 5 and info["nfe"].cpu().tolist() == [20] * 5
    assert bool(torch.isnan(out[:, -1]).all()) and same_bits(out[:, 0], z0.cpu()) and bool(torch.isfinite(out[:, 1]).all())
    for b in range(5):                                # NaN exactly in the rows past the last accepted step's end
        rows = info["attempts"][b, :3].cpu().double()
        reached = float((rows[:, 1] * rows[:, 3]).sum())
        for i, r in enumerate(rel_of(times)):
            assert bool(torch.isnan(out[b, i]).all()) == (r > reached * (1 + 1e-6)) or abs(r - reached) <= 1e-6 * reached, (b, i, r, reached)
    ops.check_deferred_errors()                       # drained: the error is reported once
    out, info = solve(model, z0, times, 1e-6, 1e-6)   # the library is still usable afterwards
    ops.check_deferred_errors()
    assert bool(torch.isfinite(out).all()) and int((info["accepted"] + info["rejected"]).min()) > 3
    ops.latent_dopri5(z0, times.to(dev), 1e-6, 1e-6, wts, max_attempts=3)
    torch.cuda.synchronize()
    with pytest.raises(CasprHipError, match="max_attempts"):      # ... or by the next solve on that stream
        ops.latent_dopri5(z0, times.to(dev), 1e-3, 1e-3, wts)
    ops.check_deferred_errors()
    td = times.to(dev)
    call = lambda z_=z0, t_=td, rtol=1e-3, atol=1e-3, **kw: ops.latent_dopri5(z_, t_, rtol, atol, wts, **kw)
    with pytest.raises(ValueError):
        call(z_=z0[:, :32].contiguous())
    with pytest.raises(ValueError):
        call(z_=z0.cpu())
    with pytest.raises(ValueError):
        call(z_=z0.t().contiguous().t())
    with pytest.raises(ValueError):
        call(t_=td.view(1, -1))
    with pytest.raises(ValueError):
        call(rtol=0.0)
    with pytest.raises(ValueError):
        call(atol=float("nan"))
    with pytest.raises(ValueError):
        call(rtol=float("inf"))
    with pytest.raises(ValueError):
        call(max_attempts=0)
    with pytest.raises(ValueError):
        call(z_=z0.clone().requires_grad_(True))      # grad enabled: no gradient through the adaptive solve
    ops.check_deferred_errors()


@pytest.mark.gpu
def test_model_surface(dev, seeded_sd, monkeypatch):
    """CaSPR(latent_method="dopri5") loads the same state_dict; reconstruct() with the early latent solve on and off gives the same bits,
    equal to ops.latent_dopri5 on the same z0 and sorted stamps followed by the plan's gather; get_nfe()[0] is the counters' maximum;
    no RK4 (check) solve is launched for the latent ODE and no latent guard warning appears; with grad enabled the option raises;
    latent_ode.solver(z0, t) returns the transposed solution; with cnf_method="dopri5" get_nfe() is two measured numbers."""
    import warnings
    from caspr_amd import ops
    from caspr_amd.models import CaSPR, caspr as caspr_mod
    from caspr_amd.utils.synthetic import dense_sequences
    m = CaSPR(latent_method="dopri5")
    m.load_state_dict(seeded_sd)
    m = m.to(dev).eval()
    assert m.latent_ode.method == "dopri5"
    x, sp = dense_sequences(2, 3, 1024)
    y = rnd(61, 2, 3, 200, 3).to(dev)
    ts = torch.tensor([0.9, 0.1, 0.4]).to(dev)        # unsorted: solve_at sorts

    def no_rk4(*a, **k):
        raise AssertionError("a dopri5 latent ODE must not launch an RK4 (check) solve")
    monkeypatch.setattr(ops, "latent_rk4", no_rk4)
    res = {}
    for early in (True, False):
        monkeypatch.setattr(caspr_mod, "EARLY_LATENT", early)
        with torch.no_grad(), warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            _, _, gx, _ = m.reconstruct(x.to(dev), num_points=200, timestamps=ts, y=y)
            ops.check_deferred_errors()
            torch.cuda.synchronize()
        assert m._early_latent_used == early
        assert not [w for w in caught if "latent ODE" in str(w.message)], [str(w.message) for w in caught]
        nfe = m.latent_ode.last_nfe_per_sequence.cpu()
        assert int(m.get_nfe()[0]) == int(nfe.max()) and nfe.shape == (2,) and int(nfe.min()) >= 8
        with torch.no_grad():
            z0, _ = m.encode(x.to(dev))
            codes = m.aggregate_and_solve_latent(z0, ts.view(1, -1).repeat(2, 1))
        res[early] = (gx.cpu(), codes.cpu(), nfe)
    assert same_bits(res[True][0], res[False][0]) and same_bits(res[True][1], res[False][1]) and res[True][2].tolist() == res[False][2].tolist()
    with torch.no_grad():
        tt = ts.view(1, -1).repeat(2, 1)
        plan = m.latent_ode.plan_times(tt)
        want, info = ops.latent_dopri5(z0[:, :64], plan["sorted_t"], 1e-3, 1e-3, m.latent_ode._weights(), return_trace=True)
        want = want[plan["rows"], plan["pos"], :]
        assert same_bits(res[False][1][:, :, :64].contiguous(), want.cpu()) and info["nfe"].cpu().tolist() == res[False][2].tolist()
        # the reference's solver object: (T, B, H), at the solver's own rtol = atol = 1e-3
        t = torch.tensor([0.0, 0.3, 0.3, 1.0]).to(dev)
        sol = m.latent_ode.solver(z0[:, :64], t)
        direct = ops.latent_dopri5(z0[:, :64], t, 1e-3, 1e-3, m.latent_ode._weights())
        assert tuple(sol.shape) == (4, 2, 64) and same_bits(sol.permute(1, 0, 2).contiguous().cpu(), direct.cpu())
        fw = m.latent_ode(z0[:, :64], t)
        assert same_bits(fw.cpu(), direct.cpu())
    with pytest.raises(ValueError, match="dopri5"):
        m.latent_ode(z0[:, :64], t)                   # grad enabled
    both = CaSPR(cnf_method="dopri5", latent_method="dopri5")
    both.load_state_dict(seeded_sd)
    both = both.to(dev).eval()
    with torch.no_grad():
        both.reconstruct(x.to(dev), num_points=200, timestamps=ts, y=y)
        ops.check_deferred_errors()
    n = both.get_nfe()
    assert int(n[0]) == int(both.latent_ode.last_nfe_per_sequence.max()) and int(n[1]) == int(both.point_cnf.chain[1].last_nfe_per_frame.max())
    assert int(n[0]) >= 8 and int(n[1]) >= 8 and (int(n[0]) - 2) % 6 == 0 and (int(n[1]) - 2) % 6 == 0
