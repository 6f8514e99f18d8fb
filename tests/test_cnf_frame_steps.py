"""Per-frame RK4 step counts of the point-CNF sampling solve (CaSPR(cnf_steps="frame"); include/caspr_hip.h:
caspr_cnf_rk4_x6_frames_f32 / caspr_cnf_rk4_h3_frames_f32 / caspr_cnf_steps_update_f32 / caspr_cnf_steps_order).

CPU: the controller's rule (tests/frame_steps_ref.py) on the f64 solve of tests/test_cnf_solve_kernels.py, the order restatement, the
constructor's surface.  GPU: a table launch equals per-frame uniform launches bit for bit on all three sampling kernels (whatever the
launch order), a zero entry skips the frame, table entries are clamped, the update and order kernels equal their restatement exactly,
and the model option: bits, decisions, independence of the batch, NFE, guard.

Inputs of the rule test: six frames of 64 points, contexts rnd(11, 6, 1600) scaled per frame by SCALES, base_samples(12, 6, 64),
tol 1e-5, safety 1.2, S_max 64."""
import numpy as np
import pytest
import torch

import frame_steps_ref as R
from test_cnf_solve_kernels import (Checks, Weights, X_TOL, base_samples, block_params, cnf_solve_f64, hyper_of, mbn_of, mbn_pair, reference,
                                    rnd, solve_args)
from test_hip_parity import REPORT, record

SCALES = [0.25, 0.5, 1.0, 1.0, 1.5, 2.0]
TOL, SAFETY, S_MAX = 1e-5, 1.2, 64


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
def _f64_setup(sd):
    sd = {k: v.double() for k, v in sd.items()}
    P = block_params(sd)
    c = rnd(11, 6, 1600).double() * torch.tensor(SCALES, dtype=torch.float64).view(6, 1)
    y = base_samples(12, 6, 64).double()
    hyper = hyper_of(P, c)
    mi, mo = mbn_of(sd, 2), mbn_of(sd, 0)

    def solve(S, frames=None):
        f = slice(None) if frames is None else frames
        return cnf_solve_f64(y[f], hyper[f], *solve_args(P), P["t_end"], S, True, mi, mo)[0]
    return solve


def test_rule_on_the_f64_solve_stress(stress_sd):
    """The controller on the stress weights chooses [28, 32, 32, 32, 41, 32], and every frame then passes the accuracy guard's own
    check at (S_f, S_f // 2): estimate / bound <= 1 (measured when the rule was fixed: worst 0.725)."""
    solve = _f64_setup(stress_sd)
    with torch.no_grad():
        steps, capped, stats, pilot = R.ladder(solve, 6, TOL, SAFETY, S_MAX)
        assert [int(s) for s in steps] == [28, 32, 32, 32, 41, 32], (steps, stats)
        assert int(capped.sum()) == 0
        assert [int(p) for p in pilot] == [63, 63, 63, 63, 127, 63]
        ratios = []
        for S in sorted(set(int(s) for s in steps)):
            fr = [f for f in range(6) if int(steps[f]) == S]
            xs, xh = solve(S, fr), solve(S // 2, fr)
            ratios += [R.guard_ratio(xs[i], xh[i], S, S // 2, TOL) for i in range(len(fr))]
    print("guard estimate / bound per frame (grouped by count):", ratios)
    assert max(ratios) <= 1.0, ratios


def test_rule_on_the_f64_solve_seeded(seeded_sd):
    solve = _f64_setup(seeded_sd)
    with torch.no_grad():
        steps, capped, stats, pilot = R.ladder(solve, 6, TOL, SAFETY, S_MAX)    # (every frame is decided at rung 2: the ladder ends there)
    assert [int(s) for s in steps] == [2] * 6 and int(capped.sum()) == 0 and [int(p) for p in pilot] == [3] * 6, (steps, stats)


def _tied_steps(BT):
    return torch.from_numpy(np.random.default_rng(BT).integers(2, 7, BT).astype(np.int32))


@pytest.mark.parametrize("BT", [1, 5, 64, 65, 1000])
def test_order_restatement(BT):
    s = _tied_steps(BT)
    want = torch.sort(s, stable=True, descending=True).indices.to(torch.int32)
    assert torch.equal(R.order(s), want)
    assert BT < 64 or len(set(int(v) for v in s)) <= 5          # heavy ties


def test_surface():
    from caspr_amd import lib
    from caspr_amd.csrc import build
    from caspr_amd.models import CaSPR
    with pytest.raises(ValueError):
        CaSPR(cnf_steps="frame", cnf_method="dopri5")
    with pytest.raises(ValueError):
        CaSPR(cnf_steps="adaptive")
    with pytest.raises(ValueError):
        CaSPR(cnf_steps="frame", cnf_steps_max=48)
    m = CaSPR(cnf_steps="frame", cnf_steps_tol=1e-4, cnf_steps_safety=1.5, cnf_steps_max=32, cnf_steps_points=32)
    assert (m.cnf_steps, m.cnf_steps_tol, m.cnf_steps_safety, m.cnf_steps_max, m.cnf_steps_points) == ("frame", 1e-4, 1.5, 32, 32)
    d = CaSPR()
    assert (d.cnf_steps, d.cnf_steps_tol, d.cnf_steps_safety, d.cnf_steps_max, d.cnf_steps_points) == ("uniform", None, 1.2, 64, 64)
    assert sorted(d.state_dict()) == sorted(m.state_dict())
    blk = d.point_cnf.chain[1]
    assert blk.frame_steps is None and blk.frame_order is None
    for name, nargs in (("caspr_cnf_rk4_x6_frames_f32", 24), ("caspr_cnf_rk4_h3_frames_f32", 25), ("caspr_cnf_steps_update_f32", 13), ("caspr_cnf_steps_order", 4)):
        assert len(lib.SIGNATURES[name][1]) == nargs
    assert "cnf_frame_steps.hip" in build.SOURCES and build.EXTRA["cnf_frame_steps.hip"] == ["-ffp-contract=off"]


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
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


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def itab(v, dev="cuda:0"):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def run(img, W, y, hyper, steps, reverse, mi=None, mo=None, **kw):
    """One sampling launch on image "x6w" | "h3" | "x6n"; steps an int or a (BT,) int32 device tensor."""
    from caspr_amd import ops
    g = lambda v: None if v is None else v.to("cuda:0").contiguous()
    D = W.dev
    return ops.cnf_rk4(g(y), g(hyper), D["tcol"], D["w0"], D["b0"], W.w1p, D["b1"], W.w2p, D["b2"], D["w3"], D["b3"], W.t_end, steps, reverse, g(mi), g(mo),
                       w1x=W.w1x, w2x=W.w2x, narrow=img == "x6n", w1h=W.w1h if img == "h3" else None, w2h=W.w2h if img == "h3" else None, **kw)


KERNEL = {"x6w": "cnf_rk4_x6w_kernel", "h3": "cnf_rk4_h3w_kernel", "x6n": "cnf_rk4_x6_kernel<false>"}
TABLE = [3, 1, 8, 2, 5]
IMG_N = [(img, n) for img in ("x6w", "h3") for n in (128, 129, 257)] + [("x6n", n) for n in (1, 63, 64, 65, 200)]


@pytest.mark.gpu
@pytest.mark.parametrize("img,n", IMG_N, ids=["%s-n%d" % c for c in IMG_N])
def test_table_equals_per_frame_uniform_launches(dev, weights, img, n):
    """Frame k of a table launch == the plain launch of frame k alone at steps = table[k], bit for bit: both directions, MBN at both
    ends and at neither; without an order, with the identity and with a permutation."""
    W = weights["stress"]
    BT = 5
    c, y = rnd(500 + n, BT, 1600), base_samples(501 + n, BT, n)
    hyper = W.hyper(c, 3091)
    ck = Checks("frame_table_%s_n%d" % (img, n))
    for reverse in (True, False):
        for mbn in ("both", "none"):
            mi, mo = mbn_pair(reverse, mbn)
            tag = "%s_mbn_%s" % ("rev" if reverse else "fwd", mbn)
            want = torch.cat([run(img, W, y[k:k + 1], hyper[k:k + 1], TABLE[k], reverse, mi, mo) for k in range(BT)])
            for oname, order in (("no_order", None), ("identity", itab([0, 1, 2, 3, 4])), ("permuted", itab([3, 0, 4, 2, 1]))):
                got = run(img, W, y, hyper, itab(TABLE), reverse, mi, mo, order=order, max_steps=8)
                ck.exact("%s:%s" % (tag, oname), got, want, KERNEL[img])
            if (img, n, reverse, mbn) in (("x6w", 129, True, "both"), ("h3", 129, True, "both"), ("x6n", 65, True, "both")):
                for k in range(BT):
                    ref = reference(W, y[k:k + 1], hyper[k:k + 1], TABLE[k], reverse, mi, mo)[0]
                    ck.close("%s:frame%d_vs_f64" % (tag, k), got[k:k + 1], ref, X_TOL, KERNEL[img])
    ck.done()


@pytest.mark.gpu
@pytest.mark.parametrize("img,n", [("x6w", 129), ("h3", 129), ("x6n", 65)])
def test_uniform_table_equals_scalar_launch(dev, weights, img, n):
    W = weights["stress"]
    BT, S = 5, 3
    c, y = rnd(520, BT, 1600), base_samples(521, BT, n)
    hyper = W.hyper(c, 3078)
    mi, mo = mbn_pair(True, "both")
    ck = Checks("frame_uniform_%s" % img)
    ck.exact("table_vs_scalar", run(img, W, y, hyper, itab([S] * BT), True, mi, mo), run(img, W, y, hyper, S, True, mi, mo), KERNEL[img])
    ck.done()


@pytest.mark.gpu
@pytest.mark.parametrize("img,n", [("x6w", 129), ("h3", 129), ("x6n", 65)])
def test_skip_and_clamp(dev, weights, img, n):
    """A zero entry skips the frame: its rows keep the NaN payload pattern they were filled with.  A negative entry is a zero, an
    entry above max_steps is max_steps (the launch returns with the max_steps result)."""
    W = weights["stress"]
    BT = 5
    c, y = rnd(530, BT, 1600), base_samples(531, BT, n)
    hyper = W.hyper(c, 3080)
    mi, mo = mbn_pair(True, "both")
    ck = Checks("frame_skip_%s" % img)
    payload = (0x7fc00000 + 1 + torch.arange(BT * n * 3, dtype=torch.int32) % 4096).view(BT, n, 3)
    for tag, tab, eff, max_steps in (("skip", [2, 0, 3, 0, 1], [2, 0, 3, 0, 1], 8), ("clamp", [2, -7, 10 ** 9, 0, 4], [2, 0, 4, 0, 4], 4)):
        out = payload.to(dev).view(torch.float32).clone()
        got = run(img, W, y, hyper, itab(tab), True, mi, mo, max_steps=max_steps, out=out)
        assert got.data_ptr() == out.data_ptr()
        want = payload.view(torch.float32).clone().to(dev)
        for k in range(BT):
            if eff[k]:
                want[k:k + 1] = run(img, W, y[k:k + 1], hyper[k:k + 1], eff[k], True, mi, mo)
        ck.exact(tag, got, want, KERNEL[img])
        assert bool(torch.isnan(got[1]).all()) and bool(torch.isnan(got[3]).all())
    ck.done()


@pytest.mark.gpu
def test_validation(dev, weights):
    from caspr_amd import ops
    W = weights["seeded"]
    BT, n = 3, 8
    y, hyper = base_samples(540, BT, n).to(dev), W.hyper(rnd(541, BT, 1600), 3078).to(dev)
    D = W.dev
    seen = []
    L = ops._lib.load()
    names = ("caspr_cnf_rk4_f32", "caspr_cnf_rk4_x6_f32", "caspr_cnf_rk4_h3_f32", "caspr_cnf_rk4_x6_frames_f32", "caspr_cnf_rk4_h3_frames_f32")
    real = {k: getattr(L, k) for k in names}

    def call(steps, **kw):
        kw.setdefault("w1x", W.w1x)
        kw.setdefault("w2x", W.w2x)
        return ops.cnf_rk4(y, hyper, D["tcol"], D["w0"], D["b0"], W.w1p, D["b1"], W.w2p, D["b2"], D["w3"], D["b3"], W.t_end, steps, True, **kw)
    try:
        for k in names:
            setattr(L, k, lambda *a, _k=k: seen.append(_k) or real[_k](*a))
        good = itab([1, 2, 1])
        e, lp = rnd(542, BT, n, 3).to(dev), torch.zeros(BT, n, 1, device=dev)
        for bad in (dict(steps=good, e=e, logp=lp), dict(steps=good, w1x=None, w2x=None), dict(steps=good.long()), dict(steps=good.cpu()),
                    dict(steps=good[:BT - 1].contiguous()), dict(steps=itab([1, 0, 2, 0, 1])[::2]), dict(steps=good, max_steps=0), dict(steps=good, max_steps=5000),
                    dict(steps=good, order=itab([0, 1])), dict(steps=2, order=itab([0, 1, 2])), dict(steps=2, max_steps=4)):
            with pytest.raises(ValueError):
                call(**bad)
        assert seen == [], seen                   # raised before any launch
        call(good, max_steps=4096)
        assert seen == ["caspr_cnf_rk4_x6_frames_f32"], seen
    finally:
        for k in names:
            setattr(L, k, real[k])
    torch.cuda.synchronize()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(ck, name, got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    bad = int((_bits(got) != _bits(want)).sum())
    REPORT["%s:%s" % (ck.tag, name)] = {"mismatches": bad, "count": got.numel()}
    if bad:
        ck.bad.append("%s: %d / %d values differ in their bits\n got  %s\n want %s" % (name, bad, got.numel(), got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("which,g", [("stress", 64), ("stress", 40), ("seeded", 64), ("seeded", 40)])
def test_update_kernel_on_the_pilot(dev, weights, which, g):
    """The ladder on rung outputs of the narrow kernel: after every rung steps / next_tab / capped / stats of the update kernel equal
    the restatement applied to the same tensors, bit for bit; and ops.cnf_frame_steps (table launches that skip decided frames) ends
    with the same table."""
    from caspr_amd import ops
    W = weights[which]
    BT = 6
    c = rnd(11, BT, 1600) * torch.tensor(SCALES).view(BT, 1)
    y, hyper = base_samples(12, BT, g), W.hyper(c, 3078)
    mi, mo = mbn_pair(True, "both")
    ck = Checks("frame_update_%s_g%d" % (which, g))
    steps, capped, stats = torch.zeros(BT, dtype=torch.int32, device=dev), torch.zeros(BT, dtype=torch.int32, device=dev), torch.zeros(BT, 4, dtype=torch.float64, device=dev)
    rs, rc, rst = steps.cpu(), capped.cpu(), stats.cpu()
    x_prev, P = run("x6n", W, y, hyper, 1, True, mi, mo), 2
    while P <= S_MAX:
        x_cur = run("x6n", W, y, hyper, P, True, mi, mo)
        nxt = torch.full((BT,), -1, dtype=torch.int32, device=dev)
        ops.cnf_steps_update(x_prev, x_cur, P, TOL, SAFETY, S_MAX, steps, nxt, capped, stats)
        rs, rn, rc, rst = R.update(x_prev, x_cur, P, TOL, SAFETY, S_MAX, rs, rc, rst)
        for name, a, b in (("steps", steps, rs), ("next_tab", nxt, rn), ("capped", capped, rc), ("stats", stats, rst)):
            _same(ck, "rung%d:%s" % (P, name), a, b)
        x_prev, P = x_cur, 2 * P
    fs, fo, info = ops.cnf_frame_steps(lambda tab: run("x6n", W, y, hyper, tab, True, mi, mo, max_steps=S_MAX), BT, g, TOL, SAFETY, S_MAX, device=dev)
    _same(ck, "driver:steps", fs, rs)
    _same(ck, "driver:stats", info["stats"], rst)
    _same(ck, "driver:capped", info["capped"], rc)
    _same(ck, "driver:order", fo, R.order(rs))
    _same(ck, "driver:pilot_steps", info["pilot_steps"], (2 * rst[:, 3] - 1).to(torch.int32))
    ops.check_deferred_errors()
    hist = sorted(int(s) for s in rs)
    REPORT["frame_steps:kernel_pilot_%s_g%d:steps" % (which, g)] = hist
    assert int(rc.sum()) == 0 and (max(hist) < 8 if which == "seeded" else 8 < max(hist) <= S_MAX), hist
    ck.done()


@pytest.mark.gpu
def test_update_kernel_synthetic(dev):
    """Hand-made solution pairs on every branch: pass at P = 2; pass refined to P/2 + 1, in between, and to P; NaN and infinity;
    fail below and at S_max."""
    from caspr_amd import ops
    BT, g = 7, 5
    bound = 1e-5 * 2.0
    x_cur = torch.zeros(BT, g, 3)
    x_cur[:, 0, 0] = 1.0                                     # max |x| = 1: bound = 2e-5
    x_prev = x_cur.clone()
    for f, ratio in enumerate((1e-6, 0.9, 0.1, 30.0, 0.0)):  # e / bound
        x_prev[f, 3, 1] = 15.0 * ratio * bound
    x_cur[5, 2, 2] = float("nan")
    x_prev[6, 4, 0] = float("inf")
    ck = Checks("frame_update_synthetic")
    for P, s_max, want in ((2, 8, [2, 2, 2, 0, 2, 0, 0]), (4, 8, [3, 4, 3, 0, 3, 0, 0]), (8, 8, [5, 8, 6, 8, 5, 8, 8]), (8, 16, [5, 8, 6, 0, 5, 0, 0]),
                           (64, 64, [33, 64, 44, 64, 33, 64, 64])):
        steps = torch.zeros(BT, dtype=torch.int32, device=dev)
        capped, stats = torch.zeros(BT, dtype=torch.int32, device=dev), torch.zeros(BT, 4, dtype=torch.float64, device=dev)
        nxt = torch.full((BT,), -1, dtype=torch.int32, device=dev)
        ops.cnf_steps_update(x_prev.to(dev), x_cur.to(dev), P, 1e-5, 1.2, s_max, steps, nxt, capped, stats)
        rs, rn, rc, rst = R.update(x_prev, x_cur, P, 1e-5, 1.2, s_max, torch.zeros(BT, dtype=torch.int32))
        tag = "P%d_max%d" % (P, s_max)
        for name, a, b in (("steps", steps, rs), ("next_tab", nxt, rn), ("capped", capped, rc), ("stats", stats, rst)):
            _same(ck, "%s:%s" % (tag, name), a, b)
        assert [int(s) for s in rs] == want, (tag, rs)
        assert [int(v) for v in rc] == [int(P == s_max and w == s_max and f in (3, 5, 6)) for f, w in enumerate(want)], (tag, rc)
    # a decided frame is left alone: table entry 0, statistics and flag untouched
    steps = torch.tensor([5, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)
    stats = torch.full((BT, 4), 7.0, dtype=torch.float64, device=dev)
    capped, nxt = torch.zeros(BT, dtype=torch.int32, device=dev), torch.full((BT,), -1, dtype=torch.int32, device=dev)
    ops.cnf_steps_update(x_prev.to(dev), x_cur.to(dev), 8, 1e-5, 1.2, 8, steps, nxt, capped, stats)
    assert int(steps[0]) == 5 and int(nxt[0]) == 0 and stats[0].tolist() == [7.0] * 4
    ck.done()


@pytest.mark.gpu
@pytest.mark.parametrize("BT", [1, 5, 64, 65, 1000])
def test_order_kernel(dev, BT):
    from caspr_amd import ops
    s = _tied_steps(BT)
    got = ops.cnf_steps_order(s.to(dev))
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), R.order(s))


# ------------------------------------------------------------------------------------------------------------------- the model
def _model(sd, dev, **kw):
    from caspr_amd.models import CaSPR
    m = CaSPR(**kw)
    m.load_state_dict(sd)
    return m.to(dev).eval()


def _zy(dev, n=128):
    z = (rnd(11, 4, 1600) * torch.tensor([0.5, 1.0, 1.5, 2.0]).view(4, 1)).view(1, 4, 1600).to(dev)
    return z, base_samples(12, 4, n).view(1, 4, n, 3).to(dev)


@pytest.mark.gpu
def test_model_frame_mode(dev, stress_sd, seeded_sd, monkeypatch):
    """decode() with cnf_steps="frame" on the stress weights, B T = 4, n = 128: frame k is bit for bit the default model's decode of
    that frame alone at cnf_rk4_steps = S_k; the decisions are the restatement's on the pilot's own outputs; a frame alone, in the
    batch and in a permuted batch gets the same count and the same bits; forward() is the default model's; NFE; seeded weights stay
    below the default 8."""
    from caspr_amd import ops
    from caspr_amd.utils.synthetic import car_sequences
    z, y = _zy(dev)
    mf = _model(stress_sd, dev, cnf_steps="frame", check_tol=None)
    md = _model(stress_sd, dev, check_tol=None)
    rungs = []
    real = ops.cnf_steps_update

    def spy(x_prev, x_cur, P, *a):
        rungs.append((x_prev.clone(), x_cur.clone(), P))
        return real(x_prev, x_cur, P, *a)
    monkeypatch.setattr(ops, "cnf_steps_update", spy)
    x = mf.decode(z, 128, y=y)[2]
    monkeypatch.setattr(ops, "cnf_steps_update", real)
    nfe = int(mf.get_nfe()[1])
    steps, order, info = mf.last_frame_steps
    blk = mf.point_cnf.chain[1]
    ck = Checks("frame_model")
    _same(ck, "block:last_steps", blk.last_steps_per_frame, steps)
    _same(ck, "block:last_pilot_steps", blk.last_pilot_steps_per_frame, info["pilot_steps"])
    S = [int(s) for s in steps]
    REPORT["frame_steps:model_stress:steps"] = S
    assert nfe == 4 * max(S) + 4 * int(info["pilot_steps"].max()), (nfe, S, info["pilot_steps"])
    assert blk.frame_steps is None and blk.frame_order is None and blk._hyper is None
    # decisions == the restatement on the pilot's own outputs
    assert [r[2] for r in rungs] == [2, 4, 8, 16, 32, 64]
    rs, rc, rst = torch.zeros(4, dtype=torch.int32), None, None
    for x_prev, x_cur, P in rungs:
        rs, _, rc, rst = R.update(x_prev, x_cur, P, 1e-5, 1.2, 64, rs, rc, rst)
    _same(ck, "decisions:steps", steps, rs)
    _same(ck, "decisions:stats", info["stats"], rst)
    _same(ck, "decisions:order", order, R.order(rs))
    assert int(rc.sum()) == 0 and max(S) > 8, S
    # frame k == the default model on that frame alone at S_k
    for k in range(4):
        for b in md.point_cnf.chain:
            if hasattr(b, "rk4_steps"):
                b.rk4_steps = S[k]
        ck.exact("frame%d_vs_uniform_alone" % k, x[:, k:k + 1], md.decode(z[:, k:k + 1], 128, y=y[:, k:k + 1])[2])
        xa = mf.decode(z[:, k:k + 1], 128, y=y[:, k:k + 1])[2]
        assert int(mf.last_frame_steps[0][0]) == S[k]
        ck.exact("frame%d_alone" % k, xa, x[:, k:k + 1])
    perm = [2, 0, 3, 1]
    xp = mf.decode(z[:, perm].contiguous(), 128, y=y[:, perm].contiguous())[2]
    assert [int(s) for s in mf.last_frame_steps[0]] == [S[p] for p in perm]
    ck.exact("permuted_batch", xp, x[:, perm].contiguous())
    # forward() (density direction) is untouched by the option
    xs, sp = car_sequences(1, 2, 1024, seed=5)
    e = rnd(13, 2, 1024, 3).to(dev)
    for b in md.point_cnf.chain:
        if hasattr(b, "rk4_steps"):
            b.rk4_steps = 8
    lf, ld = mf(xs.to(dev), sp.to(dev), e=e), md(xs.to(dev), sp.to(dev), e=e)
    ck.exact("forward:recon_loss", lf[0], ld[0])
    ck.exact("forward:tnocs_loss", lf[1], ld[1])
    # gradients through decode are refused
    with torch.enable_grad(), pytest.raises(ValueError):
        mf.decode(z, 128, y=y)
    # seeded weights: fewer steps than the default everywhere
    ms = _model(seeded_sd, dev, cnf_steps="frame", check_tol=None)
    ms.decode(z, 128, y=y)
    Ss = [int(s) for s in ms.last_frame_steps[0]]
    REPORT["frame_steps:model_seeded:steps"] = Ss
    assert all(2 <= s < 8 for s in Ss), Ss
    ops.check_deferred_errors()
    ck.done()


@pytest.mark.gpu
def test_model_guard(dev, stress_sd):
    """Stress weights, check_action="raise": the default model at 8 steps trips the guard; the frame-mode model passes it (the worst
    frame's estimate / bound goes to the report); with cnf_steps_max = 8 the capped frames come through the deferred channel."""
    from caspr_amd import ops
    z, y = _zy(dev)
    ops.reset_guard()
    md = _model(stress_sd, dev, cnf_rk4_steps=8, check_tol=1e-5, check_action="raise")
    with pytest.raises(ops.CasprAccuracyError, match="point CNF"):
        md.decode(z, 128, y=y)
        ops.check_deferred_errors()
    ops.reset_guard()
    mf = _model(stress_sd, dev, cnf_steps="frame", check_tol=1e-5, check_action="raise")
    mf.decode(z, 128, y=y)
    ops.check_deferred_errors()
    rep = dict(ops.GUARD_LAST["cnf"])
    ratio = rep["estimate"] / rep["bound"]
    print("frame-mode guard: worst frame estimate / bound = %.4f" % ratio, rep)
    REPORT["frame_steps:model_guard"] = dict(rep, ratio=ratio, steps_per_frame=[int(s) for s in mf.last_frame_steps[0]])
    assert rep["ok"]
    record("frame_steps:model_guard:worst_estimate_over_bound", ratio, 0.0, 1.0)
    ops.reset_guard()
    mc = _model(stress_sd, dev, cnf_steps="frame", cnf_steps_max=8, check_tol=None)
    try:
        with pytest.raises(ops.CasprAccuracyError, match="capped at 8 steps"):
            mc.decode(z, 128, y=y)
            ops.check_deferred_errors()
        assert int(mc.last_frame_steps[2]["capped"].sum()) >= 1 and int(mc.last_frame_steps[0].max()) == 8
    finally:
        try:
            ops.check_deferred_errors()
        except ops.CasprAccuracyError:
            pass
