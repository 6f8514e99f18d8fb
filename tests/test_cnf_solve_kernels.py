"""The point-CNF inference solve, launch by launch: every image behind ops.cnf_rk4 against a plain f64 restatement of the C contract
(include/caspr_hip.h, caspr_cnf_rk4_f32 / caspr_cnf_rk4_x6_f32), called with raw arguments rather than through the model.

    entry / flags                                    kernel                                 points per workgroup
    caspr_cnf_rk4_f32                                cnf_rk4_kernel<false / true>           32 sampling, 16 with divergence
    caspr_cnf_rk4_x6_f32, e == NULL                  cnf_rk4_x6w_kernel                     128
    caspr_cnf_rk4_x6_f32, e given, or NARROW flag    cnf_rk4_x6_kernel<true / false>        32 with divergence, 64 sampling

The restatement (cnf_solve_f64) shares no code with the kernels or the model: ConcatSquash layers with softplus as oracle/model.py's
odenet evaluates them, but with the gates / biases read from the kernels' `hyper` / `tcol` columns; the Hutchinson divergence by
forward-mode autograd (torch.func.jvp); classic RK4 as oracle.rk4_solve; the MovingBatchNorm formulas of oracle.mbn_forward /
mbn_reverse before and after the block in the direction of travel.  test_restatement_matches_oracle (CPU) pins it to
oracle.point_cnf in f64.

Bounds are the suite's: state 1e-5 x max(1, |x|max), log-density 1e-4 x max(1, |logp|max), the bf16x6 images within 5e-6 x
max(1, |x|max) of the f32-MFMA kernel, and the 64-point sampling kernel within the same 5e-6 of the 128-point one.  Every measured
error lands in test_hip_parity's JSON report (REPORT, written by its record()), keyed "cnf_solve:<test>:<check>", with its bound and the
kernel that produced it.
"""
import inspect
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import model as O
from test_hip_parity import REPORT, record

H = 512
BOFF = 3 * H + 3          # first bias column of hyper / tcol: [gate l0 | .. | gate l3 | bias l0 | .. | bias l3]
LIVE = 2 * BOFF           # 3078 live columns; hyper rows may be wider (ldh)
X_TOL, LP_TOL, IMG_TOL = 1e-5, 1e-4, 5e-6

# (entry image, divergence) -> the kernel it dispatches to, and that kernel's points per workgroup
KERNEL = {("f32", False): ("cnf_rk4_kernel<false>", 32), ("f32", True): ("cnf_rk4_kernel<true>", 16),
          ("x6w", False): ("cnf_rk4_x6w_kernel", 128), ("x6n", False): ("cnf_rk4_x6_kernel<false>", 64),
          ("x6", True): ("cnf_rk4_x6_kernel<true>", 32)}
IMAGES = {False: ("f32", "x6w", "x6n"), True: ("f32", "x6")}


def rnd(seed, *shape, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).normal(0, 1, shape) * scale).astype(np.float32))


class Checks:
    """Collects every comparison of one test, records each in the report (also when one fails) and asserts at the end."""

    def __init__(self, tag):
        self.tag, self.bad = "cnf_solve:" + tag, []

    def close(self, name, got, want, tol, kernel=None):
        """|got - want| <= tol x max(1, |want|max)."""
        got, want = got.detach().cpu().double(), want.detach().cpu().double()
        assert got.shape == want.shape, "%s:%s: shape %s vs %s" % (self.tag, name, tuple(got.shape), tuple(want.shape))
        scale = max(1.0, float(want.abs().max()))
        err = float((got - want).abs().max())
        REPORT["%s:%s" % (self.tag, name)] = {"max_abs_err": err, "bound": tol * scale, "tol": tol, "ref_absmax": scale, "kernel": kernel}
        if not (bool(torch.isfinite(got).all()) and err <= tol * scale):
            self.bad.append("%s: max abs err %.3e > %.2e x %.3g" % (name, err, tol, scale))

    def exact(self, name, got, want, kernel=None):
        """Bit for bit."""
        assert got.shape == want.shape, "%s:%s: shape %s vs %s" % (self.tag, name, tuple(got.shape), tuple(want.shape))
        bad = int((got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)).sum())
        REPORT["%s:%s" % (self.tag, name)] = {"mismatches": bad, "count": got.numel(), "kernel": kernel}
        if bad:
            self.bad.append("%s: %d / %d values differ in their bits" % (name, bad, got.numel()))

    def done(self):
        try:            # one more entry, the count of failed checks; record() writes the whole report with it
            record(self.tag + ":failed_checks", len(self.bad), 0, 0)
        except AssertionError:
            pass
        assert not self.bad, self.tag + "\n" + "\n".join(self.bad)


# ---------------------------------------------------------------------------------------------
# the f64 restatement of the C contract
# ---------------------------------------------------------------------------------------------
def _cols(l, bias):
    """hyper / tcol columns of layer l's gate (bias=False) or hyper bias (bias=True)."""
    lo = l * H + (BOFF if bias else 0)
    return slice(lo, lo + (H if l < 3 else 3))


def odenet_f64(t, y, hyper, tcol, W):
    """The gated 3-512-512-512-3 ODE function on y (BT, n, 3): per layer (y w^T + b) * sigmoid(hyper[gate] + t tcol[gate])
    + hyper[bias] + t tcol[bias], softplus after the three hidden layers."""
    dx = y
    for l in range(4):
        gate = torch.sigmoid(hyper[:, _cols(l, False)] + t * tcol[_cols(l, False)])
        beta = hyper[:, _cols(l, True)] + t * tcol[_cols(l, True)]
        dx = F.linear(dx, W["w%d" % l], W["b%d" % l]) * gate.unsqueeze(1) + beta.unsqueeze(1)
        if l < 3:
            dx = F.softplus(dx)
    return dx


def mbn_f64(p, x, lp, reverse):
    """MovingBatchNorm with its running statistics, p = [weight(3) | bias(3) | running_mean(3) | running_var(3)]."""
    w, b, mean, var = p[0:3], p[3:6], p[6:9], p[9:12]
    if reverse:
        x = (x - b) * torch.exp(-w)
        x = x * torch.exp(0.5 * torch.log(var + 1e-4)) + mean
    else:
        x = (x - mean) * torch.exp(-0.5 * torch.log(var + 1e-4))
        x = x * torch.exp(w) + b
    if lp is not None:
        logdet = (-0.5 * torch.log(var + 1e-4) + w).sum()
        lp = lp + logdet if reverse else lp - logdet
    return x, lp


def cnf_solve_f64(y, hyper, tcol, w0, b0, w1, b1, w2, b2, w3, b3, t_end, steps, reverse, mbn_in=None, mbn_out=None, e=None, logp=None):
    """What one caspr_cnf_rk4_* launch computes, in f64 on the CPU: (x (BT,n,3), logp (BT,n,1) or None).  Reads only the 3078 live
    columns of every hyper row; t_end as given (the kernels take it as a float)."""
    d = lambda v: None if v is None else v.detach().cpu().double()
    y, hyper, tcol, e, logp, mbn_in, mbn_out = d(y), d(hyper), d(tcol), d(e), d(logp), d(mbn_in), d(mbn_out)
    W = {k: d(v) for k, v in (("w0", w0), ("b0", b0), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2), ("w3", w3), ("b3", b3))}
    x, lp = y, logp
    if mbn_in is not None:
        x, lp = mbn_f64(mbn_in, x, lp, reverse)

    def f(t, x_):
        if e is None:
            return odenet_f64(t, x_, hyper, tcol, W), None
        dy, je = torch.func.jvp(lambda z: odenet_f64(t, z, hyper, tcol, W), (x_,), (e,))
        return dy, -(je * e).sum(-1, keepdim=True)          # d logp / dt = -e^T J e

    T = float(t_end)
    t0, t1 = (T, 0.0) if reverse else (0.0, T)
    h = (t1 - t0) / steps
    for s in range(steps):
        t = t0 + s * h
        k1, l1 = f(t, x)
        k2, l2 = f(t + 0.5 * h, x + 0.5 * h * k1)
        k3, l3 = f(t + 0.5 * h, x + 0.5 * h * k2)
        k4, l4 = f(t + h, x + h * k3)
        x = x + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        if e is not None:
            lp = lp + (h / 6.0) * (l1 + 2.0 * l2 + 2.0 * l3 + l4)
    if mbn_out is not None:
        x, lp = mbn_f64(mbn_out, x, lp, reverse)
    return x, (lp if e is not None else None)


# ---------------------------------------------------------------------------------------------
# kernel inputs from a state dict, assembled as CNF._weights / CNF.integrate assemble them
# ---------------------------------------------------------------------------------------------
LAYER = "point_cnf.chain.1.odefunc.diffeq.layers.%d."


def block_params(sd, dtype=torch.float64):
    L = [LAYER % l for l in range(4)]
    g = lambda k: sd[k].to(dtype)
    whyp = torch.cat([torch.cat([g(l + "_hyper_gate.weight") for l in L]), torch.cat([g(l + "_hyper_bias.weight") for l in L])])
    gate_b = torch.cat([g(l + "_hyper_gate.bias") for l in L])
    P = {"whyp": whyp, "hyp_bias": torch.cat([gate_b, torch.zeros_like(gate_b)]), "tcol": whyp[:, 0].contiguous(),
         "t_end": float(g("point_cnf.chain.1.sqrt_end_time").reshape(())) ** 2}
    for l in range(4):
        P["w%d" % l], P["b%d" % l] = g(L[l] + "_layer.weight").contiguous(), g(L[l] + "_layer.bias").contiguous()
    return P


def hyper_of(P, c):
    """The hyper-network conv of CNF.integrate: columns 1.. of the hyper weights times the context, plus the gate biases."""
    return c.to(P["whyp"].dtype) @ P["whyp"][:, 1:].T + P["hyp_bias"]


def mbn_of(sd, i, dtype=torch.float64):
    pre = "point_cnf.chain.%d." % i
    return torch.cat([sd[pre + k].to(dtype) for k in ("weight", "bias", "running_mean", "running_var")])


def solve_args(P):
    return [P[k] for k in ("tcol", "w0", "b0", "w1", "b1", "w2", "b2", "w3", "b3")]


# ---------------------------------------------------------------------------------------------
# 1. the restatement against the oracle (CPU)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["seeded", "stress"])
def test_restatement_matches_oracle(which, seeded_sd, stress_sd):
    """cnf_solve_f64 on hyper / tcol built as the model builds them == oracle.point_cnf (MBN, CNF block, MBN) and oracle.cnf_block (no
    MBN) in f64, to round-off: sampling and density direction, with and without the divergence."""
    sd = {k: v.double() for k, v in (seeded_sd if which == "seeded" else stress_sd).items()}
    P = block_params(sd)
    BT, n, steps = 2, 40, 3
    c, y = rnd(1, BT, 1600).double(), rnd(2, BT, n, 3, scale=1.5).double()
    e, lp0 = rnd(3, BT, n, 3).double(), rnd(4, BT, n, 1).double()
    hyper = hyper_of(P, c)
    assert hyper.shape == (BT, LIVE)
    ck = Checks("pin_%s" % which)
    for reverse in (True, False):
        for div in (False, True):
            tag = "%s_%s" % ("rev" if reverse else "fwd", "div" if div else "nodiv")
            mi, mo = (mbn_of(sd, 2), mbn_of(sd, 0)) if reverse else (mbn_of(sd, 0), mbn_of(sd, 2))
            gx, glp = cnf_solve_f64(y, hyper, *solve_args(P), P["t_end"], steps, reverse, mi, mo, e=e if div else None, logp=lp0 if div else None)
            want = O.point_cnf(sd, y, c, lp0 if div else None, reverse, "rk4", steps, e if div else None)
            wx, wlp = want if div else (want, None)
            ck.close(tag + ":x", gx, wx, 1e-12)
            if div:
                ck.close(tag + ":logp", glp, wlp, 1e-12)
            # no MBN at either end: the bare block
            gx, glp = cnf_solve_f64(y, hyper, *solve_args(P), P["t_end"], steps, reverse, e=e if div else None, logp=lp0 if div else None)
            wx, wlp = O.cnf_block(sd, "point_cnf.chain.1", y, c, lp0 if div else None, reverse, "rk4", steps, e if div else None)
            ck.close(tag + "_nombn:x", gx, wx, 1e-12)
            if div:
                ck.close(tag + "_nombn:logp", glp, wlp, 1e-12)
    ck.done()


# ---------------------------------------------------------------------------------------------
# GPU side: weights, inputs, launches
# ---------------------------------------------------------------------------------------------
# MovingBatchNorm parameter sets [weight | bias | running_mean | running_var], chosen per position and direction so that the state the
# ODE sees stays within |y| ~ 7 while every set holds weight = +-2 and a running_var at or below the 1e-4 floor.
MBN_SETS = {
    (True, "in"): [-2.0, 2.0, -0.5, 0.3, -0.2, 0.1, 0.8, -1.2, 0.5, 0.0, 1e-5, 0.5],      # sampling, first: shrinks
    (True, "out"): [2.0, -2.0, 0.3, -0.1, 0.4, 0.0, 0.05, 0.2, -0.3, 1e-6, 3.0, 0.0],      # sampling, last
    (False, "in"): [-2.0, 0.5, 2.0, 0.2, -0.1, 0.3, 0.1, -0.3, 0.2, 3.0, 1.5, 30.0],       # density direction, first
    (False, "out"): [2.0, -2.0, 0.7, -0.3, 0.2, 0.1, 0.4, -0.6, 0.0, 0.0, 2e-5, 1.0],      # density direction, last: x 739 on x
}


class Weights:
    """One weight set: f32 CPU copies (the restatement's inputs, upcast) and the device tensors / packs the launches take."""

    def __init__(self, sd, dev):
        from caspr_amd import ops
        P32 = block_params(sd, torch.float32)
        self.P64 = block_params(sd)
        self.cpu = {k: P32[k] for k in ("tcol", "w0", "b0", "w1", "b1", "w2", "b2", "w3", "b3")}
        self.dev = {k: v.to(dev).contiguous() for k, v in self.cpu.items()}
        self.w1p, self.w2p = ops.PackedWeight(self.dev["w1"]), ops.PackedWeight(self.dev["w2"])
        self.w1x, self.w2x = ops.pack_cnf_x6(self.dev["w1"]), ops.pack_cnf_x6(self.dev["w2"])
        self.t_end = float(np.float32(P32["t_end"]))          # what the float argument of the C entry holds

    def hyper(self, c, ldh):
        """(BT, ldh) f32 rows: the live columns in f64, rounded once; columns past 3078 hold NaN."""
        hy = hyper_of(self.P64, c).float()
        out = torch.full((c.shape[0], ldh), float("nan"), dtype=torch.float32)
        out[:, :LIVE] = hy
        return out.contiguous()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights(dev, seeded_sd, stress_sd):
    return {"seeded": Weights(seeded_sd, dev), "stress": Weights(stress_sd, dev)}


def launch(img, W, y, hyper, steps, reverse, mbn_in=None, mbn_out=None, e=None, logp=None, narrow=None):
    """One ops.cnf_rk4 call on image img ("f32" | "x6w" | "x6n" | "x6"); CPU tensors are moved to the device."""
    from caspr_amd import ops
    g = lambda v: None if v is None else v.to("cuda:0").contiguous()
    D = W.dev
    x6 = img != "f32"
    return ops.cnf_rk4(g(y), g(hyper), D["tcol"], D["w0"], D["b0"], W.w1p, D["b1"], W.w2p, D["b2"], D["w3"], D["b3"], W.t_end, steps,
                       reverse, g(mbn_in), g(mbn_out), e=g(e), logp=g(logp), w1x=W.w1x if x6 else None, w2x=W.w2x if x6 else None,
                       narrow=(img == "x6n") if narrow is None else narrow)


def reference(W, y, hyper, steps, reverse, mbn_in=None, mbn_out=None, e=None, logp=None):
    return cnf_solve_f64(y, hyper, *[W.cpu[k] for k in ("tcol", "w0", "b0", "w1", "b1", "w2", "b2", "w3", "b3")], W.t_end, steps, reverse,
                         mbn_in, mbn_out, e=e, logp=logp)


def base_samples(seed, BT, n):
    """|y| up to 5: N(0, 1.3^2) clipped, and the first point of every frame at a corner of the [-5, 5] box."""
    y = rnd(seed, BT, n, 3, scale=1.3).clamp(-5.0, 5.0)
    y[:, 0] = torch.tensor([5.0, -5.0, 5.0])
    return y.contiguous()


def mbn_pair(reverse, which):
    mk = lambda pos: torch.tensor(MBN_SETS[(bool(reverse), pos)], dtype=torch.float32)
    return (mk("in") if which in ("both", "in") else None), (mk("out") if which in ("both", "out") else None)


# ---------------------------------------------------------------------------------------------
# 2. route x edge matrix
# ---------------------------------------------------------------------------------------------
N_EDGES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 1000)
MBNS = ("both", "in", "out", "none")
LDHS = (3078, 3091, 3080)


def _cases():
    """Every route sees every n edge (each case runs all images of its divergence setting); the (direction, MBN) combinations
    cycle with period 8 along the n list, so each of the 8 appears on every route; ldh, BT, steps and the weight set cycle too."""
    out = []
    for div in (False, True):
        for i, n in enumerate(N_EDGES):
            j = i + (3 if div else 0)
            reverse, mbn = j % 2 == 0, MBNS[(j // 2) % 4]
            steps = 2 if n > 129 else (1, 2, 8)[i % 3]
            BT = 17 if n == (65 if not div else 31) else (5 if i % 2 else 1)
            out.append(dict(div=div, n=n, BT=BT, steps=steps, reverse=reverse, mbn=mbn, ldh=LDHS[i % 3], w="seeded" if i % 4 == 3 else "stress"))
        # the stressed dynamics at a step count where RK4 has converged
        out.append(dict(div=div, n=33, BT=2, steps=40, reverse=not div, mbn="both", ldh=3091, w="stress"))
    return out


CASES = _cases()


def _case_id(c):
    return "%s-n%d-bt%d-s%d-%s-mbn_%s-ldh%d-%s" % ("div" if c["div"] else "nodiv", c["n"], c["BT"], c["steps"], "rev" if c["reverse"] else "fwd",
                                                c["mbn"], c["ldh"], c["w"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_route_matrix(dev, weights, case):
    """Every image of the case's divergence setting against the f64 restatement, against the f32-MFMA kernel (the bf16x6 images) and
    the narrow sampling kernel against the 128-point one; every launch twice, bit for bit."""
    W = weights[case["w"]]
    BT, n, steps, reverse, div = case["BT"], case["n"], case["steps"], case["reverse"], case["div"]
    seed = 1000 + n
    c, y = rnd(seed, BT, 1600), base_samples(seed + 1, BT, n)
    e, lp0 = (rnd(seed + 2, BT, n, 3), rnd(seed + 3, BT, n, 1)) if div else (None, None)
    hyper = W.hyper(c, case["ldh"])
    mi, mo = mbn_pair(reverse, case["mbn"])
    wx, wlp = reference(W, y, hyper, steps, reverse, mi, mo, e, lp0)
    ck = Checks("route:" + _case_id(case))
    got = {}
    for img in IMAGES[div]:
        kern = KERNEL[(img, div)][0]
        r1 = launch(img, W, y, hyper, steps, reverse, mi, mo, e, lp0)
        r2 = launch(img, W, y, hyper, steps, reverse, mi, mo, e, lp0)
        torch.cuda.synchronize()
        x1, l1 = (r1 if div else (r1, None))
        x2, l2 = (r2 if div else (r2, None))
        got[img] = (x1, l1)
        ck.close(img + ":x", x1, wx, X_TOL, kern)
        ck.exact(img + ":repeat_x", x2, x1, kern)
        if div:
            ck.close(img + ":logp", l1, wlp, LP_TOL, kern)
            ck.exact(img + ":repeat_logp", l2, l1, kern)
    for img in IMAGES[div][1:]:
        ck.close(img + "_vs_f32:x", got[img][0], got["f32"][0], IMG_TOL, KERNEL[(img, div)][0])
        if div:
            ck.close(img + "_vs_f32:logp", got[img][1], got["f32"][1], LP_TOL, KERNEL[(img, div)][0])
    if not div:
        ck.close("x6n_vs_x6w:x", got["x6n"][0], got["x6w"][0], IMG_TOL, KERNEL[("x6n", False)][0])
    ck.done()


# ---------------------------------------------------------------------------------------------
# 3. invariances the kernels promise
# ---------------------------------------------------------------------------------------------
ALL_ROUTES = [("f32", False), ("x6w", False), ("x6n", False), ("f32", True), ("x6", True)]


@pytest.mark.gpu
@pytest.mark.parametrize("img,div", ALL_ROUTES, ids=["%s-%s" % (i, "div" if d else "nodiv") for i, d in ALL_ROUTES])
def test_frame_invariance(dev, weights, img, div):
    """include/caspr_hip.h: a frame's result does not depend on the batch around it.  Frame k of a BT = 5 launch == frame k launched
    alone == frame k inside a launch with the frames permuted, bit for bit (a frame is grid row blockIdx.y; nothing in a workgroup's
    arithmetic depends on it)."""
    W = weights["stress"]
    BT, n, steps = 5, 100, 2
    reverse = not div
    c, y = rnd(71, BT, 1600), base_samples(72, BT, n)
    e, lp0 = (rnd(73, BT, n, 3), rnd(74, BT, n, 1)) if div else (None, None)
    hyper = W.hyper(c, 3091)
    mi, mo = mbn_pair(reverse, "both")
    kern = KERNEL[(img, div)][0]
    sel = lambda v, idx: None if v is None else v[idx].contiguous()
    split = lambda r: r if div else (r, None)
    ck = Checks("frames:%s-%s" % (img, "div" if div else "nodiv"))
    bx, blp = split(launch(img, W, y, hyper, steps, reverse, mi, mo, e, lp0))
    perm = [3, 0, 4, 1, 2]
    px, plp = split(launch(img, W, sel(y, perm), sel(hyper, perm), steps, reverse, mi, mo, sel(e, perm), sel(lp0, perm)))
    for k in range(BT):
        ax, alp = split(launch(img, W, sel(y, [k]), sel(hyper, [k]), steps, reverse, mi, mo, sel(e, [k]), sel(lp0, [k])))
        ck.exact("frame%d_alone:x" % k, bx[k:k + 1], ax, kern)
        ck.exact("frame%d_permuted:x" % k, px[perm.index(k)], bx[k], kern)
        if div:
            ck.exact("frame%d_alone:logp" % k, blp[k:k + 1], alp, kern)
            ck.exact("frame%d_permuted:logp" % k, plp[perm.index(k)], blp[k], kern)
    wx, wlp = reference(W, y, hyper, steps, reverse, mi, mo, e, lp0)
    ck.close("batch:x", bx, wx, X_TOL, kern)
    if div:
        ck.close("batch:logp", blp, wlp, LP_TOL, kern)
    ck.done()


@pytest.mark.gpu
@pytest.mark.parametrize("img", ["f32", "x6w", "x6n"])
def test_point_independence(dev, weights, img):
    """Without the divergence every point's trajectory is its own: the first m points of an n-point launch == an m-point launch, for m
    one below and one above the kernel's workgroup edge.  Bitwise: a point is one column of every matrix product (an MFMA's output
    column depends on its own input column only), the output layer and the RK4 update run per point, padding lanes of a ragged
    workgroup only feed their own columns, and the point keeps its workgroup (hence the f32 kernel's k-order rotation) in both
    launches."""
    W = weights["stress"]
    kern, pt = KERNEL[(img, False)]
    BT, n, steps = 2, 300, 2
    c, y = rnd(81, BT, 1600), base_samples(82, BT, n)
    hyper = W.hyper(c, 3078)
    mi, mo = mbn_pair(True, "both")
    full = launch(img, W, y, hyper, steps, True, mi, mo)
    wx, _ = reference(W, y, hyper, steps, True, mi, mo)
    ck = Checks("points:" + img)
    ck.close("n%d:x" % n, full, wx, X_TOL, kern)
    for m in (pt - 1, pt + 1):
        part = launch(img, W, y[:, :m].contiguous(), hyper, steps, True, mi, mo)
        ck.exact("first%d_of_%d:x" % (m, n), full[:, :m], part, kern)
        ck.close("first%d_vs_f64:x" % m, part, wx[:, :m], X_TOL, kern)
    ck.done()


@pytest.mark.gpu
def test_narrow_flag_does_not_leak(dev, weights, monkeypatch):
    """ops.cnf_rk4 passes CASPR_CNF_NARROW only to the bf16x6 entry and only without the divergence: with e given, narrow=True runs
    the same launch as narrow=False (same bits), and the f32 entry never sees the flag (same bits, its `reverse` argument is 0 / 1)."""
    from caspr_amd import lib as _lib
    from caspr_amd import ops
    W = weights["stress"]
    BT, n, steps = 3, 70, 2
    c, y = rnd(91, BT, 1600), base_samples(92, BT, n)
    e, lp0 = rnd(93, BT, n, 3), rnd(94, BT, n, 1)
    hyper = W.hyper(c, 3080)
    L = _lib.load()
    seen = []

    def spy(name):
        real = getattr(L, name)

        def call(*a):
            seen.append((name, int(a[15])))          # the `reverse` argument (include/caspr_hip.h)
            return real(*a)
        return call
    monkeypatch.setattr(L, "caspr_cnf_rk4_f32", spy("caspr_cnf_rk4_f32"))
    monkeypatch.setattr(L, "caspr_cnf_rk4_x6_f32", spy("caspr_cnf_rk4_x6_f32"))
    ck = Checks("flag")
    for reverse in (True, False):
        mi, mo = mbn_pair(reverse, "both")
        for img in ("f32", "x6"):
            seen.clear()
            a = launch(img, W, y, hyper, steps, reverse, mi, mo, e, lp0, narrow=False)
            b = launch(img, W, y, hyper, steps, reverse, mi, mo, e, lp0, narrow=True)
            kern = KERNEL[(img, True)][0]
            tag = "%s_div_%s" % (img, "rev" if reverse else "fwd")
            ck.exact(tag + ":x", b[0], a[0], kern)
            ck.exact(tag + ":logp", b[1], a[1], kern)
            assert [f for _, f in seen] == [int(reverse)] * 2, (tag, seen)
        seen.clear()
        a = launch("f32", W, y, hyper, steps, reverse, mi, mo, narrow=False)
        b = launch("f32", W, y, hyper, steps, reverse, mi, mo, narrow=True)
        ck.exact("f32_nodiv_%s:x" % ("rev" if reverse else "fwd"), b, a, KERNEL[("f32", False)][0])
        assert seen == [("caspr_cnf_rk4_f32", int(reverse))] * 2, seen
        seen.clear()
        launch("x6n", W, y, hyper, steps, reverse, mi, mo)
        assert seen == [("caspr_cnf_rk4_x6_f32", int(reverse) | ops.CNF_NARROW)], seen
    ck.done()


# ---------------------------------------------------------------------------------------------
# 4. the accuracy guard's check solve, end to end
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_guard_check_solve_is_narrow_and_exact(dev, seeded_sd, stress_sd, monkeypatch):
    """CaSPR.reconstruct with the accuracy guard on (test_accuracy_guard's setup: 256 samples per frame, check_points = 64): the check
    solve is ONE ops.cnf_rk4 call on the 64-point sampling kernel at half the step count; its samples equal the f64 restatement on the
    very arguments it was given; and the guard's verdict is the one the f64 step-halving estimate gives -- quiet on the seeded weights at
    8 steps, tripped on the stress weights at 8 steps with an estimate in test_accuracy_guard's range."""
    from caspr_amd import ops
    from caspr_amd.models import CaSPR
    from caspr_amd.utils.synthetic import car_sequences
    x, sp = car_sequences(2, 4, 1024, seed=5)
    ts = sp[0, :, 0, 3].to(dev)
    torch.manual_seed(9)
    yb = torch.randn(2, 4, 256, 3).to(dev)
    real = ops.cnf_rk4
    names = list(inspect.signature(real).parameters)
    calls = []

    def spy(*args, **kw):
        out = real(*args, **kw)
        bound = dict(zip(names, args))
        bound.update(kw)
        # the clone runs on the caller's stream (the guard's own for the check solve): ordered after the launch
        calls.append((bound, out.clone() if torch.is_tensor(out) else tuple(o.clone() for o in out)))
        return out
    monkeypatch.setattr(ops, "cnf_rk4", spy)
    prev = ops.set_matmul_mode(cnf=True)
    ck = Checks("guard")
    try:
        for which, sd, lat, quiet in (("seeded", seeded_sd, 2, True), ("stress", stress_sd, 16, False)):
            m = CaSPR(cnf_rk4_steps=8, latent_rk4_steps=lat, check_tol=1e-5, check_action="warn")
            m.load_state_dict(sd)
            m = m.to(dev).eval()
            ops.reset_guard()
            calls.clear()
            with torch.no_grad(), warnings.catch_warnings(record=True) as wrec:
                warnings.simplefilter("always")
                m.reconstruct(x.to(dev), num_points=256, timestamps=ts, y=yb)
                ops.check_deferred_errors()
            torch.cuda.synchronize()
            main = [cl for cl in calls if not cl[0].get("narrow")]
            check = [cl for cl in calls if cl[0].get("narrow")]
            assert len(main) == 1 and len(check) == 1, [(cl[0].get("narrow"), tuple(cl[0]["y"].shape)) for cl in calls]
            a, got = check[0]
            am, gm = main[0]
            assert a["e"] is None and a["w1x"] is not None and a["steps"] == 4 and am["steps"] == 8, a["steps"]
            assert a["y"].shape[1] == 64 and am["y"].shape[1] == 256 and bool(a["reverse"]), tuple(a["y"].shape)
            assert torch.equal(a["y"], am["y"][:, :64]) and torch.equal(a["hyper"][:, :LIVE], am["hyper"][:, :LIVE])
            Wc = {k: a[k].cpu() for k in ("tcol", "w0", "b0", "b1", "b2", "w3", "b3")}
            P = block_params(sd, torch.float32)          # the hidden weights the two packs were made from
            args = [Wc["tcol"], Wc["w0"], Wc["b0"], P["w1"], Wc["b1"], P["w2"], Wc["b2"], Wc["w3"], Wc["b3"]]
            t_end = float(np.float32(a["t_end"]))
            w4, _ = cnf_solve_f64(a["y"], a["hyper"], *args, t_end, 4, True, a["mbn_in"], a["mbn_out"])
            w8, _ = cnf_solve_f64(a["y"], a["hyper"], *args, t_end, 8, True, a["mbn_in"], a["mbn_out"])
            ck.close(which + ":check_solve_x", got, w4, X_TOL, KERNEL[("x6n", False)][0])
            ck.close(which + ":main_solve_first64_x", gm[:, :64], w8, X_TOL, KERNEL[("x6w", False)][0])
            rep = dict(ops.GUARD_LAST)["cnf"]
            xmax = max(1.0, float(w8.abs().max()))
            est64 = float((w8 - w4).abs().max()) / 15.0
            bound64 = 1e-5 * (1.0 + float(w8.abs().max()))
            REPORT["cnf_solve:guard:%s:verdict" % which] = {"guard": rep, "f64_estimate": est64, "f64_bound": bound64}
            assert rep["steps"] == 8 and rep["other_steps"] == 4, rep
            assert rep["ok"] == quiet == (est64 <= bound64), (rep, est64, bound64)
            # each of the two solves is within the state bound of its f64 value: so is the estimate, to 2 / 15 of it
            assert abs(rep["estimate"] - est64) <= 2.0 * X_TOL * xmax / 15.0, (rep, est64)
            if quiet:
                assert rep["estimate"] <= 1e-6 and not any("point CNF" in str(w_.message) for w_ in wrec), rep
            else:
                assert 2e-4 <= rep["estimate"] <= 2e-1 and any("point CNF" in str(w_.message) for w_ in wrec), rep
    finally:
        ops.set_matmul_mode(cnf=prev[1])
    ck.done()
