"""What the three adaptive Dormand-Prince solves share (csrc/dp5_rules.h, dp5.h): the pure rules agree with
oracle.model.dopri5_solve's arithmetic, and the one host driver behind caspr_cnf_dopri5_f32 and caspr_cnf_dopri5_h3_f32 refuses and
gives up on every route as each entry did on its own.  (That each shared text exists once: test_cnf_dopri5_f16x3_surface.py.)"""
import math
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.join(os.path.dirname(__file__), "..")
CSRC = os.path.join(ROOT, "caspr_amd", "csrc")


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """tools/dp5_rules_check.cpp built by the host compiler: dp5_rules.h needs neither HIP nor a GPU."""
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("dp5") / "dp5_rules_check")
    subprocess.check_call([cxx, "-O2", "-std=c++11", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tools", "dp5_rules_check.cpp")])
    return lambda *a: float(subprocess.check_output([exe] + [repr(float(x)) if not isinstance(x, str) else x for x in a]).decode())


def test_pure_rules_against_the_oracle_arithmetic(rules):
    """The step-size rule, the initial step and the interpolant as oracle.model.dopri5_solve writes them (model.py:228-233, 252-257,
    263-275), in f64.  The f32 rules round at most eight times (sqrt, pow, two divisions, min, max and the operands' conversions; powf
    within 2 ulp): 1e-6 relative holds 16 f32 roundings.  The interpolant is f64 in the same order of operations: 1e-14."""
    def next_dt(r, dt):
        if r == 0:
            return dt * 10.0
        dfactor = 1.0 if r < 1 else 0.2
        return dt / max(1.0 / 10.0, min(math.sqrt(r) ** (1.0 / 5.0) / 0.9, 1.0 / dfactor))
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    # r = 0; far below 1 (growth capped at 10); just under and just over 1; moderate; large enough for the 1 / DFACTOR clamp
    for r in (0.0, 1e-20, 0.999999, 1.000001, 4.0, 3e3, 1e12):
        for dt in (0.1, 3.7e-4):
            r_, dt_ = f32(r), f32(dt)
            got, want = rules("next", r_, dt_), next_dt(r_, dt_)
            assert abs(got - want) <= 1e-6 * want, (r, dt, got, want)
    assert abs(rules("next", 1e-20, 0.5) - 5.0) <= 5e-6 and abs(rules("next", 1e12, 0.5) - 0.1) <= 1e-7      # the two clamps: x 10, x 0.2
    assert rules("h0", 1e-6, 3.0) == 1e-6 and rules("h0", 2.0, 1e-6) == 1e-6
    assert rules("h0", 2.0, 3.0) == 0.01 * (2.0 / 3.0)
    for d1, d2, h0 in ((3.0, 1e-4, 2e-2), (3.0, 7.0, 2e-2), (0.3, 0.2, 1e-6), (0.0, 0.0, 1e-2)):
        d1_, d2_, h0_ = f32(d1), f32(d2), f32(h0)
        h1 = max(1e-6, h0_ * 1e-3) if (d1_ <= 1e-15 and d2_ <= 1e-15) else (0.01 / max(d1_, d2_)) ** (1.0 / 5.0)
        want = min(100 * h0_, h1)
        assert abs(rules("first", d1_, d2_, h0_) - want) <= 1e-6 * want, (d1, d2, h0)
    y0, y1, ym, fa, fb, h = 0.3, 0.9, 0.55, 1.7, 2.4, 0.25
    A = 2 * h * (fb - fa) - 8 * (y1 + y0) + 16 * ym
    B = h * (5 * fa - 3 * fb) + 18 * y0 + 14 * y1 - 32 * ym
    C = h * (fb - 4 * fa) - 11 * y0 - 5 * y1 + 16 * ym
    D = h * fa
    for x in (0.0, 0.5, 1.0, 0.3125):
        want = ((((A * x) + B) * x + C) * x + D) * x + y0
        assert abs(rules("interp", y0, y1, ym, fa, fb, h, x) - want) <= 1e-14, x
    assert rules("interp", y0, y1, ym, fa, fb, h, 0.0) == y0
    assert abs(rules("interp", y0, y1, ym, fa, fb, h, 1.0) - y1) <= 1e-14 and abs(rules("interp", y0, y1, ym, fa, fb, h, 0.5) - ym) <= 1e-14


# ---------------------------------------------------------------------------------------------
# GPU: the one host driver (dp5.h: dp5_check, dp5_run) behind both entries, every route
# ---------------------------------------------------------------------------------------------
EINVAL, EUNSUP, ENOCONV = -1, -3, -4
# (route, entry's name in its messages, n): the smallest n that crosses a workgroup boundary -- 64 points a workgroup, 32 with the
# divergence, 128 on the f16x3 route (one full workgroup and one with two points)
ROUTES = (("bf16x6", "cnf_dopri5", 65), ("bf16x6-div", "cnf_dopri5", 33), ("f16x3", "cnf_dopri5_h3", 130))
BT = 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def W(dev, stress_sd):
    from caspr_amd import ops
    from test_cnf_solve_kernels import Weights
    w = Weights(stress_sd, dev)
    w.w1h, w.w2h = ops.pack_cnf_h3(w.dev["w1"]), ops.pack_cnf_h3(w.dev["w2"])
    return w


class Call:
    """One direct call of a route's C entry (ops.cnf_dopri5 sizes the workspace itself and refuses a capture before the entry sees
    it).  Everything is allocated here, nothing inside the call."""

    def __init__(self, W, dev, route, n, max_attempts):
        from caspr_amd import lib
        from test_cnf_solve_kernels import base_samples, rnd
        self.L, self.W, self.route, self.n, self.max_attempts = lib.load(), W, route, n, max_attempts
        self.y = base_samples(61, BT, n).to(dev).contiguous()
        self.hyper = W.hyper(rnd(62, BT, 1600, scale=0.5), 3080).to(dev).contiguous()
        div = route == "bf16x6-div"
        self.e = rnd(63, BT, n, 3).to(dev).contiguous() if div else None
        self.lp = rnd(64, BT, n, 1).to(dev).contiguous() if div else None
        self.lp_out = torch.empty(BT, n, 1, device=dev) if div else None
        self.out = torch.empty_like(self.y)
        self.trace = torch.empty(BT, 8 + 5 * max_attempts, device=dev)
        self.counters = torch.full((BT, 4), -1, device=dev, dtype=torch.int32)
        self.word = torch.zeros(1, device=dev, dtype=torch.int32)
        self.ws_bytes = (self.L.caspr_cnf_dopri5_h3_ws_bytes if route == "f16x3" else self.L.caspr_cnf_dopri5_ws_bytes)
        self.need = self.ws_bytes(BT, n, max_attempts)
        self.ws = torch.empty(self.need + 256, device=dev, dtype=torch.uint8)
        assert self.ws.data_ptr() % 256 == 0

    def __call__(self, ws_ptr=None, ws_bytes=None, tol=1e-6):
        from caspr_amd.ops import _p, _stream
        import ctypes
        W, D, L = self.W, self.W.dev, self.L
        ws_ptr = ctypes.c_void_p(self.ws.data_ptr() if ws_ptr is None else ws_ptr)
        ws_bytes = self.need if ws_bytes is None else ws_bytes
        if self.route == "f16x3":
            rc = L.caspr_cnf_dopri5_h3_f32(_p(self.y), _p(self.hyper), self.hyper.shape[1], _p(D["tcol"]), _p(D["w0"]), _p(D["b0"]), _p(W.w1h), _p(D["b1"]),
                                           _p(W.w2h), _p(D["b2"]), _p(D["w3"]), _p(D["b3"]), D["w0"].shape[0], float(W.t_end), tol, tol, self.max_attempts, 1,
                                           _p(None), _p(None), _p(self.word), _p(self.out), BT, self.n, ws_ptr, ws_bytes, _p(self.trace), _p(self.counters), _stream())
        else:
            rc = L.caspr_cnf_dopri5_f32(_p(self.y), _p(self.hyper), self.hyper.shape[1], _p(D["tcol"]), _p(D["w0"]), _p(D["b0"]), _p(W.w1x), _p(D["b1"]),
                                        _p(W.w2x), _p(D["b2"]), _p(D["w3"]), _p(D["b3"]), D["w0"].shape[0], float(W.t_end), tol, tol, self.max_attempts, 1,
                                        _p(None), _p(None), _p(self.e), _p(self.lp), _p(self.lp_out), _p(self.out), BT, self.n, ws_ptr, ws_bytes,
                                        _p(self.trace), _p(self.counters), _stream())
        return rc, (L.caspr_last_error_string() or b"").decode()


@pytest.mark.gpu
@pytest.mark.parametrize("route,name,n", ROUTES, ids=[r[0] for r in ROUTES])
def test_host_driver_refusals(dev, W, route, name, n):
    """Workspace one byte short, workspace misaligned by 16, a capturing stream, and *_ws_bytes of non-positive sizes: refused on the
    host, with the entry's own name in the message, before anything is launched (the counters keep their fill)."""
    call = Call(W, dev, route, n, 5)
    assert call.need > 0 and call.need % 256 == 0
    for bad in ((0, n, 5), (BT, 0, 5), (BT, n, 0), (-1, n, 5), (BT, -3, 5), (BT, n, -1)):
        assert call.ws_bytes(*bad) == 0, bad
    want = "%s: workspace of %d bytes, 256-byte aligned, needed" % (name, call.need)
    assert call(ws_bytes=call.need - 1) == (EINVAL, want)
    assert call(ws_ptr=call.ws.data_ptr() + 16, ws_bytes=call.need + 240) == (EINVAL, want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc, msg = call()
    assert rc == EUNSUP and msg == "%s: the host loop reads the device after every attempt and cannot run under stream capture" % name
    torch.cuda.synchronize()
    assert bool((call.counters == -1).all()), "a refused call launched something"


@pytest.mark.gpu
@pytest.mark.parametrize("route,name,n", ROUTES, ids=[r[0] for r in ROUTES])
def test_host_driver_budget(dev, W, route, name, n):
    """max_attempts = 1 at 1e-6 on the stress weights: four launches, then CASPR_ENOCONV; both frames unfinished with their one
    attempt and its eight evaluations counted, and the message names the frames."""
    call = Call(W, dev, route, n, 1)
    rc, msg = call()
    torch.cuda.synchronize()
    c = call.counters.cpu()
    assert rc == ENOCONV and msg.startswith("%s: %d of %d frames did not reach t_end within max_attempts = 1 " % (name, BT, BT)), (rc, msg)
    assert c[:, 3].tolist() == [0] * BT and (c[:, 0] + c[:, 1]).tolist() == [1] * BT and c[:, 2].tolist() == [8] * BT, c
