"""The f16x3 point-CNF sampling kernel (csrc/ode_f16x3w.hip, ops.cnf_rk4(w1h=, w2h=), config.cnf_split = "f16x3") launch by launch:
against the f64 restatement of test_cnf_solve_kernels, against the bf16x6 128-point image, its routing, frame invariance, weight
range, range guard, and the option at model level.  Bounds are that file's: X_TOL = 1e-5 against f64, IMG_TOL = 5e-6 between images,
both x max(1, |x|max); the model-level comparison of the two splits is held to 5e-6 flat."""
import copy
import os
import subprocess
import warnings

import pytest
import torch

from test_hip_parity import REPORT, record
from test_cnf_solve_kernels import (Checks, IMG_TOL, LDHS, MBNS, X_TOL, Weights, base_samples, cnf_solve_f64, dev, launch, mbn_pair,  # noqa: F401
                                    reference, rnd, weights)

pytestmark = pytest.mark.gpu
KERN = "cnf_rk4_h3w_kernel"
MODEL_TOL = 5e-6            # |x_f16x3 - x_bf16x6| at model level, flat (no scaling by |x|)


def _packs(W):
    from caspr_amd import ops
    if not hasattr(W, "w1h"):
        W.w1h, W.w2h = ops.pack_cnf_h3(W.dev["w1"]), ops.pack_cnf_h3(W.dev["w2"])
    return W


def launch_h3(W, y, hyper, steps, reverse, mbn_in=None, mbn_out=None, e=None, logp=None, narrow=False, h3=True):
    """ops.cnf_rk4 with the bf16x6 packs and (h3) the f16 packs: the f16x3 kernel where the routing rule allows it."""
    from caspr_amd import ops
    _packs(W)
    g = lambda v: None if v is None else v.to("cuda:0").contiguous()
    D = W.dev
    return ops.cnf_rk4(g(y), g(hyper), D["tcol"], D["w0"], D["b0"], W.w1p, D["b1"], W.w2p, D["b2"], D["w3"], D["b3"], W.t_end, steps,
                       reverse, g(mbn_in), g(mbn_out), e=g(e), logp=g(logp), w1x=W.w1x, w2x=W.w2x, narrow=narrow,
                       w1h=W.w1h if h3 else None, w2h=W.w2h if h3 else None)


def _cases():
    out = []
    for i, n in enumerate((128, 129, 255, 256, 257, 1000)):
        for rep in (0, 1):
            j = 2 * i + rep
            out.append(dict(n=n, BT=5 if j % 4 in (1, 2) else 1, steps=2 if n == 1000 else (1, 2, 8)[j % 3], reverse=j % 2 == 0,
                            mbn=MBNS[(j // 2) % 4], ldh=LDHS[j % 3], w="seeded" if j % 4 == 3 else "stress"))
    out.append(dict(n=129, BT=2, steps=40, reverse=True, mbn="both", ldh=3091, w="stress"))
    return out


CASES = _cases()
_id = lambda c: "n%d-bt%d-s%d-%s-mbn_%s-ldh%d-%s" % (c["n"], c["BT"], c["steps"], "rev" if c["reverse"] else "fwd", c["mbn"], c["ldh"], c["w"])


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_route_matrix(dev, weights, case):
    from caspr_amd import ops
    W = weights[case["w"]]
    BT, n, steps, reverse = case["BT"], case["n"], case["steps"], case["reverse"]
    c, y = rnd(3000 + n, BT, 1600), base_samples(3001 + n, BT, n)
    hyper = W.hyper(c, case["ldh"])
    mi, mo = mbn_pair(reverse, case["mbn"])
    wx, _ = reference(W, y, hyper, steps, reverse, mi, mo)
    x1 = launch_h3(W, y, hyper, steps, reverse, mi, mo)
    x2 = launch_h3(W, y, hyper, steps, reverse, mi, mo)
    x6 = launch("x6w", W, y, hyper, steps, reverse, mi, mo)
    ops.check_deferred_errors()
    ck = Checks("f16x3_route:" + _id(case))
    ck.close("h3:x", x1, wx, X_TOL, KERN)
    ck.close("h3_vs_x6w:x", x1, x6, IMG_TOL, KERN)
    ck.exact("h3:repeat_x", x2, x1, KERN)
    ck.done()


def test_routing_keeps_the_other_entries(dev, weights):
    """n <= 127, narrow=True or e given: the old entries run, same bits as a call without w1h / w2h."""
    W = weights["stress"]
    ck = Checks("f16x3_routing")
    for tag, n, kw in (("n127", 127, {}), ("narrow", 200, dict(narrow=True)), ("div", 200, dict(div=True))):
        BT = 2
        c, y = rnd(3100 + n, BT, 1600), base_samples(3101 + n, BT, n)
        e, lp0 = (rnd(3102, BT, n, 3), rnd(3103, BT, n, 1)) if kw.get("div") else (None, None)
        hyper = W.hyper(c, 3080)
        mi, mo = mbn_pair(True, "both")
        a = launch_h3(W, y, hyper, 2, True, mi, mo, e, lp0, narrow=bool(kw.get("narrow")), h3=True)
        b = launch_h3(W, y, hyper, 2, True, mi, mo, e, lp0, narrow=bool(kw.get("narrow")), h3=False)
        if e is None:
            ck.exact(tag + ":x", a, b)
        else:
            ck.exact(tag + ":x", a[0], b[0])
            ck.exact(tag + ":logp", a[1], b[1])
    # and n = 128 does take the new kernel: not the bits of the bf16x6 image
    c, y = rnd(3110, 1, 1600), base_samples(3111, 1, 128)
    hyper = W.hyper(c, 3078)
    assert not torch.equal(launch_h3(W, y, hyper, 2, True), launch_h3(W, y, hyper, 2, True, h3=False))
    ck.done()


def test_frame_invariance(dev, weights):
    """Frame k of BT = 5 is bitwise the frame launched alone and the frame inside a permuted batch."""
    W = weights["stress"]
    BT, n, steps = 5, 200, 2
    c, y = rnd(3200, BT, 1600), base_samples(3201, BT, n)
    hyper = W.hyper(c, 3091)
    mi, mo = mbn_pair(True, "both")
    full = launch_h3(W, y, hyper, steps, True, mi, mo)
    perm = torch.tensor([3, 0, 4, 2, 1])
    pm = launch_h3(W, y[perm], hyper[perm], steps, True, mi, mo)
    ck = Checks("f16x3_frames")
    for k in range(BT):
        ck.exact("alone_%d" % k, launch_h3(W, y[k:k + 1], hyper[k:k + 1], steps, True, mi, mo), full[k:k + 1], KERN)
        ck.exact("permuted_%d" % k, pm[int((perm == k).nonzero())][None], full[k:k + 1], KERN)
    ck.done()


def _variant(W, **repl):
    """A copy of the weight set with hidden layers replaced (CPU f32 tensors), all packs rebuilt."""
    from caspr_amd import ops
    V = copy.copy(W)
    V.cpu, V.dev = dict(W.cpu), dict(W.dev)
    for k, v in repl.items():
        V.cpu[k] = v.contiguous()
        V.dev[k] = v.to("cuda:0").contiguous()
    V.w1p, V.w2p = ops.PackedWeight(V.dev["w1"]), ops.PackedWeight(V.dev["w2"])
    V.w1x, V.w2x = ops.pack_cnf_x6(V.dev["w1"]), ops.pack_cnf_x6(V.dev["w2"])
    V.w1h, V.w2h = ops.pack_cnf_h3(V.dev["w1"]), ops.pack_cnf_h3(V.dev["w2"])
    return V


def test_weight_range(dev, weights):
    """The per-layer weight scale found on the device: one layer scaled by 2^9, and one with a quarter of its entries x 2^-20.  The
    scaled layer's gate logits are lowered by 6.25 (gate ~ 2^-9), so that its activations stay where the unscaled layer's are (largest:
    92 in f64) and inside the kernel's range: the products themselves are 512 times larger, which is what the case is about."""
    from caspr_amd import ops
    W = weights["seeded"]
    mask = (torch.arange(512 * 512).reshape(512, 512) % 4 == 1)
    variants = {"w1_x512": _variant(W, w1=W.cpu["w1"] * 512.0),
                "w2_quarter_tiny": _variant(W, w2=torch.where(mask, W.cpu["w2"] * 2.0 ** -20, W.cpu["w2"]))}
    ck = Checks("f16x3_weight_range")
    for tag, V in variants.items():
        BT, n, steps = 2, 130, 2
        c, y = rnd(3300, BT, 1600), base_samples(3301, BT, n)
        hyper = V.hyper(c, 3078)
        if tag == "w1_x512":
            hyper[:, 512:1024] -= 6.25          # layer 1's gate columns (test_cnf_solve_kernels._cols(1, False))
        wx, _ = reference(V, y, hyper, steps, True)
        got = launch_h3(V, y, hyper, steps, True)
        ops.check_deferred_errors()
        ck.close(tag + ":x", got, wx, X_TOL, KERN)
    ck.done()


def test_range_guard(dev, weights):
    """A layer-1 bias that takes one unit's activation past 4094 on ONE frame: that frame's points are NaN, the other frames keep their
    bits, check_deferred_errors raises with the remedy, and a following clean call is quiet."""
    from caspr_amd import lib as _lib
    from caspr_amd import ops
    W = weights["seeded"]
    BT, n, steps = 3, 130, 2
    c, y = rnd(3400, BT, 1600), base_samples(3401, BT, n)
    hyper = W.hyper(c, 3078)
    clean = launch_h3(W, y, hyper, steps, True)
    ops.check_deferred_errors()
    # the hyper BIAS column of layer 1, unit 7, frame 1: added to the pre-activation whatever the gate is
    hot = hyper.clone()
    hot[1, (3 * 512 + 3) + 512 + 7] = 5000.0
    got = launch_h3(W, y, hot, steps, True)
    with pytest.raises(_lib.CasprHipError, match='cnf_split="bf16x6"'):
        ops.check_deferred_errors()
    assert bool(torch.isnan(got[1]).all())
    ck = Checks("f16x3_range_guard")
    ck.exact("frame0", got[0], clean[0], KERN)
    ck.exact("frame2", got[2], clean[2], KERN)
    again = launch_h3(W, y, hyper, steps, True)
    ops.check_deferred_errors()
    ck.exact("clean_again", again, clean, KERN)
    ck.done()


def test_mfma_f16_subnormals_recorded():
    """Records (asserts nothing: the kernel flushes explicitly) whether v_mfma_f32_32x32x16_f16 honours f16 subnormal operands."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "micro", "f16_subnormal_check")
    if not os.path.exists(exe):
        # build() leaves the compiler's message beside the missing binary: record it and say so in the run's warnings summary
        log = exe + ".build_err"
        err = open(log).read().strip()[-400:] if os.path.exists(log) else "no build log: build() did not reach this step"
        REPORT["f16x3:mfma_f16_subnormals"] = {"honoured": None, "note": "tools/micro/f16_subnormal_check not built", "build_error": err}
        warnings.warn("tools/micro/f16_subnormal_check was not built, nothing recorded: " + err)
        return
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    REPORT["f16x3:mfma_f16_subnormals"] = {"honoured": "honoured=1" in r.stdout, "output": r.stdout.strip()[:200]}
    print(r.stdout.strip())


@pytest.mark.parametrize("check_points", (64, 128))
def test_guard_check_solve_stays_on_bf16x6(dev, seeded_sd, monkeypatch, check_points):
    """The accuracy guard's check solve never gets the f16 packs, also at check_points = 128, where it is too wide for the narrow kernel
    and would otherwise be routed to the f16x3 one; the main solve gets them.  And a misspelt ops.CNF_SPLIT raises instead of selecting
    bf16x6 silently."""
    from caspr_amd import ops
    from caspr_amd.models import CaSPR
    from caspr_amd.utils.synthetic import car_sequences
    x, sp = car_sequences(1, 2, 1024, seed=5)
    ts = sp[0, :, 0, 3].to(dev)
    torch.manual_seed(9)
    yb = torch.randn(1, 2, 256, 3).to(dev)
    m = CaSPR(cnf_rk4_steps=2, latent_rk4_steps=2, check_tol=1e-5, check_action="warn", check_points=check_points)
    m.load_state_dict(seeded_sd)
    m = m.to(dev).eval()
    calls, real = [], ops.cnf_rk4

    def spy(x_, *a, **kw):
        calls.append((x_.shape[1], kw.get("w1h") is not None, bool(kw.get("narrow"))))
        return real(x_, *a, **kw)
    monkeypatch.setattr(ops, "cnf_rk4", spy)
    monkeypatch.setattr(ops, "CNF_SPLIT", "f16x3")
    prev = ops.set_matmul_mode(cnf=True)
    try:
        ops.reset_guard()
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m.reconstruct(x.to(dev), num_points=256, timestamps=ts, y=yb)
            ops.check_deferred_errors()
        torch.cuda.synchronize()
        assert calls == [(256, True, False), (check_points, False, check_points <= 64)], calls
        monkeypatch.setattr(ops, "CNF_SPLIT", "fp16x3")
        with torch.no_grad(), pytest.raises(ValueError, match="CNF_SPLIT"):
            m.reconstruct(x.to(dev), num_points=256, timestamps=ts, y=yb)
        torch.cuda.synchronize()
    finally:
        ops.set_matmul_mode(cnf=prev[1])
        ops.reset_guard()


def test_model_level_option(dev, seeded_sd, stress_sd):
    """reconstruct() on 2 x 4 x 1024 with 256 samples: |x_f16x3 - x_bf16x6| <= 5e-6 FLAT, T-NOCS bitwise, guard quiet on the seeded
    weights and warning on the stress weights at 8 steps."""
    from caspr_amd import ops
    from caspr_amd.models import CaSPR
    from caspr_amd.utils.synthetic import car_sequences
    x, sp = car_sequences(2, 4, 1024, seed=5)
    ts = sp[0, :, 0, 3].to(dev)
    torch.manual_seed(9)
    yb = torch.randn(2, 4, 256, 3).to(dev)
    prev_split, prev = ops.CNF_SPLIT, ops.set_matmul_mode(cnf=True)
    ck = Checks("f16x3_model")
    try:
        for which, sd, lat, quiet in (("seeded", seeded_sd, 2, True), ("stress", stress_sd, 16, False)):
            m = CaSPR(cnf_rk4_steps=8, latent_rk4_steps=lat, check_tol=1e-5, check_action="warn")
            m.load_state_dict(sd)
            m = m.to(dev).eval()
            res = {}
            for split in ("bf16x6", "f16x3"):
                ops.CNF_SPLIT = split
                ops.reset_guard()
                with torch.no_grad(), warnings.catch_warnings(record=True) as wrec:
                    warnings.simplefilter("always")
                    _, _, gx, gt = m.reconstruct(x.to(dev), num_points=256, timestamps=ts, y=yb)
                    ops.check_deferred_errors()
                torch.cuda.synchronize()
                warned = any("point CNF" in str(w_.message) for w_ in wrec)
                res[split] = (gx.clone(), gt.clone(), warned)
                assert warned == (not quiet), (which, split, [str(w_.message)[:80] for w_ in wrec])
            # a FLAT bound here, not Checks.close's tol x max(1, |x|max): |x| reaches 7 (seeded) and 15 (stress)
            dx = float((res["f16x3"][0].double() - res["bf16x6"][0].double()).abs().max())
            REPORT["cnf_solve:f16x3_model:%s:x_flat" % which] = {"max_abs_err": dx, "bound": MODEL_TOL, "kernel": KERN,
                                                                 "ref_absmax": float(res["bf16x6"][0].abs().max())}
            print("f16x3_model %s: max |x_f16x3 - x_bf16x6| = %.3e (bound %.1e flat)" % (which, dx, MODEL_TOL))
            if not (bool(torch.isfinite(res["f16x3"][0]).all()) and dx <= MODEL_TOL):
                ck.bad.append("%s:x: max abs diff %.3e > %.1e (flat)" % (which, dx, MODEL_TOL))
            ck.exact(which + ":tnocs", res["f16x3"][1], res["bf16x6"][1])
            assert not torch.equal(res["f16x3"][0], res["bf16x6"][0]), "the option did not change the kernel"
    finally:
        ops.CNF_SPLIT = prev_split
        ops.set_matmul_mode(cnf=prev[1])
    ck.done()
