"""Time ops.cnf_dopri5 (csrc/ode_dp5.hip) at the cfg-2 size (160 frames x 2048 points, sampling direction) on seeded and stress
weights, and in the same process the fixed-step kernels it is compared with PER EVALUATION: ops.cnf_rk4(..., narrow=True) (the same
64-point geometry, one launch for all evaluations) and the default RK4 launch (the 128-point kernel).

    PYTHONPATH=. timeout -k 10 600 python tools/cnf_dp5_bench.py [--frames 160] [--points 2048] [--tol 1e-5] [--iters 3]

A dopri5 call is 2 + (attempts + 1) launches (initial-step selection, one launch per attempt, one that only decides); the slowest
frame decides how many.  ms per evaluation = call time / (2 + 6 x attempts of the slowest frame): what a frame that needs all of
them pays, relaunches, weight re-staging and the 20-float carry-over per point included."""
import argparse
import json

import numpy as np
import torch

from caspr_amd import ops
from caspr_amd.models import CaSPR
from caspr_amd.utils.synthetic import seeded_state_dict, stress_state_dict


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--rk4-steps", type=int, default=8)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    BT, n, S = a.frames, a.points, a.rk4_steps
    base = CaSPR().state_dict()
    res = {"BT": BT, "n": n, "tol": a.tol, "device": torch.cuda.get_device_name(0)}
    for name, sd in (("seeded", seeded_state_dict(base, 0)), ("stress", stress_state_dict(base, 0))):
        m = CaSPR()
        m.load_state_dict(sd)
        m = m.to(dev).eval()
        blk = m.point_cnf.chain[1]
        g = torch.Generator().manual_seed(1)
        y = torch.randn(BT, n, 3, generator=g).to(dev)
        z = (0.5 * torch.randn(BT, m.cnf_args.zdim, generator=g)).to(dev)
        with torch.no_grad():
            w = blk._weights()
            hyper = ops.conv1x1(w["hyp"], w["hyp_bias"], z.view(1, BT, -1), row_invariant=True)[0]
            w1x, w2x = blk._weights_x6()
            mi, mo = m.point_cnf.chain[2].kernel_params(), m.point_cnf.chain[0].kernel_params()
            T = blk.end_time()
            rk4 = lambda narrow: ops.cnf_rk4(y, hyper, w["tcol"], w["w0"], w["b0"], w["w1p"], w["b1"], w["w2p"], w["b2"], w["w3"], w["b3"], T, S, True,
                                             mi, mo, w1x=w1x, w2x=w2x, narrow=narrow)
            dp5 = lambda: ops.cnf_dopri5(y, hyper, w["tcol"], w["w0"], w["b0"], w["b1"], w["b2"], w["w3"], w["b3"], w1x, w2x, T, a.tol, a.tol, True,
                                         mi, mo, return_trace=True)
            ms_n, _ = timed(lambda: rk4(True), a.iters)
            ms_w, _ = timed(lambda: rk4(False), a.iters)
            ms_d, (x, info) = timed(dp5, a.iters)
        att = (info["accepted"] + info["rejected"]).cpu().numpy()
        nfe = info["nfe"].cpu().numpy()
        launches = int(att.max()) + 3
        res[name] = {"dopri5_ms": round(ms_d, 3), "launches": launches, "ms_per_launch": round(ms_d / launches, 3),
                     "ms_per_evaluation": round(ms_d / float(nfe.max()), 3),
                     "rk4_narrow_ms": round(ms_n, 3), "rk4_narrow_ms_per_evaluation": round(ms_n / (4 * S), 3),
                     "rk4_default_ms": round(ms_w, 3), "rk4_default_ms_per_evaluation": round(ms_w / (4 * S), 3),
                     "attempts_max": int(att.max()), "attempts_mean": round(float(att.mean()), 2),
                     "rejected_share": round(float(info["rejected"].sum()) / float(att.sum()), 3),
                     "nfe_max": int(nfe.max()), "nfe_mean": round(float(nfe.mean()), 1), "finite": bool(torch.isfinite(x).all())}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
