"""A/B of the point CNF's ADAPTIVE sampling solve (ops.cnf_dopri5, rtol = atol = 1e-5, reverse direction) at the headline shape (160 frames
x 2048 points): the bf16x6 64-point kernel (cnf_dp5_kernel<false>) against the f16x3 128-point kernel (cnf_dp5_h3w_kernel), in ONE
process, alternating rounds after a warm-up, on both synthetic weight sets.  Per route: ms per solve (host loop included: one launch
and one device word read per attempt), launches' attempts, mean and max evaluations per frame; max |x_f16x3 - x_bf16x6| is recorded
only (two free-running adaptive solves choose their own steps).  Writes profiles/cnf_dopri5_f16x3_bench.json and prints it."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cnf_dopri5_f16x3_bench.json"))
    args = ap.parse_args()
    if args.rounds < 3:
        ap.error("--rounds must be at least 3")
    from caspr_amd import ops
    from caspr_amd.models import CaSPR
    from caspr_amd.models.cnf import CNF
    from caspr_amd.utils.synthetic import seeded_state_dict, stress_state_dict
    dev = torch.device("cuda:0")
    out = {"shape": {"frames": args.frames, "points": args.points, "rtol": args.tol, "atol": args.tol, "reverse": True}, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "weights": {}}
    for which, make in (("seeded", seeded_state_dict), ("stress", stress_state_dict)):
        m = CaSPR()
        m.load_state_dict(make(m.state_dict(), 0))
        m = m.to(dev).eval()
        blk = next(b for b in m.modules() if isinstance(b, CNF))
        w = blk._weights()
        w1x, w2x = blk._weights_x6()
        w1h, w2h = blk._weights_h3()
        g = torch.Generator().manual_seed(1)
        ctx = torch.randn(args.frames, w["hyp"].cin, generator=g).to(dev)
        y = (torch.randn(args.frames, args.points, 3, generator=g) * 1.3).clamp(-5, 5).to(dev)
        hyper = ops.conv1x1(w["hyp"], w["hyp_bias"], ctx.view(1, args.frames, -1), row_invariant=True)[0]

        def run(h3):
            return ops.cnf_dopri5(y, hyper, w["tcol"], w["w0"], w["b0"], w["b1"], w["b2"], w["w3"], w["b3"], w1x, w2x, blk.end_time(), args.tol, args.tol,
                                  True, return_trace=True, w1h=w1h if h3 else None, w2h=w2h if h3 else None)
        (xa, ia), (xb, ib) = run(False), run(True)          # warm-up, the trace figures and the difference between the two routes
        torch.cuda.synchronize()
        ops.check_deferred_errors()
        routes = {}
        for name, info in (("bf16x6", ia), ("f16x3", ib)):
            nfe = info["nfe"].cpu().double()
            routes[name] = {"kernel": info.get("kernel", "cnf_dp5_kernel<false>"), "attempts": int((info["accepted"] + info["rejected"]).max()), "nfe_mean": round(float(nfe.mean()), 2),
                            "nfe_max": int(nfe.max()), "solve_ms": []}
        for _ in range(args.rounds):
            for name, h3 in (("bf16x6", False), ("f16x3", True)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()          # (the entry synchronises the stream itself: wall time is the solve)
                run(h3)
                torch.cuda.synchronize()
                routes[name]["solve_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
        ops.check_deferred_errors()
        for r in routes.values():
            r["mean_ms"] = round(sum(r["solve_ms"]) / len(r["solve_ms"]), 3)
        a, b = routes["bf16x6"], routes["f16x3"]
        out["weights"][which] = {"routes": routes, "ratio_f16x3_over_bf16x6": round(b["mean_ms"] / a["mean_ms"], 4),
                                 "every_f16x3_run_faster_than_every_bf16x6_run": max(b["solve_ms"]) < min(a["solve_ms"]),
                                 "max_abs_diff_x": float((xa - xb).abs().max()), "x_absmax": float(xa.abs().max())}
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
