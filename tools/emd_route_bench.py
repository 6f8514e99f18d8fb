"""The two forward routes of the approximate EMD side by side (caspr_amd/csrc/emd.hip): "frame", one workgroup per frame (caspr_emd_f32 /
caspr_emd_tape_f32), and "rows", every frame's rows over the grid in 22 launches (caspr_emd_rows_f32) -- in ONE process on one device, the
routes alternating repetition by repetition so that both see the same clocks and the same neighbours.

Per shape F x n x m: the forward alone (ops.earth_mover_distance, no tape, as utils.evaluations calls it) and forward + backward through
losses.emd_loss (tape + caspr_emd_bwd_f32, the same backward kernel on both routes).  Every repetition is timed by its own pair of device
events after `--warmup` untimed calls per route; reported are the median and the spread (min .. max) of `--reps` repetitions, the ratio of
the medians, and whether the slower route's fastest repetition is still slower than the faster route's slowest ("beyond the spread").
Before timing, the tapes of the two routes are compared bit for bit and the costs relatively: the timing is of the same quantity.

    python tools/emd_route_bench.py [--frames 1 10 16 160] [--n 2048] [--m 2048] [--reps 20] [--warmup 3] [--out profiles/emd_route_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
ROUTES = ("frame", "rows")


def _forward(ops, p, q, route):
    return ops.earth_mover_distance(p, q, transpose=False, route=route)


def _forward_backward(ops, p, q, route):
    from caspr_amd.losses import emd_loss
    before = ops.EMD_ROUTE
    ops.EMD_ROUTE = route
    try:
        p.grad = None
        emd_loss(p, q).backward()
    finally:
        ops.EMD_ROUTE = before


def _time(fn, ops, p, q, reps, warmup):
    """-> {route: [ms per repetition]}; the routes alternate inside every repetition."""
    for route in ROUTES:
        for _ in range(warmup):
            fn(ops, p, q, route)
    torch.cuda.synchronize()
    ms = {r: [] for r in ROUTES}
    for _ in range(reps):
        for route in ROUTES:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn(ops, p, q, route)
            t1.record()
            t1.synchronize()
            ms[route].append(t0.elapsed_time(t1))
    return ms


def _summary(ms):
    out = {r: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for r, v in ms.items()}
    f, r = out["frame"], out["rows"]
    out["frame_over_rows"] = f["median_ms"] / r["median_ms"]
    out["beyond_spread"] = bool(f["min_ms"] > r["max_ms"] or r["min_ms"] > f["max_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 10, 16, 160])
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--m", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if a.reps < 20:
        raise SystemExit("emd_route_bench: --reps must be at least 20 (a median and a spread of fewer say little)")
    if not torch.cuda.is_available():
        raise SystemExit("emd_route_bench needs a GPU: a time measured elsewhere says nothing about it")
    from caspr_amd import ops
    dev = torch.device("cuda:0")
    lines = ["emd_route_bench: %s, n = %d, m = %d, %d repetitions after %d warm-up calls per route, routes alternating; ms per call as median (min .. max)"
             % (torch.cuda.get_device_name(0), a.n, a.m, a.reps, a.warmup),
             "%5s  %-9s  %-30s  %-30s  %12s  %s" % ("F", "what", "frame", "rows", "frame / rows", "beyond the spread")]
    results = []
    for F in a.frames:
        gen = torch.Generator().manual_seed(F)
        p = torch.rand(F, a.n, 3, generator=gen).to(dev)
        q = torch.rand(F, a.m, 3, generator=gen).to(dev)
        cost_f, tape_f = ops.earth_mover_distance(p, q, transpose=False, return_tape=True, route="frame")
        cost_r, tape_r = ops.earth_mover_distance(p, q, transpose=False, return_tape=True, route="rows")
        same = {"tape_bit_identical": bool(torch.equal(tape_f, tape_r)), "cost_max_rel_diff": float((cost_r.double() / cost_f.double() - 1).abs().max())}
        del tape_f, tape_r
        res = {"shape": [F, a.n, a.m], "outputs": same, "forward": _summary(_time(_forward, ops, p, q, a.reps, a.warmup))}
        pg = p.clone().requires_grad_(True)
        res["forward_backward"] = _summary(_time(_forward_backward, ops, pg, q, a.reps, a.warmup))
        results.append(res)
        for what in ("forward", "forward_backward"):
            s = res[what]
            cell = lambda d: "%9.3f (%9.3f .. %9.3f)" % (d["median_ms"], d["min_ms"], d["max_ms"])
            lines.append("%5d  %-9s  %-30s  %-30s  %12.2f  %s" % (F, "fwd" if what == "forward" else "fwd+bwd", cell(s["frame"]), cell(s["rows"]),
                                                                   s["frame_over_rows"], "yes" if s["beyond_spread"] else "no"))
        lines.append("%5d  outputs: tape bit-identical %s, cost max rel diff %.3e" % (F, same["tape_bit_identical"], same["cost_max_rel_diff"]))
    lines.append(json.dumps({"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "results": results}))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
