"""The exact EMD (caspr_amd/csrc/emd_exact.hip: one workgroup per frame, a forward auction in LDS) timed beside the two routes of the
approximate EMD (csrc/emd.hip: "frame" and "rows") on the same tensors in ONE process on one device, and the distance of the approximation
from it: (approx - exact) / exact per frame.

Inputs at F x n x n, F in --frames: uniform clouds; two tight clusters against a uniform cloud; and a decoded-vs-target pair from the
seeded model (the target is the decode of a latent, the prediction the decode of that latent perturbed, on the same base samples: what
fit_latent and the evaluation see).  Per input: forward (ops.earth_mover_distance_exact) and forward + backward
(losses.emd_exact_loss(...).backward()), every repetition timed by its own pair of device events after --warmup untimed calls, the three
contenders alternating repetition by repetition; median (min .. max) of --reps.  Rounds and bids per frame come from the kernel's info.
No time is promised anywhere: the feature is the exactness, and the numbers say what it costs.

    python tools/emd_exact_bench.py [--frames 1 16 160] [--n 2048] [--reps 20] [--warmup 3] [--out profiles/emd_exact_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
CONTENDERS = ("exact", "frame", "rows")


def _uniform(F, n, dev):
    gen = torch.Generator().manual_seed(F)
    return torch.rand(F, n, 3, generator=gen).to(dev), torch.rand(F, n, 3, generator=gen).to(dev)


def _clustered(F, n, dev):
    rng = np.random.default_rng(F)
    centres = np.array([[0.25, 0.25, 0.25], [0.75, 0.7, 0.8]])
    p = centres[rng.integers(0, 2, (F, n))] + rng.normal(0, 0.01, (F, n, 3))
    return torch.from_numpy(p.astype(np.float32)).to(dev), torch.from_numpy(rng.uniform(0, 1, (F, n, 3)).astype(np.float32)).to(dev)


def _decoded(F, n, dev):
    from caspr_amd.models import CaSPR
    from caspr_amd.utils.synthetic import seeded_state_dict
    m = CaSPR(check_tol=None)
    m.load_state_dict(seeded_state_dict(CaSPR().state_dict(), 0))
    m = m.to(dev).eval()
    gen = torch.Generator().manual_seed(1000 + F)
    z = torch.randn(1, F, 1600, generator=gen).to(dev)
    y = torch.randn(1, F, n, 3, generator=gen).to(dev)
    with torch.no_grad():
        target = m.decode(z, n, y=y)[2].reshape(F, n, 3).contiguous()
        pred = m.decode(z + 0.05 * torch.randn(1, F, 1600, generator=gen).to(dev), n, y=y)[2].reshape(F, n, 3).contiguous()
    return pred, target


def _forward(ops, losses, p, q, who):
    if who == "exact":
        return ops.earth_mover_distance_exact(p, q, transpose=False)
    return ops.earth_mover_distance(p, q, transpose=False, route=who)


def _forward_backward(ops, losses, p, q, who):
    p.grad = None
    if who == "exact":
        losses.emd_exact_loss(p, q).backward()
        return
    before = ops.EMD_ROUTE
    ops.EMD_ROUTE = who
    try:
        losses.emd_loss(p, q).backward()
    finally:
        ops.EMD_ROUTE = before


def _time(fn, ops, losses, p, q, reps, warmup):
    for who in CONTENDERS:
        for _ in range(warmup):
            fn(ops, losses, p, q, who)
    torch.cuda.synchronize()
    ms = {w: [] for w in CONTENDERS}
    for _ in range(reps):
        for who in CONTENDERS:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn(ops, losses, p, q, who)
            t1.record()
            t1.synchronize()
            ms[who].append(t0.elapsed_time(t1))
    return {w: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for w, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 16, 160])
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inputs", nargs="+", default=["uniform", "clustered", "decoded"], choices=["uniform", "clustered", "decoded"])
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("emd_exact_bench needs a GPU: a time measured elsewhere says nothing about it")
    from caspr_amd import losses, ops
    dev = torch.device("cuda:0")
    make = {"uniform": _uniform, "clustered": _clustered, "decoded": _decoded}
    cell = lambda d: "%9.3f (%9.3f .. %9.3f)" % (d["median_ms"], d["min_ms"], d["max_ms"])
    lines = ["emd_exact_bench: %s, n = %d, eps = %g, %d repetitions after %d warm-up calls each, contenders alternating; ms per call as median (min .. max)"
             % (torch.cuda.get_device_name(0), a.n, a.eps, a.reps, a.warmup),
             "%-9s %5s  %-7s  %-32s  %-32s  %-32s" % ("input", "F", "what", "exact", "approx frame", "approx rows")]
    results = []
    for name in a.inputs:
        for F in a.frames:
            p, q = make[name](F, a.n, dev)
            cost, assign, prices, info = ops.earth_mover_distance_exact(p, q, transpose=False, eps=a.eps, return_match=True)
            info = info.cpu()
            res = {"input": name, "shape": [F, a.n, a.n], "converged": int(info[:, 0].sum()),
                   "rounds": {"min": int(info[:, 2].min()), "median": float(info[:, 2].double().median()), "max": int(info[:, 2].max())},
                   "bids": {"min": int(info[:, 3].min()), "median": float(info[:, 3].double().median()), "max": int(info[:, 3].max())},
                   "phases": int(info[:, 1].max()), "exact_over_n_mean": float((cost / a.n).mean())}
            for route in ("frame", "rows"):
                gap = (ops.earth_mover_distance(p, q, transpose=False, route=route).double() - cost.double()) / cost.double()
                res["rel_gap_" + route] = {"min": float(gap.min()), "mean": float(gap.mean()), "max": float(gap.max())}
            res["forward"] = _time(_forward, ops, losses, p, q, a.reps, a.warmup)
            pg = p.clone().requires_grad_(True)
            res["forward_backward"] = _time(_forward_backward, ops, losses, pg, q, a.reps, a.warmup)
            results.append(res)
            for what in ("forward", "forward_backward"):
                s = res[what]
                lines.append("%-9s %5d  %-7s  %-32s  %-32s  %-32s" % (name, F, "fwd" if what == "forward" else "fwd+bwd", cell(s["exact"]), cell(s["frame"]),
                                                                       cell(s["rows"])))
            lines.append("%-9s %5d  converged %d / %d, phases %d, rounds per frame %d .. %d (median %.0f), bids per frame %d .. %d (median %.0f), mean exact EMD / n %.6f"
                         % (name, F, res["converged"], F, res["phases"], res["rounds"]["min"], res["rounds"]["max"], res["rounds"]["median"],
                            res["bids"]["min"], res["bids"]["max"], res["bids"]["median"], res["exact_over_n_mean"]))
            lines.append("%-9s %5d  (approx - exact) / exact: frame route %+.4f .. %+.4f (mean %+.4f), rows route %+.4f .. %+.4f (mean %+.4f)"
                         % (name, F, res["rel_gap_frame"]["min"], res["rel_gap_frame"]["max"], res["rel_gap_frame"]["mean"],
                            res["rel_gap_rows"]["min"], res["rel_gap_rows"]["max"], res["rel_gap_rows"]["mean"]))
            sys.stdout.write("\n".join(lines[-4:]) + "\n")
            sys.stdout.flush()
    lines.append(json.dumps({"device": torch.cuda.get_device_name(0), "n": a.n, "eps": a.eps, "reps": a.reps, "warmup": a.warmup, "results": results}))
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
