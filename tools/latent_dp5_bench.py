"""Time ops.latent_dopri5 (csrc/ode_latent_dp5.hip) at the reference tolerance for the cars.cfg shape (16 sequences, 160 sorted stamps
of which 10 are distinct) on seeded and stress weights, and in the same process the fixed-step solve it is compared with:
ops.latent_rk4 at the default 2 steps per interval on its two routes (single-workgroup kernel, 32-workgroup team kernel).

    PYTHONPATH=. timeout -k 10 600 python tools/latent_dp5_bench.py [--batch 16] [--frames 10] [--tol 1e-3] [--iters 200] [--rounds 5]

The three solves alternate inside every round (same box, same clocks); a figure is the median over the rounds of the mean time of
`iters` back-to-back calls between two device events.  The adaptive solve is one launch; its cost is set by the sequence of the
workgroup that needs the most attempts (2 + 6 x attempts evaluations), RK4's by 4 x steps x distinct intervals."""
import argparse
import json

import numpy as np
import torch

from caspr_amd import ops
from caspr_amd.models import CaSPR
from caspr_amd.utils.synthetic import seeded_state_dict, stress_state_dict


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--rk4-steps", type=int, default=2)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T, S = a.batch, a.frames, a.rk4_steps
    base = CaSPR().state_dict()
    res = {"B": B, "stamps": B * T, "distinct": T, "tol": a.tol, "rk4_steps": S, "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    times = torch.sort(torch.linspace(0.0, 1.0, T).repeat(B))[0].contiguous().to(dev)
    for name, sd in (("seeded", seeded_state_dict(base, 0)), ("stress", stress_state_dict(base, 0))):
        m = CaSPR()
        m.load_state_dict(sd)
        m = m.to(dev).eval()
        g = torch.Generator().manual_seed(1)
        z0 = torch.randn(B, 1600, generator=g).to(dev)[:, :64]                       # the encoder's layout: a column slice
        wts = m.latent_ode._weights()
        with torch.no_grad():
            runs = {"dopri5": lambda: ops.latent_dopri5(z0, times, a.tol, a.tol, wts),
                    "rk4_single": lambda: ops.latent_rk4(z0, times, S, wts, team=False),
                    "rk4_team": lambda: ops.latent_rk4(z0, times, S, wts, team=True)}
            for fn in runs.values():                                                  # warm every shape of the timed window
                timed(fn, 3)
            ms = {k: [] for k in runs}
            for _ in range(a.rounds):
                for k, fn in runs.items():
                    ms[k].append(timed(fn, a.iters))
            out, info = ops.latent_dopri5(z0, times, a.tol, a.tol, wts, return_trace=True)
            ref = ops.latent_rk4(z0, times, 64, wts, team=False)
            rk = ops.latent_rk4(z0, times, S, wts, team=False)
            ops.check_deferred_errors()
        nfe = info["nfe"].cpu().numpy()
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res[name] = {"dopri5_ms": round(med["dopri5"], 4), "rk4_single_ms": round(med["rk4_single"], 4), "rk4_team_ms": round(med["rk4_team"], 4),
                     "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
                     "dopri5_nfe_max": int(nfe.max()), "dopri5_nfe_mean": round(float(nfe.mean()), 1), "rk4_nfe": 4 * S * (T - 1),
                     "rejected": int(info["rejected"].sum()),
                     "dopri5_us_per_evaluation": round(1e3 * med["dopri5"] / float(nfe.max()), 2),
                     "rk4_single_us_per_evaluation": round(1e3 * med["rk4_single"] / (4 * S * (T - 1)), 2),
                     "rk4_team_us_per_evaluation": round(1e3 * med["rk4_team"] / (4 * S * (T - 1)), 2),
                     "dopri5_vs_rk4_64_steps": float((out - ref).abs().max()), "rk4_vs_rk4_64_steps": float((rk - ref).abs().max()),
                     "finite": bool(torch.isfinite(out).all())}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
