"""Time forward + backward of the adaptive latent solve's autograd node (train/flow_grad.py: LatentSolveDopri5; csrc/ode_latent_dp5.hip with
the tape, csrc/ode_latent_dp5_adjoint.inc, one weight-gradient product per layer) and, in the same process on the same tensors, of the
node training uses by default: LatentSolve (RK4, 2 steps per interval, team tape + team adjoint).

    PYTHONPATH=. timeout -k 10 900 python tools/latent_dp5_train_bench.py [--frames 10] [--iters 50] [--rounds 5] [--out profiles/latent_dp5_train_bench.txt]

B = 8 and B = 64 sequences, `frames` distinct stamps over [0, 1], seeded and stress weights, rtol = atol = 1e-3 and 1e-5.  The nodes
alternate inside every round (same box, same clocks); a figure is the median over the rounds of the mean time of `iters` back-to-back
forward + backward passes between two device events, [min, max] over the rounds beside it.  Accepted steps and evaluations are the
forward's counters (the backward makes 1 + 6 x accepted evaluations and as many vector-Jacobian products for the slowest sequence of
a workgroup).  No pass mark: the file is where the numbers go."""
import argparse
import json

import numpy as np
import torch

from caspr_amd import ops
from caspr_amd.models import CaSPR
from caspr_amd.train import flow_grad as FG
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
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--rk4-steps", type=int, default=2)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    T, S = a.frames, a.rk4_steps
    base = CaSPR().state_dict()
    res = {"distinct": T, "rk4_steps": S, "iters": a.iters, "rounds": a.rounds, "max_steps": 64, "device": torch.cuda.get_device_name(0)}
    times = torch.linspace(0.0, 1.0, T).contiguous().to(dev)
    rows = []
    for name, sd in (("seeded", seeded_state_dict(base, 0)), ("stress", stress_state_dict(base, 0))):
        m = CaSPR()
        m.load_state_dict(sd)
        lat = m.to(dev).latent_ode
        wb = [x for i in (0, 2, 4, 6) for x in (lat.ode_func.dynamics_net[i].weight, lat.ode_func.dynamics_net[i].bias)]
        for B in (8, 64):
            g = torch.Generator().manual_seed(1)
            z0 = torch.randn(B, 64, generator=g).to(dev).requires_grad_(True)
            wgt = torch.randn(B, T, 64, generator=g).to(dev)

            def step(apply):
                out = apply()
                torch.autograd.grad((out * wgt).sum(), [z0] + wb)
            runs = {"rk4": lambda: step(lambda: FG.LatentSolve.apply(z0, times, S, *wb))}
            for tol in (1e-3, 1e-5):
                runs["dopri5_%g" % tol] = lambda tol=tol: step(lambda: FG.LatentSolveDopri5.apply(z0, times, tol, tol, 1000, 64, *wb))
            for fn in runs.values():                                                  # warm every shape of the timed window
                timed(fn, 3)
            ms = {k: [] for k in runs}
            for _ in range(a.rounds):
                for k, fn in runs.items():
                    ms[k].append(timed(fn, a.iters))
            ops.check_deferred_errors()
            ent = {"rk4_ms": round(float(np.median(ms["rk4"])), 4), "rk4_spread_ms": [round(min(ms["rk4"]), 4), round(max(ms["rk4"]), 4)],
                   "rk4_evaluations": 4 * S * (T - 1)}
            rows.append("  %-7s B = %-3d RK4 node (%d evaluations)            %8.3f ms  [%.3f, %.3f]"
                        % (name, B, ent["rk4_evaluations"], ent["rk4_ms"], *ent["rk4_spread_ms"]))
            for tol in (1e-3, 1e-5):
                k = "dopri5_%g" % tol
                runs[k]()
                info = FG.LatentSolveDopri5.last_info
                acc, nfe = info["accepted"].cpu().numpy(), info["nfe"].cpu().numpy()
                ent[k] = {"ms": round(float(np.median(ms[k])), 4), "spread_ms": [round(min(ms[k]), 4), round(max(ms[k]), 4)],
                          "accepted_min": int(acc.min()), "accepted_max": int(acc.max()), "rejected": int(info["rejected"].sum()),
                          "forward_nfe_max": int(nfe.max()), "backward_evaluations_max": int(1 + 6 * acc.max())}
                rows.append("  %-7s B = %-3d dopri5 node at %-5g (%d-%d steps, %d forward evaluations)  %8.3f ms  [%.3f, %.3f]"
                            % (name, B, tol, acc.min(), acc.max(), nfe.max(), ent[k]["ms"], *ent[k]["spread_ms"]))
            res["%s_B%d" % (name, B)] = ent
    head = ("tools/latent_dp5_train_bench.py on one %s, one process: forward + backward of LatentSolveDopri5 (the adaptive solve with its step tape,\n"
            "one reverse-sweep launch, four weight-gradient products) against LatentSolve (RK4, %d steps per interval, team tape + team adjoint) on the\n"
            "same tensors, %d distinct stamps over [0, 1].  Median over %d alternating rounds of the mean of %d back-to-back passes between device\n"
            "events, [min, max] over the rounds.\n\n" % (res["device"], S, T, a.rounds, a.iters))
    text = head + "\n".join(rows) + "\n\n" + json.dumps(res) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
