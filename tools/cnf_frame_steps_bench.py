"""Time decode() with per-frame RK4 step counts (CaSPR(cnf_steps="frame"): csrc/cnf_frame_steps.hip) against the uniform route at the
cars.cfg shape (16 sequences x 10 frames x 2048 points), in ONE process, alternating rounds, device events, after a warm-up:

    seeded weights   uniform at the default 8 steps                                    | frame mode
    stress weights   uniform at the count calibrate_rk4_steps(tol=1e-5) installs       | frame mode

    PYTHONPATH=. timeout -k 10 900 python tools/cnf_frame_steps_bench.py [--rounds 5] [--safeties 1.2,1.5] [--out profiles/cnf_frame_steps_bench.json]

Per leg: decode ms (median over the rounds; the guard's check solve runs on its side stream behind it and is not inside), for frame
mode the pilot and the main solve separately (ops.timed "cnf_pilot" / "cnf_main"), the histogram of S_f, the guard's verdict and
max |x_frame - x_uniform| -- over all points, and frame by frame against tol (1 + max |x_f|): how many frames are farther from the
uniform solution than the bound, and with which counts.  One frame leg per safety factor.  No speed threshold: the baseline is the uniform route of the same process."""
import argparse
import json
import os

import numpy as np
import torch

from caspr_amd import ops
from caspr_amd.models import CaSPR
from caspr_amd.utils.synthetic import car_sequences, seeded_state_dict, stress_state_dict


def model(sd, dev, **kw):
    m = CaSPR(check_tol=1e-5, check_action="warn", **kw)
    m.load_state_dict(sd)
    return m.to(dev).eval()


def pair_ms(name):
    return [a.elapsed_time(b) for a, b in ops.TIMERS.get(name, [])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=16)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--safeties", default="1.2,1.5", help="cnf_steps_safety of the frame legs, comma separated (the first is the default's)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "cnf_frame_steps_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T, N = a.seqs, a.frames, a.points
    base = CaSPR().state_dict()
    x, _ = car_sequences(B, T, N, seed=1234)
    x = x.to(dev)
    ts = x[0, :, 0, 3].contiguous()
    safeties = [float(s) for s in a.safeties.split(",")]
    res = {"shape": [B, T, N], "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "cnf_split": ops.cnf_split(), "tol": 1e-5, "safeties": safeties,
           "cnf_steps_max": 64}
    import warnings
    with torch.no_grad():
        for name, sd in (("seeded", seeded_state_dict(base, 0)), ("stress", stress_state_dict(base, 0))):
            mu = model(sd, dev)
            mfs = {s: model(sd, dev, cnf_steps="frame", cnf_steps_safety=s) for s in safeties}
            uniform = 8
            if name == "stress":
                mu.latent_ode.rk4_steps = 16
                uniform = int(mu.calibrate_rk4_steps(x, tol=1e-5)[0])
            z0, _ = mu.encode(x)
            z = mu.aggregate_and_solve_latent(z0, ts.view(1, -1).repeat(B, 1))
            y = torch.randn(B, T, N, 3, generator=torch.Generator().manual_seed(1)).to(dev)
            legs = {"uniform": (mu, [])}
            legs.update({"frame_%g" % s: (m, []) for s, m in mfs.items()})
            verdict, outs, parts = {}, {}, {}
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                for r in range(a.warmup + a.rounds):
                    if r == a.warmup:
                        ops.TIMERS.clear()
                        ops.TIMING, ops.TIMING_ONLY = True, {"cnf_pilot", "cnf_main"}
                    for leg, (m, ms) in legs.items():
                        ops.reset_guard()
                        ops.TIMERS.clear()
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        outs[leg] = m.decode(z, N, y=y)[2]
                        e1.record()
                        torch.cuda.synchronize()
                        ops.check_deferred_errors()
                        verdict[leg] = dict(ops.GUARD_LAST.get("cnf", {}))
                        if r >= a.warmup:
                            ms.append(e0.elapsed_time(e1))
                            if leg != "uniform":
                                parts.setdefault(leg, []).append((pair_ms("cnf_pilot")[0], pair_ms("cnf_main")[0]))
                ops.TIMING, ops.TIMING_ONLY = False, None
            torch.cuda.synchronize()
            g = lambda v: {"ok": v.get("ok"), "estimate": v.get("estimate"), "bound": v.get("bound"),
                           "ratio": (v["estimate"] / v["bound"]) if v.get("bound") else None}
            xu = outs["uniform"].reshape(B * T, N, 3)
            u_ms = float(np.median(legs["uniform"][1]))
            res[name] = {"uniform_steps": uniform, "uniform_decode_ms": round(u_ms, 3), "nfe_uniform": int(mu.get_nfe()[1]), "guard_uniform": g(verdict["uniform"]),
                         "warnings": sorted(set(str(w.message)[:160] for w in caught))}
            for s, mf in mfs.items():
                leg = "frame_%g" % s
                steps, info = mf.last_frame_steps[0], mf.last_frame_steps[2]
                S = steps.cpu().numpy()
                xf = outs[leg].reshape(B * T, N, 3)
                # frame by frame: the distance from the uniform solution over the guard's bound for that frame
                rel = ((xf - xu).abs().flatten(1).amax(1) / (1e-5 * (1.0 + xu.abs().flatten(1).amax(1)))).cpu().numpy()
                over = rel > 1.0
                f_ms = float(np.median(legs[leg][1]))
                res[name][leg] = {
                    "decode_ms": round(f_ms, 3), "over_uniform": round(f_ms / u_ms, 3),
                    "pilot_ms": round(float(np.median([p[0] for p in parts[leg]])), 3), "main_ms": round(float(np.median([p[1] for p in parts[leg]])), 3),
                    "steps_hist": {str(int(k)): int(v) for k, v in zip(*np.unique(S, return_counts=True))},
                    "steps_mean": round(float(S.mean()), 2), "steps_max": int(S.max()),
                    "pilot_steps_max": int(info["pilot_steps"].max()), "capped": int(info["capped"].sum()), "nfe": int(mf.get_nfe()[1]),
                    "guard": g(verdict[leg]),
                    "max_abs_x_frame_minus_x_uniform": float((xf - xu).abs().max()),
                    "frames_farther_than_bound_from_uniform": int(over.sum()), "worst_distance_over_bound": round(float(rel.max()), 3),
                    "steps_hist_of_those_frames": {str(int(k)): int(v) for k, v in zip(*np.unique(S[over], return_counts=True))},
                }
            ops.TIMERS.clear()
    print(json.dumps(res))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
