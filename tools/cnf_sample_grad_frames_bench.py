"""Time and peak memory of decode(differentiable=True) forward + backward with ONE RK4 step count against a count PER FRAME, at the cfg-3
shard (80 frames x 1024 points), in ONE process and in alternating rounds (the boxes of the pool differ by a few per cent and drift
with their neighbours' load: only figures of the same run compare):

    uniform_max    (a) the uniform route at S = max_f S_f: what a caller must run without the table for the same accuracy on every frame
    table          (b) decode(differentiable=True, frame_steps=<the pilot's counts, chosen once before the rounds>)
    table_pilot    (c) decode(differentiable=True, frame_steps="pilot"): the pilot ladder inside every iteration
    uniform_default    for orientation: the uniform route at the constructor's default cnf_rk4_steps = 8, whatever accuracy that gives

    PYTHONPATH=. timeout -k 10 600 python tools/cnf_sample_grad_frames_bench.py [--weights stress|seeded|PATH] [--rounds 5] [--iters 3]
                                                                                [--out profiles/cnf_sample_grad_frames_bench.json]

--weights: the stress weights (default), the seeded weights, or a checkpoint written by tools/train_and_eval.py (a state dict).
--latents randn (default for the synthetic weights): the contexts are randn scaled per frame by --scales, cycling along the batch, so
that the frames differ in how hard they are to integrate (tests/test_cnf_frame_steps.py does the same).  --latents encoder (default for a
checkpoint): the model's own latents of frames / 10 synthetic rigid-car sequences of 10 frames (encode -> latent solve), what a trained
flow is conditioned on.  Next to the times: the histogram of the counts and sum_f S_f / (BT max_f S_f), the share
of the uniform route's evaluations the table route performs -- the ceiling of its gain; the late steps run on a short prefix of the
frames and fill the chip less well, so the measured ratio sits above it.  Per leg: ms per iteration of every round (device events around
`iters` iterations), median and spread over the rounds, torch.cuda.max_memory_allocated over a round.  Every leg is warmed up once."""
import argparse
import collections
import json

import numpy as np
import torch

from caspr_amd import ops
from caspr_amd.models import CaSPR
from caspr_amd.models.cnf import CNF
from caspr_amd.utils.synthetic import seeded_state_dict, stress_state_dict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", default="stress")
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--num-pts", type=int, default=1024)
    ap.add_argument("--scales", default="0.25,0.5,1.0,1.0,1.5,2.0")
    ap.add_argument("--latents", choices=("randn", "encoder"), default=None)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--steps-max", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    BT, n = a.frames, a.num_pts
    model = CaSPR(check_tol=None, cnf_steps_tol=a.tol, cnf_steps_max=a.steps_max)
    if a.weights == "stress":
        sd = stress_state_dict(CaSPR().state_dict(), 0)
    elif a.weights == "seeded":
        sd = seeded_state_dict(CaSPR().state_dict(), 0)
    else:
        sd = torch.load(a.weights, map_location="cpu")
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(4321)
    latents = a.latents or ("randn" if a.weights in ("stress", "seeded") else "encoder")
    if latents == "randn":
        scales = torch.tensor([float(v) for v in a.scales.split(",")], device=dev)
        z = torch.randn(1, BT, 1600, device=dev, generator=gen) * scales[torch.arange(BT, device=dev) % scales.numel()].view(1, BT, 1)
        where = "contexts randn x %s cycling" % a.scales
    else:
        from caspr_amd.utils.synthetic import car_sequences
        assert BT % 10 == 0, "--latents encoder takes sequences of 10 frames"
        xs, sp = car_sequences(BT // 10, 10, 1024, seed=777100)
        with torch.no_grad():
            z0, _ = model.encode(xs.to(dev))
            z = model.aggregate_and_solve_latent(z0, sp[0, :, 0, 3].to(dev).view(1, -1).repeat(BT // 10, 1)).reshape(1, BT, 1600).contiguous()
        where = "contexts = the model's latents of %d synthetic car sequences x 10 frames" % (BT // 10)
    y = torch.randn(1, BT, n, 3, device=dev, generator=gen)
    blocks = [b for b in model.point_cnf.chain if isinstance(b, CNF)]

    def fwd_bwd(**kw):
        model.zero_grad(set_to_none=True)
        x = model.decode(z.detach().requires_grad_(True), n, y=y, differentiable=True, **kw)[2]
        (x * x).sum().backward()
        return x
    fwd_bwd(frame_steps="pilot")                       # the counts of legs (a) and (b), chosen once
    table = model.last_frame_steps[0].clone()
    counts = [int(s) for s in table.cpu()]
    ops.check_deferred_errors()                        # a capped frame is an error here: raise --steps-max
    s_max = max(counts)

    def uniform(S):
        for b in blocks:
            b.rk4_steps = S
        return fwd_bwd()
    legs = {"uniform_max": lambda: uniform(s_max), "table": lambda: fwd_bwd(frame_steps=table), "table_pilot": lambda: fwd_bwd(frame_steps="pilot"),
            "uniform_default": lambda: uniform(8)}

    def run(fn, iters):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            out = fn()
        t1.record()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        return t0.elapsed_time(t1) / iters, torch.cuda.max_memory_allocated()
    for fn in legs.values():
        run(fn, 1)                                     # warm-up: code objects, weight packs, workspaces, the allocator's pools
    per = {k: {"ms": [], "peak": []} for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            ms, peak = run(fn, a.iters)
            per[k]["ms"].append(ms)
            per[k]["peak"].append(peak)
    hist = collections.Counter(counts)
    res = {"workload": "cfg-3 shard: BT=%d frames, n=%d points, %s weights, %s; decode(differentiable=True) forward + backward of "
                       "sum(x^2); pilot tol %g, cnf_steps_max %d" % (BT, n, a.weights, where, a.tol, a.steps_max),
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters_per_round": a.iters,
           "counts_histogram": {str(k): hist[k] for k in sorted(hist)}, "max_count": s_max, "sum_counts": sum(counts),
           "evaluations_share_of_uniform": round(sum(counts) / float(BT * s_max), 4),
           "tape_bytes": s_max * 4 * BT * n * 24, "legs": {}}
    for k in legs:
        ms = per[k]["ms"]
        res["legs"][k] = {"ms_median": round(float(np.median(ms)), 3), "ms_rounds": [round(v, 3) for v in ms], "spread_ms": round(max(ms) - min(ms), 3),
                          "max_memory_allocated_GB": round(max(per[k]["peak"]) / 1e9, 3)}
    base = res["legs"]["uniform_max"]["ms_median"]
    res["table_over_uniform_max"] = round(res["legs"]["table"]["ms_median"] / base, 4)
    res["table_pilot_over_uniform_max"] = round(res["legs"]["table_pilot"]["ms_median"] / base, 4)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
