"""Time and peak memory of the point CNF's sampling solve with and without its gradient at the cfg-3 shard (80 frames x 1024 points, 8 RK4
steps, seeded weights), in ONE process and in alternating rounds (the boxes of the pool differ by a few per cent and drift with their
neighbours' load: only figures of the same run compare):

    decode         (a) CaSPR.decode() as it is: the inference launch, forward only, under torch.no_grad()
    decode_grad    (b) CaSPR.decode(differentiable=True) forward + backward of a sum-of-squares loss (train/flow_grad.py: CnfSampleSolve)
    block_node     (c) the NLL-direction block node on the same tensors: CnfBlockSolve forward + backward (value AND tangent rows: twice
                   the rows of (b)), sum-of-squares loss on (x_T, logp_T)
    decode_grad_h3 (d) as (b) with ops.CNF_TAPE_SPLIT = "f16x3": the taped forward on the 128-point f16x3 kernel (csrc/ode_sample_tape_h3w.hip),
                   the same reverse sweep
    tape_fwd       (e) the taped forward launch of (b) alone, on the block's own tensors: train_ops.cnf_sample_tape (64-point bf16x6)
    tape_fwd_h3    (f) the taped forward launch of (d) alone: train_ops.cnf_sample_tape_h3 (128-point f16x3)

    PYTHONPATH=. timeout -k 10 600 python tools/cnf_sample_grad_bench.py [--rounds 5] [--iters 8] [--out profiles/cnf_sample_grad_bench.json]

Per leg: ms per iteration of every round (device events around `iters` iterations, 8 x `iters` for the short legs (a), (e), (f)), their median and spread (max - min over the rounds)
and torch.cuda.max_memory_allocated over a round (reset before it).  Every leg is warmed up once before the first timed round.  After the
rounds, one more iteration of (b) and (c) each runs with the per-kernel timers on (ops.TIMING = 2): the breakdown by kernel that explains
the ratio of the two.  The tape of (b) is not a measurement: steps x 4 x BT x n x 24 bytes."""
import argparse
import json

import numpy as np
import torch

from caspr_amd import ops
from caspr_amd import train_ops as T
from caspr_amd.models import CaSPR
from caspr_amd.train import flow_grad
from caspr_amd.utils.synthetic import seeded_state_dict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--num-pts", type=int, default=1024)
    ap.add_argument("--cnf-steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8, help="iterations per round of (b) and (c); (a), ten times shorter, runs 8 x as many")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    BT, n, S = a.frames, a.num_pts, a.cnf_steps
    model = CaSPR(cnf_rk4_steps=S, check_tol=None)
    model.load_state_dict(seeded_state_dict(CaSPR().state_dict(), 0))
    model = model.to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(4321)
    z = torch.randn(1, BT, 1600, device=dev, generator=gen)
    y = torch.randn(1, BT, n, 3, device=dev, generator=gen)
    e = torch.randn(BT, n, 3, device=dev, generator=gen)
    lp0 = torch.zeros(BT, n, 1, device=dev)
    block = model.point_cnf.chain[1]

    def leg_decode():
        with torch.no_grad():
            return model.decode(z, n, y=y)[2]

    def leg_decode_grad():
        model.zero_grad(set_to_none=True)
        x = model.decode(z.detach().requires_grad_(True), n, y=y, differentiable=True)[2]
        (x * x).sum().backward()
        return x

    def leg_block_node():
        model.zero_grad(set_to_none=True)
        prev, flow_grad.BLOCK_NODE = flow_grad.BLOCK_NODE, True
        try:
            xT, lp = flow_grad.cnf_block_train(block, y[0], z[0].detach().requires_grad_(True), lp0, e)
            assert block._block_node_used
        finally:
            flow_grad.BLOCK_NODE = prev
        ((xT * xT).sum() + (lp * lp).sum()).backward()
        return xT

    def leg_decode_grad_h3():
        prev, ops.CNF_TAPE_SPLIT = ops.CNF_TAPE_SPLIT, "f16x3"
        try:
            return leg_decode_grad()
        finally:
            ops.CNF_TAPE_SPLIT = prev

    # the taped forward launches alone, on what the block node hands them (train/flow_grad.py: CnfSampleSolve.forward)
    with torch.no_grad():
        (G_lm, Bb_lm, tg_lm, tb_lm, widths), t_end, w1x, w2x, wb = flow_grad._block_node_inputs(block, z[0], dev)
        hyper, tcol = flow_grad._hyper_for_kernel(G_lm, Bb_lm, tg_lm, tb_lm, BT, widths)
        w0, b0, _, b1, _, b2, w3, b3 = [t_.detach().contiguous() for t_ in wb]
        w1h, w2h = block._weights_h3()
        t_dev = t_end.detach().reshape(1).contiguous()
        yb = y[0].contiguous()

    def leg_tape_fwd():
        return T.cnf_sample_tape(yb, hyper, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, t_dev, S)[0]

    def leg_tape_fwd_h3():
        return T.cnf_sample_tape_h3(yb, hyper, tcol, w0, b0, w1h, b1, w2h, b2, w3, b3, t_dev, S)[0]
    legs = {"decode": leg_decode, "decode_grad": leg_decode_grad, "block_node": leg_block_node, "decode_grad_h3": leg_decode_grad_h3,
            "tape_fwd": leg_tape_fwd, "tape_fwd_h3": leg_tape_fwd_h3}
    short = ("decode", "tape_fwd", "tape_fwd_h3")

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

    def breakdown(fn):
        """One iteration with the per-kernel timers on -> {timer: [launches, total ms]}, largest first."""
        prev, ops.TIMING = ops.TIMING, 2
        ops.TIMERS.clear()
        try:
            fn()
            torch.cuda.synchronize()
            tab = {k: [len(v), round(sum(s.elapsed_time(t) for s, t in v), 3)] for k, v in ops.TIMERS.items()}
        finally:
            ops.TIMING = prev
            ops.TIMERS.clear()
        return dict(sorted(tab.items(), key=lambda kv: -kv[1][1]))

    for fn in legs.values():
        run(fn, 1)                                     # warm-up: code objects, weight packs, workspaces, the allocator's pools
    per = {k: {"ms": [], "peak": []} for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            ms, peak = run(fn, a.iters * (8 if k in short else 1))      # every timed window several hundred milliseconds long
            per[k]["ms"].append(ms)
            per[k]["peak"].append(peak)
    res = {"workload": "cfg-3 shard: BT=%d frames, n=%d points, %d RK4 steps, seeded weights; (a) decode() forward, (b) decode(differentiable=True) "
                       "forward + backward, (c) CnfBlockSolve forward + backward on the same tensors, (d) as (b) with CNF_TAPE_SPLIT = f16x3, "
                       "(e) / (f) the taped forward launch of (b) / (d) alone" % (BT, n, S),
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters_per_round": a.iters,
           "tape_bytes_decode_grad": S * 4 * BT * n * 24, "legs": {}}
    for k in legs:
        ms = per[k]["ms"]
        res["legs"][k] = {"ms_median": round(float(np.median(ms)), 3), "ms_rounds": [round(v, 3) for v in ms], "spread_ms": round(max(ms) - min(ms), 3),
                          "max_memory_allocated_bytes": int(max(per[k]["peak"])), "max_memory_allocated_GB": round(max(per[k]["peak"]) / 1e9, 3)}
    res["decode_grad_over_block_node"] = round(res["legs"]["decode_grad"]["ms_median"] / res["legs"]["block_node"]["ms_median"], 4)
    med = lambda k: res["legs"][k]["ms_median"]
    res["tape_fwd_h3_over_tape_fwd"] = round(med("tape_fwd_h3") / med("tape_fwd"), 4)
    res["decode_grad_h3_over_decode_grad"] = round(med("decode_grad_h3") / med("decode_grad"), 4)
    res["x_max_abs_diff_h3_vs_bf16x6"] = float((leg_tape_fwd_h3() - leg_tape_fwd()).abs().max())
    ops.check_deferred_errors()
    res["per_kernel_ms"] = {"decode_grad": breakdown(leg_decode_grad), "block_node": breakdown(leg_block_node), "decode_grad_h3": breakdown(leg_decode_grad_h3)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
