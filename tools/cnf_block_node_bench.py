"""Time and peak memory of one TRAINING step at the cfg-3 shard (8 sequences x 10 frames x 1024 points, 8 RK4 steps in the CNF) on the three
routes of train/flow_grad.py: cnf_block_train, in ONE process and in alternating rounds (the boxes of the pool differ by a few per cent
and drift with their neighbours' load: only figures of the same run compare):

    taped          the default: every evaluation's layer products stay on the autograd tape until the backward pass
    checkpointed   config.train_cnf_checkpoint: the state per RK4 step, a step's four evaluations recomputed in the backward pass
    node           config.train_cnf_block_node: CnfBlockSolve -- forward in one launch that writes no layer product
                   (csrc/ode_train_fwd.hip), the reverse sweep tapes one evaluation at a time

    PYTHONPATH=. timeout -k 10 900 python tools/cnf_block_node_bench.py [--rounds 3] [--steps 3] [--out profiles/cnf_block_node_bench.json]

Per route: ms per step of every round (a host clock around `steps` full train_step calls ending in a device synchronise), their median
and spread (max - min over the rounds), and torch.cuda.max_memory_allocated over a round (reset before it).  The same model, data, noise
and optimizer serve all three; every route is warmed up once before the first timed round."""
import argparse
import json
import time

import numpy as np
import torch

from caspr_amd.models import CaSPR
from caspr_amd.train import flow_grad
from caspr_amd.train.loop import train_step
from caspr_amd.utils.synthetic import car_sequences, seeded_state_dict

ROUTES = {"taped": (False, False), "checkpointed": (False, True), "node": (True, False)}      # (BLOCK_NODE, CHECKPOINT_STEPS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq-len", type=int, default=10)
    ap.add_argument("--num-pts", type=int, default=1024)
    ap.add_argument("--cnf-steps", type=int, default=8)
    ap.add_argument("--latent-steps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--routes", default="taped,checkpointed,node")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T, N = a.batch, a.seq_len, a.num_pts
    model = CaSPR(cnf_rk4_steps=a.cnf_steps, latent_rk4_steps=a.latent_steps)
    model.load_state_dict(seeded_state_dict(CaSPR().state_dict(), 0))
    model = model.to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
    x, sp = (t.to(dev) for t in car_sequences(B, T, N, seed=1234))
    e = torch.randn(B * T, N, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(4321))
    routes = [r for r in a.routes.split(",") if r]
    prev = (flow_grad.BLOCK_NODE, flow_grad.CHECKPOINT_STEPS)
    cnf = model.point_cnf.chain[1]

    def run(route, steps):
        flow_grad.BLOCK_NODE, flow_grad.CHECKPOINT_STEPS = ROUTES[route]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = train_step(model, opt, x, sp, e=e)[0]
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / steps
        assert cnf._block_node_used is ROUTES[route][0], "route %s did not run" % route
        return ms, torch.cuda.max_memory_allocated(), loss

    res = {"workload": "cfg-3 shard: B=%d sequences, T=%d, N=%d, cnf_rk4_steps=%d, latent_rk4_steps=%d; full train_step (forward, backward, Adam)"
                       % (B, T, N, a.cnf_steps, a.latent_steps),
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps_per_round": a.steps, "routes": {}}
    try:
        for r in routes:
            run(r, 1)                                  # warm-up: code objects, weight packs, workspaces, the allocator's pools
        per = {r: {"ms": [], "peak": [], "loss": []} for r in routes}
        for _ in range(a.rounds):
            for r in routes:
                ms, peak, loss = run(r, a.steps)
                per[r]["ms"].append(ms)
                per[r]["peak"].append(peak)
                per[r]["loss"].append(loss)
    finally:
        flow_grad.BLOCK_NODE, flow_grad.CHECKPOINT_STEPS = prev
    for r in routes:
        ms = per[r]["ms"]
        res["routes"][r] = {"ms_per_step_median": round(float(np.median(ms)), 3), "ms_per_step_rounds": [round(v, 3) for v in ms],
                            "spread_ms": round(max(ms) - min(ms), 3), "max_memory_allocated_bytes": int(max(per[r]["peak"])),
                            "max_memory_allocated_GB": round(max(per[r]["peak"]) / 1e9, 3), "last_loss": per[r]["loss"][-1],
                            "finite": bool(np.isfinite(per[r]["loss"]).all())}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
