"""Time and peak memory of one REGULARISED training step at the cfg-3 shard (8 sequences x 10 frames x 1024 points, 8 RK4 steps in the
CNF; kinetic_weight = jacobian_weight = 0.01) on the routes of train/flow_grad.py: cnf_block_train that carry the regularisers, beside the
block node without them, in ONE process and in alternating rounds (the boxes of the pool differ by a few per cent and drift with their
neighbours' load: only figures of the same run compare):

    taped_reg          the default tape with CnfOutReg: every evaluation's layer products stay on the tape until the backward pass
    checkpointed_reg   config.train_cnf_checkpoint: the state (y, logp, r) per RK4 step, a step's four evaluations recomputed
    node               config.train_cnf_block_node, CaSPR(cnf_reg=False), weights 0: CnfBlockSolve, the cost of the option's baseline
    node_reg           config.train_cnf_block_node + config.train_cnf_block_node_reg: CnfBlockSolveReg -- the forward in one launch
                       that also integrates and tapes (|a|^2, |J e|^2) (csrc/ode_train_fwd.hip, REG), three tapes in the reverse sweep

    PYTHONPATH=. timeout -k 10 900 python tools/cnf_block_reg_bench.py [--rounds 3] [--steps 3] [--out profiles/cnf_block_reg_bench.json]

Per route: ms per step of every round (a host clock around `steps` full train_step calls ending in a device synchronise), their median
and spread (max - min over the rounds), and torch.cuda.max_memory_allocated over a round (reset before it).  The regularised routes share
one model built with cnf_reg=True, `node` has its own from the same seeded weights; data and noise are shared; every route is warmed up
once before the first timed round.  The ratios at the end: node_reg against each of the two routes that carried the regularisers
before it, and against the node without them."""
import argparse
import json
import time

import numpy as np
import torch

from caspr_amd.models import CaSPR
from caspr_amd.train import flow_grad
from caspr_amd.train.loop import train_step
from caspr_amd.utils.synthetic import car_sequences, seeded_state_dict

# route -> (BLOCK_NODE, BLOCK_NODE_REG, CHECKPOINT_STEPS, CaSPR(cnf_reg=), kinetic_weight = jacobian_weight)
ROUTES = {"taped_reg": (False, False, False, True, 0.01), "checkpointed_reg": (False, False, True, True, 0.01),
          "node": (True, False, False, False, 0.0), "node_reg": (True, True, False, True, 0.01)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq-len", type=int, default=10)
    ap.add_argument("--num-pts", type=int, default=1024)
    ap.add_argument("--cnf-steps", type=int, default=8)
    ap.add_argument("--latent-steps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--routes", default=",".join(ROUTES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T, N = a.batch, a.seq_len, a.num_pts
    sd = seeded_state_dict(CaSPR().state_dict(), 0)
    models = {}
    for reg in (False, True):
        m = CaSPR(cnf_rk4_steps=a.cnf_steps, latent_rk4_steps=a.latent_steps, cnf_reg=reg)
        m.load_state_dict(sd)
        m = m.to(dev).train()
        models[reg] = (m, torch.optim.Adam(m.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8))
    x, sp = (t.to(dev) for t in car_sequences(B, T, N, seed=1234))
    e = torch.randn(B * T, N, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(4321))
    routes = [r for r in a.routes.split(",") if r]
    prev = (flow_grad.BLOCK_NODE, flow_grad.BLOCK_NODE_REG, flow_grad.CHECKPOINT_STEPS)

    def run(route, steps):
        node, node_reg, ckpt, reg, w = ROUTES[route]
        flow_grad.BLOCK_NODE, flow_grad.BLOCK_NODE_REG, flow_grad.CHECKPOINT_STEPS = node, node_reg, ckpt
        model, opt = models[reg]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = train_step(model, opt, x, sp, e=e, kinetic_weight=w, jacobian_weight=w)[0]
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / steps
        assert model.point_cnf.chain[1]._block_node_used is node, "route %s did not run" % route
        return ms, torch.cuda.max_memory_allocated(), loss

    res = {"workload": "cfg-3 shard: B=%d sequences, T=%d, N=%d, cnf_rk4_steps=%d, latent_rk4_steps=%d; full train_step (forward, backward, Adam); "
                       "kinetic_weight = jacobian_weight = 0.01 on the *_reg routes" % (B, T, N, a.cnf_steps, a.latent_steps),
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
        flow_grad.BLOCK_NODE, flow_grad.BLOCK_NODE_REG, flow_grad.CHECKPOINT_STEPS = prev
    for r in routes:
        ms = per[r]["ms"]
        res["routes"][r] = {"ms_per_step_median": round(float(np.median(ms)), 3), "ms_per_step_rounds": [round(v, 3) for v in ms],
                            "spread_ms": round(max(ms) - min(ms), 3), "max_memory_allocated_bytes": int(max(per[r]["peak"])),
                            "max_memory_allocated_GB": round(max(per[r]["peak"]) / 1e9, 3), "last_loss": per[r]["loss"][-1],
                            "finite": bool(np.isfinite(per[r]["loss"]).all())}
    if "node_reg" in res["routes"]:
        nr = res["routes"]["node_reg"]
        res["node_reg_over"] = {r: {"time": round(nr["ms_per_step_median"] / v["ms_per_step_median"], 4),
                                    "memory": round(nr["max_memory_allocated_bytes"] / v["max_memory_allocated_bytes"], 4)}
                                for r, v in res["routes"].items() if r != "node_reg"}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
