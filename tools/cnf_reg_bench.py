"""What the point CNF's kinetic / Jacobian regularisers cost per TRAINING step at the cfg-3 shard (8 sequences x 10 frames x 1024 points, 8 RK4
steps in the CNF), in ONE process and in alternating rounds (the boxes of the pool differ by a few per cent and drift with their
neighbours' load: only figures of the same run compare):

    off   CaSPR(cnf_reg=False), weights 0: the step as it was (CnfOut, the (x, logp) state)
    on    CaSPR(cnf_reg=True), kinetic_weight = jacobian_weight = 0.01: CnfOutReg, the two extra state components, their cotangents

    PYTHONPATH=. timeout -k 10 900 python tools/cnf_reg_bench.py [--rounds 5] [--steps 5] [--checkpoint] [--out profiles/cnf_reg_bench.json]

Per leg: ms per step of every round (a host clock around `steps` full train_step calls ending in a device synchronise), their median and
spread (max - min over the rounds), and torch.cuda.max_memory_allocated over a round (reset before it).  Each leg has its own model, built
with its option from the same seeded weights, and its own optimizer; data and noise are shared; each is warmed up once before the first
timed round.
--checkpoint: both legs on config.train_cnf_checkpoint's per-step tape (the low-memory route that carries the regularisers)."""
import argparse
import json
import time

import numpy as np
import torch

from caspr_amd.models import CaSPR
from caspr_amd.train import flow_grad
from caspr_amd.train.loop import train_step
from caspr_amd.utils.synthetic import car_sequences, seeded_state_dict

LEGS = {"off": (False, 0.0), "on": (True, 0.01)}      # (CaSPR(cnf_reg=), kinetic_weight = jacobian_weight)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq-len", type=int, default=10)
    ap.add_argument("--num-pts", type=int, default=1024)
    ap.add_argument("--cnf-steps", type=int, default=8)
    ap.add_argument("--latent-steps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--checkpoint", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T, N = a.batch, a.seq_len, a.num_pts
    sd = seeded_state_dict(CaSPR().state_dict(), 0)
    models = {}
    for leg, (reg, _) in LEGS.items():
        m = CaSPR(cnf_rk4_steps=a.cnf_steps, latent_rk4_steps=a.latent_steps, cnf_reg=reg)
        m.load_state_dict(sd)
        m = m.to(dev).train()
        models[leg] = (m, torch.optim.Adam(m.parameters(), lr=1e-4, betas=(0.9, 0.999), eps=1e-8))
    x, sp = (t.to(dev) for t in car_sequences(B, T, N, seed=1234))
    e = torch.randn(B * T, N, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(4321))
    prev = (flow_grad.BLOCK_NODE, flow_grad.CHECKPOINT_STEPS)

    def run(leg, steps):
        (model, opt), w = models[leg], LEGS[leg][1]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = train_step(model, opt, x, sp, e=e, kinetic_weight=w, jacobian_weight=w)[0]
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps, torch.cuda.max_memory_allocated(), loss

    res = {"workload": "cfg-3 shard: B=%d sequences, T=%d, N=%d, cnf_rk4_steps=%d, latent_rk4_steps=%d; full train_step (forward, backward, Adam); %s tape"
                       % (B, T, N, a.cnf_steps, a.latent_steps, "per-step checkpointed" if a.checkpoint else "full"),
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps_per_round": a.steps, "legs": {}}
    try:
        flow_grad.BLOCK_NODE, flow_grad.CHECKPOINT_STEPS = False, bool(a.checkpoint)
        for leg in LEGS:
            run(leg, 1)                                # warm-up: code objects, weight packs, workspaces, the allocator's pools
        per = {leg: {"ms": [], "peak": [], "loss": []} for leg in LEGS}
        for _ in range(a.rounds):
            for leg in LEGS:
                ms, peak, loss = run(leg, a.steps)
                per[leg]["ms"].append(ms)
                per[leg]["peak"].append(peak)
                per[leg]["loss"].append(loss)
    finally:
        flow_grad.BLOCK_NODE, flow_grad.CHECKPOINT_STEPS = prev
    for leg in LEGS:
        ms = per[leg]["ms"]
        res["legs"][leg] = {"ms_per_step_median": round(float(np.median(ms)), 3), "ms_per_step_rounds": [round(v, 3) for v in ms],
                            "spread_ms": round(max(ms) - min(ms), 3), "max_memory_allocated_bytes": int(max(per[leg]["peak"])),
                            "max_memory_allocated_GB": round(max(per[leg]["peak"]) / 1e9, 3), "last_loss": per[leg]["loss"][-1],
                            "finite": bool(np.isfinite(per[leg]["loss"]).all())}
    off, on = res["legs"]["off"], res["legs"]["on"]
    res["on_over_off"] = {"time": round(on["ms_per_step_median"] / off["ms_per_step_median"], 4),
                          "memory": round(on["max_memory_allocated_bytes"] / off["max_memory_allocated_bytes"], 4)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
