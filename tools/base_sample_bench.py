"""Time decode's base-sample draw both ways at the headline shape (160 frames x 2048 points) and the cfg-5 shape (1280 x 4096):

  host    what CaSPR._draw_early does: torch.randn on the CPU generator into a pinned buffer, the copy to the device, and
          standard_normal_logprob(y).sum(2) behind it;
  device  one ops.base_samples launch (csrc/base_sample.hip), which writes y and logp_y.

One process, the two sides alternating round by round after `--warmup` rounds each; every measurement is a host clock around
work that ends in a device synchronise (the host draw is host time, so device events alone would miss it), plus the device-event
time of the launch on the device side.  Standalone: the draw hidden under the encoder in reconstruct() is not modelled here.

    PYTHONPATH=. timeout -k 10 300 python tools/base_sample_bench.py [--rounds 20] [--out profiles/base_sample_bench.json]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from caspr_amd import ops
from caspr_amd.models.utils import standard_normal_logprob

SHAPES = {"headline": (160, 2048), "cfg5": (1280, 4096)}


def host_draw(buf, dev):
    F, n, _ = buf.shape
    torch.randn(*buf.shape, out=buf)
    y = buf.to(dev, non_blocking=True)
    return y, standard_normal_logprob(y).view(F, n, -1).sum(2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "base_sample_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "base_sample_bench needs a ROCm GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "torch_threads": torch.get_num_threads(), "shapes": {}}
    for name, (F, n) in SHAPES.items():
        buf = torch.empty(F, n, 3, dtype=torch.float32, pin_memory=True)
        ids = torch.arange(F, device=dev, dtype=torch.int64)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        host_ms, dev_ms, dev_event_ms = [], [], []
        for r in range(a.warmup + a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_draw(buf, dev)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            e0.record()
            ops.base_samples(F, n, 0, r, ids)
            e1.record()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if r >= a.warmup:
                host_ms.append((t1 - t0) * 1e3)
                dev_ms.append((t2 - t1) * 1e3)
                dev_event_ms.append(e0.elapsed_time(e1))
        stat = lambda v: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(min(v)), 4), "max_ms": round(float(max(v)), 4)}
        res["shapes"][name] = {"frames": F, "points": n, "values": F * n * 3, "host_draw_copy_logprob": stat(host_ms),
                               "device_launch_wall": stat(dev_ms), "device_launch_events": stat(dev_event_ms)}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
