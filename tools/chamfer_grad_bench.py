"""Forward + backward of the Chamfer loss: caspr_amd.losses.chamfer_loss (caspr_chamfer_idx_f32 + caspr_chamfer_bwd_f32) against the route a
user had before it -- torch.cdist -> ** 2 -> min -> autograd -- on the same tensors.  Reports the time per forward + backward (device
events around `iters` iterations after `warmup`) and the peak allocated memory above the inputs, for both, as one JSON line.  Nothing is
asserted on the numbers; the two losses and gradients are compared so that the timing is known to be of the same quantity.

    python tools/chamfer_grad_bench.py [--frames 160] [--n 2048] [--m 2048] [--iters 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def _ours(p, q):
    from caspr_amd.losses import chamfer_loss
    return chamfer_loss(p, q)


def _cdist(p, q):
    d = torch.cdist(p, q) ** 2
    return (d.min(dim=2).values.mean(dim=1) + d.min(dim=1).values.mean(dim=1)).mean()


def _measure(fn, p, q, iters, warmup):
    """-> (ms per forward + backward, peak bytes allocated above what was allocated before the call, loss, dL/dp)."""
    for _ in range(warmup):
        p.grad = None
        fn(p, q).backward()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        p.grad = None
        loss = fn(p, q)
        loss.backward()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters, torch.cuda.max_memory_allocated() - base, float(loss.detach()), p.grad.detach().clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--m", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chamfer_grad_bench needs a GPU: a time measured elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    p = torch.randn(a.frames, a.n, 3, generator=gen).to(dev).requires_grad_(True)
    q = torch.randn(a.frames, a.m, 3, generator=gen).to(dev)
    ms_o, mem_o, loss_o, g_o = _measure(_ours, p, q, a.iters, a.warmup)
    ms_c, mem_c, loss_c, g_c = _measure(_cdist, p, q, a.iters, a.warmup)
    out = {"shape": [a.frames, a.n, a.m], "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "hip": {"ms_fwd_bwd": ms_o, "peak_bytes": mem_o, "loss": loss_o},
           "cdist_autograd": {"ms_fwd_bwd": ms_c, "peak_bytes": mem_c, "loss": loss_c},
           "loss_rel_diff": abs(loss_o - loss_c) / abs(loss_c), "dp_rel_l2_diff": float((g_o - g_c).norm() / g_c.norm())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
