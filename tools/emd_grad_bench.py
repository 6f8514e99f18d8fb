"""Forward + backward of the approximate-EMD loss: caspr_amd.losses.emd_loss (caspr_emd_tape_f32 + caspr_emd_bwd_f32) against a torch-on-GPU
restatement that materialises the (n, m) match matrix the way the reference's extension does (emd_cuda.approxmatch_forward -> match,
matchcost_forward / matchcost_backward on it; utils/emd.py:5-21), at a batch that fits: the ten levels on (F, n, m) tensors, the gradient
by autograd through (match.detach() * dist).sum().  Reports the time per forward + backward (device events around `iters` iterations after
`warmup`) and the peak allocated memory above the inputs, for both, as one JSON line.  Nothing is asserted on the numbers; the two losses
and gradients are compared on the baseline's frames so that the timing is known to be of the same quantity.

    python tools/emd_grad_bench.py [--frames 160] [--n 2048] [--m 2048] [--baseline-frames 16] [--iters 10] [--warmup 2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def _ours(p, q):
    from caspr_amd.losses import emd_loss
    return emd_loss(p, q)


def _match_matrix(p, q):
    """emd_loss restated on (F, n, m) tensors: approxmatch level by level without a graph, then cost / n through the stored match."""
    n, m = p.shape[1], q.shape[1]
    with torch.no_grad():
        d2 = ((p[:, :, None, :] - q[:, None, :, :]) ** 2).sum(-1)
        multiL, multiR = (1.0, float(n // m)) if n >= m else (float(m // n), 1.0)
        remainL = torch.full(p.shape[:2], multiL, device=p.device)
        remainR = torch.full(q.shape[:2], multiR, device=p.device)
        match = torch.zeros_like(d2)
        for j in range(7, -3, -1):
            K = torch.exp((0.0 if j == -2 else -(4.0 ** j)) * d2)
            ratioL = remainL / (1e-9 + (K * remainR[:, None, :]).sum(2))
            sumr = (K * ratioL[:, :, None]).sum(1) * remainR
            ratioR = torch.clamp(remainR / (sumr + 1e-9), max=1.0) * remainR
            remainR = torch.clamp(remainR - sumr, min=0.0)
            K *= ratioL[:, :, None]
            K *= ratioR[:, None, :]
            match += K
            remainL = torch.clamp(remainL - K.sum(2), min=0.0)
        del K, d2
    dist = ((p[:, :, None, :] - q[:, None, :, :]) ** 2).sum(-1).clamp_min(1e-20).sqrt()
    return ((match * dist).sum((1, 2)) / n).mean()


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


def _forward_ms(p, q, iters):
    from caspr_amd import ops
    ops.earth_mover_distance(p, q, transpose=False, return_tape=True)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        ops.earth_mover_distance(p, q, transpose=False, return_tape=True)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--m", type=int, default=2048)
    ap.add_argument("--baseline-frames", type=int, default=16, help="frames the match-matrix baseline runs on (it keeps several (F, n, m) tensors)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("emd_grad_bench needs a GPU: a time measured elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    p = torch.rand(a.frames, a.n, 3, generator=gen).to(dev).requires_grad_(True)
    q = torch.rand(a.frames, a.m, 3, generator=gen).to(dev)
    fb = min(a.baseline_frames, a.frames)
    ms_o, mem_o, loss_o, _ = _measure(_ours, p, q, a.iters, a.warmup)
    ms_f = _forward_ms(p.detach(), q, a.iters)
    pb, qb = p.detach()[:fb].clone().requires_grad_(True), q[:fb].clone()
    ms_s, mem_s, loss_s, g_s = _measure(_ours, pb, qb, a.iters, a.warmup)
    ms_t, mem_t, loss_t, g_t = _measure(_match_matrix, pb, qb, a.iters, a.warmup)
    out = {"shape": [a.frames, a.n, a.m], "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "hip": {"ms_fwd_bwd": ms_o, "ms_fwd": ms_f, "ms_bwd": ms_o - ms_f, "peak_bytes": mem_o, "loss": loss_o},
           "baseline_frames": fb,
           "hip_on_baseline_frames": {"ms_fwd_bwd": ms_s, "peak_bytes": mem_s, "loss": loss_s},
           "torch_match_matrix": {"ms_fwd_bwd": ms_t, "peak_bytes": mem_t, "loss": loss_t},
           "loss_rel_diff": abs(loss_s - loss_t) / abs(loss_t), "dp_rel_l2_diff": float((g_s - g_t).norm() / g_t.norm())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
