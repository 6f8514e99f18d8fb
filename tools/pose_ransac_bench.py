"""Time ops.ransac_rigid_from_correspondences (csrc/pose.hip) at the camera-pose protocol size: F = 160 frames (B = 16 x T = 10),
N = 2048 correspondences, K = 5000 hypotheses of 4, on planted rigid frames (3 mm noise, 40 % outliers).  HIP events around
`--iters` calls after `--warmup` calls; prints ms per call and the rate of the residual tests' f64 arithmetic.

    PYTHONPATH=. timeout -k 10 300 python tools/pose_ransac_bench.py [--frames 160] [--points 2048] [--hypotheses 5000] [--refine]

Op count: a residual test is 27 f64 operations as the kernel writes it without contraction (R src: 9 mul + 6 add; + t: 3 add;
- dst: 3 sub; |r|^2: 3 mul + 2 add; the masked sum: 1 add), plus 6 f32 -> f64 conversions not counted; the estimates and the
selection pass are a few per cent of it and not counted either."""
import argparse
import json

import numpy as np
import torch

from caspr_amd import ops

OPS_PER_TEST = 27


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--hypotheses", type=int, default=5000)
    ap.add_argument("--refine", action="store_true")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    F, N, K = a.frames, a.points, a.hypotheses
    src = rng.rand(F, N, 3) - 0.5
    q = rng.randn(F, 4)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                  np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)
    t = rng.randn(F, 3) * 0.5 + np.array([0.0, 0.0, 2.0])
    dst = np.einsum("fij,fnj->fni", R, src) + t[:, None] + rng.randn(F, N, 3) * 0.003
    bad = rng.rand(F, N) < 0.4
    dst = np.where(bad[..., None], rng.rand(F, N, 3) - 0.5 + t[:, None], dst)
    s = torch.from_numpy(src.astype(np.float32)).cuda()
    d = torch.from_numpy(dst.astype(np.float32)).cuda()
    for _ in range(a.warmup):
        out = ops.ransac_rigid_from_correspondences(s, d, num_hypotheses=K, refine=a.refine)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(a.iters):
        e0.record()
        out = ops.ransac_rigid_from_correspondences(s, d, num_hypotheses=K, refine=a.refine)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    T = out[0].cpu().numpy()
    cosang = np.clip((np.einsum("fji,fji->f", T[:, :3, :3], R) - 1) / 2, -1, 1)
    rot = np.degrees(np.arccos(cosang))
    tr = np.linalg.norm(T[:, :3, 3] - t, axis=1)
    ms = float(np.median(times))
    tests = float(F) * K * N
    print(json.dumps({"F": F, "N": N, "K": K, "refine": a.refine, "ms_median": round(ms, 4), "ms_min": round(min(times), 4),
                      "ms_max": round(max(times), 4), "residual_tests": tests, "f64_tflops": round(tests * OPS_PER_TEST / ms / 1e9, 2),
                      "max_rot_err_deg": round(float(rot.max()), 4), "max_trans_err_m": round(float(tr.max()), 5),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
