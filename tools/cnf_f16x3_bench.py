"""A/B of the point CNF's sampling launch at the headline shape (160 frames x 2048 points, 8 RK4 steps): the bf16x6 128-point kernel
(cnf_rk4_x6w_kernel) against the f16x3 kernel (cnf_rk4_h3w_kernel), in ONE process, alternating rounds, on both synthetic weight sets.
Prints one JSON document (committed as profiles/cnf_f16x3_bench.json).
--libs NAME=PATH ...: other builds of the library (the parent's, a CASPR_XW_EXP flavour), loaded into the same process; the f16x3 launch
of each joins the alternating rounds under NAME, and its output is compared with this tree's bit for bit."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--libs", nargs="*", default=[])
    args = ap.parse_args()
    from caspr_amd import lib, ops
    from caspr_amd.models import CaSPR
    from caspr_amd.models.cnf import CNF
    from caspr_amd.utils.synthetic import seeded_state_dict, stress_state_dict
    dev = torch.device("cuda:0")
    here = lib.load()
    others = {}
    for spec in args.libs:
        name, path = spec.split("=", 1)
        so = ctypes.CDLL(os.path.abspath(path))
        for fn, (res, argtypes) in lib.SIGNATURES.items():
            getattr(so, fn).restype, getattr(so, fn).argtypes = res, argtypes
        others[name] = so
    out = {"shape": {"frames": args.frames, "points": args.points, "rk4_steps": args.steps}, "rounds": args.rounds, "weights": {}}
    for which, make in (("seeded", seeded_state_dict), ("stress", stress_state_dict)):
        m = CaSPR()
        m.load_state_dict(make(m.state_dict(), 0))
        m = m.to(dev).eval()
        blk = next(b for b in m.modules() if isinstance(b, CNF))
        w = blk._weights()
        w1x, w2x = blk._weights_x6()
        w1h, w2h = blk._weights_h3()
        g = torch.Generator().manual_seed(1)
        ctx = torch.randn(args.frames, w["hyp"].cin, generator=g).to(dev)
        y = (torch.randn(args.frames, args.points, 3, generator=g) * 1.3).clamp(-5, 5).to(dev)
        hyper = ops.conv1x1(w["hyp"], w["hyp_bias"], ctx.view(1, args.frames, -1), row_invariant=True)[0]

        def run(h3, so=here):
            lib._lib = so
            try:
                return ops.cnf_rk4(y, hyper, w["tcol"], w["w0"], w["b0"], w["w1p"], w["b1"], w["w2p"], w["b2"], w["w3"], w["b3"], blk.end_time(),
                                   args.steps, True, w1x=w1x, w2x=w2x, w1h=w1h if h3 else None, w2h=w2h if h3 else None)
            finally:
                lib._lib = here
        xa, xb = run(False), run(True)          # warm-up, and the difference between the two images
        same = {name: bool(torch.equal(run(True, so).view(torch.int32), xb.view(torch.int32))) for name, so in others.items()}
        torch.cuda.synchronize()
        ops.check_deferred_errors()
        ms = {name: [] for name in ["bf16x6", "f16x3"] + list(others)}
        for _ in range(args.rounds):
            for name, h3, so in [("bf16x6", False, here), ("f16x3", True, here)] + [(name, True, so) for name, so in others.items()]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(h3, so)
                e1.record()
                e1.synchronize()
                ms[name].append(round(e0.elapsed_time(e1), 3))
        ops.check_deferred_errors()
        mean = {k: sum(v) / len(v) for k, v in ms.items()}
        out["weights"][which] = {"launch_ms": ms, "mean_ms": {k: round(v, 3) for k, v in mean.items()}, "ratio_f16x3_over_bf16x6": round(mean["f16x3"] / mean["bf16x6"], 4),
                                 "max_abs_diff_x": float((xa - xb).abs().max()), "x_absmax": float(xa.abs().max())}
        if others:
            out["weights"][which]["bits_equal_to_f16x3"] = same
    print(json.dumps(out))


if __name__ == "__main__":
    main()
