#!/usr/bin/env python
"""Phase split of one RK4 step of the f16x3 point-CNF kernel (cnf_rk4_h3w_kernel, csrc/ode_f16x3w.hip) at the headline shape (160
frames x 2048 points, 8 steps): the s_memtime stamps of workgroup (0,0), thread 0, RK4 step 0, all four stages (XH_STAMP in the
kernel), in s_memtime ticks (shader cycles, as the other phase traces print them).
Needs the debug flavour: CASPR_BUILD_DEBUG=1 python caspr_amd/csrc/build.py (or a CASPR_XW_EXP flavour: --lib NAME).
The stamped kernel spills registers (its scratch traffic shares vmcnt with the weight ring): a stamped stage is much slower than a
real one, compare stamped runs with stamped runs only and size nothing on them alone.   usage: tools/cnf_h3w_trace.py [--lib NAME] [--json PATH]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from caspr_amd import lib

PHASES = [("tables (zeroing, barriers, gate / bias tables)", 0, 1), ("chunk 0 of the input layer (exposed)", 1, 2), ("layer 1 (64 pieces; MFMA floor 49152)", 2, 3),
          ("pass 0 K loop (floor 12288)", 3, 4), ("epilogue 0", 4, 5), ("pass 1 K loop (floor 12288)", 5, 6), ("epilogue 1", 6, 7),
          ("pass 2 K loop (floor 12288)", 7, 8), ("epilogue 2", 8, 9), ("pass 3 K loop (floor 12288)", 9, 10), ("epilogue 3", 10, 11),
          ("output layer + RK4 update", 11, 12)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="libcaspr_hip_debug.so")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    lib.SO_PATH = lib.SO_PATH.replace("libcaspr_hip.so", args.lib)
    from caspr_amd import config
    from caspr_amd.models import CaSPR
    from caspr_amd.utils.synthetic import seeded_state_dict
    assert config.load().cnf_split == "f16x3", "the f16x3 kernel is not the configured route"
    dev = torch.device("cuda:0")
    m = CaSPR()
    m.load_state_dict(seeded_state_dict(m.state_dict(), 0))
    m = m.to(dev).eval()
    BT, n = 160, 2048
    g = torch.Generator().manual_seed(5)
    y, c = torch.randn(BT, n, 3, generator=g).to(dev), torch.randn(BT, 1600, generator=g).to(dev)
    so = ctypes.CDLL(lib.SO_PATH)
    buf = torch.zeros(64, dtype=torch.int64, device=dev)
    with torch.no_grad():
        m.point_cnf(y, c, reverse=True)
        torch.cuda.synchronize()
        so.caspr_debug_set_h3_trace(ctypes.c_void_p(buf.data_ptr()))
        m.point_cnf(y, c, reverse=True)
        torch.cuda.synchronize()
        so.caspr_debug_set_h3_trace(ctypes.c_void_p(0))
    t = buf.cpu().view(4, 16).tolist()
    assert all(t[s][12] > t[s][0] > 0 for s in range(4)), "no stamps: is %s a debug flavour with the stamps on?" % args.lib
    k = 1
    out = {"lib": args.lib, "ticks": t, "stages": []}
    print("%-52s %9s %9s %9s %9s   (cycles)" % ("phase", "stage 0", "stage 1", "stage 2", "stage 3"))
    for nm, a_, b_ in PHASES:
        print("%-52s %9d %9d %9d %9d" % ((nm,) + tuple(round((t[s][b_] - t[s][a_]) * k) for s in range(4))))
    print("%-52s %9d %9d %9d %9d   (MFMA floor 98304)" % (("stage total",) + tuple(round((t[s][12] - t[s][0]) * k) for s in range(4))))
    for s in range(4):
        out["stages"].append({nm: round((t[s][b_] - t[s][a_]) * k) for nm, a_, b_ in PHASES} | {"total": round((t[s][12] - t[s][0]) * k)})
    print("step 0, stage head to stage head: %s" % [round((t[s + 1][0] - t[s][0]) * k) for s in range(3)])
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
