#!/usr/bin/env python
"""Record the output bits of the f16x3 point-CNF kernel (csrc/ode_f16x3w.hip) on THIS tree's build, for the launches of
tests/test_cnf_f16x3_planes.py (its CASES and its range-guard launch, with that file's own functions): the fixture
tests/golden/cnf_h3w_parent_bits.npz the test compares every later build with, bit for bit.

Run it on the GPU box against a build of the commit whose arithmetic is the reference -- the parent of a change that must not move a
bit, or, after a DELIBERATE change of the kernel's arithmetic, the new commit itself (and say so in that commit).
--band: the launches of tests/test_cnf_f16x3_flush_band.py instead (hidden activations in the f16 flush band), into
tests/golden/cnf_h3w_flush_band_bits.npz, with a census of where layer 0's activations of the edited units start out.
usage: python tools/record_cnf_h3w_bits.py [--band] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def band_census(T, W):
    """Where X = 16 softplus(layer 0) of the edited units starts out (stage 0 of a reverse solve, f32 on the CPU): counts per binade."""
    import torch
    from test_cnf_solve_kernels import base_samples, rnd
    hy, y = T.band(W.hyper(rnd(5600 + 128, 2, 1600), T.LDH)), base_samples(5601 + 128, 2, 128)
    P, t = W.cpu, W.t_end
    for f in (0, 1):
        gate = torch.sigmoid(hy[f, :160] + t * P["tcol"][:160])
        x = (y[f] @ P["w0"][:160].T + P["b0"][:160]) * gate + hy[f, T.BOFF:T.BOFF + 160] + t * P["tcol"][T.BOFF:T.BOFF + 160]
        X = 16.0 * torch.nn.functional.softplus(x)
        e = torch.floor(torch.log2(X.clamp_min(1e-30))).long()
        p1 = X.half().float()
        r = (X - torch.where(p1 < 2.0 ** -14, torch.zeros_like(p1), p1))
        print("frame %d: X of units 0..159 per binade 2^e: %s" % (f, {int(k): int((e == k).sum()) for k in range(-22, 3) if int((e == k).sum())}))
        print("         plane-1 values flushed: %d; remainders in (0, 2^-14): %d, in (-2^-14, 0): %d, at or beyond +-2^-14: %d / %d" % (
            int(((X < 2.0 ** -14) & (X > 0)).sum()), int(((r > 0) & (r < 2.0 ** -14)).sum()), int(((r < 0) & (r > -2.0 ** -14)).sum()),
            int((r >= 2.0 ** -14).sum()), int((r <= -2.0 ** -14).sum())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--band", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "tests", "golden", "cnf_h3w_flush_band_bits.npz" if args.band else "cnf_h3w_parent_bits.npz")
    import torch
    if args.band:
        import test_cnf_f16x3_flush_band as T
    else:
        import test_cnf_f16x3_planes as T
    from caspr_amd.models import CaSPR
    from caspr_amd.utils.synthetic import seeded_state_dict, stress_state_dict
    dev = torch.device("cuda:0")
    skel = CaSPR().state_dict()
    W = {"seeded": T.Weights(seeded_state_dict(skel, 0), dev), "stress": T.Weights(stress_state_dict(skel, 0), dev)}
    out = {}
    for c in T.CASES:
        out[T.case_id(c)] = T.run_case(W[c["w"]], c)
        again = T.run_case(W[c["w"]], c)
        assert np.array_equal(out[T.case_id(c)], again), "%s: two launches differ" % T.case_id(c)
        x = out[T.case_id(c)].view(np.float32)
        assert np.isfinite(x).all()
        print("%-40s %s |x|max %.4f" % (T.case_id(c), x.shape, float(np.abs(x).max())))
    if args.band:
        band_census(T, W["seeded"])
        np.savez_compressed(args.out, **out)
        print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))
        return
    g, word = T.run_guard(W["seeded"])
    out["guard"], out["guard_status"] = g, np.int64(word)
    nan = np.isnan(g.view(np.float32))
    print("guard: NaN points per frame %s of %d, status word %d" % (nan.all(axis=2).sum(axis=1).tolist(), g.shape[1], word))
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
