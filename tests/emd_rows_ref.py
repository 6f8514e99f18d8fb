"""CPU restatement of the row-parallel route of the approximate EMD (caspr_amd/csrc/emd.hip: caspr_emd_rows_f32) for
tests/test_emd_rows_cases.py and tests/test_emd_rows.py: numpy, f32, every sum in the order the kernels take it.

  pass A   suml[k] = 1e-9 + sum_l K(k,l) remainR[l], l ascending;   ratioL[k] = remainL[k] / suml[k]
  pass B   sumr[l] = (sum_k K(k,l) ratioL[k]) remainR[l], k ascending;  ratioR[l] = min(rr / (sumr + 1e-9), 1) rr;  remainR[l] = max(0, rr - sumr)
  pass C   v = K(k,l) ratioL[k] ratioR[l], l ascending:  suml += v, rowcost[k] += v sqrt(d2);  remainL[k] = max(0, remainL[k] - suml)
  cost     partial[t] = rowcost[t] + rowcost[t + 256] + ... (ascending), then the binary tree partial[t] += partial[t + w], w = 128 .. 1

with K = exp(level d2), level = -4^j for j = 7 .. -1 and 0 on the last of the ten levels, and rowcost ONE f32 accumulator per row carried
through all levels.  numpy's exp is not the device's expf bit for bit: this file pins the ORDER to the f64 oracle (oracle/model.py:
approx_emd), the kernels' bits are pinned to the other route's on the GPU.

`wrong` selects one of three subtly wrong variants, each of which a comparison at 1e-4 must catch:
  "drop_tile"    the last partial 1024-point tile of the other cloud is never visited (the sums of all three passes stop at the last
                 multiple of 1024)
  "multiplier"   the smaller cloud's weight m // n (or n // m) left at 1
  "last_level"   the tenth level (level = 0) skipped
"""
import numpy as np

F = np.float32
TILE = 1024
SHAPES = [(1, 1), (1, 7), (5, 1), (37, 37), (100, 300), (255, 257), (256, 256), (257, 255), (64, 1000), (1000, 333), (1025, 1024)]
WRONG = ("drop_tile", "multiplier", "last_level")


def clouds(n, m, B=2):
    """The inputs of tests/test_point_ops_edges.py::test_emd_small_clouds_multipliers_and_the_tile_edge: uniform [0,1]^3, seed n + m."""
    g = np.random.default_rng(n + m)
    return g.uniform(0, 1, (B, n, 3)).astype(F), g.uniform(0, 1, (B, m, 3)).astype(F)


def cost_order(rowcost):
    """sum_k rowcost[k] in the order of emd_rows_cost_kernel: a function of len(rowcost) alone."""
    part = np.zeros(256, F)
    for k0 in range(0, len(rowcost), 256):
        chunk = rowcost[k0:k0 + 256]
        part[:len(chunk)] = (part[:len(chunk)] + chunk).astype(F)
    w = 128
    while w >= 1:
        part[:w] = (part[:w] + part[w:2 * w]).astype(F)
        w >>= 1
    return float(part[0])


def rows_f32(p, q, wrong=None):
    """One frame: p (n,3), q (m,3) f32 -> (cost, tape (10, n + m) f32: per level ratioL then ratioR)."""
    assert wrong is None or wrong in WRONG
    n, m = len(p), len(q)
    mL, mR = (1.0, float(n // m)) if n >= m else (float(m // n), 1.0)
    if wrong == "multiplier":
        mL = mR = 1.0
    lend, kend = (m // TILE * TILE, n // TILE * TILE) if wrong == "drop_tile" else (m, n)
    remL, remR, rowcost = np.full(n, mL, F), np.full(m, mR, F), np.zeros(n, F)
    d2 = np.zeros((n, m), F)
    for c in range(3):                                  # dx*dx + dy*dy + dz*dz, left to right; the sign of dx does not reach d2
        d = (q[None, :, c] - p[:, None, c]).astype(F)
        d2 = (d2 + d * d).astype(F)
    dist = np.sqrt(d2).astype(F)
    tape = np.zeros((10, n + m), F)
    for j in range(7, -3, -1):
        if j == -2 and wrong == "last_level":
            break
        lev = F(0.0) if j == -2 else F(-(4.0 ** j))
        K = np.exp((lev * d2).astype(F)).astype(F)
        s = np.full(n, 1e-9, F)
        for l in range(lend):
            s = (s + (K[:, l] * remR[l]).astype(F)).astype(F)
        rL = (remL / s).astype(F)
        sr = np.zeros(m, F)
        for k in range(kend):
            sr = (sr + (K[k, :] * rL[k]).astype(F)).astype(F)
        sr = (sr * remR).astype(F)
        rR = (np.minimum((remR / (sr + F(1e-9)).astype(F)).astype(F), F(1.0)) * remR).astype(F)
        remR = np.maximum(F(0), (remR - sr).astype(F)).astype(F)
        s3 = np.zeros(n, F)
        for l in range(lend):
            v = ((K[:, l] * rL).astype(F) * rR[l]).astype(F)
            s3 = (s3 + v).astype(F)
            rowcost = (rowcost + (v * dist[:, l]).astype(F)).astype(F)
        remL = np.maximum(F(0), (remL - s3).astype(F)).astype(F)
        tape[7 - j, :n], tape[7 - j, n:] = rL, rR
    return cost_order(rowcost), tape


def rows_cost(p, q, wrong=None):
    """p (B,n,3), q (B,m,3) -> cost (B,) f64 array of the f32 results."""
    return np.array([rows_f32(p[b], q[b], wrong)[0] for b in range(len(p))], np.float64)
