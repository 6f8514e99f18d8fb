"""The exact EMD of caspr_amd/csrc/emd_exact.hip (caspr_emd_exact_f32) restated on the CPU in numpy f64, operation for operation as
include/caspr_hip.h states it, and the comparison functions the tests hold the kernel to.

  cost_matrix(p, q)      c[i,j] = sqrtf(dx*dx + dy*dy + dz*dz) in f32 in that association, promoted to f64
  auction(p, q, eps)     the forward Jacobi auction with eps scaling -> assign, prices, info = [converged, phases, rounds, bids]
  dual_bound(C, prices)  sum_i min_j (C[i,j] + p[j]) - sum_j p[j]: a lower bound of the optimal assignment cost for ANY prices (weak
                         duality of the assignment problem), so primal - dual_bound bounds the distance to the optimum from above
  primal(C, assign)      sum_i C[i, assign[i]] in f64; refuses anything but a permutation
Why n * eps: when a phase ends every point i holds an object within eps of its best value at the final prices (eps-complementary
slackness: the bid raised p[j1] to exactly eps above indifference with the second best, and prices only rise, which only lowers the value
of the others), so sum_i (C[i,a_i] + p[a_i]) <= sum_i min_j (C[i,j] + p[j]) + n eps; a_i is a permutation, so the prices cancel.
"""
import itertools

import numpy as np

MAX_PHASES = 64


def cost_matrix(p, q):
    p, q = np.asarray(p, dtype=np.float32), np.asarray(q, dtype=np.float32)
    dx = p[:, None, 0] - q[None, :, 0]
    dy = p[:, None, 1] - q[None, :, 1]
    dz = p[:, None, 2] - q[None, :, 2]
    c = np.sqrt(dx * dx + dy * dy + dz * dz)          # f32 throughout: numpy keeps the operands' type, no contraction
    assert c.dtype == np.float32
    return c.astype(np.float64)


def diagonal(p, q):
    """D: the f32 diagonal of the bounding box of both clouds."""
    both = np.concatenate([np.asarray(p, dtype=np.float32), np.asarray(q, dtype=np.float32)], axis=0)
    e = (both.max(axis=0) - both.min(axis=0)).astype(np.float32)
    d = np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
    assert d.dtype == np.float32
    return d


def auction(p, q, eps, max_bids=None):
    """-> assign (n,) int32 (-1 everywhere if the frame stopped), prices (n,) f64, info [converged, phases, rounds, bids]."""
    C = cost_matrix(p, q)
    n = C.shape[0]
    if max_bids is None:
        max_bids = 4096 * n
    eps = float(eps)
    prices = np.zeros(n, dtype=np.float64)
    e = float(diagonal(p, q)) / 4.0
    if not e > eps:
        e = eps
    bids = rounds = phases = 0
    converged = False
    owner = np.full(n, -1, dtype=np.int64)
    while phases < MAX_PHASES:
        phases += 1
        owner[:] = -1                                   # owner[j]: the point of cloud 1 that holds object j
        unassigned = np.arange(n)
        stopped = False
        while unassigned.size:
            if bids + unassigned.size > max_bids:
                stopped = True
                break
            bids += unassigned.size
            rounds += 1
            V = -C[unassigned] - prices[None, :]        # every bid from the prices at the start of the round
            j1 = V.argmax(axis=1)                       # the lowest index among equal values
            rows = np.arange(unassigned.size)
            v1 = V[rows, j1]
            if n == 1:
                v2 = v1
            else:
                V[rows, j1] = -np.inf
                v2 = V.max(axis=1)
            bid = prices[j1] + (v1 - v2) + e
            nxt = []
            for j in np.unique(j1):
                cand = np.nonzero(j1 == j)[0]
                top = bid[cand].max()                   # the object takes its highest bid ...
                winner = unassigned[cand[bid[cand] == top]].min()   # ... ties to the lowest bidder index
                if owner[j] >= 0:
                    nxt.append(owner[j])                # the previous owner bids again
                owner[j] = winner
                prices[j] = top
                nxt.extend(i for i in unassigned[cand] if i != winner)
            unassigned = np.array(sorted(nxt), dtype=np.int64)
        if stopped:
            break
        if e <= eps:
            converged = True
            break
        e = e / 5.0
        if not e > eps:
            e = eps
    assign = np.full(n, -1, dtype=np.int32)
    if converged:
        assign[owner] = np.arange(n, dtype=np.int32)
    return assign, prices, np.array([int(converged), phases, rounds, bids], dtype=np.int32)


def is_permutation(assign):
    a = np.asarray(assign)
    return a.ndim == 1 and np.array_equal(np.sort(a), np.arange(a.shape[0]))


def primal(C, assign):
    if not is_permutation(assign):
        raise ValueError("not a permutation: a cost summed over it is not an assignment cost")
    return float(C[np.arange(C.shape[0]), np.asarray(assign)].sum())


def dual_bound(C, prices):
    prices = np.asarray(prices, dtype=np.float64)
    return float((C + prices[None, :]).min(axis=1).sum() - prices.sum())


def certificate_gap(C, assign, prices):
    """primal - dual_bound >= 0: how far the assignment can be from the optimum at most."""
    return primal(C, assign) - dual_bound(C, prices)


def certified(C, assign, prices, eps):
    return is_permutation(assign) and certificate_gap(C, assign, prices) <= C.shape[0] * eps * (1 + 1e-9)


def brute_force(C):
    """The optimum over all permutations (n <= 8)."""
    n = C.shape[0]
    assert n <= 8
    perms = np.array(list(itertools.permutations(range(n))), dtype=np.int64)
    return float(C[np.arange(n)[None, :], perms].sum(axis=1).min())


# ---- the inputs of the GPU tests (tests/test_emd_exact.py), deterministic ----
def uniform(n, B, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, (B, n, 3)).astype(np.float32), rng.uniform(0, 1, (B, n, 3)).astype(np.float32)


def clustered(n, B, seed):
    """two tight clusters against a uniform cloud"""
    rng = np.random.default_rng(seed)
    centres = np.array([[0.25, 0.25, 0.25], [0.75, 0.7, 0.8]], dtype=np.float64)
    p = centres[rng.integers(0, 2, (B, n))] + rng.normal(0, 0.01, (B, n, 3))
    return p.astype(np.float32), rng.uniform(0, 1, (B, n, 3)).astype(np.float32)


def duplicated(n, B, seed, times=16):
    """every point repeated `times` times on both sides (n a multiple of `times`, or the tail is cut from the repetition)"""
    rng = np.random.default_rng(seed)
    k = -(-n // times)
    p = np.repeat(rng.uniform(0, 1, (B, k, 3)), times, axis=1)[:, :n]
    q = np.repeat(rng.uniform(0, 1, (B, k, 3)), times, axis=1)[:, :n]
    return p.astype(np.float32), q.astype(np.float32)


def permuted(n, B, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0, 1, (B, n, 3)).astype(np.float32)
    q = np.stack([p[b][rng.permutation(n)] for b in range(B)])
    return p, q
