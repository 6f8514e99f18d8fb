"""CPU reference of the Chamfer loss and its gradient for tests/test_chamfer_grad.py: torch in f64.

  distances  squared distances by torch.cdist (the direct form, no |a|^2 + |b|^2 - 2ab cancellation), then min;
  indices    the f64 argmin (equal to an f32 argmin only without near-ties: min_rel_gap states how far the inputs are from one);
  gradients  torch autograd through cdist -> ** 2 -> min (reference_grads);
  formula    the same gradient from the index vectors, as caspr_chamfer_bwd_f32 states it (grads_from_indices) -- and three WRONG
             variants of it, which the test requires the autograd reference to refuse.
"""
import functools

import torch

B = 3
SHAPES = [(1, 1), (3, 5), (255, 257), (1024, 1025), (1100, 700)]
# one generator per shape, p drawn first, then q, then the loss weights w1, w2; the seed is one at which min_rel_gap >= MIN_GAP at every
# shape (1000: 1.0e-4 .. 2.0e-2; 1001 and 1002 hold too)
SEED = 1000
MIN_GAP = 1e-5


@functools.lru_cache(maxsize=None)
def clouds(n, m):
    """-> p (B,n,3), q (B,m,3), w1 (B,n), w2 (B,m) f32: a function of the shape alone.  Treat as read-only (shared by every test)."""
    gen = torch.Generator().manual_seed(SEED)
    p = torch.randn(B, n, 3, generator=gen)
    q = torch.randn(B, m, 3, generator=gen)
    w1 = torch.randn(B, n, generator=gen)
    w2 = torch.randn(B, m, generator=gen)
    return p, q, w1, w2


def sqdist64(p, q):
    return torch.cdist(p.double(), q.double(), compute_mode="donot_use_mm_for_euclid_dist") ** 2


def min_rel_gap(p, q):
    """Smallest (second nearest - nearest) / second nearest squared distance over every point of both clouds (inf where a point
    has one candidate only)."""
    d = sqdist64(p, q)
    gap = float("inf")
    for dd in (d, d.transpose(1, 2)):
        if dd.shape[2] < 2:
            continue
        two = dd.topk(2, dim=2, largest=False).values
        gap = min(gap, float(((two[..., 1] - two[..., 0]) / two[..., 1]).min()))
    return gap


def reference_grads(p, q, w1, w2):
    """-> d1, d2 (f64), idx1, idx2 (int64), dp, dq (f64) of loss = sum(w1 d1) + sum(w2 d2); w1 / w2 None = that term is absent."""
    p6, q6 = p.double().requires_grad_(True), q.double().requires_grad_(True)
    d = sqdist64(p6, q6)
    m1, m2 = d.min(dim=2), d.min(dim=1)
    loss = 0.0
    if w1 is not None:
        loss = loss + (w1.double() * m1.values).sum()
    if w2 is not None:
        loss = loss + (w2.double() * m2.values).sum()
    dp, dq = torch.autograd.grad(loss, [p6, q6])
    return m1.values.detach(), m2.values.detach(), m1.indices, m2.indices, dp, dq


@functools.lru_cache(maxsize=None)
def reference(n, m):
    """reference_grads of clouds(n, m), computed once."""
    return reference_grads(*clouds(n, m))


def _one_side(a, b, idx_ab, idx_ba, g_a, g_b, scatter=True):
    """Gradient for cloud a: 2 g_a (a_i - b_idx_ab[i])  +  sum over j with idx_ba[j] == i of 2 g_b[j] (a_i - b_j)."""
    Bn = a.shape[0]
    rows = torch.arange(Bn).unsqueeze(1)
    out = 2.0 * g_a.unsqueeze(2) * (a - b[rows, idx_ab])
    if scatter:
        for k in range(Bn):
            out[k].index_add_(0, idx_ba[k], 2.0 * g_b[k].unsqueeze(1) * (a[k][idx_ba[k]] - b[k]))
    return out


def grads_from_indices(p, q, idx1, idx2, w1, w2, variant=None):
    """dp, dq in f64 from the index vectors.  variant None is the formula of include/caspr_hip_train.h; the others are mistakes such a
    kernel is prone to: "no_scatter" drops the sum over the other direction's matches, "dq_sign" flips dq, "idx_swapped" looks the own
    term's neighbour up in idx2 where idx1 belongs (wrapped to the sizes where n != m)."""
    p6, q6, g1, g2 = p.double(), q.double(), w1.double(), w2.double()
    n, m = p.shape[1], q.shape[1]
    own1 = idx1
    if variant == "idx_swapped":
        own1 = idx2[:, torch.arange(n) % m] % m
    dp = _one_side(p6, q6, own1, idx2, g1, g2, scatter=variant != "no_scatter")
    dq = _one_side(q6, p6, idx2, idx1, g2, g1, scatter=variant != "no_scatter")
    if variant == "dq_sign":
        dq = -dq
    return dp, dq


def rel_l2(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).norm() / want.norm().clamp_min(1e-300))
