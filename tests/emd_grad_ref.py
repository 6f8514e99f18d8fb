"""CPU reference of the approximate EMD and its gradient for tests/test_emd_grad.py: torch, f64 unless asked otherwise, self-contained.

  approx_match  the ten annealing levels as oracle/model.py:approx_emd states them (approxmatch + matchcost of Fan et al., "A Point Set
                Generation Network"), also returning the match matrix and the per-level ratios in the layout of caspr_emd_tape_f32:
                tape (B, 10, n + m), level i = ratioL_i (n) | ratioR_i (m);
  gradients     torch autograd through (match.detach() * dist).sum(): the match is held fixed, as emd_cuda's matchcost_backward holds it
                (utils/emd.py:17-21), dist = sqrt(max(|p - q|^2, 1e-20)) so that a coincident pair has a zero gradient, not 0 * inf;
  formula       the same gradient from a tape, as caspr_emd_bwd_f32 states it (grads_from_tape) -- and five WRONG variants of it, which
                the test requires the autograd reference to refuse.
"""
import functools

import torch

B = 2
UNIFORM_SHAPES = [(1, 1), (3, 5), (5, 3), (255, 257), (1024, 256), (1025, 1024)]
SHAPES = UNIFORM_SHAPES + [(1100, 700)]             # the last one is randn
SEED = 2000
LEVELS = [-(4.0 ** j) for j in range(7, -2, -1)] + [0.0]                     # j = 7 .. -1, then 0 for the last level (j = -2)
VARIANTS = ("dq_sign", "squared", "no_g", "level_shift", "drop_level")


def multipliers(n, m):
    """-> (multiL, multiR): the integer ratios of the published algorithm; row sums of the match never exceed multiL, column sums multiR."""
    return (1.0, float(n // m)) if n >= m else (float(m // n), 1.0)


@functools.lru_cache(maxsize=None)
def clouds(n, m):
    """-> p (B,n,3), q (B,m,3), g (B,) f32: a function of the shape alone, one generator per shape, p drawn first, then q, then g.
    Uniform [0,1)^3 (randn at (1100, 700)); where n >= 255 the first seven points of q are those of p: coincident pairs.  g has both
    signs.  Treat as read-only (shared by every test)."""
    gen = torch.Generator().manual_seed(SEED + 7 * n + m)
    draw = torch.randn if (n, m) == (1100, 700) else torch.rand
    p = draw(B, n, 3, generator=gen)
    q = draw(B, m, 3, generator=gen)
    if n >= 255:
        q[:, :7] = p[:, :7]
    g = torch.randn(B, generator=gen).abs() + 0.25
    g[1::2] = -g[1::2]
    return p, q, g


@functools.lru_cache(maxsize=None)
def cluster_clouds():
    """-> p (B,5,3), q (B,3,3), g (B,): a (5, 3) case built so that a row of the match matrix is EXACTLY zero in f64 and in f32 (with
    uniform points it practically never is: some level always leaves exp(level d2) > 0).  The three points of q and four of p lie within
    1e-3 of one centre: at the first level (-16384) every kernel value among them is ~1, each right point is offered 4/3 of its mass and
    its remainder is clamped to exactly 0, so every later ratioR is 0.  p's fifth point is 0.5 away along each axis: its kernel values at
    that level underflow to 0 (exp(-12288)), and it never receives anything."""
    gen = torch.Generator().manual_seed(SEED + 53)
    c = torch.full((B, 1, 3), 0.25)
    p = c + 1e-3 * torch.rand(B, 5, 3, generator=gen)
    q = c + 1e-3 * torch.rand(B, 3, 3, generator=gen)
    p[:, 4] = p[:, 4] + 0.5
    g = torch.tensor([0.75, -1.5])
    return p, q, g


def sqdist(p, q):
    return ((p[:, :, None, :] - q[:, None, :, :]) ** 2).sum(-1)               # (B,n,m), the direct form


def approx_match(p, q, dtype=torch.float64):
    """-> cost (B), match (B,n,m), tape (B,10,n+m) in `dtype`: oracle/model.py:approx_emd, level by level, keeping what it discards."""
    p, q = p.to(dtype), q.to(dtype)
    Bn, n, _ = p.shape
    m = q.shape[1]
    d2 = sqdist(p, q)
    dist = d2.sqrt()
    multiL, multiR = multipliers(n, m)
    remainL = torch.full((Bn, n), multiL, dtype=dtype)
    remainR = torch.full((Bn, m), multiR, dtype=dtype)
    cost = torch.zeros(Bn, dtype=dtype)
    match = torch.zeros(Bn, n, m, dtype=dtype)
    tape = torch.zeros(Bn, len(LEVELS), n + m, dtype=dtype)
    for i, level in enumerate(LEVELS):
        K = torch.exp(level * d2)
        ratioL = remainL / (1e-9 + (K * remainR[:, None, :]).sum(2))
        sumr = (K * ratioL[:, :, None]).sum(1) * remainR
        ratioR = torch.clamp(remainR / (sumr + 1e-9), max=1.0) * remainR
        remainR = torch.clamp(remainR - sumr, min=0.0)
        inc = K * ratioL[:, :, None] * ratioR[:, None, :]
        cost = cost + (inc * dist).sum((1, 2))
        match = match + inc
        remainL = torch.clamp(remainL - inc.sum(2), min=0.0)
        tape[:, i, :n], tape[:, i, n:] = ratioL, ratioR
    return cost, match, tape


def level_increments(p, q, tape, shift=0):
    """-> (B,10,n,m): level i's addition to the match matrix, exp(level_{i+shift} d2) ratioL_i[k] ratioR_i[l], in the tape's dtype."""
    n = p.shape[1]
    d2 = sqdist(p.to(tape.dtype), q.to(tape.dtype))
    lv = torch.tensor([LEVELS[(i + shift) % len(LEVELS)] for i in range(len(LEVELS))], dtype=tape.dtype)
    return torch.exp(lv[None, :, None, None] * d2[:, None]) * tape[:, :, :n, None] * tape[:, :, None, n:]


def match_from_tape(p, q, tape):
    return level_increments(p, q, tape).sum(1)


def cost_from_tape(p, q, tape):
    """sum match * dist, in the tape's dtype."""
    return (match_from_tape(p, q, tape) * sqdist(p.to(tape.dtype), q.to(tape.dtype)).sqrt()).sum((1, 2))


def heaviest_level(p, q, tape):
    """The level that carries the largest share of the match mass (what "drop_level" leaves out)."""
    return int(level_increments(p, q, tape).sum((0, 2, 3)).argmax())


def grads_from_tape(p, q, tape, g, variant=None):
    """dp, dq in the tape's dtype from a tape.  variant None is the formula of include/caspr_hip_train.h:
        dp[k] = g sum_l match[k,l] (p_k - q_l) / sqrt(max(|p_k - q_l|^2, 1e-20)),   dq[l] = -g sum_k (the same term);
    the others are mistakes such a kernel is prone to: "dq_sign" flips dq, "squared" is the Chamfer-style term 2 match (p - q), "no_g"
    drops g, "level_shift" pairs the ratios of level i with the kernel of level i + 1 (cyclically), "drop_level" leaves out the level
    that carries the largest share of the match mass."""
    dt = tape.dtype
    p, q, g = p.to(dt), q.to(dt), g.to(dt)
    inc = level_increments(p, q, tape, shift=1 if variant == "level_shift" else 0)
    if variant == "drop_level":
        keep = torch.ones(len(LEVELS), dtype=torch.bool)
        keep[heaviest_level(p, q, tape)] = False
        inc = inc[:, keep]
    match = inc.sum(1)
    diff = p[:, :, None, :] - q[:, None, :, :]
    if variant == "squared":
        term = 2.0 * match[..., None] * diff
    else:
        term = match[..., None] * diff / sqdist(p, q).clamp_min(1e-20).sqrt()[..., None]
    if variant != "no_g":
        term = term * g[:, None, None, None]
    dp, dq = term.sum(2), -term.sum(1)
    if variant == "dq_sign":
        dq = -dq
    return dp, dq


def reference_grads(p, q, g):
    """In f64 from scratch -> cost (B), match (B,n,m), tape (B,10,n+m), dp, dq: the gradient of sum_b g_b cost_b by autograd with the
    match detached."""
    cost, match, tape = approx_match(p, q)
    p6, q6 = p.double().requires_grad_(True), q.double().requires_grad_(True)
    dist = sqdist(p6, q6).clamp_min(1e-20).sqrt()
    loss = (g.double() * (match.detach() * dist).sum((1, 2))).sum()
    dp, dq = torch.autograd.grad(loss, [p6, q6])
    return cost, match, tape, dp, dq


@functools.lru_cache(maxsize=None)
def reference(n, m):
    """reference_grads of clouds(n, m), computed once."""
    return reference_grads(*clouds(n, m))


@functools.lru_cache(maxsize=None)
def restatement_f32(n, m):
    """The same computation carried in f32 on the CPU (levels, tape, formula) -> dp, dq: how far plain f32 rounding alone moves the
    from-scratch gradient (approxmatch is sensitive to it), recorded beside the kernel's distance."""
    p, q, g = clouds(n, m)
    _, _, tape = approx_match(p, q, dtype=torch.float32)
    return grads_from_tape(p, q, tape, g)


def rel_l2(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).norm() / want.norm().clamp_min(1e-300))
