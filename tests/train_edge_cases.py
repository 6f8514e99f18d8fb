"""Case builders and f64 references for the edge tests of the training-tier kernels (test_train_edge_cases.py checks the cases on
the CPU, test_hip_train_edges.py runs the kernels on them): the encoder's GroupNorm / max / column-sum kernels (gn_stats_train,
gn_bwd, gn_rows, gn_rows_bwd, argmax_points, colsum_batched), two routes of conv1x1_wgrad and the value-only CNF layers.

A case is a function of its parameters and a seed and returns a namespace of f32 inputs (logical shapes: the GPU tests embed them in
wider buffers) and f64 expected outputs.  The references are the plain operation: torch.nn.functional.group_norm (+ relu, + max) in
f64 with torch.autograd, gated_softplus of test_hip_train_kernels.py for the CNF layers, einsum / sum for weight gradients and column
sums.  Wherever a max is involved the reference takes the FIRST index by numpy.argmax on the f64 values and routes the gradient through
an explicit gather at that index: the tie rule is stated here, not inherited from torch.max.  No GPU code is imported.
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from test_hip_train import rnd
from test_hip_train_kernels import gated_softplus

NAN = float("nan")
RELU_MARGIN = 1e-3          # min |gamma xh + beta| of a case whose backward applies a ReLU mask
MAX_GAP = 1e-4              # top-two gap of a max without intended ties, relative to the largest entry

# bounds of the GPU comparisons (relative to the reference tensor's largest entry); the CPU controls use the same ones
FWD, GRAD = 1e-5, 5e-5      # CNF layers
ENC_FWD, GN_GRAD, ROWS_GRAD, COLSUM, WGRAD = 2e-5, 5e-5, 1e-4, 1e-5, 3e-6


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def embed(t, ld=None, col0=0, rows=None, fill=NAN):
    """t (..., R, C) -> a (..., rows, ld) buffer filled with `fill` holding t in rows 0..R-1, columns col0..col0+C-1."""
    R, C = t.shape[-2], t.shape[-1]
    ld = (col0 + C + 3) // 4 * 4 + 4 if ld is None else ld
    buf = torch.full(tuple(t.shape[:-2]) + (R if rows is None else rows, ld), fill, dtype=t.dtype)
    buf[..., :R, col0:col0 + C] = t
    return buf


def first_argmax(v, dim):
    """First index of the maximum along dim, by numpy.argmax on the f64 values."""
    return torch.from_numpy(np.argmax(v.detach().double().numpy(), axis=dim))


def first_seed(build, ok, tries=20):
    """The first seed in 0..tries-1 whose case meets its input conditions."""
    for s in range(tries):
        case = build(s)
        if ok(case):
            return case
    raise AssertionError("no seed in 0..%d meets the input conditions" % (tries - 1))


def signed(g, n, lo=0.5, hi=1.5):
    return g.uniform(lo, hi, n) * g.choice([-1.0, 1.0], n)


def lattice(g, shape):
    """integer in [-3, 3] + uniform(-0.2, 0.2): at least 0.3 from every half-integer."""
    return g.integers(-3, 4, shape) + g.uniform(-0.2, 0.2, shape)


# ---------------------------------------------------------------------------------------------
# GroupNorm over points: gn_stats_train, gn_bwd
# ---------------------------------------------------------------------------------------------
def gn_pre(y, gamma, beta, groups, eps=1e-5):
    """(B, P, C) -> gamma xh + beta, by torch's group_norm (the functional form refuses a single value per channel: B = P = 1)."""
    return torch.group_norm(y.transpose(1, 2), groups, gamma, beta, eps, False).transpose(1, 2)


def gn_moments(y, groups, eps=1e-5):
    """(B, P, C) f64 -> mean, rstd (B, groups)."""
    B, P, C = y.shape
    var, mean = torch.var_mean(y.reshape(B, P, groups, C // groups), dim=(1, 3), unbiased=False)
    return mean, (var + eps).rsqrt()


def per_channel(m, C):
    return m.repeat_interleave(C // m.shape[-1], dim=-1)


def case_gn_stats(B, P, C, groups=16, seed=0, eps=1e-5, drop_row=None, pmax_rule="first principles"):
    """y normal with the LAST batch entry around 1000 (unit spread); gamma with negative entries and an exact zero.
    drop_row / pmax_rule build the controls: the moments without one row; the max of y where the scale is negative."""
    g = np.random.default_rng(1000 + seed)
    y = g.normal(0, 1, (B, P, C))
    if B > 1:
        y[B - 1] += 1000.0
    gamma = signed(g, C)
    gamma[0], gamma[1], gamma[C - 1] = 0.0, -abs(gamma[1]), -abs(gamma[C - 1])
    beta = g.normal(0, 0.3, C)
    y, gamma, beta = f32(y), f32(gamma), f32(beta)
    y6, ga6, be6 = y.double(), gamma.double(), beta.double()
    keep = [p for p in range(P) if p != drop_row]
    mean, rstd = gn_moments(y6[:, keep], groups, eps)
    scale = ga6 * per_channel(rstd, C)
    shift = be6 - per_channel(mean, C) * scale
    if drop_row is None and pmax_rule == "first principles":
        pmax = gn_pre(y6, ga6, be6, groups, eps).max(dim=1).values
    elif pmax_rule == "max under negative scale":
        pmax = y6.max(dim=1).values * scale + shift
    else:
        pmax = (y6 * scale.unsqueeze(1) + shift.unsqueeze(1)).max(dim=1).values
    return SimpleNamespace(y=y, gamma=gamma, beta=beta, groups=groups, eps=eps,
                           want=dict(scale=scale, shift=shift, mean=mean, rstd=rstd, pmax=pmax))


def pmax_f32_error(case, b):
    """Error of pmax[b] when the SAME formula runs in plain f32 torch on the CPU: max over points of y scale + shift with the f64
    scale / shift rounded to f32 -- the best the affine form can do in f32 -- relative to the largest f64 entry."""
    sc, sf = case.want["scale"][b].float(), case.want["shift"][b].float()
    got = (case.y[b] * sc + sf).max(dim=0).values
    return float((got.double() - case.want["pmax"][b]).abs().max() / case.want["pmax"][b].abs().max())


def pmax_bound(case, b):
    """2e-5, or twice the f32 affine form's own error where that is larger (the batch entry around 1000: y scale + shift cancels two
    numbers of size ~1000 gamma rstd to a result of size ~1, leaving ~1e-4 / |pmax|max whatever computes it in f32); never above 2e-4."""
    return min(2e-4, max(ENC_FWD, 2.0 * pmax_f32_error(case, b)))


GN_BWD_SHAPES = [(3, 1025, 64), (2, 1030, 192), (2, 37, 1600), (1, 5, 4096), (3, 2049, 128), (2, 1, 64), (2, 3, 64)]


def case_gn_bwd(B, P, C, groups=16, seed=0):
    """The lattice construction: y = integer in [-3, 3] + uniform(-0.2, 0.2), |gamma| in [0.5, 1.5] with random sign and
    beta_c = -gamma_c (h_c - mean_g) rstd_g with h_c a half-integer and the moments of batch entry 0, so that
    gamma xh + beta ~ gamma rstd (y - h) stays away from 0 with about half of the elements rectified.  Every channel's maximum over
    points is planted (|y| = 4 on the side of gamma's sign) in the last row, in row 0 or in the middle row, by (channel + entry) % 3."""
    g = np.random.default_rng(2000 + seed)
    y = lattice(g, (B, P, C))
    gamma = signed(g, C)
    where = np.array([P - 1, 0, P // 2])
    for b in range(B):
        rows = where[(np.arange(C) + b) % 3]
        y[b, rows, np.arange(C)] = 4.0 * np.sign(gamma) + g.uniform(-0.2, 0.2, C)
    y, gamma = f32(y), f32(gamma)
    y6, ga6 = y.double(), gamma.double()
    mean, rstd = gn_moments(y6, groups)
    h = g.choice([-1.5, -0.5, 0.5, 1.5], C)
    beta = f32((-ga6 * (torch.from_numpy(h) - per_channel(mean[0], C)) * per_channel(rstd[0], C)).numpy())
    pre = gn_pre(y6, ga6, beta.double(), groups)
    return SimpleNamespace(y=y, gamma=gamma, beta=beta, groups=groups, mean=mean, rstd=rstd, pre=pre,
                           da=rnd(2100 + seed, B, P, C), dmax=rnd(2200 + seed, B, C), amax=first_argmax(pre, 1).to(torch.int32),
                           dgamma0=rnd(2300 + seed, C), dbeta0=rnd(2400 + seed, C))


def gn_bwd_want(case, use_da, use_dmax, relu):
    """dY, dgamma, dbeta of sum(da relu?(a)) + sum(dmax a[amax]) by autograd (the max is of the un-rectified feature)."""
    y6, ga6, be6 = (t.double().requires_grad_(True) for t in (case.y, case.gamma, case.beta))
    a = gn_pre(y6, ga6, be6, case.groups)
    loss = 0.0
    if use_da:
        loss = loss + ((F.relu(a) if relu else a) * case.da.double()).sum()
    if use_dmax:
        loss = loss + (a.gather(1, case.amax.long().unsqueeze(1)).squeeze(1) * case.dmax.double()).sum()
    loss.backward()
    return dict(dY=y6.grad, dgamma=ga6.grad, dbeta=be6.grad)


def gn_bwd_formula(case, relu, n=None, mask_shift=0, drop_row=None):
    """The closed form of the dense gn_bwd (f64), for the controls: n of the mean term, the ReLU mask rolled by rows, a row left
    out of the parameter sums."""
    y6, ga6 = case.y.double(), case.gamma.double()
    B, P, C = y6.shape
    G = case.groups
    n = (C // G) * P if n is None else n
    mu, rs = per_channel(case.mean, C).unsqueeze(1), per_channel(case.rstd, C).unsqueeze(1)
    xh = (y6 - mu) * rs
    gq = case.da.double()
    if relu:
        gq = gq * torch.roll(case.pre > 0, mask_shift, dims=1)
    keep = [p for p in range(P) if p != drop_row]
    sg, sgx = gq.sum(1), (gq * xh).sum(1)
    s1 = per_channel((ga6 * sg).reshape(B, G, -1).sum(-1), C).unsqueeze(1)
    s2 = per_channel((ga6 * sgx).reshape(B, G, -1).sum(-1), C).unsqueeze(1)
    return dict(dY=rs * (gq * ga6 - (s1 + xh * s2) / n), dgamma=(gq * xh)[:, keep].sum((0, 1)), dbeta=gq[:, keep].sum((0, 1)))


# ---------------------------------------------------------------------------------------------
# GroupNorm(16) per neighbourhood: gn_rows, gn_rows_bwd
# ---------------------------------------------------------------------------------------------
def rows_pre(y, gamma, beta, eps):
    """(NB, ns, C) -> gamma xh + beta with the statistics per (neighbourhood, group) over cpg channels x ns rows."""
    return gn_pre(y, gamma, beta, 16, eps)


def source_row(ns, dup):
    """The row that repeats: dup = k -> the last k rows repeat row 0 (the ball query's padding); dup = (a, b) -> row b repeats row a."""
    return dup[0] if isinstance(dup, tuple) else 0


def repeated_rows(ns, dup):
    return [dup[1]] if isinstance(dup, tuple) else list(range(ns - dup, ns))


def distinct_rows(ns, dup):
    return [r for r in range(ns) if r not in repeated_rows(ns, dup)]


def _repeat(y, ns, dup):
    y[:, repeated_rows(ns, dup)] = y[:, source_row(ns, dup)][:, None]


def _push_extremes(y, sign, rows):
    """Every column's extreme on the side of gamma's sign (over the distinct rows) moves out by 1: the max over rows has a gap."""
    r = np.array(rows)[np.argmax(y[:, rows] * sign, axis=1)][:, None, :]
    np.put_along_axis(y, r, np.take_along_axis(y, r, axis=1) + sign, axis=1)


def _rows_data(g, NB, ns, C, kind, dup, eps):
    """kind "normal": N(0, 1).  "lattice": ONE (ns, C) lattice block (with the rows `dup` names repeating another, see source_row);
    every neighbourhood permutes the channels inside each group and, without repeats, the rows -- all share their moments, beta is the lattice
    construction of case_gn_bwd.  In both, gamma has one sign per group and every column's extreme on that side is moved out by 1 (a
    lattice point again), so that the max over rows has a clear winner.  "column": every column a permutation of {0, 0.5, ...} +
    uniform(-0.1, 0.1), |beta| = 0.3 |gamma|."""
    cpg = C // 16
    gamma = g.uniform(0.5, 1.5, C) * np.repeat(g.choice([-1.0, 1.0], 16), cpg)
    sign = np.sign(gamma)
    if kind == "normal":
        y = g.normal(0, 1, (NB, ns, C))
        _push_extremes(y, sign, distinct_rows(ns, dup))
        _repeat(y, ns, dup)
        beta = g.normal(0, 0.3, C)
    elif kind == "column":
        y = g.permuted(np.tile(0.5 * np.arange(ns)[None, :, None], (NB, 1, C)), axis=1) + g.uniform(-0.1, 0.1, (NB, ns, C))
        beta = 0.3 * np.abs(gamma) * g.choice([-1.0, 1.0], C)
    else:
        base = lattice(g, (1, ns, C))
        _push_extremes(base, sign, distinct_rows(ns, dup))
        _repeat(base, ns, dup)
        base = base[0]
        m = base.reshape(ns, 16, cpg).mean(axis=(0, 2))
        rs = 1.0 / np.sqrt(base.reshape(ns, 16, cpg).var(axis=(0, 2)) + eps)
        h = g.choice([-1.5, -0.5, 0.5, 1.5], C)
        beta = -gamma * (h - np.repeat(m, cpg)) * np.repeat(rs, cpg)
        y = np.tile(base[None], (NB, 1, 1)).reshape(NB, ns, 16, cpg)
        perm = np.argsort(g.random((NB, 16, cpg)), axis=2)                      # channels inside each group, the same for all rows
        y = np.take_along_axis(y, perm[:, None], axis=3).reshape(NB, ns, C)
        if not dup:
            rp = np.argsort(g.random((NB, ns)), axis=1)
            y = np.take_along_axis(y, rp[:, :, None], axis=1)
    return y, gamma, beta


def case_gn_rows(B, M, ns, C, relu, kind="normal", dup=0, seed=0, eps=1e-5, backward=True):
    """y (B, M ns, C); expected A, mean, rstd, max over the ns rows (of the rectified value when relu) with its first index, and the
    gradients of sum(da A) (dense) and of sum(dmax max) routed through a gather at that index."""
    NB = B * M
    g = np.random.default_rng(3000 + seed)
    y, gamma, beta = _rows_data(g, NB, ns, C, kind, dup, eps)
    y, gamma, beta = f32(y), f32(gamma), f32(beta)
    da, dmax = rnd(3100 + seed, NB, ns, C), rnd(3200 + seed, NB, C)
    y6, ga6, be6 = (t.double().requires_grad_(True) for t in (y, gamma, beta))
    pre = rows_pre(y6, ga6, be6, eps)
    A = F.relu(pre) if relu else pre
    arg = first_argmax(A, 1)
    mx = A.gather(1, arg.unsqueeze(1)).squeeze(1)
    yg = y6.detach().reshape(NB, ns, 16, C // 16)
    var, mean = torch.var_mean(yg, dim=(1, 3), unbiased=False)
    want = dict(A=A.detach().reshape(B, M * ns, C), mean=mean, rstd=(var + eps).rsqrt(), max=mx.detach().reshape(B, M, C), arg=arg.to(torch.int32))
    if backward:
        for mode, loss in (("dense", (A * da.double()).sum()), ("dmax", (mx * dmax.double()).sum())):
            gy, gg, gb = torch.autograd.grad(loss, (y6, ga6, be6), retain_graph=True)
            want[mode] = dict(dY=gy.reshape(B, M * ns, C), dgamma=gg, dbeta=gb)
    return SimpleNamespace(y=y.reshape(B, M * ns, C), gamma=gamma, beta=beta, ns=ns, C=C, relu=relu, eps=eps, dup=dup, NB=NB,
                           da=da.reshape(B, M * ns, C), dmax=dmax.reshape(B, M, C), pre=pre.detach(), want=want,
                           dgamma0=rnd(3300 + seed, C), dbeta0=rnd(3400 + seed, C))


def relu_margin(pre):
    return float(pre.abs().min())


def max_gap_ok(v, distinct=None):
    """v (NB, rows, C): the top-two gap over the rows `distinct` lists (all by default) is >= MAX_GAP x the largest entry in every
    column -- or the column's maximum is an exact 0 (every row rectified: an exact tie, first index 0 on both sides)."""
    v = v[:, distinct] if distinct is not None else v
    if v.shape[1] < 2:
        return True
    top = torch.topk(v, 2, dim=1).values
    return bool((((top[:, 0] - top[:, 1]) >= MAX_GAP * float(v.abs().max())) | (top[:, 0] == 0)).all())


def rows_case_ok(c):
    A = F.relu(c.pre) if c.relu else c.pre
    return (not c.relu or relu_margin(c.pre) >= RELU_MARGIN) and max_gap_ok(A, distinct_rows(c.ns, c.dup))


# Groups of at most TWO elements (ns cpg <= 2: xh = 0 or ~ +-1).  The data gradient of a two-element group is proportional to
# 1 - xh^2 = eps / (var + eps): with eps = 1e-5 that is ~1e-4 or less, a difference f32 cannot form to 1e-4 of itself whatever the
# kernel does (dY = rstd (g gamma - (s1 + xh s2) / n) in plain f32 torch on the CPU against f64, ns = 2, C = 16: 7.2e-4 on the
# grid-stride data, 4.7e-3 / 1.7e-2 on the small normal / lattice cases -- above the 2e-4 no bound may exceed; 2e-7 .. 2e-6 with
# eps = 0.05), so these cases normalise with eps = 0.05.  A one-element group has dY = 0 identically: the GPU test compares it
# against the scale of the formula's first term (dy_scale) instead of the reference's rounding noise.
ROWS_TINY_EPS = 0.05
ROWS_C = [16, 32, 64, 96, 128, 256, 512]
ROWS_NS = [1, 2, 3, 5, 16, 33]
ROWS_NB = [1, 5]
# (C, ns, dup): dup = k -> the last k rows repeat row 0; dup = (a, b) -> row b repeats row a.  (2, 5): the later row sits in the EARLIER
# row phase (5 % 4 = 1 < 2); (3, 4): the later row sits in phase 0.  First occurrence = smallest row, whatever the phase.
ROWS_DUP = [(64, 5, 4), (64, 16, 5), (16, 3, 1), (512, 5, 2), (96, 33, 32), (64, 8, (2, 5)), (32, 9, (3, 4)), (256, 7, (1, 6))]
ROWS_FWD_STRIDE = 4 * 8192 + 3      # neighbourhoods: the forward's grid of 8192 workgroups x 4 strides once more
ROWS_BWD_STRIDE = 4 * 2048 + 3


def rows_eps(ns, C):
    return ROWS_TINY_EPS if ns * (C // 16) <= 2 else 1e-5


def small_rows_case(B, M, ns, C, relu, dup=0):
    """The small gn_rows cases: normal data without ReLU, the shared-moment lattice with it; the first seed that meets the conditions."""
    return first_seed(lambda s: case_gn_rows(B, M, ns, C, relu, "lattice" if relu else "normal", dup, s, rows_eps(ns, C)), rows_case_ok)


def stride_rows_case(direction, C=16, ns=2):
    """The grid-stride passes: ns = 2, C = 16 on per-column permutations of {0, 0.5} + noise; backward also C = 512, ns = 1 (lattice)."""
    if direction == "fwd":
        return first_seed(lambda s: case_gn_rows(1, ROWS_FWD_STRIDE, ns, C, True, "column", 0, s, 1e-5, backward=False), rows_case_ok, 3)
    kind = "column" if C == 16 else "lattice"
    return first_seed(lambda s: case_gn_rows(1, ROWS_BWD_STRIDE, ns, C, True, kind, 0, s, rows_eps(ns, C)), rows_case_ok, 3)


def dy_scale(case, mode):
    """Largest |rstd gamma g|: the first term of dY = rstd (g gamma - (s1 + xh s2) / n)."""
    g = case.da.abs().max() if mode == "dense" else case.dmax.abs().max()
    return float(case.want["rstd"].max() * case.gamma.abs().max() * g)


GN_STATS_CASES = [(3, P, 64, 16) for P in (1, 3, 1023, 1024, 1025, 2049)] + [
    (3, 37, 1024, 16), (3, 1025, 16, 4), (3, 3, 16, 4), (3, 1025, 192, 16), (3, 3, 192, 16), (3, 37, 1600, 16), (3, 5, 4096, 16), (3, 1, 4096, 16)]
ARGMAX_CASES = [(2, 1, 1, []), (2, 1, 65, []), (2, 9, 65, [(1, 5), (5, 2)]), (2, 9, 1, [(1, 5)]), (2, 9, 1, [(5, 2)]),
                (2, 1025, 65, [(1023, 1024), (3, 7)]), (2, 1025, 1, [(1023, 1024)]), (2, 2049, 65, [(1023, 1024), (1500, 100)]),
                (2, 2049, 1, [(1500, 100)])]
COLSUM_C = [1, 63, 64, 65, 130]
COLSUM_P = [1, 3, 511, 512, 513, 1030]
WGRAD_SKINNY = [(1, 5, 256, 3), (2, 1027, 260, 1), (3, 700, 516, 4), (1, 4099, 512, 3)]
WGRAD_RELU_FROM = [(2, 300, 132, 260, 100), (1, 520, 512, 512, 8), (2, 130, 64, 64, 64)]


# ---------------------------------------------------------------------------------------------
# argmax_points, colsum_batched
# ---------------------------------------------------------------------------------------------
AM_SCALES = [1.0, -2.0, 0.5, 0.0, -0.25, 4.0]


def case_argmax(B, P, C, pairs, seed=0, last=False):
    """y integer-valued in [-62, 62] with ONE +63 and ONE -63 per column (unique extremes), scale +- a power of two or 0 and shift a
    small integer per (entry, column): fmaf(y, scale, shift) is exact, so ties are the planted ones -- column c of entry b gets the
    pair pairs[(c + b) % (len(pairs) + 1)] (none for the last index) at +-64 on the side its scale's sign makes the maximum -- and the
    all-equal columns of scale 0 (-> 0).  last = True builds the control: the LAST index of the maximum."""
    g = np.random.default_rng(4000 + seed)
    y = g.integers(-62, 63, (B, P, C)).astype(np.float64)
    scale = np.array([[AM_SCALES[(c + 2 * b) % len(AM_SCALES)] for c in range(C)] for b in range(B)])
    shift = g.integers(-3, 4, (B, C)).astype(np.float64)
    planted = np.zeros((B, C), dtype=bool)
    for b in range(B):
        for c in range(C):
            k = (c + b) % (len(pairs) + 1)
            pair = pairs[k] if k < len(pairs) else ()
            if P >= 4 + len(pair):
                free = [p for p in g.permutation(P)[:4 + len(pair)] if p not in pair]
                y[b, free[0], c], y[b, free[1], c] = 63.0, -63.0
            for p in pair:
                y[b, p, c] = 64.0 if scale[b, c] >= 0 else -64.0
            planted[b, c] = len(pair) > 0 and scale[b, c] != 0
    v = y * scale[:, None, :] + shift[:, None, :]
    want = (P - 1 - np.argmax(v[:, ::-1], axis=1)) if last else np.argmax(v, axis=1)
    return SimpleNamespace(y=f32(y), scale=f32(scale), shift=f32(shift), v=torch.from_numpy(v), planted=planted,
                           want=torch.from_numpy(want.astype(np.int32)))


def case_colsum(B, P, C, seed=0, drop_row=None):
    a = rnd(5000 + seed, B, P, C)
    keep = [p for p in range(P) if p != drop_row]
    return SimpleNamespace(a=a, want=a.double()[:, keep].sum(dim=1))


# ---------------------------------------------------------------------------------------------
# conv1x1_wgrad: the skinny route and in_relu_from
# ---------------------------------------------------------------------------------------------
def case_wgrad_skinny(B, P, Cin, Cout, seed=0, drop_row=None):
    """dy four columns wide with zeros past Cout, as the callers pass it."""
    x, dy = rnd(6000 + seed, B, P, Cin), rnd(6100 + seed, B, P, 4)
    dy[:, :, Cout:] = 0.0
    rows = [r for r in range(B * P) if r != drop_row]
    want = torch.einsum("ro,ri->oi", dy.double().reshape(B * P, 4)[rows][:, :Cout], x.double().reshape(B * P, Cin)[rows])
    return SimpleNamespace(x=x, dy=dy, dw0=rnd(6200 + seed, Cout, Cin), want=want)


def case_wgrad_relu_from(B, P, Cin, Cout, relu_from, seed=0, ref_from=None):
    """dW = dy^T in(x), in(x) = x scale + shift with the channels >= relu_from rectified; ref_from builds the control."""
    x, dy = rnd(6300 + seed, B, P, Cin), rnd(6400 + seed, B, P, Cout)
    sc, sh = rnd(6500 + seed, B, Cin).abs() + 0.5, rnd(6600 + seed, B, Cin)
    xin = x.double() * sc.double().unsqueeze(1) + sh.double().unsqueeze(1)
    k = relu_from if ref_from is None else ref_from
    xin = torch.cat([xin[..., :k], F.relu(xin[..., k:])], dim=-1)
    return SimpleNamespace(x=x, dy=dy, scale=sc, shift=sh, relu_from=relu_from,
                           want=dict(dW=torch.einsum("bpo,bpi->oi", dy.double(), xin), db=dy.double().sum(dim=(0, 1))))


# ---------------------------------------------------------------------------------------------
# the value-only CNF layers
# ---------------------------------------------------------------------------------------------
CNF_GRID = sorted({(C, n) for C in (4, 132, 256, 260, 512) for n in (3, 257)} | {(C, n) for C in (132, 512) for n in (1, 3, 33, 255, 256, 257, 300)})
CNF_OUT_N = [1, 255, 257, 600]


def value_splits(n):
    """Point splits of the backward kernels (caspr_cnf_value_splits)."""
    return 8 if n >= 256 else 1


def _hyper(seed, frames, C):
    return torch.sigmoid(rnd(seed, frames, C, scale=1.5)), rnd(seed + 1, frames, C, scale=0.3)


def _leaves(*ts):
    return [t.detach().double().requires_grad_(True) for t in ts]


def case_cnf_in(frames, n, C, seed=0, gate_frame0=False):
    """H = gated_softplus(y W0^T, b, gate, beta) and the gradients of sum(H dh) w.r.t. y, W0, gate, beta."""
    R = frames * n
    y, w0, b = rnd(7000 + seed, R, 3), rnd(7001 + seed, C, 3, scale=0.8), rnd(7002 + seed, C, scale=0.3)
    gate, beta = _hyper(7003 + seed, frames, C)
    dh = rnd(7005 + seed, R, C)
    y6, w6, b6, g6, be6 = _leaves(y, w0, b, gate, beta)
    h = gated_softplus(y6 @ w6.t(), b6, g6[:1].expand(frames, C) if gate_frame0 else g6, be6, n)
    (h * dh.double()).sum().backward()
    return SimpleNamespace(y=y, w0=w0, b=b, gate=gate, beta=beta, dh=dh, n=n, R=R, C=C,
                           want=dict(h=h.detach(), dy=y6.grad, dW0=w6.grad, dgate=g6.grad, dbeta=be6.grad))


def case_cnf_act(frames, n, C, seed=0):
    """The hidden activation on a given product z, with beta scaled by 40 on a quarter of the channels (the softplus / sigmoid tails):
    from dh, and -- the layer in front of the output layer -- from dzo (R, 3) and wo (3, C), by autograd through h wo^T."""
    R = frames * n
    z, b = rnd(7100 + seed, R, C), rnd(7101 + seed, C, scale=0.3)
    gate, beta = _hyper(7102 + seed, frames, C)
    beta[:, :max(C // 4, 1)] *= 40.0
    dh, dzo, wo = rnd(7104 + seed, R, C), rnd(7105 + seed, R, 3), rnd(7106 + seed, 3, C, scale=1.0 / np.sqrt(C))
    want = {}
    for key in ("dh", "dzo"):
        z6, b6, g6, be6 = _leaves(z, b, gate, beta)
        h = gated_softplus(z6, b6, g6, be6, n)
        ((h * dh.double()).sum() if key == "dh" else ((h @ wo.double().t()) * dzo.double()).sum()).backward()
        want[key] = dict(dZ=z6.grad, dgate=g6.grad, dbeta=be6.grad)
    want["h"] = h.detach()
    return SimpleNamespace(z=z, b=b, gate=gate, beta=beta, dh=dh, dzo=dzo, wo=wo, n=n, R=R, C=C, want=want)


def cnf_dgate_formula(case, with_b=True, drop_point=None):
    """dgate / dbeta of case_cnf_act from dh in closed form (f64), for the controls: da = dh sigmoid(a), dgate[f] = sum da (z + b)."""
    z6, dh6 = case.z.double(), case.dh.double()
    frames = case.R // case.n
    zb = z6 + case.b.double()
    da = dh6 * torch.sigmoid(zb * case.gate.double().repeat_interleave(case.n, 0) + case.beta.double().repeat_interleave(case.n, 0))
    t = (da * (zb if with_b else z6)).reshape(frames, case.n, case.C)
    keep = [p for p in range(case.n) if p != drop_point]
    return dict(dgate=t[:, keep].sum(1), dbeta=da.reshape(frames, case.n, case.C)[:, keep].sum(1))


def case_cnf_out(frames, n, seed=0):
    """a = (zo + b) gate[f] + beta[f] on three channels and the gradients of sum(a da) w.r.t. zo, gate, beta."""
    R = frames * n
    zo, b, da = rnd(7200 + seed, R, 3), rnd(7201 + seed, 3, scale=0.3), rnd(7204 + seed, R, 3)
    gate, beta = _hyper(7202 + seed, frames, 3)
    z6, b6, g6, be6 = _leaves(zo, b, gate, beta)
    a = (z6 + b6) * g6.repeat_interleave(n, 0) + be6.repeat_interleave(n, 0)
    (a * da.double()).sum().backward()
    return SimpleNamespace(zo=zo, b=b, gate=gate, beta=beta, da=da, n=n, R=R,
                           want=dict(a=a.detach(), dzo=z6.grad, dgate=g6.grad, dbeta=be6.grad))
