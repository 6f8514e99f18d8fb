"""Case builders and plain references for the edge tests of the index chain: farthest point sampling (fps_kernel<PPT>, fps_big_kernel,
stage_cloud) and the ball queries (ball_query_kernel, ball_query_lds_kernel, ball_query2_lds_kernel and the pair's two-launch
fallback) of caspr_amd/csrc/point_ops.hip.  test_index_ops_cases.py checks the cases on the CPU (they must tell a right kernel from a
subtly wrong one), test_index_ops_edges.py runs the kernels on them.  Everything is an integer row compared bit for bit: there is no
tolerance in this file.

A case is a function of its parameters and a seed and returns a namespace with the inputs and the expected index rows.  References:
  * oracle.point_ops (the contract) for everything;
  * fps_rule: the total order of the arg-max (value descending, bit-reversed k mod block_size ascending, k ascending) restated in
    vectorised numpy, with the block size as a PARAMETER so that the controls can pass a wrong one (block_size = 1 is "the first k
    wins", numpy.argmax on the running minimum);
  * _fps_block_literal of test_oracle_golden.py, the upstream block algorithm thread by thread, where n * M <= LITERAL_MAX;
  * ball_rule / planted_row: the ball query in three lines of Python, with the comparison as a parameter.
fps_rule, _fps_block_literal and ball_rule evaluate a*a + b*b + c*c as written; they are references only on clouds where every f32
operation is exact (lattice(), planted()), which is where they are used.  No GPU code is imported.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from oracle import point_ops as P
from caspr_amd.utils.synthetic import car_sequences
from test_oracle_golden import _fps_block_literal  # noqa: F401  (re-exported: the controls call it through this module)

B = 3                       # clouds per FPS / route case: clouds 1 and 2 start b * 12 n bytes into the buffer
LITERAL_MAX = 50000         # _fps_block_literal is a Python loop over n * M (point, round) pairs
SENTINEL = -7               # what the GPU tests fill index buffers with; no case may expect it
TAIL = 64                   # sentinel elements behind every output payload


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


# ---------------------------------------------------------------------------------------------
# clouds
# ---------------------------------------------------------------------------------------------
def lattice(B, n, seed, levels=6):
    """integer in [0, levels) / 4 + (1.0, 0.5, 2.0): dyadic rationals.  Every f32 operation on them is exact, fused and unfused forms
    agree, and nearly every FPS round is an exact tie (levels^3 sites)."""
    g = np.random.default_rng(seed)
    return f32(g.integers(0, levels, (B, n, 3)) / 4.0 + np.array([1.0, 0.5, 2.0]))


def cars(B, n, seed, dup=False):
    """test_hip_parity.clouds: the model's kind of cloud, generic floats; dup repeats the leading points behind n / 2 (exact ties)."""
    x, _ = car_sequences(B, 1, n, seed=100 + seed)
    c = x[:, 0, :, :3].contiguous()
    if dup:
        c[:, n // 2:] = c[:, : n - n // 2]
    return c


def lone_point(n):
    """The point "all_but_one" leaves: past the first wave and, where the cloud has one, past the first 256-point stride."""
    return (2 * n) // 3 if n > 2 else n - 1


def guarded(cloud, which):
    """A copy with chosen points at exactly 0 (|p|^2 = 0 <= 1e-3: under the origin guard whatever the arithmetic; the threshold itself
    depends on the oracle's assumed contraction and is not probed).  "some": every 7th point, point 0 among them -- except in cloud 1,
    which keeps its point 0: a cloud that STARTS at the origin never selects another origin point with the guard off either (they are
    at distance 0 from the start), so only a cloud that starts elsewhere tells a guard that is ignored from one that works;
    "all_but_one": all but lone_point(n); "all"."""
    c = cloud.clone()
    n = c.shape[1]
    if which == "some":
        c[:, 0::7] = 0.0
        if c.shape[0] > 1:
            c[1, 0] = cloud[1, 0]
    elif which == "all_but_one":
        keep = c[:, lone_point(n)].clone()
        c[:] = 0.0
        c[:, lone_point(n)] = keep
    elif which == "all":
        c[:] = 0.0
    else:
        raise ValueError(which)
    return c


def tie_pair(cloud, a, b, level=7):
    """A copy with points a and b on one site of their own, the corner just outside the lattice (still dyadic): once that corner is the
    farthest site the round is a tie between exactly these two."""
    c = cloud.clone()
    c[:, a] = c[:, b] = f32(level / 4.0 + np.array([1.0, 0.5, 2.0]))
    return c


def planted(n, hits, centre):
    """(n, 3): point k at (100 + k, 0, 0), the points of `hits` within 0.05 of `centre` instead (distinct, on a dyadic grid of step
    1/128: |offset| <= (3/128) sqrt(3) = 0.041).  Queried with PLANTED_RADIUS nothing is near the sphere: hits are >= 0.059 inside,
    every other point >= 90 outside."""
    p = np.zeros((n, 3), np.float64)
    p[:, 0] = 100.0 + np.arange(n)
    for k in hits:
        p[k] = np.asarray(centre, np.float64) + (np.array([k % 7, (k // 7) % 7, (k // 49) % 7]) - 3) / 128.0
    return f32(p)


def planted_row(hits, ns):
    """The expected row, independent of the oracle: the first ns hits in ascending order, padded with the first; zeros without a hit."""
    h = sorted(hits)[:ns]
    return (h + [h[0]] * (ns - len(h))) if h else [0] * ns


# ---------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------
def fps_block_size(n):
    bs = 1
    while bs * 2 <= n and bs * 2 <= 512:
        bs *= 2
    return bs


def tie_order(n, block_size):
    """The points 0..n-1 in the priority order of the tie key: bit-reversed k mod block_size ascending, then k ascending."""
    k = np.arange(n)
    bits = int(block_size).bit_length() - 1
    assert 1 << bits == block_size
    return np.lexsort((k, bitrev(k % block_size, bits)))


def bitrev(t, bits):
    r = np.zeros_like(t)
    for i in range(bits):
        r |= ((t >> i) & 1) << (bits - 1 - i)
    return r


def _sq(d):
    """a*a + b*b + c*c in f32, left to right (exact on the clouds this is used on)."""
    d = d.astype(np.float32)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def fps_rule(points, M, block_size, guard):
    """One cloud (n, 3) -> list of M indices.  Round j selects, among the admissible points, the one whose running minimum distance is
    largest; among equal ones the smallest bit-reversed (k mod block_size), then the smallest k; index 0 when no point is admissible.
    block_size = 1: the first k that holds the maximum."""
    p = np.asarray(points, np.float32)
    n = p.shape[0]
    order = tie_order(n, block_size)
    ok = ~(_sq(p) <= np.float32(1e-3)) if guard else np.ones(n, bool)
    temp = np.full(n, 1e10, np.float32)
    out, old = [0], 0
    for _ in range(1, M):
        temp = np.minimum(temp, _sq(p - p[old]))
        cand = np.where(ok, temp, np.float32(-1.0))[order]
        j = int(np.argmax(cand))                                     # the first maximum in priority order
        old = int(order[j]) if cand[j] >= 0 else 0
        out.append(old)
    return out


def ball_rule(points, centres, radius, ns, closed=False):
    """(n, 3), (M, 3) -> (M, ns) rows by the three-line rule; closed=True is the WRONG comparison d2 <= r2 (a control)."""
    p, c = np.asarray(points, np.float32), np.asarray(centres, np.float32)
    r2 = np.float32(radius) * np.float32(radius)
    rows = []
    for m in range(c.shape[0]):
        d2 = _sq(c[m] - p)
        rows.append(planted_row(np.nonzero(d2 <= r2 if closed else d2 < r2)[0].tolist(), ns))
    return np.asarray(rows, np.int32).reshape(c.shape[0], ns)


def gather_rows(cloud, idx):
    """(B, n, 3), (B, M) -> (B, M, 3): the centres FPS hands on."""
    return torch.gather(cloud, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()


# ---------------------------------------------------------------------------------------------
# FPS
# ---------------------------------------------------------------------------------------------
# n -> what it is there for (fps_kernel<PPT> holds PPT = 1, 2, 4, 8, 16 points per thread in 256 threads; bs = the upstream block
# size min(512, largest power of two <= n) that the tie key reverses k over)
FPS_N = {
    1: "fps_kernel<1>, bs = 1: no tie key, a single point",
    2: "fps_kernel<1>, bs = 2",
    3: "fps_kernel<1>, bs = 2 with a second point on thread 0's upstream stride",
    63: "fps_kernel<1>, bs = 32: one wave partially filled",
    64: "fps_kernel<1>, bs = 64: exactly one wave",
    65: "fps_kernel<1>, bs = 64: one point in the second wave",
    255: "fps_kernel<1>, bs = 128: one thread short of the workgroup",
    256: "fps_kernel<1> full, bs = 256",
    257: "fps_kernel<2>, bs = 256: PPT >= 2 with the NON-permuted slot order, one point in the second slot",
    300: "fps_kernel<2>, bs = 256, non-permuted, second slot partially filled",
    511: "fps_kernel<2>, bs = 256, non-permuted, one point short of full",
    512: "fps_kernel<2> full, bs = 512: the even / odd slot permutation",
    513: "fps_kernel<4>, bs = 512: two of four slots empty but for one point",
    1023: "fps_kernel<4>, one point short of full",
    1024: "fps_kernel<4> full",
    1025: "fps_kernel<8>, one point past half of its slots' first",
    2047: "fps_kernel<8>, one point short of full",
    2049: "fps_kernel<16>, one point in slot 8",
    4095: "fps_kernel<16>, one point short of full",
    4096: "fps_kernel<16> full: the largest cloud held in registers",
    4097: "fps_big_kernel, its first cloud: 22-bit key, one point on the fifth trip of the strided loop",
    4099: "fps_big_kernel, n % 4 = 3",
    8193: "fps_big_kernel, one point past 8 trips of 1024 threads",
}
FPS_EXTRA_M = (3, 65, 300, 513)             # M = 1 and M = n + 5 in addition
FPS_ALL_SELECTED_MAX_N = 300                # M = n: every point selected, then all-zero ties
FPS_DUP_N = (65, 300, 1025, 4099)           # car clouds with duplicate padding
# the "some" pattern: one n per instantiation (PPT = 2 in both slot orders) and fps_big_kernel's `continue`
FPS_GUARD_SOME_N = {65: "fps_kernel<1>", 300: "fps_kernel<2> bs 256", 512: "fps_kernel<2> bs 512", 513: "fps_kernel<4>",
                    1025: "fps_kernel<8>", 2049: "fps_kernel<16>", 4097: "fps_big_kernel"}
FPS_GUARD_ALL_N = (65, 300, 4097)           # "all" and "all_but_one"
# One point past a power of two the tie orders of block size bs and bs / 2 differ in ONE pair: with k < bs the reversal over log2(bs) bits
# is twice the reversal of k mod bs/2 over one bit less, plus the bit that tells k from k + bs/2 -- the same order; k = bs comes right
# behind k = 0 under bs and behind k = bs/2 under bs/2.  A random lattice hardly ever ties exactly these two: the lattice clouds of these
# sizes carry the tie (tie_pair), so that the wrong block size gives another row.  (Up to n = bs the two orders are the same permutation.)
FPS_TIE_PAIR = {257: (128, 256), 513: (256, 512)}
FPS_ALIGN = (256, 1024, 4100)               # cloud buffer 4 bytes past a 16-byte boundary: stage_cloud's scalar branch with count % 4 == 0


def fps_ms(n):
    ms = [min(n, 96)]
    if n in FPS_EXTRA_M:
        ms += [1, n + 5]
    if n <= FPS_ALL_SELECTED_MAX_N:
        ms.append(n)
    return sorted(set(ms))


def fps_table(n):
    """-> [(n, M, kind, guard, pattern)] of one cloud size."""
    rows = []
    for kind in ("lattice", "cars"):
        for guard in (0, 1):
            rows += [(n, M, kind, guard, None) for M in fps_ms(n)]
            if n in FPS_GUARD_SOME_N:
                rows.append((n, min(n, 96), kind, guard, "some"))
            if n in FPS_GUARD_ALL_N:
                rows += [(n, min(n, 96), kind, guard, w) for w in ("all_but_one", "all")]
    return rows


def fps_tag(n, M, kind, guard, pattern):
    return "n%d_M%d_%s_g%d%s" % (n, M, kind, guard, "_" + pattern if pattern else "")


@functools.lru_cache(maxsize=None)
def fps_cloud(n, kind, pattern, batch=B):
    c = lattice(batch, n, seed=n) if kind == "lattice" else cars(batch, n, seed=n, dup=n in FPS_DUP_N)
    if kind == "lattice" and n in FPS_TIE_PAIR:
        c = tie_pair(c, *FPS_TIE_PAIR[n])
    return guarded(c, pattern) if pattern else c


@functools.lru_cache(maxsize=None)
def fps_case(n, M, kind, guard, pattern=None):
    """The cloud is shared between the cases of one (n, kind, pattern): do not write to it."""
    cloud = fps_cloud(n, kind, pattern)
    want = P.furthest_point_sampling(cloud, M, guard=bool(guard))
    return SimpleNamespace(tag=fps_tag(n, M, kind, guard, pattern), n=n, M=M, kind=kind, guard=guard, pattern=pattern,
                           cloud=cloud, want=want, want_xyz=gather_rows(cloud, want), bs=fps_block_size(n))


# ---------------------------------------------------------------------------------------------
# ball query: the route rule
# ---------------------------------------------------------------------------------------------
BQ_LDS_MAX_N, BQ_LDS_MIN_M, BQ_LDS_MIN_N = 12288, 64, 256


def lds_route(n, M):
    """The host rule of caspr_ball_query_f32 / caspr_ball_query2_f32 restated (B <= 65535 always holds here)."""
    return n <= BQ_LDS_MAX_N and M >= BQ_LDS_MIN_M and n >= BQ_LDS_MIN_N


# (n, M, the route the shape is MEANT to take, what it is there for)
BALL_ROUTE = [
    (255, 64, "plain", "one point below the LDS route's smallest cloud"),
    (256, 64, "lds", "the smallest shape of the LDS route: 4 waves x 16 centres, one workgroup"),
    (256, 63, "plain", "one centre below the LDS route's smallest M"),
    (257, 65, "lds", "one centre in the second workgroup's share; n % 4 = 1: scalar staging, ragged last chunk of one point"),
    (1, 1, "plain", "a single point, a single centre"),
    (63, 5, "plain", "n < 64: one partial chunk; 5 centres: a partially filled workgroup"),
    (64, 64, "plain", "n = 64: exactly one chunk"),
    (65, 64, "plain", "n = 65: a second chunk of one point"),
    (12288, 64, "lds", "the largest cloud the LDS route takes (144 KiB, opted in)"),
    (12289, 64, "plain", "the first cloud it leaves to the plain kernel"),
]
BALL_ROUTE_NS = (1, 16, 65)
BALL_ROUTE_NS_B = {1: 16, 16: 65, 65: 1}    # the pair's second scale: a different ns
BALL_ROUTE_RB = (0.5, 1.0, 2.0)             # ... with a radius below, equal to and above the first (factors)


def route_radius(n):
    """The radius test_hip_parity.py queries clouds of this size with."""
    return 0.8 if n <= 65 else 0.4 if n <= 512 else 0.02


@functools.lru_cache(maxsize=None)
def route_inputs(n, M):
    cloud = cars(B, n, seed=n)
    return cloud, gather_rows(cloud, P.furthest_point_sampling(cloud, M))


@functools.lru_cache(maxsize=None)
def route_want(n, M, radius, ns):
    cloud, centres = route_inputs(n, M)
    return P.ball_query(radius, ns, cloud, centres)


# ---------------------------------------------------------------------------------------------
# ball query: points exactly on the sphere
# ---------------------------------------------------------------------------------------------
BALL_BOUNDARY_N = (300, 1000)
BALL_BOUNDARY_M = (5, 70)                   # the plain and the LDS route (the 5 centres repeated)
BOUNDARY_RADIUS, BOUNDARY_NS = 0.5, 200     # d2 == 0.25: two lattice steps along one axis
BOUNDARY_RADIUS_B = 0.75                    # the pair's second scale: d2 == 0.5625, three steps along one axis


@functools.lru_cache(maxsize=None)
def boundary_case(n, M):
    cloud = lattice(1, n, seed=7)
    own = np.random.default_rng(n).choice(n, 5, replace=False)
    centres = cloud[:, np.resize(own, M)].contiguous()
    p, c = cloud[0].numpy(), cloud[0].numpy()[own]
    on, on_b, inside = [], [], []
    for m in range(5):
        d2 = _sq(c[m] - p)
        on.append(int((d2 == np.float32(0.25)).sum()))
        on_b.append(int((d2 == np.float32(0.5625)).sum()))
        inside.append(int((d2 < np.float32(0.25)).sum()))
    assert min(on) >= 1 and min(on_b) >= 1, "a centre without a point exactly on the sphere: %s %s" % (on, on_b)
    assert max(inside) + max(on) < BOUNDARY_NS, "the row is full before the sphere matters"
    return SimpleNamespace(tag="n%d_M%d" % (n, M), n=n, M=M, cloud=cloud, centres=centres, on=on, inside=inside,
                           want=P.ball_query(BOUNDARY_RADIUS, BOUNDARY_NS, cloud, centres),
                           want_b=P.ball_query(BOUNDARY_RADIUS_B, BOUNDARY_NS, cloud, centres))


# ---------------------------------------------------------------------------------------------
# ball query: planted hits
# ---------------------------------------------------------------------------------------------
BALL_PLANTED_N = (64, 200, 1000)
BALL_PLANTED_M = (5, 70)                    # n = 1000: the plain and the LDS route; n < 256 stays on the plain kernel
PLANTED_CENTRE = (0.5, -0.25, 2.0)
PLANTED_RADIUS, PLANTED_RADIUS_B = 0.1, 0.25
PLANTED_B = 2                               # the same cloud twice: cloud 1 starts b * 12 n bytes in


def planted_table(n):
    """-> [(name, hits, ns, what it is there for)] for a cloud of n points (entries that need more points are left out)."""
    one = 64 if n > 64 else 0               # a chunk that is not the first, where there is one
    rows = [("none", [], 16, "no hit: all zeros"),
            ("last", [n - 1], 16, "the only hit at k = n - 1, in the ragged last chunk"),
            ("last_ns130", [n - 1], 130, "... with a pad of three strides"),
            ("first", [0], 16, "the only hit at k = 0")]
    rows += [("chunk64_ns%d" % ns, list(range(one, one + 64)), ns, "64 hits inside one chunk, truncated inside a ballot / exact / padded")
             for ns in (1, 2, 63, 64, 65)]
    rows += [("lane63", [63], 2, "the last lane of a chunk"), ("lane64", [64], 2, "the first lane of the next"),
             ("lane63_64", [63, 64], 2, "the ns-th hit on the first lane of the next chunk"),
             ("end127", list(range(123, 128)), 5, "exactly ns hits, the last on the last lane of a chunk"),
             ("end128", list(range(124, 129)), 5, "exactly ns hits, the last on the first lane of the next chunk"),
             ("hits130_ns130", list(range(30, 160)), 130, "130 hits over three chunks, no pad"),
             ("hits130_ns200", list(range(30, 160)), 200, "130 hits, the pad loop takes two strides")]
    return [r for r in rows if not r[1] or max(r[1]) < n]


@functools.lru_cache(maxsize=None)
def planted_case(n, M, name):
    (hits, ns), = [(r[1], r[2]) for r in planted_table(n) if r[0] == name]
    cloud = planted(n, hits, PLANTED_CENTRE).unsqueeze(0).repeat(PLANTED_B, 1, 1).contiguous()
    centres = f32(PLANTED_CENTRE).view(1, 1, 3).repeat(PLANTED_B, M, 1).contiguous()
    ns_b = ns + 1
    row = lambda k: torch.tensor(planted_row(hits, k), dtype=torch.int32).view(1, 1, k).repeat(PLANTED_B, M, 1).contiguous()  # noqa: E731
    return SimpleNamespace(tag="n%d_M%d_%s" % (n, M, name), n=n, M=M, hits=hits, ns=ns, ns_b=ns_b, cloud=cloud, centres=centres,
                           want=row(ns), want_b=row(ns_b))
