"""The cases of index_ops_cases.py, checked on the CPU: the expected rows are what three independent statements of the operators give
(oracle/point_ops.c, the vectorised total order, the upstream block algorithm taken literally; the ball query in three lines), and
every case that is there to pin a rule gives a DIFFERENT row under the nearest wrong rule -- so that a kernel that implements the
wrong rule cannot pass test_index_ops_edges.py.  A case that fails one of these conditions is a defect of the case.  No GPU."""
import numpy as np
import pytest
import torch

import index_ops_cases as X
from oracle import point_ops as P

LATTICE = [t for n in X.FPS_N for t in X.fps_table(n) if t[2] == "lattice"]


def _ids(rows):
    return [X.fps_tag(*r) for r in rows]


def test_tables_cover_what_they_name():
    """Every instantiation and block size in the table; the sentinel is no possible index."""
    ppt = {n: (0 if n > 4096 else next(p for p in (1, 2, 4, 8, 16) if -(-n // 256) <= p)) for n in X.FPS_N}
    assert set(ppt.values()) == {0, 1, 2, 4, 8, 16}
    assert {n for n in X.FPS_N if ppt[n] == 2 and X.fps_block_size(n) == 256} == {257, 300, 511}      # PPT >= 2, non-permuted slots
    assert {ppt[n] for n in X.FPS_GUARD_SOME_N} == {0, 1, 2, 4, 8, 16}
    assert {X.fps_block_size(n) for n in X.FPS_GUARD_SOME_N if ppt[n] == 2} == {256, 512}
    assert all(n % 4 == 0 for n in X.FPS_ALIGN)                      # count % 4 == 0: only the pointer sends stage_cloud to its scalar branch
    for n, M, route, _ in X.BALL_ROUTE:
        assert ("lds" if X.lds_route(n, M) else "plain") == route, (n, M)
    assert {r for _, _, r, _ in X.BALL_ROUTE} == {"lds", "plain"}
    assert X.SENTINEL < 0
    assert len(set(_ids(LATTICE))) == len(LATTICE)


@pytest.mark.parametrize("n", list(X.FPS_N))
def test_fps_oracle_is_the_total_order_and_the_block_algorithm(n):
    """The oracle equals fps_rule with the right block size on every lattice case, guard off and on (clouds under a guard pattern
    included), and the literal block algorithm (which always guards: lattice points are never under the threshold, so it stands for
    both settings on a plain cloud and for guard = 1 on a pattern) where n * M <= LITERAL_MAX."""
    for row in X.fps_table(n):
        if row[2] != "lattice":
            continue
        c = X.fps_case(*row)
        assert c.want.shape == (X.B, c.M) and int(c.want.min()) >= 0 and int(c.want.max()) < n
        for b in range(X.B):
            assert X.fps_rule(c.cloud[b].numpy(), c.M, c.bs, c.guard) == c.want[b].tolist(), "%s cloud %d" % (c.tag, b)
        if not c.guard and not c.pattern:
            assert torch.equal(c.want, X.fps_case(n, c.M, "lattice", 1, None).want), c.tag   # ... whose row the literal form checks
        elif c.guard and n * c.M <= X.LITERAL_MAX:
            assert X._fps_block_literal(c.cloud[0].numpy(), c.M) == c.want[0].tolist(), c.tag


def _decides(c):
    """Cases whose row a tie rule can change: more than one round, and more than one admissible point."""
    return c.M > 1 and c.pattern in (None, "some")


@pytest.mark.parametrize("n", [n for n in X.FPS_N if n >= 63])
def test_fps_cases_reject_first_k_wins(n):
    """numpy.argmax on the running minimum (fps_rule with block size 1) gives a different row for every cloud of every lattice case."""
    seen = 0
    for row in X.fps_table(n):
        c = X.fps_case(*row)
        if c.kind != "lattice" or not _decides(c):
            continue
        for b in range(X.B):
            wrong = X.fps_rule(c.cloud[b].numpy(), c.M, 1, c.guard)
            assert wrong != c.want[b].tolist(), "%s cloud %d: the first-k rule gives the same row" % (c.tag, b)
        seen += 1
    assert seen >= 2


@pytest.mark.parametrize("n", [n for n in X.FPS_N if n >= 257])
def test_fps_cases_reject_every_wrong_block_size(n):
    """Every wrong block size in {64, 128, 256, 512} that is <= n gives a different row for every cloud of every lattice case.  (i = s
    in place of the even / odd slot permutation of fps_kernel is the order of block size 256 inside a thread.)"""
    seen = 0
    for row in X.fps_table(n):
        c = X.fps_case(*row)
        if c.kind != "lattice" or not _decides(c):
            continue
        for bs in (64, 128, 256, 512):
            if bs > n or bs == c.bs:
                continue
            if np.array_equal(X.tie_order(n, bs), X.tie_order(n, c.bs)):
                # the SAME total order over 0..n-1 (index_ops_cases.FPS_TIE_PAIR: bs / 2 up to n = bs): there is no wrong row to give, and
                # no kernel can be wrong in this way.  The only such pair of the table:
                assert (n, bs) == (512, 256)
                continue
            for b in range(X.B):
                wrong = X.fps_rule(c.cloud[b].numpy(), c.M, bs, c.guard)
                assert wrong != c.want[b].tolist(), "%s cloud %d: block size %d gives the same row" % (c.tag, b, bs)
        seen += 1
    assert seen >= 2


@pytest.mark.parametrize("n", X.FPS_GUARD_ALL_N)
@pytest.mark.parametrize("kind", ["lattice", "cars"])
def test_fps_guard_controls(n, kind):
    """Guarded entirely: no admissible point, every round returns the identity index 0.  All but one: index 0, then the one admissible
    point for every later entry.  "some": no guarded point is ever selected after the start index, with the guard on."""
    M = min(n, 96)
    assert not X.fps_case(n, M, kind, 1, "all").want.any()
    want = X.fps_case(n, M, kind, 1, "all_but_one").want
    assert (want[:, 0] == 0).all() and (want[:, 1:] == X.lone_point(n)).all() and X.lone_point(n) not in (0, n)
    if n in X.FPS_GUARD_SOME_N:
        c = X.fps_case(n, M, kind, 1, "some")
        assert float(c.cloud[0::2, 0].abs().max()) == 0.0 and float(c.cloud[1, 0].abs().min()) > 0.0
        sel = c.want[:, 1:]
        assert (sel[0::2] % 7 != 0).all() and ((sel[1] % 7 != 0) | (sel[1] == 0)).all()      # (cloud 1's own point 0 may come back in a tie)
        off = X.fps_case(n, M, kind, 0, "some").want
        # (a cloud that starts at the origin keeps the other origin points at distance 0 with the guard off too: guarded())
        assert not torch.equal(off[1], c.want[1]) and off[1, 1] % 7 == 0      # ... one that starts elsewhere selects an origin point at once


@pytest.mark.parametrize("n", X.BALL_BOUNDARY_N)
def test_ball_boundary_cases_reject_the_closed_ball(n):
    """Every centre has points at d2 == r2 exactly (the builder asserts it); the oracle excludes them, `<=` in place of `<` changes every
    row, for either radius of the pair."""
    for M in X.BALL_BOUNDARY_M:
        c = X.boundary_case(n, M)
        p, ctr = c.cloud[0].numpy(), c.centres[0].numpy()
        for want, r in ((c.want, X.BOUNDARY_RADIUS), (c.want_b, X.BOUNDARY_RADIUS_B)):
            assert np.array_equal(X.ball_rule(p, ctr, r, X.BOUNDARY_NS), want[0].numpy())
            closed = X.ball_rule(p, ctr, r, X.BOUNDARY_NS, closed=True)
            assert (closed != want[0].numpy()).any(axis=1).all(), "a row that `<=` does not change"
        assert min(c.on) >= 1 and max(c.inside) < X.BOUNDARY_NS
    c = X.boundary_case(300, 5)
    assert (c.on, c.inside) == ([5, 6, 10, 4, 5], [16, 27, 13, 27, 38])       # as counted when the case was written


@pytest.mark.parametrize("n", X.BALL_PLANTED_N)
def test_ball_planted_expectation_is_the_oracle(n):
    """The three-line expectation equals the oracle for both scales of the pair, and each entry is what its name says."""
    names = [r[0] for r in X.planted_table(n)]
    assert len(set(names)) == len(names) and {"none", "last", "first", "chunk64_ns63", "chunk64_ns65"} <= set(names)
    if n > 160:
        assert {"lane63", "lane64", "lane63_64", "end127", "end128", "hits130_ns130", "hits130_ns200"} <= set(names)
    for name in names:
        for M in X.BALL_PLANTED_M:
            c = X.planted_case(n, M, name)
            assert torch.equal(P.ball_query(X.PLANTED_RADIUS, c.ns, c.cloud, c.centres), c.want), c.tag
            assert torch.equal(P.ball_query(X.PLANTED_RADIUS_B, c.ns_b, c.cloud, c.centres), c.want_b), c.tag
            assert int(c.want.min()) >= 0
    # a `first` taken from the LAST hit of the first non-empty chunk changes every padded row with two hits in that chunk
    c = X.planted_case(n, 5, "chunk64_ns65")
    assert c.want[0, 0, -1] == c.hits[0] != c.hits[-1]


@pytest.mark.parametrize("n,M,route,why", X.BALL_ROUTE, ids=["n%d_M%d" % (r[0], r[1]) for r in X.BALL_ROUTE])
def test_ball_route_cases_exercise_truncation_and_padding(n, M, route, why):
    """Over the three ns of a shape the oracle rows hold both a full ball (truncated) and, where the cloud has more than one point, a
    padded one; the radii of the pair give different rows."""
    cloud, centres = X.route_inputs(n, M)
    assert centres.shape == (X.B, M, 3)
    r = X.route_radius(n)
    full = padded = False
    for f in X.BALL_ROUTE_RB:
        every = P.ball_query(r * f, n + 1, cloud, centres)                  # all hits, then the pad
        hits = (every[:, :, 1:] != every[:, :, :1]).sum(2) + 1              # (a centre is a point of its cloud: at least itself)
        for ns in X.BALL_ROUTE_NS:
            w = X.route_want(n, M, r * f, ns)
            assert w.shape == (X.B, M, ns) and int(w.min()) >= 0 and int(w.max()) < n
            full |= bool((hits > ns).any())
            padded |= bool((hits < ns).any())
    assert full == (n > 1) and padded
    if n > 1:
        assert not torch.equal(X.route_want(n, M, r * 0.5, 16), X.route_want(n, M, r * 2.0, 16))
