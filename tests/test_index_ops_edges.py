"""The index chain at the head of every forward pass -- farthest point sampling (fps_kernel<PPT> in its five instantiations,
fps_big_kernel), the ball queries (ball_query_kernel, ball_query_lds_kernel, ball_query2_lds_kernel, the pair's two-launch fallback)
and stage_cloud's two copies -- on the cases of index_ops_cases.py: every instantiation partially filled, full and one point past,
the origin guard on every route, clouds 4 bytes off 16, the host's route thresholds, points exactly on the sphere, hits planted on
the lanes and chunk edges where the ballot arithmetic can go wrong.  test_index_ops_cases.py shows on the CPU that these cases tell the
right rule from the nearest wrong ones.

Every call goes through the C entries (caspr_fps_f32, caspr_ball_query_f32, caspr_ball_query2_f32) with output buffers filled with
a sentinel and TAIL sentinel elements behind the payload: afterwards no payload slot holds the sentinel and the tail is untouched.
Everything is compared bit for bit; there is no tolerance in this file.  Results land in the parity report under edges:fps_* and
edges:ball_*.
"""
import pytest
import torch

import index_ops_cases as X
from oracle import point_ops as P
from test_hip_parity import REPORT, exact, record
from test_point_ops_edges import L, _p, _stream, _check, DEV  # noqa: F401  (L is a fixture)

pytestmark = pytest.mark.gpu

NAN = float("nan")


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _report(request):
    """exact() fills REPORT, record() also writes the report file: each test ends with one record() of its own total of mismatches."""
    before = set(REPORT)
    yield
    mine = [REPORT[k] for k in set(REPORT) - before]
    record("edges:index_mismatches_%s" % request.node.name, [sum(e["mismatches"] for e in mine)], [0], 0.0)


def _idx_buf(count):
    return torch.full((count + X.TAIL,), X.SENTINEL, dtype=torch.int32, device=DEV)


def _payload(name, buf, shape):
    """The payload of a sentinel buffer, after the checks every call gets: the tail untouched, no slot left unwritten."""
    count = 1
    for s in shape:
        count *= s
    tail, body = buf[count:].cpu(), buf[:count].cpu()
    if buf.dtype == torch.int32:
        assert bool((tail == X.SENTINEL).all()), "%s: a write past the end of the index rows" % name
        assert not bool((body == X.SENTINEL).any()), "%s: %d index slots left unwritten" % (name, int((body == X.SENTINEL).sum()))
    else:
        assert bool(torch.isnan(tail).all()), "%s: a write past the end of new_xyz" % name
        assert not bool(torch.isnan(body).any()), "%s: new_xyz slots left unwritten" % name
    return body.view(*shape)


def misaligned(t):
    """A copy of t on the device that starts 4 bytes past a 16-byte boundary (a slice of a flat tensor)."""
    flat = torch.zeros(t.numel() + 5, dtype=t.dtype, device=DEV)
    off = 1 + (-(flat.data_ptr() // 4) % 4)                   # (allocations are 16-byte aligned; stated, not assumed)
    out = flat[off:off + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def run_fps(L, cloud_dev, M, guard, with_xyz=True):
    """caspr_fps_f32 into sentinel buffers -> idx (B, M) int32, new_xyz (B, M, 3) | None, on the host."""
    Bc, n, _ = cloud_dev.shape
    idx = _idx_buf(Bc * M)
    xyz = torch.full((Bc * M * 3 + X.TAIL,), NAN, device=DEV) if with_xyz else None
    _check(L.caspr_fps_f32(_p(cloud_dev), Bc, n, M, int(guard), _p(idx), _p(xyz), _stream()), "caspr_fps_f32")
    torch.cuda.synchronize()
    return _payload("fps idx", idx, (Bc, M)), (_payload("fps new_xyz", xyz, (Bc, M, 3)) if with_xyz else None)


def run_ball(L, cloud_dev, centres_dev, radius, ns):
    Bc, n, _ = cloud_dev.shape
    M = centres_dev.shape[1]
    idx = _idx_buf(Bc * M * ns)
    _check(L.caspr_ball_query_f32(_p(cloud_dev), _p(centres_dev), Bc, n, M, float(radius), ns, _p(idx), _stream()), "caspr_ball_query_f32")
    torch.cuda.synchronize()
    return _payload("ball_query", idx, (Bc, M, ns))


def run_pair(L, cloud_dev, centres_dev, ra, nsa, rb, nsb):
    Bc, n, _ = cloud_dev.shape
    M = centres_dev.shape[1]
    ia, ib = _idx_buf(Bc * M * nsa), _idx_buf(Bc * M * nsb)
    _check(L.caspr_ball_query2_f32(_p(cloud_dev), _p(centres_dev), Bc, n, M, float(ra), nsa, _p(ia), float(rb), nsb, _p(ib), _stream()),
           "caspr_ball_query2_f32")
    torch.cuda.synchronize()
    return _payload("ball_query2 a", ia, (Bc, M, nsa)), _payload("ball_query2 b", ib, (Bc, M, nsb))


def check_fps(L, tag, cloud_dev, M, guard, want, want_xyz):
    got, gxyz = run_fps(L, cloud_dev, M, guard)
    exact("edges:fps_idx_%s" % tag, got, want)
    exact("edges:fps_newxyz_%s" % tag, gxyz.view(torch.int32), want_xyz.view(torch.int32))      # bits: -0.0 and 0.0 differ
    bare, _ = run_fps(L, cloud_dev, M, guard, with_xyz=False)
    exact("edges:fps_idx_nullxyz_%s" % tag, bare, got)
    again, axyz = run_fps(L, cloud_dev, M, guard)
    exact("edges:fps_repeat_%s" % tag, again, got)
    assert torch.equal(axyz.view(torch.int32), gxyz.view(torch.int32))
    return got


# ---------------------------------------------------------------------------------------------
# farthest point sampling
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(X.FPS_N))
def test_fps_instantiation_edges(L, n):
    """Every (M, cloud kind, guard, guard pattern) of one cloud size against the oracle: X.FPS_N says which kernel and which edge of it
    the size is there for."""
    for row in X.fps_table(n):
        c = X.fps_case(*row)
        check_fps(L, c.tag, c.cloud.to(DEV), c.M, c.guard, c.want, c.want_xyz)


@pytest.mark.parametrize("n", X.FPS_ALIGN)
def test_fps_cloud_4_bytes_off_16(L, n):
    """count % 4 == 0 and the base pointer 4 bytes past a 16-byte boundary: stage_cloud's scalar branch for a size that otherwise never
    takes it (n = 4100: fps_big_kernel, which reads the cloud in place).  The same rows as the aligned call, and the oracle's."""
    for kind in ("lattice", "cars"):
        cloud = X.fps_cloud(n, kind, None)
        M = 96
        want = P.furthest_point_sampling(cloud, M, guard=True)
        aligned = cloud.to(DEV)
        assert aligned.data_ptr() % 16 == 0
        tag = "n%d_%s" % (n, kind)
        got_a = check_fps(L, "aligned_" + tag, aligned, M, 1, want, X.gather_rows(cloud, want))
        got_m = check_fps(L, "off4_" + tag, misaligned(cloud), M, 1, want, X.gather_rows(cloud, want))
        exact("edges:fps_off4_is_aligned_" + tag, got_m, got_a)


# ---------------------------------------------------------------------------------------------
# ball queries
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,M,route,why", X.BALL_ROUTE, ids=["n%d_M%d" % (r[0], r[1]) for r in X.BALL_ROUTE])
def test_ball_query_route_thresholds(L, n, M, route, why):
    """Both sides of each threshold of the host's route rule, and the smallest clouds, with ns = 1, 16, 65, through the single query
    and through the pair (second radius below, equal to and above the first, with a different ns).  The rule is restated here (a check
    of the table, not of the binary): the LDS kernels take n <= 12288 with M >= 64 and n >= 256."""
    assert route == ("lds" if (n <= 12288 and M >= 64 and n >= 256) else "plain"), why
    cloud, centres = X.route_inputs(n, M)
    cd, ctr = cloud.to(DEV), centres.to(DEV)
    r = X.route_radius(n)
    single = {}

    def one(radius, ns):
        if (radius, ns) not in single:
            got = run_ball(L, cd, ctr, radius, ns)
            exact("edges:ball_route_n%d_M%d_r%g_ns%d" % (n, M, radius, ns), got, X.route_want(n, M, radius, ns))
            single[(radius, ns)] = got
        return single[(radius, ns)]

    for ns in X.BALL_ROUTE_NS:
        one(r, ns)
        nsb = X.BALL_ROUTE_NS_B[ns]
        for f in X.BALL_ROUTE_RB:
            rb = r * f
            ga, gb = run_pair(L, cd, ctr, r, ns, rb, nsb)
            tag = "n%d_M%d_r%g_ns%d_rb%g_ns%d" % (n, M, r, ns, rb, nsb)
            exact("edges:ball_pair_a_is_single_" + tag, ga, one(r, ns))
            exact("edges:ball_pair_b_is_single_" + tag, gb, one(rb, nsb))
            exact("edges:ball_pair_a_" + tag, ga, X.route_want(n, M, r, ns))
            exact("edges:ball_pair_b_" + tag, gb, X.route_want(n, M, rb, nsb))
    if n % 4 == 0 and route == "lds":
        # the LDS kernels stage through stage_cloud too: the same cloud 4 bytes off 16
        cm = misaligned(cloud)
        exact("edges:ball_route_off4_n%d_M%d" % (n, M), run_ball(L, cm, ctr, r, 16), X.route_want(n, M, r, 16))
        ga, gb = run_pair(L, cm, ctr, r, 16, r * 0.5, 65)
        exact("edges:ball_pair_a_off4_n%d_M%d" % (n, M), ga, X.route_want(n, M, r, 16))
        exact("edges:ball_pair_b_off4_n%d_M%d" % (n, M), gb, X.route_want(n, M, r * 0.5, 65))


@pytest.mark.parametrize("n", X.BALL_BOUNDARY_N)
@pytest.mark.parametrize("M", X.BALL_BOUNDARY_M)
def test_ball_query_is_strict_on_the_sphere(L, n, M):
    """Lattice clouds: every centre has points at d2 == r2 exactly, computed without a rounding.  They are outside (`<`), on the plain
    kernel (M = 5), the LDS kernel and the pair kernel (M = 70), for either radius of the pair in either position."""
    c = X.boundary_case(n, M)
    cd, ctr = c.cloud.to(DEV), c.centres.to(DEV)
    ra, rb, ns = X.BOUNDARY_RADIUS, X.BOUNDARY_RADIUS_B, X.BOUNDARY_NS
    exact("edges:ball_boundary_%s_r%g" % (c.tag, ra), run_ball(L, cd, ctr, ra, ns), c.want)
    exact("edges:ball_boundary_%s_r%g" % (c.tag, rb), run_ball(L, cd, ctr, rb, ns), c.want_b)
    ga, gb = run_pair(L, cd, ctr, ra, ns, rb, ns)
    exact("edges:ball_boundary_pair_a_%s" % c.tag, ga, c.want)
    exact("edges:ball_boundary_pair_b_%s" % c.tag, gb, c.want_b)
    ga, gb = run_pair(L, cd, ctr, rb, ns, ra, ns)
    exact("edges:ball_boundary_pair_swapped_a_%s" % c.tag, ga, c.want_b)
    exact("edges:ball_boundary_pair_swapped_b_%s" % c.tag, gb, c.want)


@pytest.mark.parametrize("n", X.BALL_PLANTED_N)
@pytest.mark.parametrize("M", X.BALL_PLANTED_M)
def test_ball_query_planted_hits(L, n, M):
    """Hits planted where the slot arithmetic can go wrong (X.planted_table names each): the expected row is the first ns hits padded
    with the first, all zeros without a hit -- stated without the oracle.  Single query, and the pair with a wider second ball that
    holds the same hits and one more slot."""
    for name, hits, ns, why in X.planted_table(n):
        c = X.planted_case(n, M, name)
        cd, ctr = c.cloud.to(DEV), c.centres.to(DEV)
        exact("edges:ball_planted_%s" % c.tag, run_ball(L, cd, ctr, X.PLANTED_RADIUS, c.ns), c.want)
        ga, gb = run_pair(L, cd, ctr, X.PLANTED_RADIUS, c.ns, X.PLANTED_RADIUS_B, c.ns_b)
        exact("edges:ball_planted_pair_a_%s" % c.tag, ga, c.want)
        exact("edges:ball_planted_pair_b_%s" % c.tag, gb, c.want_b)
