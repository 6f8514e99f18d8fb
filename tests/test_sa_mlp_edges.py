"""The set-abstraction kernels (csrc/sa_mlp.hip, all behind sa_mlp_max_impl) on every route at its edges, against f64.

The suite ran this family at the model's own shapes only (B = 2, M a multiple of every centres-per-workgroup count, feat_kind = 0).  Here:
ragged M on every route (the four register shapes with their per-cloud list and the three f64 re-evaluation launches, the four LDS
instantiations, split_last, the pre-aggregated first layer), the production flags of the first two levels (QUAD / PAIRS, LO_OUT, LO_IN and
their chain), the silent fallback of an unaligned output slice, the C ABI without a workspace and in two halves,
PointNetFeatureExtractor.forward, the pre-aggregated entries and the refusals -- on clouds whose ball sizes are fixed by construction
(tests/sa_mlp_ref.py), so that K = 1, repair_kmax, repair_kmax + 1 and ns sit where a kernel changes path.

The bound is the project's: |hip - f64| <= 1e-5, flat (test_hip_parity.record_f64, which also records the f32 oracle's distance).  The CPU
tests of this file keep that a statement about the kernel: on every row a GPU test compares, the f32 evaluation of the same graph stays
within 2e-6 of f64 (test_conditioning; seeds picked there, no kernel involved).  Every measured error lands in test_hip_parity's JSON
report under "sa_edges:...".
"""
import numpy as np
import pytest
import torch

import sa_mlp_ref as R
from oracle import model as O
from oracle import point_ops as P
from test_hip_parity import REPORT, exact, record, record_f64

NAN = float("nan")
gpu = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    return torch.device("cuda:0")


def _note(name, **kw):
    """Extra fields of a report entry (route, M, ...), or an entry that carries no assertion of record()'s kind.  Like exact()'s entries
    they reach the report file with the next record() / record_f64(); the last ones with _worst_of_the_family's."""
    REPORT.setdefault(name, {}).update(kw)


@pytest.fixture(scope="module", autouse=True)
def _worst_of_the_family():
    """Behind the module's last test: the largest |hip - f64| of every entry held to the flat bound, as one entry with that bound."""
    yield
    errs = [v["max_abs_err_vs_f64"] for k, v in REPORT.items() if k.startswith("sa_edges:") and v.get("bound") == R.FLAT and "max_abs_err_vs_f64" in v]
    if errs:
        record("sa_edges:worst_vs_f64", max(errs), 0.0, R.FLAT)


def _ids(specs):
    return [R.spec_id(s) for s in specs]


def _uniq(specs):
    seen, out = set(), []
    for s in specs:
        if R.spec_id(s) not in seen:
            seen.add(R.spec_id(s))
            out.append(s)
    return out


# ---------------------------------------------------------------------------------------------
# CPU: the inputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,radius", [(R.SIZES, R.RADIUS), (R.DENSE, R.RADIUS), (R.FLAG_SIZES, R.FLAG_RADIUS)])
def test_cluster_cloud_geometry_and_ball_sizes(sizes, radius):
    """A cluster lies within radius / 4 of its first point, clusters are >= 4 radius apart, the first point is stored first -- so the
    oracle's ball query about every first point returns exactly K = min(size, ns) distinct samples, first hit the centre itself."""
    for seed in (0, 1001, 2002):
        xyz, firsts = R.cluster_cloud(sizes, radius, seed)
        n = xyz.shape[0]
        assert n == sum(sizes) and n <= 400
        owner = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
        d = torch.cdist(xyz.double(), xyz.double())
        assert float((d[torch.arange(n), torch.tensor(firsts)[owner]]).max()) <= radius / 4
        assert float(d[owner.unsqueeze(0) != owner.unsqueeze(1)].min()) >= 4 * radius
        ctr = xyz[firsts].unsqueeze(0).contiguous()
        for ns in (16, 32):
            idx = P.ball_query(radius, ns, xyz.unsqueeze(0).contiguous(), ctr)
            assert idx[0, :, 0].tolist() == firsts
            assert R.count_k(idx)[0].tolist() == [min(s, ns) for s in sizes]
            if sizes is R.SIZES:
                assert {1, 2, 4, 5, 8, 9, ns - 1, ns} <= set(R.count_k(idx)[0].tolist())
            if sizes is R.FLAG_SIZES:       # (eight clusters, the corners of a cube: what the 8-sample f64 launch and the register kernel need)
                assert {1, 4, 8, 9, ns} <= set(R.count_k(idx)[0].tolist())
                assert 1.5 <= float(xyz.abs().min()) and float(xyz.abs().max()) <= 2.5


@pytest.mark.parametrize("spec", _uniq(R.all_specs()), ids=_ids(_uniq(R.all_specs())))
def test_designed_ball_sizes(spec):
    """The counted K of every centre is the designed one, every index lies in [0, n), n <= 400 and M <= 257; on the clouds with small
    balls K = 1, repair_kmax, repair_kmax + 1 and ns sit in the first rows, in the last rows and around row 128."""
    k = R.get(spec)
    assert torch.equal(k.K, k.K_designed)
    assert int(k.idx.min()) >= 0 and int(k.idx.max()) < k.xyz.shape[1] <= 400 and k.M <= 257 and k.M * k.ns <= 8224
    if spec.get("sizes", R.SIZES) is not R.DENSE:
        kd = k.kmax if k.kmax else 4
        want = {1, kd, kd + 1, k.ns}
        for b in range(k.B):
            K = k.K[b].tolist()
            assert set(K[:4]) <= want and set(K[-4:]) <= want
            if k.M >= 4:
                assert set(K[-4:]) == want
            if k.M >= 8:
                assert set(K[:4]) == want
            if k.M >= 129:
                assert {K[127], K[128]} <= want and K[127] != K[128]
            if k.M > 129:
                assert set(K[126:130]) == want


def test_routes_of_the_matrix():
    """The matrix reaches every kernel of the family, each with M = 1, (where one exists) an M below its centres per workgroup, an odd M
    above it, and -- register routes -- 129 and 257; C takes multiples of 4, other counts and 0; B is 1 and 3; both row paddings occur."""
    specs = R.route_specs()
    by_route = {}
    for s, extra in specs:
        by_route.setdefault(R.route(s["widths"], s["C"], s["ns"], s.get("pre", False)), []).append(s)
    assert set(by_route) == {"reg16", "reg32", "lds16x64", "lds32x64", "lds16x32", "lds32x32", "lds16x32split", "lds32x32split", "lds16x32pre", "lds32x32pre"}
    for name, ss in by_route.items():
        Ms = {s["M"] for s in ss}
        cpw = R.centres_per_workgroup(ss[0]["widths"], ss[0]["C"], ss[0]["ns"], ss[0].get("pre", False))
        assert 1 in Ms and any(M % 2 and M > cpw for M in Ms), name
        assert cpw == 1 or any(M < cpw for M in Ms), name
        if name.startswith("reg"):
            assert {129, 257} <= Ms and len({s["widths"] for s in ss}) == 2
    Cs = {s["C"] for s, _ in specs}
    assert {0, 5, 6, 97} <= Cs and any(C and C % 4 == 0 for C in Cs)
    assert {s["B"] for s, _ in specs} == {1, 3} and {e for _, e in specs} == {0, 4}
    assert R.split_last((128, 256, 256), 256) == 1 and R.split_last((128, 256, 256), 253) == 1 and R.split_last((64, 96, 128), 128) == 0
    assert R.lds_bytes((768, 768, 768), 6) > 160 * 1024 >= R.lds_bytes((128, 256, 256), 256)
    assert R.repair_kmax((32, 32, 64), 6, 3) == 8 and R.repair_kmax((32, 32, 64), 96) == 4 and R.repair_kmax((32, 32, 64), 97) == 4
    assert R.repair_kmax((16, 16, 32), 3, 1) == 8 and R.repair_kmax((16, 32, 48), 6) == 0 and R.repair_kmax((32, 32, 64), 6, 0, aligned=False) == 0


def test_reference_pinned_to_the_oracle(seeded_sd):
    """sa_ref_f64 is O.set_abstraction's per-scale output (second level, the seeded weights) to 1e-12.  The cloud lies on a grid of
    2^-10, where the f32 subtraction sa_ref mirrors and the f64 one of the oracle's f64 route are both exact."""
    gen = torch.Generator().manual_seed(5)
    B, n, M, C = 2, 200, 24, 96
    xyz = (torch.randint(-1024, 1025, (B, n, 3), generator=gen).double() / 1024.0)
    feat = torch.randn(B, n, C, generator=gen)
    pre = "encoder.local_extract.set_abstractions.1"
    sd64 = {k: v.double() for k, v in seeded_sd.items() if k.startswith(pre)}
    inter = []
    _, want = O.set_abstraction(sd64, pre, xyz, feat.double().transpose(1, 2).contiguous(), M, [0.3, 0.5], inter)
    ctr, off = inter[0]["new_xyz"].float(), 0
    for i, idx in enumerate(inter[0]["ball_idx"]):
        got = R.sa_ref_f64(xyz.float(), ctr, feat, idx, sd64, prefix="%s.pointnet_modules.%d" % (pre, i))
        w = want[:, off:off + got.shape[2]].transpose(1, 2)
        assert got.shape == w.shape and float((got - w).abs().max()) <= 1e-12
        off += got.shape[2]
    assert off == want.shape[1]


@pytest.mark.parametrize("spec", _uniq(R.all_specs()), ids=_ids(_uniq(R.all_specs())))
def test_conditioning(spec):
    """The f32 evaluation of the graph stays within 2e-6 of f64 on every row the register or the LDS kernel computes (K > repair_kmax;
    every row where the route has no f64 re-evaluation).  The seeds of sa_mlp_ref.SEEDS are picked so that this holds: a flat GPU bound
    is then a statement about the kernel and not about a cancelling GroupNorm group (csrc/sa_mlp.hip: the 4e-4 case).  With feat_kind the
    f32 graph reads the rounded products and sa_ref_f64 the exact ones, as the issue states the check."""
    k = R.get(spec)
    assert R.f32_distance(k) <= R.COND


def test_conditioning_of_the_other_inputs():
    for ns in (16, 32):
        r = R.lo_in_case(ns)
        assert torch.equal(r.K, r.K_designed) and r.kmax == 4
        big = r.K > r.kmax
        assert float((r.want32.double() - r.want_true).abs().amax(dim=2)[big].max()) <= R.COND
    c = R.chain_case()
    for ns in (16, 32):
        big = c.K1[ns] > c.kmax
        if bool(big.any()):
            assert float((c.want32[ns].double() - c.want[ns]).abs().amax(dim=2)[big].max()) <= R.COND
    assert bool((c.K1[16] <= c.kmax).any()) and bool((c.K1[32] > c.kmax).any())       # both halves of the second level see the chain
    for (w, C, ns) in R.FE_SHAPES:
        _, _, w32, w64 = R.fe_input(w, C, ns)
        assert float((w32.double() - w64).abs().max()) <= R.COND


def test_lo_in_inputs_separate_the_two_references():
    """With lo = 1e-3 randn the reference on hi + lo is >= 1e-4 away from the reference on hi alone on EVERY small ball: a kernel whose
    f64 re-evaluation ignores lo cannot meet 1e-5 there.  With the true residual the two agree to the f32 rounding of the input."""
    for ns in (16, 32):
        r = R.lo_in_case(ns)
        small = r.K <= r.kmax
        assert int(small.sum()) >= 8
        assert float((r.want_rand - r.want_hi).abs().amax(dim=2)[small].min()) >= 1e-4
        assert float(r.lo_true.abs().max()) <= 2.0 ** -24 * float(r.hi.abs().max())


def test_longdouble_reference_agrees_with_f64():
    k = R.get(R.FLAG_SPECS[2])
    rows = [(0, m) for m in range(0, k.M, 5)]
    ld = R.sa_ref_ld(k.xyz, k.ctr, None, k.idx, k.sd, rows, feat_kind=3)
    want = np.stack([k.want64[b, m].numpy() for (b, m) in rows])
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "numpy.longdouble is not wider than float64 here"
    assert float(np.abs(ld - want.astype(np.longdouble)).max()) <= 1e-12


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def _guarded(B, M, ldo, dev):
    """NaN-filled (B, M, ldo) output in front of four guard rows: -> out, guard (a store past the last centre lands in the guard)."""
    buf = torch.full((B * M + 4, ldo), NAN, device=dev)
    return buf[:B * M].view(B, M, ldo), buf[B * M:]


def _only_nan(*ts):
    return all(bool(torch.isnan(t).all()) for t in ts)


def _inputs(k, dev, extra=0):
    """-> xyz, ctr, feat (padded: 7.0 in [C, C4), NaN behind C4), idx on the device.  With feat_kind, feat is ops.prep_input's."""
    from caspr_amd import ops
    if k.feat_kind & 3:
        x = torch.cat([k.xyz, torch.zeros(k.B, k.xyz.shape[1], 1)], dim=2).view(k.B, 1, -1, 4).contiguous()
        xyz, feat = ops.prep_input(x.to(dev), quad=bool(k.feat_kind & 1), pairs=bool(k.feat_kind & 2))
        assert torch.equal(xyz.cpu(), k.xyz) and torch.equal(feat[:, :, :k.C].cpu(), k.feat)
        return xyz, k.ctr.to(dev), feat, k.idx.to(dev)
    fpad = None if k.feat is None else R.pad_feat(k.feat, (k.C + 3) // 4 * 4 + extra).to(dev)
    return k.xyz.to(dev), k.ctr.to(dev), fpad, k.idx.to(dev)


def _net(k, dev):
    return R.net_on(k.C, k.widths, k.seed, str(dev))


def _run(k, dev, out, out_off, extra=0, feat_kind=None, part=None):
    from caspr_amd import ops
    xyz, ctr, feat, idx = _inputs(k, dev, extra)
    m = _net(k, dev)
    if k.pre:
        pw_f, wx = m.pre_layers()
        pre = ops.conv1x1(pw_f, None, k.feat.to(dev).contiguous())
        return ops.sa_mlp_max_pre(xyz, ctr, pre, idx, wx, m.kernel_layers(), out, out_off)
    return ops.sa_mlp_max(xyz, ctr, feat, idx, k.C, m.kernel_layers(), out, out_off, feat_kind=k.feat_kind if feat_kind is None else feat_kind, part=part)


def _raw(k, dev, out, ldo, out_off, feat_kind=0, workspace=None, entry="caspr_sa_mlp_max_ws_f32", extra=0):
    """The C entries themselves (caspr_amd.lib): `out` any float32 device tensor, rows of ldo floats."""
    from caspr_amd import lib, ops
    xyz, ctr, feat, idx = _inputs(k, dev, extra)
    args = []
    for (pw, b, g, be) in _net(k, dev).kernel_layers():
        args += [ops._p(pw.data), ops._p(b), ops._p(g), ops._p(be), pw.cout]
    head = [ops._p(xyz), ops._p(ctr), ops._p(feat), 0 if feat is None else feat.shape[2], ops._p(idx), k.B, k.xyz.shape[1], k.M, k.C, k.ns, int(feat_kind)]
    tail = [ops._p(out), ldo, out_off] + ([ops._p(workspace)] if entry.endswith("_ws_f32") else []) + [ops._stream()]
    lib.check(getattr(lib.load(), entry)(*head, *args, *tail), entry)
    torch.cuda.synchronize()


ROUTE_SPECS = R.route_specs()


@gpu
@pytest.mark.parametrize("spec,extra", ROUTE_SPECS, ids=_ids([s for s, _ in ROUTE_SPECS]))
def test_route_at_ragged_m(dev, spec, extra):
    """Every route at M = 1, below and above its centres per workgroup and across the f64 kernel's 128-row survey: every output row
    within the flat bound of f64, nothing written outside [out_off, out_off + C3) or past the last centre, and the same bits twice."""
    k = R.get(spec)
    C3, off = k.widths[2], 8
    outs = []
    for _ in range(2):
        out, guard = _guarded(k.B, k.M, off + C3 + 8, dev)
        _run(k, dev, out, off, extra)
        outs.append((out, guard))
    out, guard = outs[0]
    name = "sa_edges:route:" + R.spec_id(spec)
    try:
        record_f64(name, out[:, :, off:off + C3], k.want32, k.want64, R.FLAT)
    finally:
        _note(name, route=k.route, M=k.M, B=k.B, C=k.C, ns=k.ns, repair_kmax=k.kmax, feat_row_padding=extra)
    assert _only_nan(out[:, :, :off], out[:, :, off + C3:], guard), "a store outside the output slice"
    exact(name + ":second_launch", outs[1][0][:, :, off:off + C3], out[:, :, off:off + C3])


@gpu
@pytest.mark.parametrize("spec", R.FLAG_SPECS, ids=_ids(R.FLAG_SPECS))
def test_feat_kind(dev, spec):
    """(a) QUAD, PAIRS and both (C = 3, 3, 6) on the first level's two register shapes, feat from ops.prep_input, coordinates of magnitude
    ~2: every row within the flat bound of the f64 graph on the EXACT products; the rows of K <= 8 (evaluated in f64 from exact products
    by sa_repair_f64_kernel<1,1>, <2,4> and <5,8>) recorded separately."""
    k = R.get(spec)
    assert k.kmax == 8
    out, guard = _guarded(k.B, k.M, k.widths[2], dev)
    _run(k, dev, out, 0)
    name = "sa_edges:feat_kind:" + R.spec_id(spec)
    small = k.K <= 8
    _note(name + ":input_rounding", f64_on_rounded_products_vs_exact=float((k.same64 - k.want64).abs().max()), rows_with_K_le_8=int(small.sum()), rows=int(small.numel()))
    got = out.cpu()
    record(name + ":K<=8", got[small], k.want64[small], R.FLAT)
    record_f64(name, got, k.want32, k.want64, R.FLAT)
    assert _only_nan(guard)


@gpu
@pytest.mark.parametrize("spec", [s for s in R.FLAG_SPECS if s["feat_kind"] == 3], ids=_ids([s for s in R.FLAG_SPECS if s["feat_kind"] == 3]))
def test_lo_out(dev, spec):
    """(b) QUAD | PAIRS | LO_OUT, the first level's call.  hi is the plain call's output bit for bit.  On the rows the f64 kernel wrote
    (K <= repair_kmax) lo = (float)(mx - (double)hi): |lo| <= 2^-24 |hi| (+ the smallest denormal), and hi + lo, summed in f64, is the
    f64 result -- held to 32 e64 + 2^-45 max(1, |ref|) against a numpy.longdouble evaluation of those rows, e64 being sa_ref_f64's own
    distance from it (another summation order over three layers).  On the other rows hi + lo is within the flat bound."""
    k = R.get(spec)
    C3, off = k.widths[2], 4
    W = C3 + 8
    plain, _ = _guarded(k.B, k.M, 2 * W, dev)
    _run(k, dev, plain, off)
    out, guard = _guarded(k.B, k.M, 2 * W, dev)
    _run(k, dev, out, off, feat_kind=k.feat_kind | R.FEAT_LO_OUT)
    assert _only_nan(out[:, :, :off], out[:, :, off + C3:W + off], out[:, :, W + off + C3:], guard, plain[:, :, off + C3:])
    hi, lo = out[:, :, off:off + C3].cpu(), out[:, :, W + off:W + off + C3].cpu()
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all()
    name = "sa_edges:lo_out:" + R.spec_id(spec)
    exact(name + ":hi_vs_plain_call", hi, plain[:, :, off:off + C3])
    small = k.K <= k.kmax
    ratio = lo[small].abs().double() / hi[small].abs().double().clamp_min(2.0 ** -125)
    _note(name + ":lo_over_hi:K<=kmax", max_ratio=float(ratio.max()), bound=2.0 ** -24)
    assert bool((lo[small].abs().double() <= 2.0 ** -24 * hi[small].abs().double() + 2.0 ** -149).all())
    total = hi.double() + lo.double()
    record(name + ":hi+lo:K>kmax", total[~small], k.want64[~small], R.FLAT)
    rows = [(int(b), int(m)) for b, m in small.nonzero()]
    ld = R.sa_ref_ld(k.xyz, k.ctr, None, k.idx, k.sd, rows, feat_kind=3)
    e64 = float(np.abs(k.want64[small].numpy().astype(np.longdouble) - ld).max())
    err = np.abs(total[small].numpy().astype(np.longdouble) - ld)
    bound = 32.0 * e64 + 2.0 ** -45 * np.maximum(1.0, np.abs(ld))
    _note(name + ":hi+lo:K<=kmax", e64=e64, max_abs_err=float(err.max()), bound=float(bound.min()), rows=len(rows),
          hi_alone_max_abs_err=float(np.abs(hi[small].numpy().astype(np.longdouble) - ld).max()))
    assert bool((err <= bound).all()), "hi + lo is %.3e from the longdouble evaluation (bound %.3e, e64 %.3e)" % (float(err.max()), float(bound.min()), e64)


@gpu
@pytest.mark.parametrize("ns", [16, 32])
def test_lo_in(dev, ns):
    """(c) LO_IN on the second level's register shapes (C = 96, feat rows [96 hi | 96 lo]).  With lo the true f32 residual of an f64
    feature tensor every row is within the flat bound of the reference on hi + lo.  With lo = 1e-3 randn the rows of K <= repair_kmax
    are (their reference on hi alone is >= 1e-4 away: test_lo_in_inputs_separate_the_two_references); the rows of K > repair_kmax are
    not compared in that sub-case -- the MFMA's deviation columns read hi by contract (include/caspr_hip.h)."""
    from caspr_amd import ops
    r = R.lo_in_case(ns)
    m = R.net_on(r.C, r.widths, r.seed, str(dev))
    small = r.K <= r.kmax
    for which, lo, want in (("true_residual", r.lo_true, r.want_true), ("random_low_part", r.lo_rand, r.want_rand)):
        feat = torch.cat([r.hi, lo], dim=2).contiguous().to(dev)
        out, guard = _guarded(r.B, r.M, 64, dev)
        ops.sa_mlp_max(r.xyz.to(dev), r.ctr.to(dev), feat, r.idx.to(dev), r.C, m.kernel_layers(), out, 0, feat_kind=R.FEAT_LO_IN)
        got = out.cpu()
        assert torch.isfinite(got).all() and _only_nan(guard)
        name = "sa_edges:lo_in:ns%d:%s" % (ns, which)
        if which == "true_residual":
            record_f64(name, got, r.want32, want, R.FLAT)
        else:
            record(name + ":K<=kmax", got[small], want[small], R.FLAT)
            _note(name + ":K<=kmax", reference_on_hi_alone_is_away_by=float((r.want_rand - r.want_hi).abs().amax(dim=2)[small].min()))


@gpu
def test_lo_out_chained_into_lo_in(dev):
    """(d) The first level (both scales into one [hi | lo] row, QUAD | PAIRS | LO_OUT) feeding the second (LO_IN), as PointNet2feat.run
    chains them, against the two-level f64 reference at the flat bound."""
    from caspr_amd import ops
    c = R.chain_case()
    B, n = c.xyz.shape[:2]
    x = torch.cat([c.xyz, torch.zeros(B, n, 1)], dim=2).view(B, 1, n, 4).contiguous()
    xyz, feat = ops.prep_input(x.to(dev))
    ctr = c.ctr.to(dev)
    M0 = ctr.shape[1]
    out0, guard0 = _guarded(B, M0, 192, dev)
    off = 0
    for i in range(2):
        m = R.net_on(6, [(16, 16, 32), (32, 32, 64)][i], R.CHAIN_SEED + i, str(dev))
        ops.sa_mlp_max(xyz, ctr, feat, c.idx0[i].to(dev), 6, m.kernel_layers(), out0, off, feat_kind=R.FEAT_QUAD | R.FEAT_PAIRS | R.FEAT_LO_OUT)
        off += [32, 64][i]
    assert torch.isfinite(out0).all() and _only_nan(guard0)
    record("sa_edges:chain:level0:hi+lo", out0[:, :, :96].cpu().double() + out0[:, :, 96:].cpu().double(), c.F1, R.FLAT)
    ctr1 = c.ctr1.to(dev)
    for ns in (16, 32):
        m = R.net_on(96, (32, 32, 64), R.CHAIN_SEED + 2 + ns, str(dev))
        out1, guard1 = _guarded(B, ctr1.shape[1], 64, dev)
        ops.sa_mlp_max(ctr, ctr1, out0, c.idx1[ns].to(dev), 96, m.kernel_layers(), out1, 0, feat_kind=R.FEAT_LO_IN)
        assert _only_nan(guard1)
        record_f64("sa_edges:chain:level1:ns%d" % ns, out1, c.want32[ns], c.want[ns], R.FLAT)
        _note("sa_edges:chain:level1:ns%d" % ns, rows_with_K_le_kmax=int((c.K1[ns] <= c.kmax).sum()), rows=int(c.K1[ns].numel()))


@gpu
@pytest.mark.parametrize("spec", R.ALIGN_SPECS, ids=_ids(R.ALIGN_SPECS))
def test_unaligned_output_slice_falls_back_to_the_lds_kernel(dev, spec):
    """A register shape whose output slice is not 16-byte aligned (out_off = 2; a row stride of C3 + 6 floats, through the C entry:
    ops refuses such a tensor) runs on the LDS kernel.  On a dense cloud (every K = ns) the call is within the flat bound and the
    neighbours of the slice stay untouched.  On a cloud with small balls the aligned call is held to the flat bound; the unaligned one
    has no f64 re-evaluation and is RECORDED only (a finding, see include/caspr_hip.h).  With FEAT_LO_* the unaligned call is refused."""
    from caspr_amd import lib
    C3 = spec["widths"][2]
    d = R.get(R.dense(spec))
    assert int(d.K.min()) == d.ns
    name = "sa_edges:align:" + R.spec_id(spec)
    out, guard = _guarded(d.B, d.M, C3 + 8, dev)
    _run(d, dev, out, 2)
    record_f64(name + ":dense:out_off2", out[:, :, 2:2 + C3], d.want32, d.want64, R.FLAT)
    assert _only_nan(out[:, :, :2], out[:, :, 2 + C3:], guard)
    ldo = C3 + 6
    out, guard = _guarded(d.B, d.M, ldo, dev)
    _raw(d, dev, out, ldo, 0, workspace=torch.empty(d.B * (d.M + 1), dtype=torch.int32, device=dev))
    record_f64(name + ":dense:ldo%d" % ldo, out[:, :, :C3], d.want32, d.want64, R.FLAT)
    assert _only_nan(out[:, :, C3:], guard)
    k = R.get(spec)
    small = k.K <= k.kmax
    assert k.kmax == 4 and bool(small.any())
    out, _ = _guarded(k.B, k.M, C3 + 8, dev)
    _run(k, dev, out, 4)
    record_f64(name + ":small_balls:aligned", out[:, :, 4:4 + C3], k.want32, k.want64, R.FLAT)
    out, guard = _guarded(k.B, k.M, C3 + 8, dev)
    _run(k, dev, out, 2)
    got = out[:, :, 2:2 + C3].cpu().double()
    assert torch.isfinite(got).all() and _only_nan(out[:, :, :2], out[:, :, 2 + C3:], guard)
    err = (got - k.want64).abs().amax(dim=2)
    _note(name + ":small_balls:unaligned", held_to_the_bound=False, flat_bound=R.FLAT, max_abs_err_vs_f64=float(err.max()),
          max_abs_err_vs_f64_K_le_kmax=float(err[small].max()), max_abs_err_vs_f64_K_gt_kmax=float(err[~small].max()),
          oracle32_vs_f64=float((k.want32.double() - k.want64).abs().max()))
    W = C3 + 8
    out, _ = _guarded(k.B, k.M, 2 * W, dev)
    with pytest.raises(lib.CasprHipError, match="register kernel's shapes only"):
        _run(k, dev, out, 2, feat_kind=R.FEAT_LO_OUT)
    assert _only_nan(out)
    from caspr_amd import ops
    half = R.pad_feat(k.feat, (k.C + 3) // 4 * 4)
    feat2 = torch.cat([half, half], dim=2).contiguous().to(dev)                 # rows [C | C]: what a FEAT_LO_IN call reads
    out, _ = _guarded(k.B, k.M, C3 + 8, dev)
    with pytest.raises(lib.CasprHipError, match="register kernel's shapes only"):
        ops.sa_mlp_max(k.xyz.to(dev), k.ctr.to(dev), feat2, k.idx.to(dev), k.C, _net(k, dev).kernel_layers(), out, 2, feat_kind=R.FEAT_LO_IN)
    torch.cuda.synchronize()
    assert _only_nan(out)


@gpu
@pytest.mark.parametrize("spec", R.ABI_SPECS, ids=_ids(R.ABI_SPECS))
def test_entry_without_workspace_writes_the_same_bits(dev, spec):
    """caspr_sa_mlp_max_f32 against caspr_sa_mlp_max_ws_f32 with a workspace of exactly caspr_sa_mlp_max_workspace_ints(B, M) integers
    prefilled with 0x7fffffff ("contents irrelevant on entry"): the header promises the same outputs, bit for bit."""
    from caspr_amd import lib
    k = R.get(spec)
    C3 = k.widths[2]
    nws = lib.load().caspr_sa_mlp_max_workspace_ints(k.B, k.M)
    assert nws == k.B * (k.M + 1)
    ws = torch.full((nws + 8,), 0x7fffffff, dtype=torch.int32, device=dev)
    a, ga = _guarded(k.B, k.M, C3, dev)
    _raw(k, dev, a, C3, 0, entry="caspr_sa_mlp_max_f32")
    b, gb = _guarded(k.B, k.M, C3, dev)
    _raw(k, dev, b, C3, 0, workspace=ws[:nws])
    assert bool((ws[nws:] == 0x7fffffff).all()), "a write past the promised workspace"
    assert torch.isfinite(a).all() and _only_nan(ga, gb)
    exact("sa_edges:abi:no_workspace_vs_workspace:" + R.spec_id(spec), a, b)
    record_f64("sa_edges:abi:no_workspace:" + R.spec_id(spec), a, k.want32, k.want64, R.FLAT)


@gpu
@pytest.mark.parametrize("spec", R.HALVES_SPECS, ids=_ids(R.HALVES_SPECS))
def test_two_halves_at_ragged_m(dev, spec):
    """part="mfma" then "f64" and the reverse order write what the whole call writes, at M = 129 and M = 7."""
    k = R.get(spec)
    C3 = k.widths[2]
    whole, _ = _guarded(k.B, k.M, C3, dev)
    _run(k, dev, whole, 0)
    assert torch.isfinite(whole).all()
    for order in (("mfma", "f64"), ("f64", "mfma")):
        out, guard = _guarded(k.B, k.M, C3, dev)
        for part in order:
            _run(k, dev, out, 0, part=part)
        assert _only_nan(guard)
        exact("sa_edges:halves:%s:%s_first" % (R.spec_id(spec), order[0]), out, whole)
    _note("sa_edges:halves:%s:mfma_first" % R.spec_id(spec), rows_of_the_f64_half=int((k.K <= k.kmax).sum()))


@gpu
def test_halves_without_workspace_are_refused(dev):
    from caspr_amd import lib
    k = R.get(R.HALVES_SPECS[1])
    out, _ = _guarded(k.B, k.M, k.widths[2], dev)
    for bit in (16, 32):
        with pytest.raises(lib.CasprHipError, match="need the workspace"):
            _raw(k, dev, out, k.widths[2], 0, feat_kind=bit, entry="caspr_sa_mlp_max_f32")
    assert _only_nan(out)


@gpu
@pytest.mark.parametrize("widths,C,ns", R.FE_SHAPES)
def test_feature_extractor_forward(dev, widths, C, ns):
    """PointNetFeatureExtractor.forward, the reference signature (B' = 5 neighbourhoods as one-centre clouds: M = 1, identity index
    rows, centre at the origin), against O.feature_extractor in f64."""
    x, _, w32, w64 = R.fe_input(widths, C, ns)
    m = R.net_on(C - 3, widths, 0, str(dev))
    got = m(x.to(dev))
    assert got.shape == (5, widths[2])
    record_f64("sa_edges:forward:%s:C%d:ns%d" % ("x".join(map(str, widths)), C, ns), got, w32, w64, R.FLAT)


@gpu
def test_feature_extractor_forward_refuses_eight_samples(dev):
    from caspr_amd import lib
    m = R.net_on(0, (16, 16, 32), 0, str(dev))
    with pytest.raises(lib.CasprHipError, match="ns=8 unsupported"):
        m(torch.randn(5, 3, 8, device=dev))


@gpu
@pytest.mark.parametrize("spec", R.PRE_SPECS, ids=_ids(R.PRE_SPECS))
def test_pre_aggregated_entries_at_ragged_m(dev, spec):
    """sa_mlp_max_pre and group_rows_pre at M = 1, 3, 17 with pre rows wider than C1 (NaN behind them): group_rows_pre against the
    header's formula in f64 (2e-6 max(1, |ref|), the conv tests' bound), sa_mlp_max_pre against f64 at the flat bound and against the
    fused call at 1e-5."""
    from caspr_amd import ops
    k = R.get(spec)
    C1, C3 = k.widths[0], k.widths[2]
    xyz, ctr, _, idx = _inputs(k, dev)
    m = _net(k, dev)
    pw_f, wx = m.pre_layers()
    layers = m.kernel_layers()
    conv = ops.conv1x1(pw_f, None, k.feat.to(dev).contiguous())
    pre = torch.full((k.B, conv.shape[1], C1 + 4), NAN, device=dev)
    pre[:, :, :C1] = conv[:, :, :C1]
    name = "sa_edges:pre:" + R.spec_id(spec)
    Y = ops.group_rows_pre(xyz, ctr, pre, idx, wx, layers[0][1])
    g = P.group(k.xyz, k.ctr, None, k.idx).double()                                        # (B, M, 3, ns): the grouper's f32 subtraction
    li = k.idx.long()
    rows = pre[:, :, :C1].cpu().double()[torch.arange(k.B).view(-1, 1, 1), li]               # (B, M, ns, C1)
    want = rows + torch.einsum("cd,bmds->bmsc", wx.cpu().double(), g) + layers[0][1].detach().cpu().double()
    want = want.reshape(k.B, k.M * k.ns, C1)
    record(name + ":group_rows_pre", Y, want, 2e-6 * max(1.0, float(want.abs().max())))
    out, guard = _guarded(k.B, k.M, 8 + C3 + 4, dev)
    ops.sa_mlp_max_pre(xyz, ctr, pre, idx, wx, layers, out, 8)
    record_f64(name + ":sa_mlp_max_pre", out[:, :, 8:8 + C3], k.want32, k.want64, R.FLAT)
    assert _only_nan(out[:, :, :8], out[:, :, 8 + C3:], guard)
    fused, _ = _guarded(k.B, k.M, C3, dev)
    _run(R.get(dict(spec, pre=False)), dev, fused, 0)
    record(name + ":vs_fused", out[:, :, 8:8 + C3], fused, 1e-5)


@gpu
def test_refusals(dev):
    """Every refusal of sa_mlp_max_impl that a shape can provoke, by its message; nothing is written."""
    from caspr_amd import lib, ops
    k = R.get(dict(widths=(32, 32, 64), C=6, ns=16, M=7, B=2))
    k5 = R.get(dict(widths=(32, 32, 64), C=5, ns=16, M=7, B=2))
    xyz, ctr, feat, idx = _inputs(k, dev)
    layers = _net(k, dev).kernel_layers()
    out = torch.full((k.B, k.M, 128), NAN, device=dev)

    def refused(match, *a, **kw):
        with pytest.raises(lib.CasprHipError, match=match):
            ops.sa_mlp_max(*a, **kw)
        torch.cuda.synchronize()
        assert _only_nan(out), match

    def odd_layers(widths, cin):
        g = torch.Generator().manual_seed(1)
        dims, ls = (cin,) + widths, []
        for i in range(3):
            ls.append((ops.PackedWeight(torch.randn(dims[i + 1], dims[i] if i else cin + 3 + (-cin) % 4, generator=g).to(dev)),
                       torch.zeros(dims[i + 1], device=dev), torch.ones(dims[i + 1], device=dev), torch.zeros(dims[i + 1], device=dev)))
        return ls

    refused("multiples of 16", xyz, ctr, feat, idx, 6, odd_layers((24, 32, 48), 6), out, 0)
    refused("feat/ldf invalid", xyz, ctr, feat[:, :, :4].contiguous(), idx, 6, layers, out, 0)
    refused("bad sizes", xyz, ctr, feat, idx, 6, layers, out, 128 - 60)
    xyz5, ctr5, feat5, idx5 = _inputs(k5, dev)
    refused("does not describe C=5", xyz5, ctr5, feat5, idx5, 5, _net(k5, dev).kernel_layers(), out, 0, feat_kind=3)
    k3 = R.get(dict(widths=(32, 32, 64), C=3, ns=16, M=7, B=2))
    xyz3, ctr3, feat3, idx3 = _inputs(k3, dev, extra=4)
    refused("CASPR_FEAT_LO_IN needs", xyz3, ctr3, feat3, idx3, 3, _net(k3, dev).kernel_layers(), out, 0, feat_kind=R.FEAT_LO_IN | R.FEAT_QUAD)
    out76 = torch.full((k.B, k.M, 76), NAN, device=dev)
    with pytest.raises(lib.CasprHipError, match="CASPR_FEAT_LO_OUT needs"):
        ops.sa_mlp_max(xyz, ctr, feat, idx, 6, layers, out76, 0, feat_kind=R.FEAT_LO_OUT)
    refused("exclude each other", xyz, ctr, feat, idx, 6, layers, out, 0, feat_kind=16 | 32)
    wide = (768, 768, 768)
    assert R.lds_bytes(wide, 6) > 160 * 1024
    out768 = torch.full((k.B, k.M, 768), NAN, device=dev)
    with pytest.raises(lib.CasprHipError, match="bytes of LDS"):
        ops.sa_mlp_max(xyz, ctr, feat, idx, 6, odd_layers(wide, 6), out768, 0)
    pre = torch.zeros(k.B, k.xyz.shape[1], 32, device=dev)
    with pytest.raises(lib.CasprHipError, match="sa_mlp_max_pre: needs wx"):
        ops.sa_mlp_max_pre(xyz, ctr, pre, idx, torch.zeros(32, 3, device=dev), layers, out, 0)
    torch.cuda.synchronize()
    assert _only_nan(out, out76, out768)
    _note("sa_edges:refusals", refused_by_message=9, floats_written=0)
