"""The point operators (prep_input, gather / group, three_nn, three_interpolate, Chamfer, EMD, the two float-atomic backward
entries and the Kaolin-named surface) at the limits and edges their C entries ACCEPT, not only at the model's own shapes:
every loop stride's ragged tail, row strides wider than the payload, the 64 KiB dynamic-LDS boundary of three_nn, fewer than
three known points, exact ties, clouds smaller than a workgroup, the 1024-point LDS tile edge of Chamfer / EMD.

References: oracle.point_ops / oracle.model (whose own behaviour at these shapes tests/test_oracle_golden.py pins on the CPU) and
plain f64 torch.  Integer outputs and copies are compared bit for bit.  Floating-point sums are held to bounds DERIVED from their
rounding counts (u = 2^-24, the unit roundoff of f32), written next to each check; every measured error and its bound land in
the parity report test_hip_parity.record writes ("<name>:err_over_bound" is the largest ratio of the two, held to 1).
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import model as O
from oracle import point_ops as P
from test_hip_parity import REPORT, record, exact, clouds, rnd

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    from caspr_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def L():
    from caspr_amd import lib
    return lib.load()


def _check(rc, what):
    from caspr_amd import lib
    lib.check(rc, what)


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def within(name, got, want64, bound64):
    """|got - want| <= bound, element by element (bound derived by the caller, f64).  Records the largest error and the largest
    bound under "<name>:bound" and the largest ratio of error to bound under "<name>:err_over_bound", which record() holds to 1 and
    writes to the report (an entry whose bound is 0 must be reproduced exactly: its ratio is 0 or 1e30)."""
    got = got.detach().cpu().double().numpy()
    want = want64.detach().cpu().double().numpy()
    bound = bound64.detach().cpu().double().numpy()
    assert got.shape == want.shape == bound.shape, "%s: shapes %s %s %s" % (name, got.shape, want.shape, bound.shape)
    assert np.isfinite(got).all(), "%s: non-finite output" % name
    err = np.abs(got - want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, 1e30, 0.0))
    REPORT[name + ":bound"] = {"max_abs_err": float(err.max()), "bound_max": float(bound.max()), "ref_absmax": float(np.abs(want).max())}
    record(name + ":err_over_bound", ratio, np.zeros_like(ratio), 1.0)


def nn_weights(d):
    """pointnet2.py:516-518 on the oracle's distances, f32 like the reference (1 / (inf + 1e-8) == 0)."""
    inv = 1.0 / (d + 1e-8)
    return inv / inv.sum(dim=2, keepdim=True)


def rand_weights(seed, B, n):
    w = rnd(seed, B, n, 3).abs() + 0.05
    return (w / w.sum(dim=2, keepdim=True)).contiguous()


def rand_idx(seed, hi, *shape):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, hi, shape).astype(np.int32))


# ---------------------------------------------------------------------------------------------
# three_nn
# ---------------------------------------------------------------------------------------------
def _three_nn_vs_oracle(ops, tag, unknown, known):
    d, i = P.three_nn(unknown, known)
    gd, gi, gw = ops.three_nn(unknown.to(DEV), known.to(DEV), with_weights=True)
    exact("edges:three_nn_idx_%s" % tag, gi, i)
    filled = min(known.shape[1], 3)
    record("edges:three_nn_dist_%s" % tag, gd[:, :, :filled], d[:, :, :filled], 1e-7)
    record("edges:three_nn_weight_%s" % tag, gw, nn_weights(d), 1e-6)
    gd2, gi2 = ops.three_nn(unknown.to(DEV), known.to(DEV))             # the entry without the weight output
    assert torch.equal(gd2, gd) and torch.equal(gi2, gi)
    return d, i, gd.cpu(), gi.cpu(), gw.cpu()


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_three_nn_fewer_than_three_known_points(ops, m):
    """m < 3: the upstream loop never fills slots m..2 -- they keep +inf / index 0, and their weights are 1 / (inf + 1e-8) == 0."""
    unknown, known = clouds(2, 70, seed=40 + m), clouds(2, m, seed=50 + m)
    d, i, gd, gi, gw = _three_nn_vs_oracle(ops, "m%d" % m, unknown, known)
    for s in range(min(m, 3), 3):
        assert bool((d[:, :, s] == float("inf")).all()) and bool((i[:, :, s] == 0).all()), "the oracle's own unfilled slot %d" % s
        assert bool((gd[:, :, s] == float("inf")).all()), "slot %d: distance is not +inf" % s
        assert bool((gi[:, :, s] == 0).all()), "slot %d: index is not 0" % s
        assert bool((gw[:, :, s] == 0.0).all()), "slot %d: weight is not exactly 0" % s
    assert bool(torch.isfinite(gw).all())
    assert bool(torch.isfinite(gd[:, :, :min(m, 3)]).all())
    if m == 1:
        assert bool((gw[:, :, 0] == 1.0).all())


@pytest.mark.parametrize("m", [5461, 5462, 8192])
def test_three_nn_across_the_64k_lds_boundary(ops, m):
    """m * 12 bytes of dynamic LDS: 65,532 at m = 5461, 65,544 at 5462 (the first launch that needs the opt-in), 98,304 at the
    largest cloud the entry takes."""
    _three_nn_vs_oracle(ops, "n300_m%d" % m, clouds(2, 300, seed=7), clouds(2, m, seed=m))


def test_three_nn_refuses_the_first_cloud_past_its_limit(ops):
    from caspr_amd.lib import CasprHipError
    with pytest.raises(CasprHipError, match="three_nn"):
        ops.three_nn(clouds(2, 8, seed=1).to(DEV), torch.zeros(2, 8193, 3, device=DEV))


@pytest.mark.parametrize("n", [1, 257])
def test_three_nn_ragged_last_block(ops, n):
    """n = 257: a second block with ONE live thread (which still stages the known cloud with its 255 idle neighbours); n = 1."""
    _three_nn_vs_oracle(ops, "n%d_m33" % n, clouds(2, n, seed=60 + n), clouds(2, 33, seed=61))


def test_three_nn_exact_ties_keep_the_first_index(ops):
    """A known cloud whose second half repeats its first: every distance comes twice, bit for bit.  The strict `<` of all three
    slots keeps the earlier index: slots (k, k + 32, j) with k, j < 32."""
    known = clouds(2, 64, seed=8, dup=True)
    assert torch.equal(known[:, 32:], known[:, :32]) and not torch.equal(known[0], known[1])
    unknown = clouds(2, 200, seed=9)
    d, i, gd, gi, gw = _three_nn_vs_oracle(ops, "ties", unknown, known)
    assert bool((gi[:, :, 0] < 32).all()) and bool((gi[:, :, 1] == gi[:, :, 0] + 32).all()) and bool((gi[:, :, 2] < 32).all())
    assert torch.equal(gd[:, :, 0], gd[:, :, 1])
    # ... and with the unknown points ON the known ones: distance 0 twice
    d, i, gd, gi, gw = _three_nn_vs_oracle(ops, "ties_on_points", known[:, 10:40].contiguous(), known)
    assert bool((gd[:, :, :2] == 0.0).all())
    assert bool((gi[:, :, 0] == torch.cat([torch.arange(10, 32), torch.arange(0, 8)]).int()).all())


def test_three_nn_unknown_on_two_known_points(ops):
    """d = (0, 0, d3): 1 / 1e-8 twice against 1 / d3 -> weights (0.5, 0.5, ~0)."""
    known = rnd(70, 2, 10, 3)
    known[:, 7] = known[:, 2]
    unknown = rnd(71, 2, 5, 3)
    unknown[:, 3] = known[:, 2]
    d, i, gd, gi, gw = _three_nn_vs_oracle(ops, "coincident", unknown, known)
    assert gi[:, 3, :2].tolist() == [[2, 7], [2, 7]] and gd[:, 3, :2].tolist() == [[0.0, 0.0], [0.0, 0.0]]
    assert torch.equal(gw[:, 3, 0], gw[:, 3, 1])
    assert float((gw[:, 3, 0] - 0.5).abs().max()) <= 1e-6 and 0.0 < float(gw[:, 3, 2].max()) <= 1e-6
    assert float((gw.double().sum(2) - 1).abs().max()) <= 4 * U


# ---------------------------------------------------------------------------------------------
# three_interpolate (+ skip concat, + folded input transform)
# ---------------------------------------------------------------------------------------------
def _interp_c(L, feat_buf, C, idx, w, skip_buf, C2, ldo, in_scale=None, in_shift=None, in_relu=False):
    """caspr_three_interp_f32 with every stride spelled out: feat_buf (B,m,ldf), skip_buf (B,n,lds) | None -> out (B,n,ldo)."""
    B, m, ldf = feat_buf.shape
    n = idx.shape[1]
    lds = 0 if skip_buf is None else skip_buf.shape[2]
    out = torch.full((B, n, ldo), NAN, device=DEV)
    _check(L.caspr_three_interp_f32(_p(feat_buf), ldf, _p(idx), _p(w), _p(in_scale), _p(in_shift), int(in_relu), _p(skip_buf), lds,
                                    B, m, n, C, C2, _p(out), ldo, _stream()), "caspr_three_interp_f32")
    return out


def _interp_ref(feat, idx, w, sc=None, sh=None, relu=False):
    """f64 on the same f32 inputs -> (want, bound).
    Plain: r = (w0 f0 + w1 f1) + w2 f2 in f32: term 0 and 1 pass 3 roundings (product, two sums), term 2 passes 2; with an FMA
    contraction fewer.  |err| <= 3 u sum_k |w_k f_k| to first order, 4 u with the second-order terms.
    Transformed: f_k is first f s + t (product, sum: 2 roundings, each at most u (|f s| + |t|)), ReLU is 1-Lipschitz:
    + 3 u sum_k |w_k| (|f_k s| + |t|) (2 roundings, the third unit for their second-order terms through the sum)."""
    B = feat.shape[0]
    bi = torch.arange(B).view(B, 1, 1)
    f = feat.double()[bi, idx.long()]                                   # (B,n,3,C)
    extra = 0.0
    if sc is not None:
        s, t = sc.double().view(B, 1, 1, -1), sh.double().view(B, 1, 1, -1)
        extra = 3 * U * (w.double().abs().unsqueeze(3) * ((f * s).abs() + t.abs())).sum(2)
        f = f * s + t
        if relu:
            f = torch.relu(f)
    terms = w.double().unsqueeze(3) * f
    return terms.sum(2), 4 * U * terms.abs().sum(2) + extra


@pytest.mark.parametrize("C", [4, 132, 256, 260, 1024])
def test_three_interpolate_strides_tails_and_padding(ops, L, C):
    """The column loop strides by 256 floats (C < 256, C % 256 != 0, several trips), the skip / pad tail by 64 (C2 of 0, 3, 64, 65,
    200), feat is a column slice of a wider buffer (ldf = C + 12, the slack holds 1e30), the skip rows are wider than C2 (the slack
    holds NaN), the output is padded to 4 or 32 columns (pad exactly 0)."""
    B, m, n = 2, 40, 71                                                 # 142 rows: the last workgroup holds two
    buf = torch.full((B, m, C + 12), 1e30)
    feat = rnd(100 + C, B, m, C)
    buf[:, :, :C] = feat
    buf_d = buf.to(DEV)
    idx, w = rand_idx(C, m, B, n, 3), rand_weights(101 + C, B, n)
    idx[B - 1, n - 1] = torch.tensor([m - 1, 0, m - 1])                 # the last row of the last batch entry is addressed
    want, bound = _interp_ref(feat, idx, w)
    idx_d, w_d = idx.to(DEV), w.to(DEV)
    first = None
    for C2 in (0, 3, 64, 65, 200):
        for lds in ((C2 + 3) // 4 * 4, C2 + 8):
            if C2 == 0 and lds == 0:
                skip = skip_d = None
            else:
                skip = torch.full((B, n, lds), NAN)
                skip[:, :, :C2] = rnd(7 * C2 + lds, B, n, C2)
                skip_d = skip.to(DEV)
            for align in (4, 32):
                ldo = (C + C2 + align - 1) // align * align
                got = _interp_c(L, buf_d, C, idx_d, w_d, skip_d, C2, ldo).cpu()
                tag = "edges:three_interp[C%d,C2_%d,lds%d,ldo%d]" % (C, C2, lds, ldo)
                within(tag, got[:, :, :C], want, bound)
                if C2:
                    exact(tag + ":skip", got[:, :, C:C + C2], skip[:, :, :C2])
                assert bool((got[:, :, C + C2:] == 0.0).all()), tag + ": a pad column is not exactly 0"
                first = got if first is None else first
                assert torch.equal(got[:, :, :C], first[:, :, :C]), tag + ": the interpolated part depends on the tail's shape"
    # the same through ops (column-slice view, align = 32), where ops can express the strides
    skip = rnd(5, B, n, 8).to(DEV)
    got = ops.three_interpolate(buf_d[:, :, :C], idx_d, w_d, skip=skip, skip_channels=6, align=32).cpu()
    assert got.shape == (B, n, (C + 6 + 31) // 32 * 32)
    assert torch.equal(got[:, :, :C], first[:, :, :C]) and torch.equal(got[:, :, C:C + 6], skip.cpu()[:, :, :6])
    assert bool((got[:, :, C + 6:] == 0.0).all())


@pytest.mark.parametrize("relu", [False, True])
def test_three_interpolate_folded_input_transform(ops, L, relu):
    """feat read as (relu of) feat * scale + shift per (batch entry, channel): scale without ReLU, a negative scale, a transformed
    value that is exactly 0 (0.5 * 2 - 1) in batch entry 1 only."""
    B, m, n, C = 2, 40, 71, 132
    feat = rnd(200, B, m, C)
    sc, sh = rnd(201, B, C).abs() + 0.5, rnd(202, B, C)
    sc[:, 5] = -sc[:, 5]                                                # a channel whose scale is negative (in both entries)
    sc[1, 9], sh[1, 9] = 2.0, -1.0
    feat[1, :, 9] = 0.5                                                 # -> exactly 0 for every point of entry 1
    idx, w = rand_idx(203, m, B, n, 3), rand_weights(204, B, n)
    want, bound = _interp_ref(feat, idx, w, sc, sh, relu)
    assert bool((want[1, :, 9] == 0).all()) and bool((want[0, :, 9] != 0).any())
    buf = torch.full((B, m, C + 12), 1e30)
    buf[:, :, :C] = feat
    got = _interp_c(L, buf.to(DEV), C, idx.to(DEV), w.to(DEV), None, 0, C, sc.to(DEV), sh.to(DEV), relu).cpu()
    within("edges:three_interp_transform[relu%d]" % relu, got, want, bound)
    assert bool((got[1, :, 9] == 0.0).all())
    if relu:
        assert float(got.min()) >= 0.0
    else:
        assert float(got.min()) < 0.0                                   # no ReLU was applied
    got_ops = ops.three_interpolate(feat.to(DEV), idx.to(DEV), w.to(DEV), in_scale=sc.to(DEV), in_shift=sh.to(DEV), in_relu=relu)
    assert torch.equal(got_ops.cpu(), got)


def test_three_interpolate_repeated_neighbours_and_unit_weights(L):
    B, m, n, C = 2, 9, 70, 260
    feat = rnd(210, B, m, C)
    i1 = rand_idx(211, m, B, n, 1)
    idx = i1.expand(B, n, 3).contiguous()                               # i0 == i1 == i2
    w = rand_weights(212, B, n)
    want, bound = _interp_ref(feat, idx, w)
    got = _interp_c(L, feat.to(DEV), C, idx.to(DEV), w.to(DEV), None, 0, C).cpu()
    within("edges:three_interp_same_neighbour_thrice", got, want, bound)
    # weights (1, 0, 0): 1 * f + 0 * g + 0 * h is f, bit for bit
    idx = rand_idx(213, m, B, n, 3)
    w = torch.zeros(B, n, 3)
    w[:, :, 0] = 1.0
    got = _interp_c(L, feat.to(DEV), C, idx.to(DEV), w.to(DEV), None, 0, C).cpu()
    exact("edges:three_interp_unit_weight", got, torch.gather(feat, 1, idx[:, :, 0:1].long().expand(B, n, C)))
    # a zero weight in the middle / at the end, the others generic
    w = rand_weights(214, B, n)
    w[:, ::2, 1] = 0.0
    w[:, 1::2, 2] = 0.0
    want, bound = _interp_ref(feat, idx, w)
    got = _interp_c(L, feat.to(DEV), C, idx.to(DEV), w.to(DEV), None, 0, C).cpu()
    within("edges:three_interp_zero_weights", got, want, bound)


# ---------------------------------------------------------------------------------------------
# gather_points / group_points: copies, exact
# ---------------------------------------------------------------------------------------------
def _wide(t, ld, fill):
    """(B,P,C) -> (B,P,ld) buffer whose slack columns hold `fill`."""
    B, Pn, C = t.shape
    buf = torch.full((B, Pn, ld), fill)
    buf[:, :, :C] = t
    return buf


@pytest.mark.parametrize("C", [1, 5, 8])
@pytest.mark.parametrize("pad", [0, 3])
def test_gather_points_strides_and_repeats(ops, L, C, pad):
    """M > n with every index used at least twice, in an order that is not the identity; ldf = C + pad with NaN in the slack; an
    output stride wider than C whose slack must survive; 2 * 77 * C elements: never a multiple of 256."""
    B, n, M = 2, 37, 77
    feat = rnd(300 + C, B, n, C)
    perm = np.random.default_rng(C).permutation(M)
    idx = torch.from_numpy(np.stack([(np.arange(M) % n)[perm], (np.arange(M) % n)[perm[::-1]]]).astype(np.int32))
    idx[B - 1, M - 1] = n - 1                                           # point n - 1 of the last batch entry
    assert (B * M * C) % 256 != 0 and all(int(np.bincount(idx[b].numpy(), minlength=n).min()) >= 1 for b in range(B))
    want = torch.gather(feat, 1, idx.long().unsqueeze(-1).expand(-1, -1, C))
    ldf, ldo = C + pad, C + (2 if pad else 0)
    out = torch.full((B, M, ldo), -7.0, device=DEV)
    feat_d, idx_d = _wide(feat, ldf, NAN).to(DEV), idx.to(DEV)          # (named: they must outlive the launch)
    _check(L.caspr_gather_points_f32(_p(feat_d), ldf, _p(idx_d), B, n, M, C, _p(out), ldo, _stream()), "caspr_gather_points_f32")
    out = out.cpu()
    exact("edges:gather_points[C%d,ldf%d]" % (C, ldf), out[:, :, :C], want)
    assert bool((out[:, :, C:] == -7.0).all())
    if pad == 0:
        exact("edges:gather_points_ops[C%d]" % C, ops.gather_points(feat.to(DEV), idx.to(DEV)), want)


@pytest.mark.parametrize("C", [0, 1, 5, 8])
@pytest.mark.parametrize("ns", [1, 16])
def test_group_points_strides_and_repeats(ops, L, C, ns):
    B, n, M = 2, 37, 45                                                 # M * ns > n: indices repeat
    xyz, new_xyz = clouds(B, n, seed=30 + C), clouds(B, M, seed=31 + C)
    idx = rand_idx(320 + C + ns, n, B, M, ns)
    idx[B - 1, M - 1, ns - 1] = n - 1
    feat = rnd(321 + C, B, n, C) if C else None
    want = P.group(xyz, new_xyz, None if feat is None else feat.transpose(1, 2).contiguous(), idx)
    assert tuple(want.shape) == (B, M, 3 + C, ns)                       # 90 (3 + C) ns elements: a multiple of 256 only at C = 5, ns = 16
    xyz_d, new_d, idx_d = xyz.to(DEV), new_xyz.to(DEV), idx.to(DEV)
    for pad in ((0, 3) if C else (0,)):
        ldf = C + pad
        out = torch.full((B, M, 3 + C, ns), NAN, device=DEV)
        fb = None if feat is None else _wide(feat, ldf, NAN).to(DEV)
        _check(L.caspr_group_points_f32(_p(xyz_d), _p(new_d), _p(fb), ldf, _p(idx_d), B, n, M, C, ns, _p(out), _stream()),
               "caspr_group_points_f32")
        exact("edges:group_points[C%d,ns%d,ldf%d]" % (C, ns, ldf), out, want)
    exact("edges:group_points_ops[C%d,ns%d]" % (C, ns), ops.group_points(xyz_d, new_d, None if feat is None else feat.to(DEV), idx_d), want)


# ---------------------------------------------------------------------------------------------
# prep_input
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quad,pairs", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("B,T,N", [(1, 1, 1), (2, 3, 257)])
def test_prep_input_all_four_settings(ops, B, T, N, quad, pairs):
    """xyz and the product columns against tpointnet2.py:79-90 (oracle.model.augment_input): pairs-only puts xz, xy, yz in columns
    0..2; columns past the products are 0; the time column (1e6 and up here, against |products| < 1e3) shows up nowhere."""
    x = rnd(400 + N, B, T, N, 4, scale=2.0)
    x[..., 3] = 1e6 + torch.arange(B * T * N, dtype=torch.float32).view(B, T, N)
    want = O.augment_input(x.reshape(B * T, N, 4)[:, :, :3], quad=quad, pairs=pairs)
    k = want.shape[2] - 3
    assert k == 3 * int(quad) + 3 * int(pairs)
    xyz, feat = ops.prep_input(x.to(DEV), quad=quad, pairs=pairs)
    tag = "edges:prep_input[%d,%d,%d,q%d,p%d]" % (B, T, N, quad, pairs)
    assert tuple(xyz.shape) == (B * T, N, 3) and tuple(feat.shape) == (B * T, N, 8)
    exact(tag + ":xyz", xyz, want[:, :, :3].contiguous())
    exact(tag + ":feat", feat[:, :, :k], want[:, :, 3:].contiguous())
    assert bool((feat[:, :, k:] == 0.0).all()), "an unused feature column is not exactly 0"
    assert float(xyz.abs().max()) < 1e3 and float(feat.abs().max()) < 1e3, "the time column reached the output"


# ---------------------------------------------------------------------------------------------
# Chamfer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(1, 1), (1, 300), (255, 257), (1024, 1025), (1025, 1024), (3000, 5)])
def test_chamfer_small_clouds_and_the_tile_edge(ops, n, m):
    """Clouds of one point and below one workgroup, the 1024-point LDS tile from both sides.  The LAST point of each cloud is made
    the nearest neighbour (distance 0) of a point of the other one, so a dropped partial tile cannot go unnoticed."""
    p, q = rnd(5000 + n, 2, n, 3, scale=0.5), rnd(9000 + m, 2, m, 3, scale=0.5)        # (seed ranges that never meet)
    if n > 2 and m > 2:
        q[:, m - 1] = p[:, n // 2]
        p[:, n - 1] = q[:, m // 2]
    d1, d2 = P.chamfer(p, q)
    g1, g2 = ops.chamfer_distance(p.to(DEV), q.to(DEV))
    exact("edges:chamfer_d1[%d,%d]" % (n, m), g1, d1)
    exact("edges:chamfer_d2[%d,%d]" % (n, m), g2, d2)
    if n > 2 and m > 2:
        assert bool((g1[:, n // 2] == 0.0).all()) and bool((g2[:, m // 2] == 0.0).all())
    s2, s1 = ops.chamfer_distance(q.to(DEV), p.to(DEV))                 # swapped clouds: the two outputs swap
    assert torch.equal(s1, g1) and torch.equal(s2, g2)
    z1, z2 = ops.chamfer_distance(p.to(DEV), p.to(DEV))
    assert float(z1.abs().max()) == 0.0 and float(z2.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------
# approximate EMD
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(1, 1), (1, 7), (5, 1), (37, 37), (100, 300), (255, 257), (64, 1000), (1000, 333), (1025, 1024)])
def test_emd_small_clouds_multipliers_and_the_tile_edge(ops, n, m):
    """Relative error to the oracle's f64 restatement within the project's 1e-4 (the f32 restatement of the same algorithm is within
    1.8e-7 of its f64 form on these inputs: the bound leaves the kernel's summation order two orders of magnitude, and a dropped
    tile or a wrong m / n multiplier moves the cost by percent)."""
    B = 2
    g = np.random.default_rng(n + m)
    p = torch.from_numpy(g.uniform(0, 1, (B, n, 3)).astype(np.float32))
    q = torch.from_numpy(g.uniform(0, 1, (B, m, 3)).astype(np.float32))
    want = O.approx_emd(p.double(), q.double())
    got = ops.earth_mover_distance(p.to(DEV), q.to(DEV), transpose=False)
    record("edges:emd_rel[%d,%d]" % (n, m), got.cpu().double() / want, torch.ones_like(want), 1e-4)     # |got / want - 1|: the relative error
    got_t = ops.earth_mover_distance(p.transpose(1, 2).contiguous().to(DEV), q.transpose(1, 2).contiguous().to(DEV))    # (b,3,n), emd.py:24
    assert torch.equal(got_t, got)


# ---------------------------------------------------------------------------------------------
# the two float-atomic backward entries
# ---------------------------------------------------------------------------------------------
def _scatter_ref(init, target, addend):
    """f64 index_add of addend (B,R,C) rows into init (B,P,C) at target (B,R) -> (want, bound).
    An entry receives cnt addends on top of its initial value, in ANY order (float atomics): every addend passes at most cnt
    additions and, where it is a product, one rounding of its own -> |err| <= (cnt + 1) u (|init| + sum |addend|)."""
    B, Pn, C = init.shape
    want, mag, cnt = init.double().clone(), init.double().abs().clone(), torch.zeros(B, Pn, dtype=torch.float64)
    for b in range(B):
        want[b].index_add_(0, target[b].long(), addend[b])
        mag[b].index_add_(0, target[b].long(), addend[b].abs())
        cnt[b].index_add_(0, target[b].long(), torch.ones(target.shape[1], dtype=torch.float64))
    return want, (cnt.unsqueeze(2) + 1) * U * mag, cnt


@pytest.mark.parametrize("C", [1, 3, 61, 64, 65, 512])
def test_three_interp_bwd_accumulates_within_its_rounding_bound(L, C):
    """dFeat[b, idx[b,i,k], :C] += w[b,i,k] dOut[b,i,:C]: the 64-lane column loop's tails, strides wider than C (NaN in the slack of
    dOut, a sentinel in the slack of dFeat that must survive), a non-zero dFeat to start from, a coarse point no fine point uses
    (keeps its value bit for bit), all fine points on ONE coarse point, three batch entries."""
    B, m, n = 3, 9, 70
    ldo, ldf = C + 5, C + 3
    dout, w = rnd(600 + C, B, n, C), rand_weights(601 + C, B, n)
    init = rnd(602 + C, B, m, C)
    for case in ("spread", "one_target"):
        idx = rand_idx(603 + C, m - 1, B, n, 3) if case == "spread" else torch.full((B, n, 3), 2, dtype=torch.int32)
        addend = (w.double().unsqueeze(3) * dout.double().unsqueeze(2)).reshape(B, n * 3, C)
        want, bound, cnt = _scatter_ref(init, idx.reshape(B, n * 3), addend)
        assert float(cnt[:, m - 1].max()) == 0 and (case == "spread" or float(cnt[:, 2].min()) == 3 * n)
        dfeat = _wide(init, ldf, 123.0).to(DEV)
        dout_d, idx_d, w_d = _wide(dout, ldo, NAN).to(DEV), idx.to(DEV), w.to(DEV)      # (named: they must outlive the launch)
        _check(L.caspr_three_interp_bwd_f32(_p(dout_d), ldo, _p(idx_d), _p(w_d), B, m, n, C, _p(dfeat), ldf, _stream()),
               "caspr_three_interp_bwd_f32")
        dfeat = dfeat.cpu()
        within("edges:three_interp_bwd[C%d,%s]" % (C, case), dfeat[:, :, :C], want, bound)
        assert bool((dfeat[:, :, C:] == 123.0).all()), "the slack of dFeat was written"
        assert torch.equal(dfeat[:, m - 1, :C], init[:, m - 1]), "a coarse point no fine point uses changed"


@pytest.mark.parametrize("C", [1, 3, 61, 64, 65, 512])
@pytest.mark.parametrize("ns", [1, 16])
def test_group_rows_bwd_accumulates_within_its_rounding_bound(L, C, ns):
    """dFeat[b, idx[b,j,s], :C] += dG[(b, j, s), 3 : 3 + C] -- the same cases; the addends are not products, the bound is kept."""
    B, n, M = 3, 11, 23
    ldg, ldf = 3 + C + 6, C + 3
    dG = rnd(700 + C + ns, B, M * ns, 3 + C)
    init = rnd(701 + C, B, n, C)
    for case in ("spread", "one_target"):
        idx = rand_idx(702 + C + ns, n - 1, B, M, ns) if case == "spread" else torch.full((B, M, ns), 4, dtype=torch.int32)
        want, bound, cnt = _scatter_ref(init, idx.reshape(B, M * ns), dG[:, :, 3:].double())
        assert float(cnt[:, n - 1].max()) == 0 and (case == "spread" or float(cnt[:, 4].min()) == M * ns)
        dfeat = _wide(init, ldf, 123.0).to(DEV)
        dG_d, idx_d = _wide(dG, ldg, NAN).to(DEV), idx.to(DEV)          # (named: they must outlive the launch)
        _check(L.caspr_group_rows_bwd_f32(_p(dG_d), ldg, _p(idx_d), B, n, M, C, ns, _p(dfeat), ldf, _stream()), "caspr_group_rows_bwd_f32")
        dfeat = dfeat.cpu()
        within("edges:group_rows_bwd[C%d,ns%d,%s]" % (C, ns, case), dfeat[:, :, :C], want, bound)
        assert bool((dfeat[:, :, C:] == 123.0).all()), "the slack of dFeat was written"
        assert torch.equal(dfeat[:, n - 1, :C], init[:, n - 1]), "a point no neighbourhood uses changed"


# ---------------------------------------------------------------------------------------------
# the Kaolin-named surface at every C mod 4
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 4, 5, 6, 7, 9])
@pytest.mark.parametrize("n,M,ns", [(64, 64, 1), (300, 50, 16)])
def test_kaolin_surface_forward(n, M, ns, C):
    """The forward checks of test_hip_parity.test_kaolin_compat_forward at every residue of C mod 4 (the binding pads rows to 4)."""
    from caspr_amd.compat import kaolin_amd as K
    B = 2
    tag = "edges:kaolin[%d,%d,%d,C%d]:" % (n, M, ns, C)
    pts = torch.cat([clouds(B, n, seed=3 + C), rnd(5 + C, B, n, C)], dim=2)
    with torch.no_grad():
        xyz, feat = K.separate_xyz_and_features(pts.to(DEV))
        wxyz, wfeat = P.separate_xyz_and_features(pts)
        exact(tag + "separate_feat", feat, wfeat)
        idx = K.furthest_point_sampling(xyz, M)
        widx = P.furthest_point_sampling(wxyz, M)
        exact(tag + "fps", idx, widx)
        new_xyz = K.fps_gather_by_index(xyz.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
        wnew = P.fps_gather_by_index(wxyz.transpose(1, 2).contiguous(), widx).transpose(1, 2).contiguous()
        exact(tag + "fps_gather", new_xyz, wnew)
        gi = torch.cat([widx.repeat(1, n // M + 1), widx[:, :7]], dim=1).contiguous()     # more rows than the cloud has points
        assert gi.shape[1] > n
        exact(tag + "gather_feat", K.fps_gather_by_index(feat, gi.to(DEV)), P.fps_gather_by_index(wfeat, gi))
        grouper = K.PointNet2GroupingLayer(0.1, ns, use_xyz_feature=True, use_random_ball_query=False)
        bidx = P.ball_query(0.1, ns, wxyz, wnew)
        g = grouper(xyz, new_xyz, feat)
        assert tuple(g.shape) == (B, M, 3 + C, ns)
        exact(tag + "grouping_layer", g, P.group(wxyz, wnew, wfeat, bidx))
        exact(tag + "grouping_layer_xyz_only", grouper(xyz, new_xyz, None), P.group(wxyz, wnew, None, bidx))
        dist, i3 = K.three_nn(xyz, new_xyz)
        wdist, wi3 = P.three_nn(wxyz, wnew)
        exact(tag + "three_nn_idx", i3, wi3)
        exact(tag + "three_nn_dist", dist, wdist)
        inv = 1.0 / (dist + 1e-8)
        w = inv / inv.sum(dim=2, keepdim=True)                          # pointnet2.py:516-518
        fprev = rnd(6 + C, B, C, M)
        out = K.three_interpolate(fprev.to(DEV), i3, w)
        assert tuple(out.shape) == (B, C, n)
        record(tag + "three_interpolate", out, P.three_interpolate(fprev, wi3, w.cpu()), 1e-6)


@pytest.mark.parametrize("C", [1, 4, 5, 6, 7, 9])
@pytest.mark.parametrize("n,M,ns", [(64, 64, 1), (300, 50, 16)])
def test_kaolin_surface_gradients(n, M, ns, C):
    """The gradient checks of test_hip_parity.test_kaolin_compat_gradients (same references, same bounds) at every C mod 4, with a
    gather of more rows than the cloud has points."""
    from caspr_amd.compat import kaolin_amd as K
    B = 2
    tag = "edges:kaolin[%d,%d,%d,C%d]:" % (n, M, ns, C)
    xyz = clouds(B, n, seed=4 + C)
    idx = P.furthest_point_sampling(xyz, M)
    new_xyz = torch.gather(xyz, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    feat = rnd(8 + C, B, C, n)
    # grouping layer
    f = feat.clone().to(DEV).requires_grad_(True)
    R = rnd(9 + C, B, M, 3 + C, ns)
    (K.PointNet2GroupingLayer(0.15, ns)(xyz.to(DEV), new_xyz.to(DEV), f) * R.to(DEV)).sum().backward()
    f6 = feat.double().requires_grad_(True)
    bidx = P.ball_query(0.15, ns, xyz, new_xyz)
    (P.group(xyz.double(), new_xyz.double(), f6, bidx) * R.double()).sum().backward()
    record(tag + "grouping_grad", f.grad, f6.grad, 1e-5 * float(f6.grad.abs().max()))
    # three_interpolate
    dist, i3 = P.three_nn(xyz, new_xyz)
    w = nn_weights(dist)
    fp = rnd(10 + C, B, C, M)
    a = fp.clone().to(DEV).requires_grad_(True)
    R2 = rnd(11 + C, B, C, n)
    (K.three_interpolate(a, i3.to(DEV), w.to(DEV)) * R2.to(DEV)).sum().backward()
    a6 = fp.double().requires_grad_(True)
    (P.three_interpolate(a6, i3, w.double()) * R2.double()).sum().backward()
    record(tag + "three_interpolate_grad", a.grad, a6.grad, 1e-5 * float(a6.grad.abs().max()))
    # fps_gather_by_index, more rows than points: every index repeats
    gi = torch.cat([idx.repeat(1, n // M + 1), idx[:, :7]], dim=1).contiguous()
    assert gi.shape[1] > n
    b = feat.clone().to(DEV).requires_grad_(True)
    R3 = rnd(12 + C, B, C, gi.shape[1])
    (K.fps_gather_by_index(b, gi.to(DEV)) * R3.to(DEV)).sum().backward()
    b6 = feat.double().requires_grad_(True)
    (P.fps_gather_by_index(b6, gi) * R3.double()).sum().backward()
    record(tag + "gather_grad", b.grad, b6.grad, 1e-6 * float(b6.grad.abs().max()))


def test_kaolin_grouper_without_features_and_with_differentiable_coordinates():
    """features=None: nothing to differentiate, no gradient comes back; a coordinate that requires grad: NotImplementedError, as the
    binding's docstring promises (never a silent None)."""
    from caspr_amd.compat import kaolin_amd as K
    B, n, M, C, ns = 2, 64, 16, 5, 4
    xyz = clouds(B, n, seed=77).to(DEV)
    new_xyz = xyz[:, :M].contiguous()
    feat = rnd(78, B, C, n).to(DEV)
    grouper = K.PointNet2GroupingLayer(0.2, ns)
    out = grouper(xyz, new_xyz, None)
    assert tuple(out.shape) == (B, M, 3, ns) and not out.requires_grad and out.grad_fn is None
    f = feat.clone().requires_grad_(True)
    out = grouper(xyz, new_xyz, f)
    assert out.requires_grad
    out.sum().backward()
    assert f.grad is not None and xyz.grad is None and new_xyz.grad is None
    for which in (0, 1):
        coords = [xyz.clone(), new_xyz.clone()]
        coords[which].requires_grad_(True)
        for feats in (feat.clone().requires_grad_(True), None):
            out = grouper(coords[0], coords[1], feats)
            with pytest.raises(NotImplementedError):
                out.sum().backward()
