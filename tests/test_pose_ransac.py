"""Correspondence RANSAC for the camera-pose evaluation (csrc/pose.hip, ops.ransac_rigid_from_correspondences,
utils/evaluations.test_observed_camera_pose_ransac; reference utils/evaluations.py:297-437).

The file carries a numpy f64 restatement of the whole algorithm -- the hash, Horn's estimate with the same Jacobi sweeps, the
scoring and the selection order -- written expression for expression as the kernel evaluates it (-ffp-contract=off).  The
non-GPU tests check that the restatement recovers planted poses and the demo frames' obj_T (tests/golden/pose_demo.npz); the
GPU tests hold the kernel to the restatement and to the same bounds."""
import os

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "pose_demo.npz")
THR = 0.015
SWEEPS = 8
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _mix(x):
    x = np.asarray(x, dtype=np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = ((x.astype(np.uint64) * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)   # uint32 product mod 2^32
    x = x ^ (x >> np.uint32(15))
    x = ((x.astype(np.uint64) * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return x ^ (x >> np.uint32(16))


def sample_indices(seed, f, K, n, N):
    """(K, n) indices of the hypotheses of frame f (csrc/pose.hip: pose_key / pose_mix)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = _mix(np.uint32(seed & 0xFFFFFFFF) ^ np.uint32(0x9E3779B9))
    x = _mix(x ^ np.uint32(seed >> 32))
    x = _mix(x ^ np.uint32(f))
    key = _mix(x ^ np.arange(K, dtype=np.uint32))
    idx = _mix(key[:, None] ^ np.arange(n, dtype=np.uint32)[None, :]) % np.uint32(N)
    return idx.astype(np.int64)


def horn(S, ca, cb):
    """S (H,3,3) = sum a b^T of the centred pairs, ca / cb (H,3) -> R (H,3,3), t (H,3) with b ~ R a + t."""
    sxx, sxy, sxz = S[:, 0, 0], S[:, 0, 1], S[:, 0, 2]
    syx, syy, syz = S[:, 1, 0], S[:, 1, 1], S[:, 1, 2]
    szx, szy, szz = S[:, 2, 0], S[:, 2, 1], S[:, 2, 2]
    H = S.shape[0]
    A = np.empty((H, 4, 4))
    A[:, 0, 0] = (sxx + syy) + szz
    A[:, 0, 1] = syz - szy
    A[:, 0, 2] = szx - sxz
    A[:, 0, 3] = sxy - syx
    A[:, 1, 1] = (sxx - syy) - szz
    A[:, 1, 2] = sxy + syx
    A[:, 1, 3] = szx + sxz
    A[:, 2, 2] = (syy - sxx) - szz
    A[:, 2, 3] = syz + szy
    A[:, 3, 3] = (szz - sxx) - syy
    for i, j in PAIRS:
        A[:, j, i] = A[:, i, j]
    V = np.broadcast_to(np.eye(4), (H, 4, 4)).copy()
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q in PAIRS:
                apq = A[:, p, q].copy()
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0.0, -t, t)
                t = np.where(apq != 0.0, t, 0.0)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                c, s = c[:, None], s[:, None]
                akp, akq = A[:, :, p].copy(), A[:, :, q].copy()
                A[:, :, p] = c * akp - s * akq
                A[:, :, q] = s * akp + c * akq
                apk, aqk = A[:, p, :].copy(), A[:, q, :].copy()
                A[:, p, :] = c * apk - s * aqk
                A[:, q, :] = s * apk + c * aqk
                vkp, vkq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = c * vkp - s * vkq
                V[:, :, q] = s * vkp + c * vkq
    best = A[:, 0, 0].copy()
    qv = V[:, :, 0].copy()
    for k in range(1, 4):
        b = A[:, k, k] > best
        best = np.where(b, A[:, k, k], best)
        qv = np.where(b[:, None], V[:, :, k], qv)
    w, x, y, z = qv[:, 0], qv[:, 1], qv[:, 2], qv[:, 3]
    nrm = np.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
    ww, xx, yy, zz = w * w, x * x, y * y, z * z
    R = np.empty((H, 3, 3))
    R[:, 0, 0] = ((ww + xx) - yy) - zz
    R[:, 0, 1] = 2.0 * (x * y - w * z)
    R[:, 0, 2] = 2.0 * (x * z + w * y)
    R[:, 1, 0] = 2.0 * (x * y + w * z)
    R[:, 1, 1] = ((ww - xx) + yy) - zz
    R[:, 1, 2] = 2.0 * (y * z - w * x)
    R[:, 2, 0] = 2.0 * (x * z - w * y)
    R[:, 2, 1] = 2.0 * (y * z + w * x)
    R[:, 2, 2] = ((ww - xx) - yy) + zz
    t = np.empty((H, 3))
    for i in range(3):
        t[:, i] = cb[:, i] - ((R[:, i, 0] * ca[:, 0] + R[:, i, 1] * ca[:, 1]) + R[:, i, 2] * ca[:, 2])
    return R, t


def estimate(a, b):
    """Hypotheses from sampled pairs a, b (H,n,3) f64: centroids summed in draw order, S summed in draw order."""
    n = a.shape[1]
    ca, cb = np.zeros((a.shape[0], 3)), np.zeros((a.shape[0], 3))
    for j in range(n):
        ca = ca + a[:, j]
        cb = cb + b[:, j]
    ca, cb = ca / float(n), cb / float(n)
    S = np.zeros((a.shape[0], 3, 3))
    for j in range(n):
        da, db = a[:, j] - ca, b[:, j] - cb
        S = S + da[:, :, None] * db[:, None, :]
    return horn(S, ca, cb)


def residual2(R, t, src, dst):
    """R (H,3,3), t (H,3), src / dst (N,3) f64 -> d2 (H,N) in the kernel's order."""
    sx, sy, sz = src[None, :, 0], src[None, :, 1], src[None, :, 2]
    r = [(((R[:, i, 0:1] * sx + R[:, i, 1:2] * sy) + R[:, i, 2:3] * sz) + t[:, i:i + 1]) - dst[None, :, i] for i in range(3)]
    return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]


def score(R, t, src, dst, thr2, chunk=256):
    """-> inlier counts (H,), rmse (H,): d2 accumulated in index order, as one lane of the kernel does."""
    cnt, rm = np.empty(R.shape[0], np.int64), np.empty(R.shape[0])
    for h0 in range(0, R.shape[0], chunk):
        d2 = residual2(R[h0:h0 + chunk], t[h0:h0 + chunk], src, dst)
        inl = d2 < thr2
        c = inl.sum(1)
        s = np.cumsum(np.where(inl, d2, 0.0), axis=1)[:, -1]
        cnt[h0:h0 + chunk] = c
        with np.errstate(invalid="ignore", divide="ignore"):
            rm[h0:h0 + chunk] = np.where(c > 0, np.sqrt(s / np.maximum(c, 1)), 0.0)
    return cnt, rm


def ransac_ref(src, dst, threshold=THR, K=5000, n=4, seed=0, refine=False):
    """The whole algorithm for src, dst (F,N,3) (f32 or f64; widened exactly) -> dict of T (F,4,4), inliers, rmse, best and
    near (F,): the number of correspondences whose residual under the returned T lies within 1e-9 of the threshold."""
    src, dst = np.asarray(src, np.float64)[..., :3], np.asarray(dst, np.float64)[..., :3]
    F, N = src.shape[:2]
    thr2 = float(threshold) * float(threshold)
    out = {k: [] for k in ("T", "inliers", "rmse", "best", "near", "counts")}
    for f in range(F):
        idx = sample_indices(seed, f, K, n, N)
        R, t = estimate(src[f][idx], dst[f][idx])
        cnt, rm = score(R, t, src[f], dst[f], thr2)
        h = int(np.lexsort((np.arange(K), rm, -cnt))[0])
        Rw, tw, cw, rw = R[h], t[h], int(cnt[h]), float(rm[h])
        if refine and cw >= 3:
            inl = residual2(Rw[None], tw[None], src[f], dst[f])[0] < thr2
            a, b = src[f][inl], dst[f][inl]
            ca, cb = a.sum(0) / cw, b.sum(0) / cw
            S = (a - ca).T @ (b - cb)
            Rr, tr = horn(S[None], ca[None], cb[None])
            Rw, tw = Rr[0], tr[0]
            c2, r2 = score(Rr, tr, src[f], dst[f], thr2)
            cw, rw = int(c2[0]), float(r2[0])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rw, tw
        d = np.sqrt(residual2(Rw[None], tw[None], src[f], dst[f])[0])
        for k, v in (("T", T), ("inliers", cw), ("rmse", rw), ("best", h), ("near", int((np.abs(d - threshold) <= 1e-9).sum())),
                     ("counts", cnt)):
            out[k].append(v)
    return {k: np.array(v) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------
def random_rotation(rng):
    q = rng.randn(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def planted_frames(F, N, seed=0, sigma=0.003, outliers=0.4):
    """Rigid frames: src in the centred unit cube (as T-NOCS - 0.5), dst = R src + t + N(0, sigma^2) with a fraction of the
    correspondences replaced by uniform points of the same extent.  -> src, dst (F,N,3) f32, R (F,3,3), t (F,3)."""
    rng = np.random.RandomState(seed)
    src = rng.rand(F, N, 3) - 0.5
    Rs = np.stack([random_rotation(rng) for _ in range(F)])
    ts = rng.randn(F, 3) * 0.5 + np.array([0.0, 0.0, 2.0])
    dst = np.einsum("fij,fnj->fni", Rs, src) + ts[:, None, :] + rng.randn(F, N, 3) * sigma
    bad = rng.rand(F, N) < outliers
    junk = rng.rand(F, N, 3) - 0.5 + ts[:, None, :]
    dst = np.where(bad[..., None], junk, dst)
    return src.astype(np.float32), dst.astype(np.float32), Rs, ts


def pose_errors(T, R, t):
    """-> rotation error (deg), translation error, as evaluations.py:426-430."""
    T = np.asarray(T)
    cosang = np.clip((np.einsum("...ji,...ji->...", T[..., :3, :3], R) - 1.0) / 2.0, -1.0, 1.0)
    return np.degrees(np.arccos(cosang)), np.linalg.norm(T[..., :3, 3] - t, axis=-1)


def demo_fixture():
    d = np.load(FIXTURE)
    return (d["nocs"] - np.float32(0.5)).astype(np.float32), d["depth"], d["obj_T"]


# bounds on the demo frames (ground-truth NOCS -> depth, 5000 hypotheses, seed 0), set with a margin from the restatement's own
# numbers (test_restatement_recovers_demo_poses prints them): winner rot <= 1.00 deg, trans <= 11.2 mm; refit rot <= 0.20 deg,
# trans <= 3.4 mm
DEMO_ROT, DEMO_TRANS = 1.5, 0.02
DEMO_ROT_REFINE, DEMO_TRANS_REFINE = 0.3, 0.006


# ---------------------------------------------------------------------------------------------------------------------------
# non-GPU: the restatement itself
# ---------------------------------------------------------------------------------------------------------------------------
def test_hash_is_stable_uint32():
    """The counter hash in numpy: indices in range, a function of (seed, frame, hypothesis, draw) only, seeds differ."""
    a = sample_indices(0, 0, 1000, 4, 2048)
    assert a.shape == (1000, 4) and a.min() >= 0 and a.max() < 2048
    assert np.array_equal(a, sample_indices(0, 0, 1000, 4, 2048))
    assert np.array_equal(a[:10], sample_indices(0, 0, 10, 4, 2048))
    assert not np.array_equal(a, sample_indices(1, 0, 1000, 4, 2048))
    assert not np.array_equal(a, sample_indices(0, 1, 1000, 4, 2048))
    assert not np.array_equal(a, sample_indices(1 << 32, 0, 1000, 4, 2048))
    # near uniform over the indices (chi-square-ish sanity)
    hist = np.bincount(sample_indices(7, 3, 50000, 4, 97).ravel(), minlength=97)
    assert hist.min() > 0.8 * hist.mean() and hist.max() < 1.2 * hist.mean()


def test_horn_exact_and_degenerate():
    rng = np.random.RandomState(3)
    R0 = np.stack([random_rotation(rng) for _ in range(64)])
    t0 = rng.randn(64, 3)
    a = rng.rand(64, 5, 3) - 0.5
    b = np.einsum("hij,hnj->hni", R0, a) + t0[:, None]
    R, t = estimate(a, b)
    assert np.abs(R - R0).max() < 1e-12 and np.abs(t - t0).max() < 1e-12
    assert np.allclose(np.linalg.det(R), 1.0, atol=1e-12)
    # repeated, collinear and identical samples: finite, a rotation
    deg = np.zeros((3, 4, 3))
    deg[0] = a[0, 0]
    deg[1] = np.linspace(0, 1, 4)[:, None] * np.array([1.0, 2.0, 3.0])
    deg[2, :2], deg[2, 2:] = a[1, 0], a[1, 1]
    R, t = estimate(deg, deg + 0.25)
    assert np.isfinite(R).all() and np.isfinite(t).all()
    assert np.allclose(np.einsum("hji,hjk->hik", R, R), np.eye(3), atol=1e-12)
    assert np.abs(R[0] - np.eye(3)).max() == 0.0


def test_restatement_recovers_planted_pose():
    src, dst, Rs, ts = planted_frames(2, 2048, seed=5)
    for refine, rot_b, tr_b in ((False, 0.5, 0.005), (True, 0.2, 0.002)):
        r = ransac_ref(src, dst, K=2000, refine=refine)
        rot, tr = pose_errors(r["T"], Rs, ts)
        print("planted refine=%d: rot %s deg, trans %s m, inliers %s" % (refine, rot, tr, r["inliers"]))
        assert (rot < rot_b).all() and (tr < tr_b).all(), (rot, tr)
        assert (r["inliers"] > 0.5 * 2048).all()


def test_restatement_recovers_demo_poses():
    src, dst, obj_T = demo_fixture()
    for refine, rot_b, tr_b in ((False, DEMO_ROT, DEMO_TRANS), (True, DEMO_ROT_REFINE, DEMO_TRANS_REFINE)):
        r = ransac_ref(src, dst, refine=refine)
        rot, tr = pose_errors(r["T"], obj_T[:, :3, :3], obj_T[:, :3, 3])
        print("demo refine=%d: rot %s deg, trans %s m, inliers %s" % (refine, np.round(rot, 3), np.round(tr, 4), r["inliers"]))
        assert (rot < rot_b).all() and (tr < tr_b).all(), (rot, tr)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _op(src, dst, **kw):
    import torch
    from caspr_amd import ops
    dev = torch.device("cuda")
    out = ops.ransac_rigid_from_correspondences(torch.from_numpy(np.ascontiguousarray(src)).to(dev),
                                                torch.from_numpy(np.ascontiguousarray(dst)).to(dev), **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _with_stride(x, rs):
    if rs == 3:
        return x
    return np.concatenate([x, np.full(x.shape[:-1] + (1,), 7.0, np.float32)], axis=-1)


def _assert_matches(got, ref, tag):
    T, fitness, rmse, inl, best = got
    assert np.array_equal(best, ref["best"]), (tag, best, ref["best"])
    dif = np.abs(inl.astype(np.int64) - ref["inliers"])
    assert (dif <= ref["near"]).all(), (tag, inl, ref["inliers"], ref["near"])
    assert np.abs(T - ref["T"]).max() <= 1e-9, (tag, np.abs(T - ref["T"]).max())
    same = dif == 0
    assert np.abs(rmse - ref["rmse"])[same].max(initial=0.0) <= 1e-9, (tag, rmse, ref["rmse"])
    assert np.isfinite(T).all() and np.isfinite(fitness).all()


_REF_CACHE = {}


def _ref_cached(key, src, dst, **kw):
    if key not in _REF_CACHE:
        _REF_CACHE[key] = ransac_ref(src, dst, **kw)
    return _REF_CACHE[key]


PARITY_CASES = [  # (N, K, row_stride, n, refine)
    (2048, 5000, 4, 4, False),
    (2048, 5000, 3, 4, True),
    (1000, 777, 3, 3, False),
    (1000, 777, 4, 3, True),
    (4100, 300, 4, 6, False),
    (4100, 300, 3, 6, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,rs,n,refine", PARITY_CASES)
def test_gpu_matches_restatement(N, K, rs, n, refine):
    src, dst, _, _ = planted_frames(8, N, seed=N + K)
    ref = _ref_cached((N, K, n, refine), src, dst, K=K, n=n, seed=11, refine=refine)
    got = _op(_with_stride(src, rs), _with_stride(dst, rs), num_hypotheses=K, sample_size=n, seed=11, refine=refine)
    _assert_matches(got, ref, (N, K, rs, n, refine))
    T, fitness, rmse, inl, best = got
    assert np.array_equal(fitness, inl / float(N))
    assert best.dtype == np.int32 and inl.dtype == np.int32 and T.dtype == np.float64 and T.shape == (8, 4, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("refine", [False, True])
def test_gpu_recovers_planted_pose(refine):
    src, dst, Rs, ts = planted_frames(8, 2048, seed=21)
    T, fitness, rmse, inl, best = _op(src, dst, refine=refine)
    rot, tr = pose_errors(T, Rs, ts)
    rot_b, tr_b = (0.2, 0.002) if refine else (0.5, 0.005)
    assert (rot < rot_b).all() and (tr < tr_b).all(), (rot, tr)
    assert (fitness > 0.5).all() and (rmse > 0).all() and (rmse < THR).all()


@pytest.mark.gpu
@pytest.mark.parametrize("refine", [False, True])
def test_gpu_demo_frames(refine):
    src, dst, obj_T = demo_fixture()
    got = _op(src, dst, refine=refine)
    rot, tr = pose_errors(got[0], obj_T[:, :3, :3], obj_T[:, :3, 3])
    print("GPU demo refine=%d: rot %s deg, trans %s m" % (refine, np.round(rot, 3), np.round(tr, 4)))
    if refine:
        assert (rot < DEMO_ROT_REFINE).all() and (tr < DEMO_TRANS_REFINE).all(), (rot, tr)
    else:
        assert (rot < DEMO_ROT).all() and (tr < DEMO_TRANS).all(), (rot, tr)
    _assert_matches(got, _ref_cached(("demo", refine), src, dst, refine=refine), ("demo", refine))


@pytest.mark.gpu
def test_gpu_deterministic_and_stream_independent():
    import torch
    from caspr_amd import ops
    src, dst, _, _ = planted_frames(16, 2048, seed=3)
    s, d = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    a = [o.cpu() for o in ops.ransac_rigid_from_correspondences(s, d, seed=5, refine=True)]
    side = torch.cuda.Stream()
    other = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        b = ops.ransac_rigid_from_correspondences(s, d, seed=5, refine=True)
    for _ in range(4):
        other = other @ other.T / 4096.0     # another launch beside it on the default stream
    torch.cuda.synchronize()
    b = [o.cpu() for o in b]
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = [o.cpu() for o in ops.ransac_rigid_from_correspondences(s, d, seed=6, refine=True)]
    assert not torch.equal(a[4], c[4])       # another seed draws other hypotheses


@pytest.mark.gpu
def test_gpu_degenerate_and_bad_arguments():
    import torch
    from caspr_amd import ops
    F, N = 3, 300
    src = np.zeros((F, N, 3), np.float32)
    src[0] = 0.25                                                   # all identical
    src[1] = np.linspace(-0.5, 0.5, N, dtype=np.float32)[:, None] * np.array([1, 2, 3], np.float32)   # collinear
    src[2, :, 0] = np.linspace(-0.5, 0.5, N)                        # collinear on an axis
    dst = src + np.float32(0.1)
    for refine in (False, True):
        T, fitness, rmse, inl, best = _op(src, dst, num_hypotheses=200, refine=refine)
        assert np.isfinite(T).all() and np.isfinite(rmse).all() and np.isfinite(fitness).all()
        Rm = T[:, :3, :3]
        assert np.allclose(np.einsum("fji,fjk->fik", Rm, Rm), np.eye(3), atol=1e-9)
    s = torch.zeros(2, 5, 3, device="cuda")
    with pytest.raises(ValueError):
        ops.ransac_rigid_from_correspondences(s[:, :3], s[:, :3], sample_size=4)      # N < n
    for kw in ({"sample_size": 2}, {"sample_size": 9}, {"threshold": 0.0}, {"threshold": -1.0}, {"threshold": float("nan")},
               {"num_hypotheses": 0}):
        with pytest.raises(ValueError):
            ops.ransac_rigid_from_correspondences(s, s, **kw)
    with pytest.raises(ValueError):
        ops.ransac_rigid_from_correspondences(s, torch.zeros(2, 6, 3, device="cuda"))
    # the C entry's own checks, through lib.check
    from caspr_amd import lib
    L = lib.load()
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    outs = [torch.empty(16, dtype=torch.float64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"),
            torch.empty(1, dtype=torch.float64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")]
    p = [ops._p(o) for o in outs]
    for args in ((1, 5, 5, 10, 4, 0.01), (1, 5, 3, 10, 4, -1.0), (1, 3, 3, 10, 4, 0.01), (1, 5, 3, 0, 4, 0.01)):
        F_, N_, rs, K_, n_, thr = args
        rc = L.caspr_pose_ransac_f32(ops._p(s), ops._p(s), F_, N_, rs, K_, n_, thr, 0, 0, p[0], p[1], p[2], p[3], ops._p(ws), ws.numel(), ops._stream())
        with pytest.raises(lib.CasprHipError):
            lib.check(rc, "caspr_pose_ransac_f32")


@pytest.mark.gpu
def test_gpu_protocol_evaluation(seeded_sd):
    import torch
    from caspr_amd.models import CaSPR
    from caspr_amd.utils import evaluations as E
    dev = torch.device("cuda")
    m = CaSPR()
    m.load_state_dict(seeded_sd)
    m = m.to(dev).eval()
    B, T_, N = 2, 10, 2048
    rng = np.random.RandomState(9)
    nocs = rng.rand(B, T_, N, 3).astype(np.float32)
    pose = np.zeros((B, T_, 4, 4))
    for b in range(B):
        for s in range(T_):
            pose[b, s, :3, :3] = random_rotation(rng)
            pose[b, s, :3, 3] = rng.randn(3) * 0.3 + np.array([0, 0, 2.0])
            pose[b, s, 3, 3] = 1.0
    xyz = np.einsum("btij,btnj->btni", pose[..., :3, :3], nocs.astype(np.float64) - 0.5) + pose[:, :, None, :3, 3]
    tcol = np.broadcast_to((np.arange(T_) / (T_ - 1.0))[None, :, None, None], (B, T_, N, 1))
    pcl_in = torch.from_numpy(np.concatenate([xyz, 5.0 * tcol], -1).astype(np.float32))
    nocs_out = torch.from_numpy(np.concatenate([nocs, tcol], -1).astype(np.float32))
    pose_t = torch.from_numpy(pose)
    res = E.test_observed_camera_pose_ransac(m, [(pcl_in, nocs_out, pose_t)], dev, seed=3)
    # the same op call on the same predicted T-NOCS, then the reference formulas (evaluations.py:380-437) in numpy
    from caspr_amd import ops
    with torch.no_grad():
        _, pred = m.encode(pcl_in.to(dev))
    Tp = ops.ransac_rigid_from_correspondences((pred - 0.5).reshape(B * T_, N, -1), pcl_in.to(dev).reshape(B * T_, N, 4), seed=3)[0].cpu().numpy()
    trans, rot, point, point_mean = [], [], [], []
    for b in range(B):
        gt_nocs = (nocs_out[b, :, :, :3] - 0.5).numpy()
        inp = pcl_in[b, :, :, :3].numpy()
        for s in range(T_):
            Tf = Tp[b * T_ + s]
            Rp, tp = Tf[:3, :3], Tf[:3, 3]
            Rg, tg = pose[b, s, :3, :3], pose[b, s, :3, 3]
            pred_depth = np.dot(Rp, gt_nocs[s].T).T + tp
            d = np.linalg.norm(pred_depth - inp[s], axis=1)
            point.append(np.median(d))
            point_mean.append(np.mean(d))
            trans.append(np.linalg.norm(tp - tg))
            rot.append(np.degrees(np.arccos(np.clip((np.trace(np.dot(Rp.T, Rg)) - 1.0) / 2.0, -1.0, 1.0))))
    for k, want in (("trans", trans), ("rot", rot), ("point", point), ("point_mean", point_mean)):
        got = np.asarray(res["per_frame"][k])
        assert got.shape == (B * T_,)
        assert np.abs(got - np.asarray(want)).max() <= 1e-6, (k, got, want)
        assert abs(res[k]["mean"] - np.mean(want)) <= 1e-6 and abs(res[k]["median"] - np.median(want)) <= 1e-6
        assert np.allclose(res["per_sequence"][k], np.asarray(want).reshape(B, T_).mean(1), atol=1e-6, rtol=0)
    with pytest.raises(ValueError):
        E.test_observed_camera_pose_ransac(m, [(pcl_in[:, :5], nocs_out[:, :5], pose_t[:, :5])], dev)
    with pytest.raises(ValueError):
        E.test_observed_camera_pose_ransac(m, [(pcl_in[:, :, :1024], nocs_out[:, :, :1024], pose_t)], dev)
