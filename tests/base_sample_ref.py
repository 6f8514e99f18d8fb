"""CPU restatement of the device base sampler (csrc/base_sample.hip, ops.base_samples): Philox4x32-10, the uniform mapping,
Box-Muller, the truncation rule and the contour rule, in numpy with f64 arithmetic and f64 transcendentals.  A helper module of
tests/test_base_sample.py, not a test file.

It states the MATHEMATICAL definition -- u = ((x >> 8) + 0.5) 2^-24, normals r cos(2 pi u'), r sin(2 pi u') with
r = sqrt(-2 ln u) -- not the kernel's f32 evaluation order; the kernel is held to it within a measured tolerance, and to the
integer parts (words, chosen candidate, contour index) exactly."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr (..., 4), key (..., 2) uint32 (broadcastable) -> (..., 4) uint32.  The products in uint64."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.asarray(key[..., 0], dtype=np.uint64), np.asarray(key[..., 1], dtype=np.uint64)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def words(seed, draw, frame_ids, n, block=0):
    """(F, n, 4) uint32: the Philox block `block` of every point.  key = (seed lo, seed hi); counter = (point, frame id lo,
    frame id hi, (draw << 4) | block)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    fid = np.asarray([int(f) & 0xFFFFFFFFFFFFFFFF for f in frame_ids], dtype=np.uint64)
    F = fid.shape[0]
    ctr = np.empty((F, n, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(n, dtype=np.uint32)[None, :]
    ctr[..., 1] = (fid & MASK).astype(np.uint32)[:, None]
    ctr[..., 2] = (fid >> np.uint64(32)).astype(np.uint32)[:, None]
    ctr[..., 3] = np.uint32(((int(draw) << 4) | int(block)) & 0xFFFFFFFF)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    return philox4x32_10(ctr, key)


def uniform(x):
    """u = ((x >> 8) + 0.5) 2^-24 in f64 (exact): never 0 or 1."""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def normals(w):
    """(..., 4) words -> (..., 4) normals: words (0, 1) -> c0, c1; words (2, 3) -> c2, c3."""
    u = uniform(w)
    out = np.empty(u.shape, dtype=np.float64)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[..., a]))
        th = 2.0 * np.pi * u[..., a + 1]
        out[..., a], out[..., a + 1] = r * np.cos(th), r * np.sin(th)
    return out


def gaussian(seed, draw, frame_ids, n):
    """-> y (F, n, 3) f64."""
    return normals(words(seed, draw, frame_ids, n))[..., :3]


def truncated(seed, draw, frame_ids, n, trunc_std):
    """-> y (F, n, 3), chosen candidate index (F, n, 3), candidates (F, n, 3, 4): component c takes block c; the first candidate
    with |c| < trunc_std wins, candidate 0 if none qualifies."""
    cand = np.stack([normals(words(seed, draw, frame_ids, n, block=c)) for c in range(3)], axis=2)
    inside = np.abs(cand) < trunc_std
    chosen = np.where(inside.any(axis=-1), inside.argmax(axis=-1), 0)
    return np.take_along_axis(cand, chosen[..., None], axis=-1)[..., 0], chosen, cand


def contour_index(n, R):
    """Point -> contour: the first R - 1 contours get n // R points each, the last the rest."""
    per = n // R
    return np.minimum(np.arange(n) // per, R - 1) if per > 0 else np.full(n, R - 1)


def contours(seed, draw, frame_ids, n, radii):
    """-> y (F, n, 3) f64, contour index (n,): radius * cube / |cube| with cube = 2 u - 1 of words 0..2 of block 0."""
    cube = 2.0 * uniform(words(seed, draw, frame_ids, n)[..., :3]) - 1.0
    idx = contour_index(n, len(radii))
    # the radii as the device holds them (f32)
    r = np.asarray(radii, dtype=np.float32).astype(np.float64)[idx]
    return r[None, :, None] * cube / np.linalg.norm(cube, axis=-1, keepdims=True), idx
