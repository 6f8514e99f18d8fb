"""The POOLED GroupNorm statistics of the head's first conv (ops.conv1x1_gn(..., pool=T); tpointnet2.py: 576 -> 1600 over frames, statistics
per sequence) on every route, op by op against f64:

  h3w      caspr_conv1x1_h3w_pooled_f32            conv_split = "f16x3" (inference default)
  x6w      caspr_conv1x1_x6w_pooled_f32            conv_split = "bf16x6" (training tier)
  x6       caspr_conv1x1_gn_pooled_bf16x6_f32      CONV_X6W = False, or a layer under the 512-channel kernel's thresholds
  beside   ops.conv1x1_gn_tail_beside              the remainder's pass on a second stream, then caspr_conv_gn_finalize_f32(..., pool)
  fallback conv1x1 + gn_stats over a (B / pool, pool * P, ld) view     P % 128 != 0, or f32 mode

The suite reached these through the whole encoder only (test_head_fold_matches_the_separate_last_layer).  Here the frames of a sequence get
different in_scale / in_shift rows and a per-entry bias spread over +-3, so "statistics per entry, then averaged" is 23-82 % off in the
variance (test_discrimination), and the shapes are the smallest at which a path changes: a 48- / 64-channel remainder on the tail kernel,
a remainder above 64 channels on the 256-channel kernel (192; 132, ragged against 16 and 64), an odd tile count, pool == B, and the three
regimes of conv_gn_finalize_kernel by channels per group (several tile lanes per channel, one lane, the serial branch above 256) plus more
tile lanes than tiles.

Reference: plain f64 torch -- relu(x * in_scale[b] + in_shift[b]) @ W^T + bias + bbias[b], F.group_norm of its (B / pool, pool * P, C) view.
Bounds are those of test_conv1x1_gn_fused / test_conv1x1_x6w_kernel (2e-6 max(1, |y|max) on the output, 5e-6 on the applied normalisation,
2e-6 / 5e-6 / 5e-6 on mean / rstd / pmax, the mean's relative to its size); the CPU tests keep them a statement about the kernel: the f32
torch evaluation of the same graph stays within half the bound (test_conditioning).  Every measured error lands in test_hip_parity's JSON
report under "pooled:...".
"""
import contextlib
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_parity import REPORT, exact, record, rnd

gpu = pytest.mark.gpu
EPS = 1e-5
APPLY_TOL = 5e-6          # test_conv1x1_gn_fused's bound on the applied normalisation
LARGE_MEAN_TOL = 5e-4     # test_conv1x1_gn_fused_large_mean's (one f32 rounding of shift ~ 1e3)

# (B, pool, P, Cin, Cout, groups)
CASES = {
    "1": (6, 3, 128, 256, 560, 16),      # two sequences of three one-tile frames; 48-channel remainder on the tail kernel
    "2": (3, 3, 128, 256, 560, 16),      # pool == B; odd tile count: the tail kernel's last workgroup holds one tile
    "3": (4, 2, 256, 256, 1088, 16),     # two channel tiles + 64-channel remainder, two point tiles per entry; cpg = 68: 3 tile lanes per channel
    "4": (4, 2, 128, 256, 704, 16),      # remainder of 192 on the 256-channel kernel
    "5": (4, 2, 128, 256, 644, 4),       # remainder of 132 (ragged against 16 and 64); cpg = 161: one tile lane
    "6": (4, 4, 128, 256, 1088, 4),      # cpg = 272 > 256: the finalize's serial branch, pmax included
    "7": (4, 2, 384, 64, 128, 16),       # route x6 only: the narrowest layer the fused route accepts; cpg = 8: 32 tile lanes against 6 tiles
    "8": (6, 3, 200, 256, 560, 16),      # fallback only: P % 128 != 0
    "large_mean": (4, 2, 256, 512, 512, 16),
}
SEEDS = {}      # case -> seed offset, should test_conditioning ever need another draw (none does)
MAIN = ("1", "2", "3", "4", "5", "6")
ROUTE_CASES = [(r, k) for r in ("h3w", "x6w", "x6") for k in MAIN] + [("x6", "7")]


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def side(dev):
    """ONE side stream for the whole module: every torch.cuda.Stream() takes the next of the runtime's pooled streams, and the tests
    behind this file should find that pool where they found it before."""
    return torch.cuda.Stream(device=dev)


@pytest.fixture()
def ops():
    """caspr_amd.ops with the persistent kernel's thresholds lowered to the test shapes; the route switches restored afterwards."""
    from caspr_amd import ops as _ops
    _ops.check_deferred_errors()
    saved = (_ops._X6W_MIN_CIN, _ops._X6W_MIN_ROWS, _ops.CONV_X6W, _ops.CONV_SPLIT)
    mode = _ops.matmul_mode()["conv"] == "bf16x6"
    _ops._X6W_MIN_CIN, _ops._X6W_MIN_ROWS, _ops.CONV_X6W, _ops.CONV_SPLIT = 32, 128, True, "f16x3"
    _ops.set_matmul_mode(conv=True)
    try:
        yield _ops
        _ops.check_deferred_errors()
    finally:
        _ops._X6W_MIN_CIN, _ops._X6W_MIN_ROWS, _ops.CONV_X6W, _ops.CONV_SPLIT = saved
        _ops.set_matmul_mode(conv=mode)


@contextlib.contextmanager
def _route(ops, route):
    """Select the kernels of one route for the calls inside."""
    saved = (ops.CONV_X6W, ops.CONV_SPLIT, ops.matmul_mode()["conv"] == "bf16x6")
    ops.CONV_X6W, ops.CONV_SPLIT = {"h3w": (True, "f16x3"), "x6w": (True, "bf16x6"), "x6": (False, "bf16x6"), "f32": (True, "f16x3")}[route]
    ops.set_matmul_mode(conv=route != "f32")
    try:
        yield
    finally:
        ops.CONV_X6W, ops.CONV_SPLIT = saved[:2]
        ops.set_matmul_mode(conv=saved[2])


# ---------------------------------------------------------------------------------------------
# inputs and the f64 reference (computed once per case, never modified)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(key):
    B, pool, P_, Cin, Cout, G = CASES[key]
    s = SEEDS.get(key, 0)
    x = rnd(s + Cin + Cout, B, P_, Cin)
    gamma, beta = rnd(s + 6, Cout) * 0.2 + 1.0, rnd(s + 7, Cout) * 0.1
    gamma[::7] *= -1.0          # negative scales: pmax needs the min branch
    if key == "large_mean":     # |mean| / sigma ~ 800 per group, the frames of a sequence 0.02 ~ one sigma apart
        w = rnd(s + 1, Cout, Cin, scale=0.02 / np.sqrt(Cin))
        b = rnd(s + 2, Cout, scale=0.01) + 20.0
        bb = (0.02 * (torch.arange(B) % pool).float()).unsqueeze(1).expand(B, Cout).contiguous()
        sc_in = sh_in = None
    else:                       # every frame its own producer scale / shift and a bias offset spread over +-3
        w = rnd(s + 1, Cout, Cin, scale=1.0 / np.sqrt(Cin))
        b = rnd(s + 2, Cout, scale=0.3)
        bb = rnd(s + 3, B, Cout, scale=0.1) + 3.0 * torch.linspace(-1, 1, B).unsqueeze(1)
        sc_in, sh_in = rnd(s + 4, B, Cin).abs() + 0.5, rnd(s + 5, B, Cin)
    return dict(w=w, b=b, bb=bb, x=x, sc_in=sc_in, sh_in=sh_in, gamma=gamma, beta=beta)


def _conv(I, dtype):
    x = I["x"].to(dtype)
    if I["sc_in"] is not None:
        x = torch.relu(x * I["sc_in"].to(dtype).unsqueeze(1) + I["sh_in"].to(dtype).unsqueeze(1))
    return x @ I["w"].to(dtype).t() + I["b"].to(dtype) + I["bb"].to(dtype).unsqueeze(1)


def _moments(y, pool, G):
    """y (B, P, C) -> mean, biased variance (B / pool, G) over pool consecutive entries, in y's precision."""
    B, P_, C = y.shape
    m = y.reshape(B // pool, pool * P_, G, C // G).transpose(1, 2).reshape(B // pool, G, -1)
    return m.mean(dim=2), m.var(dim=2, unbiased=False)


def _scale_shift(mean, var, gamma, beta, G):
    rstd = 1.0 / torch.sqrt(var + EPS)
    sc = gamma * rstd.repeat_interleave(gamma.numel() // G, dim=1)
    return sc, beta - mean.repeat_interleave(gamma.numel() // G, dim=1) * sc


def _apply(y64, sc, sh):
    """scale / shift (B / pool, C) broadcast over their sequence's pool * P rows of y64 (B, P, C) -> (B, P, C) in f64."""
    B, P_, C = y64.shape
    Bs = sc.shape[0]
    return (y64.view(Bs, -1, C) * sc.double().unsqueeze(1) + sh.double().unsqueeze(1)).view(B, P_, C)


@functools.lru_cache(maxsize=None)
def _ref(key):
    B, pool, P_, Cin, Cout, G = CASES[key]
    I = _inputs(key)
    y64 = _conv(I, torch.float64)
    want = F.group_norm(y64.view(B // pool, pool * P_, Cout).transpose(1, 2), G, I["gamma"].double(), I["beta"].double(), EPS).transpose(1, 2)
    mean, var = _moments(y64, pool, G)
    return dict(y64=y64, want=want.reshape(B, P_, Cout), mean=mean, rstd=1.0 / torch.sqrt(var + EPS), pmax=want.max(dim=1)[0],
                tol_y=2e-6 * max(1.0, float(y64.abs().max())))


def _note(name, **kw):
    REPORT.setdefault(name, {}).update(kw)


# ---------------------------------------------------------------------------------------------
# CPU: the bounds are statements about the kernels, and the inputs tell pooled statistics from averaged ones
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_conditioning(key):
    """The f32 torch evaluation of the whole graph (conv, moments, scale / shift, each rounded to f32), applied to the exact output, stays
    within half the bound of the f64 pooled GroupNorm: what a kernel is held to is not the inputs' own conditioning."""
    B, pool, P_, Cin, Cout, G = CASES[key]
    I, R = _inputs(key), _ref(key)
    mean, var = _moments(_conv(I, torch.float32), pool, G)
    sc, sh = _scale_shift(mean, var, I["gamma"], I["beta"], G)
    assert sc.dtype == torch.float32 and sh.dtype == torch.float32
    err = float((_apply(R["y64"], sc, sh) - R["want"]).abs().max())
    bound = LARGE_MEAN_TOL if key == "large_mean" else APPLY_TOL
    _note("pooled:conditioning:%s" % key, f32_torch_vs_f64=err, half_bound=bound / 2)
    assert err <= bound / 2, "case %s: the f32 evaluation is %.3e from f64 (half the bound: %.1e); pick another seed" % (key, err, bound / 2)


@pytest.mark.parametrize("key", [k for k in CASES if CASES[k][1] > 1])
def test_discrimination(key):
    """Statistics per entry, then averaged over the sequence -- what a finalize that dropped the between-entry term would return --
    are more than 100 bounds away from the pooled reference on the applied normalisation."""
    B, pool, P_, Cin, Cout, G = CASES[key]
    I, R = _inputs(key), _ref(key)
    mean1, var1 = _moments(R["y64"], 1, G)
    mean_a, var_a = mean1.view(B // pool, pool, G).mean(dim=1), var1.view(B // pool, pool, G).mean(dim=1)
    sc, sh = _scale_shift(mean_a, var_a, I["gamma"].double(), I["beta"].double(), G)
    diff = float((_apply(R["y64"], sc, sh) - R["want"]).abs().max())
    var_p = 1.0 / R["rstd"] ** 2 - EPS
    off = (var_a / var_p - 1.0).abs()
    bound = LARGE_MEAN_TOL if key == "large_mean" else APPLY_TOL
    _note("pooled:discrimination:%s" % key, averaged_vs_pooled=diff, variance_off_min=float(off.min()), variance_off_max=float(off.max()), bound=bound)
    assert diff > 100 * bound, "case %s: averaged per-entry statistics are only %.3e from the pooled ones" % (key, diff)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
_DEV = {}


def _on_device(ops, dev, key):
    """The case's operands on the device and its PackedWeight (built under the fixture's lowered thresholds), once per case."""
    if key not in _DEV:
        I = _inputs(key)
        D = {k: (None if v is None else v.to(dev)) for k, v in I.items()}
        D["pw"] = ops.PackedWeight(D["w"])
        _DEV[key] = D
    return _DEV[key]


def _kw(D, lo=None):
    s = slice(lo, None)
    c = lambda t: None if t is None else t[s].contiguous()
    return dict(bbias=c(D["bb"]), in_scale=c(D["sc_in"]), in_shift=c(D["sh_in"]), in_relu=D["sc_in"] is not None)


def _gn(ops, D, key, pool, lo=None, **extra):
    G = CASES[key][5]
    x = D["x"] if lo is None else D["x"][lo:].contiguous()
    return ops.conv1x1_gn(D["pw"], D["b"], x, D["gamma"], D["beta"], groups=G, pool=pool, **_kw(D, lo), **extra)


def _against_f64(name, key, res, apply_tol=APPLY_TOL):
    """(y, scale, shift, mean, rstd, pmax) of one route against the case's f64 reference; the shapes."""
    B, pool, P_, Cin, Cout, G = CASES[key]
    R = _ref(key)
    y, sc, sh, mean, rstd, pm = res
    assert sc.shape == (B // pool, Cout) and sh.shape == (B // pool, Cout) and pm.shape == (B // pool, Cout)
    assert mean.shape == (B // pool, G) and rstd.shape == (B // pool, G)
    record(name + ":y", y[:, :, :Cout], R["y64"], R["tol_y"])
    record(name + ":apply", _apply(R["y64"], sc.cpu(), sh.cpu()), R["want"], apply_tol)     # the statistics alone, on the exact output
    record(name + ":mean", mean, R["mean"], 2e-6 * max(1.0, float(R["mean"].abs().max())))
    record(name + ":rstd", rstd, R["rstd"], 5e-6 * float(R["rstd"].max()))
    record(name + ":pmax", pm, R["pmax"], apply_tol + 2 * R["tol_y"])


@gpu
@pytest.mark.parametrize("route,key", ROUTE_CASES)
def test_pooled_route_against_f64(ops, dev, route, key):
    B, pool, P_, Cin, Cout, G = CASES[key]
    D = _on_device(ops, dev, key)
    name = "pooled:%s:%s" % (route, key)
    with _route(ops, route):
        n0 = ops.CONV_ROUTE_COUNT["h3w"]
        res = _gn(ops, D, key, pool, want_max=True, want_moments=True)
        y1 = _gn(ops, D, key, 1)[0]
        nw = _gn(ops, D, key, pool, want_max=True, want_moments=True, write=False)
        last = _gn(ops, D, key, pool, lo=B - pool, want_max=True)
        launched = ops.CONV_ROUTE_COUNT["h3w"] - n0
    # the intended route ran
    assert launched == (4 if route == "h3w" else 0), "%d launches of the f16x3 entries on route %s" % (launched, route)
    if route in ("x6w", "x6") and D["pw"].x6w_ok:
        with _route(ops, "x6" if route == "x6w" else "x6w"):
            other = _gn(ops, D, key, pool)[0]
        assert not torch.equal(res[0], other), "x6w and x6 ran the same kernel"
    if key == "7":
        assert not D["pw"].x6w_ok and D["pw"].x6_gn_ok
    _against_f64(name, key, res)
    exact(name + ":y_is_the_pool1_y", res[0], y1)                       # pooling does not touch the conv
    assert nw[0] is None                                                # statistics only
    for i, nm in ((1, "scale"), (2, "shift"), (3, "mean"), (4, "rstd"), (5, "pmax")):
        exact("%s:nowrite_%s" % (name, nm), nw[i], res[i])
    exact(name + ":shard_y", last[0], res[0][B - pool:])                # a sequence does not depend on the batch around it
    for i, j, nm in ((1, 1, "scale"), (2, 2, "shift"), (3, 5, "pmax")):
        exact("%s:shard_%s" % (name, nm), last[i], res[j][B // pool - 1:])


@gpu
@pytest.mark.parametrize("route,key", [("x6w", "8"), ("f32", "1")])
def test_pooled_fallback_against_f64(ops, dev, route, key):
    """conv1x1 + the statistics kernel over the (B / pool, pool * P, ld) view: a row count off the 128-point tile in bf16x6 mode, and f32 mode.
    (`write` is ignored on this route: y is returned.)"""
    B, pool, P_, Cin, Cout, G = CASES[key]
    D = _on_device(ops, dev, key)
    name = "pooled:fallback_%s:%s" % (route, key)
    with _route(ops, route):
        n0 = ops.CONV_ROUTE_COUNT["h3w"]
        res = _gn(ops, D, key, pool, want_max=True, want_moments=True)
        y1 = _gn(ops, D, key, 1)[0]
        yc = ops.conv1x1(D["pw"], D["b"], D["x"], **_kw(D))
        nw = _gn(ops, D, key, pool, want_max=True, want_moments=True, write=False)
        last = _gn(ops, D, key, pool, lo=B - pool, want_max=True)
        assert ops.CONV_ROUTE_COUNT["h3w"] == n0, "an f16x3 entry took a fallback shape"
    exact(name + ":y_is_conv1x1", res[0], yc)
    _against_f64(name, key, res)
    exact(name + ":y_is_the_pool1_y", res[0], y1)
    assert nw[0] is not None
    for i, nm in ((1, "scale"), (2, "shift"), (3, "mean"), (4, "rstd"), (5, "pmax")):
        exact("%s:nowrite_%s" % (name, nm), nw[i], res[i])
    exact(name + ":shard_y", last[0], res[0][B - pool:])
    for i, j, nm in ((1, 1, "scale"), (2, 2, "shift"), (3, 5, "pmax")):
        exact("%s:shard_%s" % (name, nm), last[i], res[j][B // pool - 1:])


def _direct(ops, dev, D, key, entry, pool, G=None, status=True, prefill=None):
    """One lib call of a (pooled or plain) one-call entry with every output wanted -> (rc, y, scale, shift, pmax, mean, rstd).
    pool=None: the plain entry.  prefill: the outputs' initial value."""
    from caspr_amd import lib
    from caspr_amd.ops import _p, _stream, _conv_h3_launch
    L = lib.load()
    B, _, P_, Cin, Cout, G0 = CASES[key]
    G = G0 if G is None else G
    Bs = B // pool if pool else B
    new = (lambda *s: torch.full(s, prefill, device=dev)) if prefill is not None else (lambda *s: torch.empty(*s, device=dev))
    y = new(B, P_, (Cout + 3) // 4 * 4)
    scale, shift, pmax, mean, rstd = new(Bs, Cout), new(Bs, Cout), new(Bs, Cout), new(Bs, max(G, 1)), new(Bs, max(G, 1))
    nb = L.caspr_conv_gn_ws_bytes(B, P_, Cout)
    ws = torch.zeros(nb, device=dev, dtype=torch.uint8)
    pw, kw = D["pw"], _kw(D)
    head = lambda *packs: tuple(_p(t) for t in packs) + (_p(D["b"]), _p(kw["bbias"]), _p(D["x"]), D["x"].stride(1), _p(kw["in_scale"]), _p(kw["in_shift"]),
                                                        int(kw["in_relu"]), 0, _p(y), y.stride(1), B, P_, Cin, Cout, G)
    tail = (_p(D["gamma"]), _p(D["beta"]), EPS, _p(scale), _p(shift), _p(pmax), _p(mean), _p(rstd), _p(ws), nb)
    mid = () if pool is None else (int(pool),)
    if entry == "x6":
        fn = L.caspr_conv1x1_gn_bf16x6_f32 if pool is None else L.caspr_conv1x1_gn_pooled_bf16x6_f32
        rc = fn(*(head(pw.x3()) + mid + tail + (_stream(),)))
    elif entry == "x6w":
        fn = L.caspr_conv1x1_x6w_f32 if pool is None else L.caspr_conv1x1_x6w_pooled_f32
        rc = fn(*(head(*pw.xw()) + mid + tail + (_stream(),)))
    else:
        fn = L.caspr_conv1x1_h3w_f32 if pool is None else L.caspr_conv1x1_h3w_pooled_f32
        packs = pw.xh()
        if status:
            with _conv_h3_launch(D["x"]) as word:
                rc = fn(*(head(*packs) + mid + tail + (word, _stream())))
        else:
            rc = fn(*(head(*packs) + mid + tail + (None, _stream())))
    return (rc, y, scale, shift, pmax, mean, rstd)


@gpu
@pytest.mark.parametrize("entry", ["x6", "x6w", "h3w"])
@pytest.mark.parametrize("key", ["1", "4"])
def test_pool1_through_the_pooled_entries_is_the_plain_entry(ops, dev, entry, key):
    from caspr_amd import lib
    D = _on_device(ops, dev, key)
    plain = _direct(ops, dev, D, key, entry, None)
    pooled = _direct(ops, dev, D, key, entry, 1)
    lib.check(plain[0], "plain %s entry" % entry)
    lib.check(pooled[0], "pooled %s entry" % entry)
    for i, nm in enumerate(("y", "scale", "shift", "pmax", "mean", "rstd"), 1):
        exact("pooled:pool1_%s:%s:%s" % (entry, key, nm), pooled[i], plain[i])


def _busy(dev):
    """A large product queued on the current stream: what follows on it starts late, a side stream's work does not."""
    a = torch.ones(4096, 4096, device=dev)
    return a @ a


@gpu
@pytest.mark.parametrize("split", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("key", ["1", "3", "4"])
def test_tail_beside_is_the_one_call_layer(ops, dev, side, split, key):
    """ops.conv1x1_gn_tail_beside (tpointnet2.HEAD1_TAIL_BESIDE) with pool > 1: the remainder on a side stream while the main stream is
    still busy, then the pooled finalize -- the bits of conv1x1_gn(pool=...), twice, and against f64."""
    B, pool, P_, Cin, Cout, G = CASES[key]
    D = _on_device(ops, dev, key)
    R = _ref(key)
    name = "pooled:beside_%s:%s" % (split, key)
    args = (D["pw"], D["b"], D["x"], D["gamma"], D["beta"])
    with _route(ops, "h3w" if split == "f16x3" else "x6w"):
        whole = _gn(ops, D, key, pool)
        n0 = ops.CONV_ROUTE_COUNT["h3w"]
        keep = _busy(dev)
        a = ops.conv1x1_gn_tail_beside(*args, side, groups=G, pool=pool, **_kw(D))
        launched = ops.CONV_ROUTE_COUNT["h3w"] - n0
        keep2 = _busy(dev)
        b = ops.conv1x1_gn_tail_beside(*args, side, groups=G, pool=pool, **_kw(D))
        none = ops.conv1x1_gn_tail_beside(*args, None, groups=G, pool=pool, **_kw(D))
        torch.cuda.synchronize()
    assert launched == (2 if split == "f16x3" else 0), "the pieces ran on the other split (%d f16x3 launches)" % launched
    assert len(a) == 3 and len(none) == 3 and a[1].shape == (B // pool, Cout)
    for i, nm in enumerate(("y", "scale", "shift")):
        exact("%s:%s" % (name, nm), a[i], whole[i])
        exact("%s:again_%s" % (name, nm), b[i], a[i])
        exact("%s:no_stream_%s" % (name, nm), none[i], whole[i])
    record(name + ":y", a[0][:, :, :Cout], R["y64"], R["tol_y"])
    record(name + ":apply", _apply(R["y64"], a[1].cpu(), a[2].cpu()), R["want"], APPLY_TOL)
    del keep, keep2


@gpu
@pytest.mark.parametrize("split", ["f16x3", "bf16x6"])
def test_tail_beside_without_a_remainder_is_conv1x1_gn(ops, dev, side, split):
    """Cout % 512 == 0: nothing to put beside -- conv1x1_gn's result, side stream or not."""
    key = "large_mean"
    B, pool, P_, Cin, Cout, G = CASES[key]
    D = _on_device(ops, dev, key)
    with _route(ops, "h3w" if split == "f16x3" else "x6w"):
        whole = _gn(ops, D, key, pool)
        a = ops.conv1x1_gn_tail_beside(D["pw"], D["b"], D["x"], D["gamma"], D["beta"], side, groups=G, pool=pool, **_kw(D))
        torch.cuda.synchronize()
    assert len(a) == 3
    for i, nm in enumerate(("y", "scale", "shift")):
        exact("pooled:beside_%s:no_remainder_%s" % (split, nm), a[i], whole[i])


@gpu
@pytest.mark.parametrize("split", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("key", ["1", "3", "5", "6"])
def test_finalize_in_group_ranges_with_pooling(ops, dev, split, key):
    """Partials from ONE *_part_f32 call, caspr_conv_gn_finalize_f32 over groups [0, 1) then [1, G) with `pool`: the one-call pooled
    entry's bits, and the first call leaves the other groups' columns alone."""
    from caspr_amd import lib
    from caspr_amd.ops import _p, _stream, _conv_h3_launch
    L = lib.load()
    B, pool, P_, Cin, Cout, G = CASES[key]
    D = _on_device(ops, dev, key)
    pw, kw = D["pw"], _kw(D)
    Bs, cpg = B // pool, Cout // G
    with _route(ops, "h3w" if split == "f16x3" else "x6w"):
        whole = _gn(ops, D, key, pool, want_max=True, want_moments=True)
    y = torch.zeros(B, P_, (Cout + 3) // 4 * 4, device=dev)
    nb = L.caspr_conv_gn_ws_bytes(B, P_, Cout)
    ws = torch.zeros(nb, device=dev, dtype=torch.uint8)
    x = D["x"]
    common = (_p(D["b"]), _p(kw["bbias"]), _p(x), x.stride(1), _p(kw["in_scale"]), _p(kw["in_shift"]), 1, 0, _p(y), y.stride(1), B, P_, Cin, Cout,
              0, Cout // 512, 1, 0, _p(ws), nb)
    if split == "f16x3":
        main, tail = pw.xh()
        with _conv_h3_launch(x) as word:
            lib.check(L.caspr_conv1x1_h3w_part_f32(_p(main), _p(tail), *common, word, _stream()), "caspr_conv1x1_h3w_part_f32")
    else:
        main, tail = pw.xw()
        lib.check(L.caspr_conv1x1_x6w_part_f32(_p(main), _p(tail), *common, _stream()), "caspr_conv1x1_x6w_part_f32")
    scale, shift, pmax = (torch.full((Bs, Cout), 7.0, device=dev) for _ in range(3))
    mean, rstd = (torch.full((Bs, G), 7.0, device=dev) for _ in range(2))

    def finalize(g0, g1):
        lib.check(L.caspr_conv_gn_finalize_f32(_p(ws), nb, B, P_, Cout, G, g0, g1, pool, _p(D["gamma"]), _p(D["beta"]), EPS, _p(scale), _p(shift), _p(pmax),
                                               _p(mean), _p(rstd), _stream()), "caspr_conv_gn_finalize_f32")
    finalize(0, 1)
    first = [t.clone() for t in (scale, shift, pmax, mean, rstd)]
    finalize(1, G)
    name = "pooled:finalize_ranges_%s:%s" % (split, key)
    for t, nm in zip(first[:3], ("scale", "shift", "pmax")):
        assert bool((t[:, cpg:] == 7.0).all()), "%s: finalize(0, 1) wrote %s outside group 0" % (name, nm)
    for t, nm in zip(first[3:], ("mean", "rstd")):
        assert bool((t[:, 1:] == 7.0).all()), "%s: finalize(0, 1) wrote %s outside group 0" % (name, nm)
    exact(name + ":y", y, whole[0])
    for got, want, nm in zip((scale, shift, mean, rstd, pmax), whole[1:], ("scale", "shift", "mean", "rstd", "pmax")):
        exact("%s:%s" % (name, nm), got, want)
    for t, want, nm in zip(first, (whole[1], whole[2], whole[5], whole[3], whole[4]), ("scale", "shift", "pmax", "mean", "rstd")):
        n = cpg if t.shape[1] == Cout else 1
        exact("%s:group0_%s" % (name, nm), t[:, :n], want[:, :n])


@gpu
@pytest.mark.parametrize("split", ["f16x3", "bf16x6"])
def test_conv_gn_early_with_a_tail_stream(ops, dev, side, split):
    """ops.conv1x1_gn_early with the remainder on the early solve's stream (tpointnet2.TAIL_BESIDE, the default): conv1x1_gn's bits, and
    the group-0 columns the callback sees are final."""
    B, P_, Cin, Cout, G = 2, 128, 256, 1088, 16
    w = rnd(1, Cout, Cin, scale=1.0 / np.sqrt(Cin))
    b = rnd(2, Cout, scale=0.3)
    x = rnd(3, B, P_, Cin)
    sc_in, sh_in = rnd(4, B, Cin).abs() + 0.5, rnd(5, B, Cin)
    gamma, beta = rnd(6, Cout) * 0.2 + 1.0, rnd(7, Cout) * 0.1
    gamma[::7] *= -1.0
    d = lambda t: t.to(dev)
    pw = ops.PackedWeight(d(w))
    kw = dict(in_scale=d(sc_in), in_shift=d(sh_in), in_relu=True)
    seen = {}

    def on_early(pmax):      # as the model: work on the side stream behind an event, reading group 0's columns
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            side.wait_event(ready)
            seen["g0"] = pmax[:, :Cout // G].clone()
            seen["busy"] = _busy(dev)
    with _route(ops, "h3w" if split == "f16x3" else "x6w"):
        assert ops.conv1x1_gn_early_ok(pw, B, P_, G, 64)
        whole = ops.conv1x1_gn(pw, d(b), d(x), d(gamma), d(beta), groups=G, want_max=True, **kw)
        n0 = ops.CONV_ROUTE_COUNT["h3w"]
        parts = ops.conv1x1_gn_early(pw, d(b), d(x), d(gamma), d(beta), on_early, groups=G, reserve_cus=32, tail_stream=side, **kw)
        launched = ops.CONV_ROUTE_COUNT["h3w"] - n0
        torch.cuda.synchronize()
    assert launched == (3 if split == "f16x3" else 0), "tile 0, the remainder, the other tiles: %d f16x3 launches" % launched
    for i, nm in enumerate(("y", "scale", "shift", "pmax")):
        exact("pooled:early_tail_stream_%s:%s" % (split, nm), parts[i], whole[i])
    exact("pooled:early_tail_stream_%s:group0_in_callback" % split, seen["g0"], whole[3][:, :Cout // G])
    y64 = torch.relu(x.double() * sc_in.double().unsqueeze(1) + sh_in.double().unsqueeze(1)) @ w.double().t() + b.double()
    record("pooled:early_tail_stream_%s:y" % split, parts[0][:, :, :Cout], y64, 2e-6 * max(1.0, float(y64.abs().max())))


@gpu
@pytest.mark.parametrize("route", ["x6", "x6w", "h3w"])
def test_pooled_large_mean(ops, dev, route):
    """Pooled statistics when a group's mean dwarfs its spread (|mean| / sigma ~ 800) and the frames of a sequence sit one sigma apart:
    the between-entry term 128 (sum m_t^2 - T mean^2) is a difference of numbers ~ 1e5 x its size.  Bound and reasoning of
    test_conv1x1_gn_fused_large_mean: one f32 rounding of shift ~ 1e3."""
    key = "large_mean"
    B, pool, P_, Cin, Cout, G = CASES[key]
    D = _on_device(ops, dev, key)
    R = _ref(key)
    ratio = float((R["mean"].abs() * R["rstd"]).min())
    _note("pooled:large_mean_ratio", mean_over_sigma_min=ratio, mean_over_sigma_max=float((R["mean"].abs() * R["rstd"]).max()))
    assert ratio > 500
    with _route(ops, route):
        y, sc, sh = _gn(ops, D, key, pool)
    assert sc.shape == (B // pool, Cout)
    record("pooled:%s:large_mean:y" % route, y[:, :, :Cout], R["y64"], R["tol_y"])
    record("pooled:%s:large_mean:apply" % route, _apply(R["y64"], sc.cpu(), sh.cpu()), R["want"], LARGE_MEAN_TOL)


@gpu
def test_refusals(ops, dev):
    """pool = 0, a pool that does not divide B, G = 0, a null status word, an empty group range: refused before any launch (the outputs
    keep their fill)."""
    from caspr_amd import lib
    from caspr_amd.ops import _p, _stream
    L = lib.load()
    key = "1"
    B, pool, P_, Cin, Cout, G = CASES[key]
    D = _on_device(ops, dev, key)
    for bad in (0, 4):
        with pytest.raises(ValueError, match="pool"):
            _gn(ops, D, key, bad)

    def refused(what, out, match):
        with pytest.raises(lib.CasprHipError, match=match):
            lib.check(out[0], what)
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in out[1:]), "%s launched something before it refused" % what
    for entry in ("x6", "x6w", "h3w"):
        for bad in (0, 4):
            refused("%s pooled entry, pool=%d" % (entry, bad), _direct(ops, dev, D, key, entry, bad, prefill=7.0), "pool")
    for entry in ("x6w", "h3w"):
        refused("%s pooled entry, G=0" % entry, _direct(ops, dev, D, key, entry, pool, G=0, prefill=7.0), "G > 0")
    refused("h3w pooled entry, status NULL", _direct(ops, dev, D, key, "h3w", pool, status=False, prefill=7.0), "status is NULL")
    nb = L.caspr_conv_gn_ws_bytes(B, P_, Cout)
    ws = torch.zeros(nb, device=dev, dtype=torch.uint8)
    for bad_pool, g0, g1, match in ((0, 0, G, "pool"), (4, 0, G, "pool"), (pool, 3, 3, "groups"), (pool, 5, 2, "groups")):
        outs = [torch.full((B, Cout), 7.0, device=dev) for _ in range(3)]
        rc = L.caspr_conv_gn_finalize_f32(_p(ws), nb, B, P_, Cout, G, g0, g1, bad_pool, _p(D["gamma"]), _p(D["beta"]), EPS, _p(outs[0]), _p(outs[1]),
                                          _p(outs[2]), None, None, _stream())
        refused("finalize pool=%d groups %d..%d" % (bad_pool, g0, g1), [rc] + outs, match)


@gpu
@pytest.mark.parametrize("B,P_,C,G", [(2, 200, 560, 16), (1, 1500, 510, 2), (2, 3, 16, 16), (3, 1025, 96, 16)])
def test_gn_stats_groups_no_multiple_of_four_wide(ops, dev, B, P_, C, G):
    """The two-pass statistics on groups whose width is no multiple of 4 (gn_partial_scalar_kernel: what the pooled fallback needs for
    560 channels in 16 groups): 35 channels (7 row lanes, 11 idle threads), 255 (one lane, across the 1024-row split, NaN in the pad
    columns), 1 (fewer rows than lanes), 6 (42 lanes, one row behind the split) -- test_gn_stats' inputs and bounds, and the moments of
    the training entry."""
    from caspr_amd import train_ops as T
    ld = (C + 3) // 4 * 4
    y = torch.full((B, P_, ld), float("nan"))
    y[:, :, :C] = rnd(C, B, P_, C) * 2.0 + 0.7
    gamma, beta = rnd(1, C) * 0.2 + 1.0, rnd(2, C) * 0.1
    gamma[::7] *= -1.0
    y64 = y[:, :, :C].double()
    want = F.group_norm(y64.transpose(1, 2), G, gamma.double(), beta.double(), EPS).transpose(1, 2)
    yd = y.to(dev)
    sc, sh, pm = ops.gn_stats(yd, C, gamma.to(dev), beta.to(dev), groups=G, want_max=True)
    sc2, sh2, mean, rstd, pm2 = T.gn_stats_train(yd, C, gamma.to(dev), beta.to(dev), groups=G, want_max=True)
    yd.zero_()        # the NaN pads do not stay behind in the allocator's freed blocks for the tests that follow
    name = "pooled:gn_stats_cpg%d" % (C // G)
    record(name + ":apply", y64 * sc.cpu().double().unsqueeze(1) + sh.cpu().double().unsqueeze(1), want, APPLY_TOL)
    record(name + ":pmax", pm, want.max(dim=1)[0], APPLY_TOL)
    m64, v64 = _moments(y64, 1, G)
    r64 = 1.0 / torch.sqrt(v64 + EPS)
    record(name + ":mean", mean, m64, 2e-6)
    record(name + ":rstd", rstd, r64, 5e-6 * float(r64.max()))
    for got, ref, nm in ((sc2, sc, "scale"), (sh2, sh, "shift"), (pm2, pm, "pmax")):
        exact("%s:train_%s" % (name, nm), got, ref)
