"""The f16x3 form of the persistent 128-point x 512-channel conv (csrc/gemm_f16x3w.hip, config.conv_split = "f16x3") launch by launch:
against the f64 contraction at test_conv1x1_x6w_kernel's tolerance 2e-6 max(1, |y64|max), its GroupNorm statistics against the other
conv route's at 3e-6 max(1, .), conv1x1_gn / batch / piece / grid invariance bit for bit, the weight scale found on the device, and the
range guard.  Shapes: the smallest at which the stream of chunks can go wrong (one chunk per tile, odd chunk counts, two channel tiles,
a remainder on the tail kernel, one above 64 channels on the 256-channel kernel, Cin not a multiple of 64)."""
import numpy as np
import pytest
import torch

from test_hip_parity import exact, record, rnd

pytestmark = pytest.mark.gpu

SHAPES = [(1, 128, 32, 512), (1, 128, 64, 512), (1, 256, 96, 1024), (3, 128, 512, 560), (2, 384, 544, 1536), (2, 128, 64, 704)]


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    return torch.device("cuda:0")


@pytest.fixture()
def ops():
    """caspr_amd.ops with the persistent kernel's thresholds lowered to the test shapes, f16x3 selected; restored afterwards."""
    from caspr_amd import ops as _ops
    _ops.check_deferred_errors()
    saved = (_ops._X6W_MIN_CIN, _ops._X6W_MIN_ROWS, _ops.CONV_X6W, _ops.CONV_SPLIT)
    _ops._X6W_MIN_CIN, _ops._X6W_MIN_ROWS, _ops.CONV_X6W, _ops.CONV_SPLIT = 32, 128, True, "f16x3"
    try:
        yield _ops
    finally:
        _ops._X6W_MIN_CIN, _ops._X6W_MIN_ROWS, _ops.CONV_X6W, _ops.CONV_SPLIT = saved


def _operands(B, P_, Cin, Cout):
    """Negative, tiny (2^-20 .. 2^-7: flushed planes) and large (up to 4000) activations mixed into every row; the producer's scale in
    [0.5, 1] and shift of a few units keep the transformed value below 4095."""
    g = np.random.default_rng(Cin * 7 + Cout)
    w = rnd(1, Cout, Cin, scale=1.0 / np.sqrt(Cin))
    b, bb = rnd(2, Cout, scale=0.3), rnd(3, B, Cout, scale=0.1)
    x = rnd(Cin + Cout, B, P_, Cin)
    kind = torch.from_numpy(g.integers(0, 8, size=(B, P_, Cin)))
    tiny = torch.from_numpy((2.0 ** g.uniform(-20, -7, size=(B, P_, Cin)) * g.choice([-1.0, 1.0], size=(B, P_, Cin))).astype(np.float32))
    large = torch.from_numpy((g.uniform(1000, 4000, size=(B, P_, Cin)) * g.choice([-1.0, 1.0], size=(B, P_, Cin))).astype(np.float32))
    x = torch.where(kind == 0, tiny, x)
    x = torch.where(kind == 1, large, x)
    x[:, :, 0] = 4000.0
    sc_in = torch.from_numpy(g.uniform(0.5, 1.0, size=(B, Cin)).astype(np.float32))
    sh_in = rnd(5, B, Cin, scale=0.5).clamp(-3, 3)
    gamma, beta = rnd(6, Cout) * 0.2 + 1.0, rnd(7, Cout) * 0.1
    return w, b, bb, x, sc_in, sh_in, gamma, beta


def _f64(x, w, b, bb, sc_in=None, sh_in=None):
    xin = x.double()
    if sc_in is not None:
        xin = x.double() * sc_in.double().unsqueeze(1) + sh_in.double().unsqueeze(1)
        xin[:, :, 8:] = torch.relu(xin[:, :, 8:])
    y = xin @ w.double().t() + b.double()
    return y if bb is None else y + bb.double().unsqueeze(1)


def _pieces(ops, dev, pw, b, x, gamma, beta, kw, pieces, reserve=0, groups=16):
    """The layer through caspr_conv1x1_h3w_part_f32 (channel-tile ranges `pieces`, the remainder with the last) + the finalize over all
    groups -> (y, partials, scale, shift, pmax)."""
    from caspr_amd import lib
    from caspr_amd.ops import _p, _stream, _conv_h3_launch
    L = lib.load()
    B, P_, _ = x.shape
    C = pw.cout
    y = torch.zeros(B, P_, (C + 3) // 4 * 4, device=dev)
    nb = L.caspr_conv_gn_ws_bytes(B, P_, C)
    ws = torch.zeros(nb, device=dev, dtype=torch.uint8)
    scale, shift, pmax = (torch.empty(B, C, device=dev) for _ in range(3))
    main, tail = pw.xh()
    for n, (m0, m1) in enumerate(pieces):
        with _conv_h3_launch(x) as word:
            lib.check(L.caspr_conv1x1_h3w_part_f32(_p(main), _p(tail), _p(b), _p(kw["bbias"]), _p(x), x.stride(1), _p(kw["in_scale"]), _p(kw["in_shift"]), 1, 8,
                                                   _p(y), y.stride(1), B, P_, pw.cin, C, m0, m1, int(n == len(pieces) - 1), int(reserve), _p(ws), nb, word,
                                                   _stream()), "caspr_conv1x1_h3w_part_f32")
    lib.check(L.caspr_conv_gn_finalize_f32(_p(ws), nb, B, P_, C, groups, 0, groups, 1, _p(gamma), _p(beta), 1e-5, _p(scale), _p(shift), _p(pmax), None, None,
                                           _stream()), "caspr_conv_gn_finalize_f32")
    return y, ws, scale, shift, pmax


@pytest.mark.parametrize("B,P_,Cin,Cout", SHAPES)
def test_conv_h3w_kernel(ops, dev, B, P_, Cin, Cout):
    w, b, bb, x, sc_in, sh_in, gamma, beta = _operands(B, P_, Cin, Cout)
    pw = ops.PackedWeight(w.to(dev))
    assert pw.x6w_ok
    d = lambda t: t.to(dev)
    kw = dict(bbias=d(bb), in_scale=d(sc_in), in_shift=d(sh_in), in_relu=True, in_relu_from=8)
    n0 = ops.CONV_ROUTE_COUNT["h3w"]
    y = ops.conv1x1(pw, d(b), d(x), **kw)
    yp = ops.conv1x1(pw, d(b), d(x))
    res = ops.conv1x1_gn(pw, d(b), d(x), d(gamma), d(beta), want_max=True, **kw)
    assert ops.CONV_ROUTE_COUNT["h3w"] == n0 + 3, "the f16x3 kernel did not take these calls"
    # the other split / the other conv route
    ops.CONV_SPLIT = "bf16x6"
    if Cin >= 64:
        y_x6 = ops.conv1x1(pw, d(b), d(x), **kw)
        assert not torch.equal(y, y_x6), "both splits ran the same kernel"
    ops.CONV_X6W = False
    res_old = ops.conv1x1_gn(pw, d(b), d(x), d(gamma), d(beta), want_max=True, **kw)
    ops.CONV_X6W, ops.CONV_SPLIT = True, "f16x3"
    assert ops.CONV_ROUTE_COUNT["h3w"] == n0 + 3

    y64 = _f64(x, w, b, bb, sc_in, sh_in)
    tol = 2e-6 * max(1.0, float(y64.abs().max()))
    record("conv_h3w_fused_%dx%d" % (Cin, Cout), y[:, :, :Cout], y64, tol)
    y64p = _f64(x, w, b, None)
    record("conv_h3w_plain_%dx%d" % (Cin, Cout), yp[:, :, :Cout], y64p, 2e-6 * max(1.0, float(y64p.abs().max())))
    exact("conv_h3w_gn_output_%dx%d" % (Cin, Cout), res[0], y)
    for i, nm in ((1, "scale"), (2, "shift"), (3, "max")):
        record("conv_h3w_gn_%s_%dx%d" % (nm, Cin, Cout), res[i], res_old[i], 3e-6 * max(1.0, float(res_old[i].abs().max())))
    if B > 1:
        y1 = ops.conv1x1(pw, d(b), d(x[B - 1:]).contiguous(), bbias=d(bb[B - 1:]).contiguous(), in_scale=d(sc_in[B - 1:]).contiguous(),
                         in_shift=d(sh_in[B - 1:]).contiguous(), in_relu=True, in_relu_from=8)
        exact("conv_h3w_batch_invariance_%dx%d" % (Cin, Cout), y1, y[B - 1:])
    # pieces + finalize == the whole call; the persistent stream on 1, 2, 3 workgroups == the full grid
    mt = Cout // 512
    whole = _pieces(ops, dev, pw, d(b), d(x), d(gamma), d(beta), kw, [(0, mt)])
    exact("conv_h3w_part_whole_y_%dx%d" % (Cin, Cout), whole[0], y)
    if pw.x6_gn_ok:        # (below 64 input channels conv1x1_gn is conv1x1 + gn_stats: the statistics of another kernel)
        for i, nm in ((2, "scale"), (3, "shift"), (4, "max")):
            exact("conv_h3w_part_whole_%s_%dx%d" % (nm, Cin, Cout), whole[i], res[i - 1])
    if mt > 1:
        split = _pieces(ops, dev, pw, d(b), d(x), d(gamma), d(beta), kw, [(0, 1), (1, mt)])
        for i, nm in ((0, "y"), (1, "partials"), (2, "scale"), (3, "shift"), (4, "max")):
            exact("conv_h3w_pieces_%s_%dx%d" % (nm, Cin, Cout), split[i], whole[i])
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    for g in (1, 2, 3):
        few = _pieces(ops, dev, pw, d(b), d(x), d(gamma), d(beta), kw, [(0, mt)], reserve=n_cu - g)
        exact("conv_h3w_grid%d_y_%dx%d" % (g, Cin, Cout), few[0], whole[0])
        exact("conv_h3w_grid%d_partials_%dx%d" % (g, Cin, Cout), few[1], whole[1])
    ops.check_deferred_errors()


def test_weight_scale_from_the_device(ops, dev):
    """A power of two on the weights is absorbed by the shift the pack step finds: the product scales exactly (no bias); an all-zero
    layer takes shift 0 and puts out its bias."""
    B, P_, Cin, Cout = 1, 256, 96, 1024
    w, b, bb, x, sc_in, sh_in, gamma, beta = _operands(B, P_, Cin, Cout)
    x = x.clamp(-8, 8)
    y = ops.conv1x1(ops.PackedWeight(w.to(dev)), None, x.to(dev))
    for k in (-40, 20):
        yk = ops.conv1x1(ops.PackedWeight((w * 2.0 ** k).to(dev)), None, x.to(dev))
        exact("conv_h3w_weight_scale_2^%d" % k, yk, y * 2.0 ** k)
    y0 = ops.conv1x1(ops.PackedWeight(torch.zeros_like(w).to(dev)), b.to(dev), x.to(dev), bbias=bb.to(dev))
    exact("conv_h3w_zero_layer", y0, (b + bb[0]).to(dev).expand(B, P_, Cout))
    ops.check_deferred_errors()


def test_range_guard(ops, dev):
    """A value of 5000 after the producer's transform and a NaN input: exactly those rows are NaN in all channels, every other row keeps
    its bits, the deferred channel raises and names the remedy, and the next call is clean."""
    from caspr_amd.lib import CasprHipError
    B, P_, Cin, Cout = 2, 384, 544, 1536
    w, b, bb, x, sc_in, sh_in, gamma, beta = _operands(B, P_, Cin, Cout)
    d = lambda t: t.to(dev)
    pw = ops.PackedWeight(d(w))
    kw = dict(bbias=d(bb), in_scale=d(sc_in), in_shift=d(sh_in), in_relu=True, in_relu_from=8)
    y = ops.conv1x1(pw, d(b), d(x), **kw)
    ops.check_deferred_errors()
    xb = x.clone()
    xb[0, 5, 17] = (5000.0 - sh_in[0, 17]) / sc_in[0, 17]
    xb[1, 200, 3] = float("nan")
    yb = ops.conv1x1(pw, d(b), d(xb), **kw)
    bad = torch.zeros(B, P_, dtype=torch.bool)
    bad[0, 5] = bad[1, 200] = True
    nan_rows = torch.isnan(yb).all(dim=2).cpu()
    any_nan = torch.isnan(yb).any(dim=2).cpu()
    assert torch.equal(nan_rows, bad) and torch.equal(any_nan, bad), "NaN rows %s" % (any_nan.nonzero().tolist(),)
    exact("conv_h3w_guard_other_rows", yb[~bad.to(dev)], y[~bad.to(dev)])
    with pytest.raises(CasprHipError, match="conv_split"):
        ops.check_deferred_errors()
    y2 = ops.conv1x1(pw, d(b), d(x), **kw)
    ops.check_deferred_errors()
    exact("conv_h3w_guard_next_call_clean", y2, y)
