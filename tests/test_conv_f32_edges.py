"""The f32 pointwise conv (caspr_conv1x1_f32: skinny / narrow / streaming / LDS-tiled kernels, eleven instantiations) at its edges
against f64, through ops.conv1x1 in f32 mode.  Cases, inputs, reference and the dispatcher's mirror: conv_f32_cases.py (checked on
the CPU by test_conv_f32_cases.py: coverage, conditioning at half the bound, mutations at >= 10 bounds).

Every call reads x as a column slice of a wider buffer whose other columns -- the pad columns [Cin, ldx) among them -- are NaN, and
writes into a column slice of a wider buffer prefilled with a sentinel bit pattern: whatever lies outside columns [0, Cout) of a row,
[Cout, roundup4(Cout)) included, must keep its bits.  Bounds are the project's: 2e-6 max(1, |y|max) on conv outputs, 2e-6 after the
sigmoid.  Every measured error lands in test_hip_parity's JSON report under "conv_f32:", the worst share of the bound per
instantiation under "conv_f32:worst:<route>".
"""
import numpy as np
import pytest
import torch

import conv_f32_cases as C
from test_hip_parity import REPORT, exact, record, rnd

gpu = pytest.mark.gpu
SENTINEL = 0x4B3C614E        # the bits of 12345678.0f: finite, and nothing a case computes


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
    """caspr_amd.ops with the pointwise convs in f32 mode (caspr_conv1x1_f32 on every call); the mode restored afterwards."""
    from caspr_amd import ops as _ops
    _ops.check_deferred_errors()
    prev = _ops.set_matmul_mode(conv=False)
    try:
        yield _ops
        _ops.check_deferred_errors()
    finally:
        _ops.set_matmul_mode(conv=prev[0])


# ---------------------------------------------------------------------------------------------
# one call: NaN around the input, a sentinel around the output
# ---------------------------------------------------------------------------------------------
_PW = {}


def _weight(ops, dev, c):
    if c.name not in _PW:
        _PW[c.name] = ops.PackedWeight(C.inputs(c.name).w.to(dev))
    return _PW[c.name]


def _embed_x(x, dev):
    """x (B, P, Cin) -> (the NaN-filled device buffer, its column slice [4, 4 + Cin)): ldx = roundup4(Cin) + 8."""
    B, P, Cin = x.shape
    buf = torch.full((B, P, C.roundup4(Cin) + 8), float("nan"))
    buf[:, :, 4:4 + Cin] = x
    buf = buf.to(dev)
    return buf, buf[:, :, 4:4 + Cin]


def _sentinel_out(B, P, Cout, dev):
    buf = torch.full((B, P, C.roundup4(Cout) + 8), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    return buf, buf[:, :, 4:4 + Cout]


def _untouched(name, buf, Cout):
    """Every element of the output buffer outside the slice's columns [0, Cout) kept the sentinel's bits."""
    bits = buf.view(torch.int32)
    outside = torch.cat([bits[:, :, :4], bits[:, :, 4 + Cout:]], dim=2)
    bad = int((outside != SENTINEL).sum())
    assert bad == 0, "%s: %d elements outside columns [0, %d) were written" % (name, bad, Cout)
    assert int((bits[:, :, 4:4 + Cout] == SENTINEL).sum()) == 0, "%s: output elements were not written" % name


def _call(ops, dev, c, I, rows=None, entries=None, **over):
    """ops.conv1x1 on case c's inputs (optionally a slice of its entries / rows) -> the (B, P, Cout) result, pads checked."""
    sl = lambda t: None if t is None else (t if entries is None else t[entries]).contiguous()
    x = I.x if entries is None else I.x[entries]
    x = x if rows is None else x[:, rows]
    xbuf, xv = _embed_x(x, dev)
    B, P = x.shape[0], x.shape[1]
    obuf, out = _sentinel_out(B, P, c.Cout, dev)
    d = lambda t: None if t is None else sl(t).to(dev)
    kw = dict(bbias=d(I.bb), in_scale=d(I.sc), in_shift=d(I.sh), in_relu=c.in_relu, in_relu_from=c.relu_from, act=c.act, row_invariant=c.ri)
    kw.update(over)
    got = ops.conv1x1(_weight(ops, dev, c), I.b.to(dev), xv, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    _untouched(c.name, obuf, c.Cout)
    res = out.clone()
    xbuf.zero_()          # the NaN pads do not stay behind in the allocator's freed blocks for the tests that follow
    return res


def _share(route, name, got, y64, tol):
    """The error's share of its bound, kept per instantiation (the worst so far) in the report."""
    err = C.distance(got.cpu(), y64)
    key = "conv_f32:worst:" + route
    if err / tol >= REPORT.get(key, {}).get("share_of_bound", -1.0):
        REPORT[key] = {"share_of_bound": err / tol, "case": name, "max_abs_err": err, "tol": tol}


@gpu
@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_case_against_f64(ops, dev, name):
    """The edge matrix, the fused input transform, the widths around GEMM_MAXC, the sigmoid on every instantiation, the row-invariant and
    three-entry cases: the result against f64, the surroundings of the output untouched."""
    c = C.BY_NAME[name]
    y64 = C.want(name)
    got = _call(ops, dev, c, C.inputs(name))
    tol = C.bound(c, y64)
    _share(c.route, name, got, y64, tol)
    record("conv_f32:" + name, got, y64, tol)


# ---------------------------------------------------------------------------------------------
# invariances
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("Cout", C.RI_COUT)
@pytest.mark.parametrize("Cin", C.RI_CIN)
def test_row_invariance(ops, dev, Cin, Cout, fused):
    """row_invariant=True: a row's bits depend on that row only.  One set of 300 rows; the calls on rows [0:P], on the reversed set's
    rows [0:P] and as (3, 100) return, row by row, the bits of the 300-row call -- across the skinny kernel's range (P <= 16), the
    narrow / streaming kernels' (P >= 128) and every row-tile index (the K order must not rotate with it)."""
    c = next(k for k in C.CASES if k.group == "ri" and (k.Cin, k.Cout, k.fused) == (Cin, Cout, fused))
    I, y64 = C.inputs(c.name), C.want(c.name)
    tol = C.bound(c, y64)
    tag = "conv_f32:ri:%dx%d%s" % (Cin, Cout, ":fused" if fused else "")
    whole = _call(ops, dev, c, I)
    record(tag + ":300", whole, y64, tol)
    for P in C.RI_P:
        head = _call(ops, dev, c, I, rows=slice(0, P))
        exact("%s:rows_0_%d" % (tag, P), head, whole[:, :P])
        back = torch.arange(C.RI_ROWS - 1, C.RI_ROWS - 1 - P, -1)          # the reversed set's first P rows
        rev = _call(ops, dev, c, I, rows=back)
        exact("%s:reversed_0_%d" % (tag, P), rev, whole[:, back.to(dev)])
        record("%s:reversed_0_%d:f64" % (tag, P), rev, y64[:, back], tol)
    J = type(I)(**{k: (v.view(3, 100, -1) if k == "x" else v.expand(3, -1).contiguous() if k in ("bb", "sc", "sh") and v is not None else v)
                  for k, v in vars(I).items()})
    three = _call(ops, dev, c, J)
    exact(tag + ":as_3x100", three.view(1, 300, -1), whole)


BATCH = [c.name for c in C.CASES if c.group == "batch"]


@gpu
@pytest.mark.parametrize("name", BATCH)
def test_batch_entry_invariance(ops, dev, name):
    """Entry b of a three-entry call has the bits of the one-entry call on it (its own bbias / in_scale / in_shift rows), on each of the
    four kernels and with block counts that are no multiple of 8 (6 / 6 / 12 / 12 against 2 / 2 / 4 / 4: the XCD renumbering)."""
    c = C.BY_NAME[name]
    I = C.inputs(name)
    whole = _call(ops, dev, c, I)
    for b in range(c.B):
        one = _call(ops, dev, c, I, entries=slice(b, b + 1))
        exact("conv_f32:%s:entry%d" % (name, b), one, whole[b:b + 1])


@gpu
@pytest.mark.parametrize("name", [n for n in BATCH if not C.BY_NAME[n].fused])
def test_in_relu_without_in_scale_is_ignored(ops, dev, name):
    """in(x) = x when in_scale is NULL, whatever in_relu / in_relu_from say: the bits of the plain call, on each of the four kernels."""
    c = C.BY_NAME[name]
    I = C.inputs(name)
    plain = _call(ops, dev, c, I)
    for k in (0, 4):
        exact("conv_f32:%s:in_relu_from%d_no_scale" % (name, k), _call(ops, dev, c, I, in_relu=True, in_relu_from=k), plain)


# ---------------------------------------------------------------------------------------------
# the large-P route and the refusals
# ---------------------------------------------------------------------------------------------
@gpu
def test_large_p_takes_the_128_point_tiles(ops, dev):
    """P = 4,194,241 rows of one entry: ceil(P / 64) = 65536 exceeds the grid, so the LDS-tiled kernel runs on 128-point tiles
    (conv1x1_kernel<128>, 32768 + 1 point tiles, the last one holding ONE row).  Fused (unfused, the narrow kernel would take it).
    Against the f64 evaluation done elementwise on the device, four products per output; first, last and tile-boundary rows against the
    CPU reference as well."""
    c = C.LARGE
    assert c.route == "lds<128>"
    I = C.inputs(c.name)
    pw = ops.PackedWeight(I.w.to(dev))
    x = I.x.to(dev)
    out = torch.full((1, c.P, 4), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    ops.conv1x1(pw, I.b.to(dev), x, bbias=I.bb.to(dev), in_scale=I.sc.to(dev), in_shift=I.sh.to(dev), in_relu=True, in_relu_from=0, out=out)
    assert int((out.view(torch.int32) == SENTINEL).sum()) == 0, "rows were not written"
    v = torch.relu(x.double() * I.sc.to(dev).double().unsqueeze(1) + I.sh.to(dev).double().unsqueeze(1))
    w64 = I.w.to(dev).double()
    y64 = (I.b.to(dev).double() + I.bb.to(dev).double()).expand(1, c.P, 4).clone()
    for k in range(4):
        y64 += v[:, :, k:k + 1] * w64[:, k]
    tol = C.CONV_TOL * max(1.0, float(y64.abs().max()))
    err = float((out.double() - y64).abs().max())
    assert bool(torch.isfinite(out).all())
    REPORT["conv_f32:worst:lds<128>"] = {"share_of_bound": err / tol, "case": c.name, "max_abs_err": err, "tol": tol}
    rows = torch.tensor(sorted({0, 1, 63, 64, 127, 128, 129, c.P // 2, c.P - 130, c.P - 129, c.P - 2, c.P - 1}))
    sub = type(c)(**{**vars(c), "P": len(rows)})
    Isub = type(I)(**{**vars(I), "x": I.x[:, rows]})
    record("conv_f32:large:rows_vs_cpu", out[:, rows.to(dev)], C.reference(sub, Isub), tol)
    record("conv_f32:large:device_f64", torch.tensor([err]), torch.zeros(1), tol)


@gpu
def test_rows_beyond_the_grid_are_refused(ops, dev):
    """P = 65535 * 128 + 1 rows per entry: refused with the message about the grid, the output untouched."""
    from caspr_amd import lib
    P = C.REFUSED_P
    assert C.f32_route(P, 4, 4, True, False) == "refused"
    pw = ops.PackedWeight(rnd(1, 4, 4).to(dev))
    x = torch.zeros(1, P, 4, device=dev)
    ss = torch.ones(1, 4, device=dev)
    out = torch.full((1, P, 4), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    with pytest.raises(lib.CasprHipError, match="exceed the grid"):
        ops.conv1x1(pw, None, x, in_scale=ss, in_shift=ss, in_relu=True, out=out)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == SENTINEL).all())


@gpu
def test_refusals(ops, dev):
    """ldx < roundup4(Cin), ldy < Cout, in_relu_from % 4 != 0, a fused transform with Cin % 4 != 0, in_scale without in_shift: refused
    before any launch, the output untouched."""
    from caspr_amd import lib
    from caspr_amd.ops import _p, _stream
    L = lib.load()
    B, P = 2, 20

    def refused(what, match, Cin, Cout, ldx=None, ldy=None, scale=True, shift=True, relu_from=0, through_ops=True):
        pw = ops.PackedWeight(rnd(1, Cout, Cin).to(dev))
        ldx = C.roundup4(Cin) if ldx is None else ldx
        ldy = C.roundup4(Cout) if ldy is None else ldy
        x = torch.zeros(B, P, max(ldx, 4), device=dev)
        out = torch.full((B, P, max(ldy, 4)), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        sc = torch.ones(B, Cin, device=dev) if scale else None
        sh = torch.ones(B, Cin, device=dev) if shift else None
        rc = L.caspr_conv1x1_f32(_p(pw.data), None, None, _p(x), ldx, _p(sc), _p(sh), 1, relu_from, _p(out), ldy, B, P, Cin, Cout, 0, _stream())
        with pytest.raises(lib.CasprHipError, match=match):
            lib.check(rc, what)
        if through_ops:
            with pytest.raises(lib.CasprHipError, match=match):
                ops.conv1x1(pw, None, x, in_scale=sc, in_shift=sh, in_relu=True, in_relu_from=relu_from, out=out)
        torch.cuda.synchronize()
        assert bool((out.view(torch.int32) == SENTINEL).all()), "%s launched something before it refused" % what

    refused("ldx < roundup4(Cin)", "ldx=8", 10, 8, ldx=8, scale=False, shift=False, through_ops=False)
    refused("ldy < Cout", "ldy=8", 8, 10, ldy=8)
    refused("in_relu_from % 4 != 0", "in_relu_from=6", 8, 8, relu_from=6)
    refused("fused with Cin % 4 != 0", "Cin %% 4 == 0|Cin % 4 == 0", 10, 8)
    refused("in_scale without in_shift", "given together", 8, 8, shift=False)
    with pytest.raises(ValueError, match="input rows hold"):        # the host's own check of the same rule as ldx < roundup4(Cin)
        ops.conv1x1(ops.PackedWeight(rnd(1, 8, 10).to(dev)), None, torch.zeros(B, P, 8, device=dev))
