"""The bf16x6 pointwise convs -- conv1x1_bf16x6_kernel, conv1x1_x6tail_kernel (csrc/gemm_bf16x6.hip) and conv1x1_x6w_kernel
(csrc/gemm_bf16x6w.hip), four instantiations each -- at their edges against f64, through the C entries (lib.load()) with packs from
caspr_pack_weight_bf16x3 / caspr_pack_weight_x6w.  Cases, inputs, reference and the host's mirror: conv_bf16x6_cases.py (checked on the
CPU by test_conv_bf16x6_cases.py: coverage, conditioning at half the bound, mutations at >= 10 bounds).

Every call reads x as a 16-byte-aligned column slice (offset 4 floats, ldx = Cin + 8) of a NaN buffer, a weight window out of a NaN
matrix where the case has one, and writes into slices of buffers prefilled with a sentinel bit pattern: the output's columns outside
[0, Cout), the rows around scale / shift / pmax / mean / rstd and the bytes behind the workspace must keep their bits, and on a refused
or empty call everything does.  Bounds are the project's: 2e-6 max(1, |y64|max) on conv outputs, 2e-6 after the sigmoid, 5e-6 on the
applied normalisation, 2e-6 / 5e-6 / 5e-6 on mean / rstd / pmax as test_conv_gn_pooled.  Every measured error lands in test_hip_parity's
JSON report under "conv_bf16x6:", the worst share of the bound per instantiation under "conv_bf16x6:worst:<route>".

The grid-1 / 2 / 3 / 5 cases of group "stream" are the first op-level run of conv1x1_x6w_kernel's multi-tile stream (advance() across a
tile end, finish() in the middle, the next tile's in_scale row and weights staged under the running one).

conv_x6tail_launch's own CASPR_REQUIRE cannot be reached from a public entry (its callers have checked the same things and never pass
more than 64 channels), so no refusal names it.
"""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import conv_bf16x6_cases as C
from test_hip_parity import REPORT, exact, record

pytestmark = pytest.mark.gpu
SENTINEL = 0x4B3C614E        # test_conv_f32_edges.SENTINEL: the bits of 12345678.0f
GUARD = 256                  # sentinel bytes behind the workspace


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from caspr_amd import lib
    return lib.load()


@pytest.fixture()
def ops():
    """caspr_amd.ops in bf16x6 mode with the thresholds lowered to the test shapes; restored afterwards."""
    from caspr_amd import ops as _ops
    _ops.check_deferred_errors()
    saved = (_ops._X6_MIN_CIN, _ops._X6W_MIN_CIN, _ops._X6W_MIN_ROWS, _ops.CONV_X6W, _ops.CONV_SPLIT)
    mode = _ops.matmul_mode()["conv"] == "bf16x6"
    _ops._X6_MIN_CIN, _ops._X6W_MIN_CIN, _ops._X6W_MIN_ROWS, _ops.CONV_X6W, _ops.CONV_SPLIT = 32, 64, 128, True, "bf16x6"
    _ops.set_matmul_mode(conv=True)
    try:
        yield _ops
        _ops.check_deferred_errors()
    finally:
        _ops._X6_MIN_CIN, _ops._X6W_MIN_CIN, _ops._X6W_MIN_ROWS, _ops.CONV_X6W, _ops.CONV_SPLIT = saved
        _ops.set_matmul_mode(conv=mode)


# ---------------------------------------------------------------------------------------------
# one call: NaN around the input and the weight window, a sentinel around every output
# ---------------------------------------------------------------------------------------------
def _sentinel(dev, *shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def _is_sentinel(t):
    return bool((t.contiguous().view(torch.int32) == SENTINEL).all())


_PACKS = {}


def _weight_on_device(c, I, dev, contiguous):
    """The (Cout, ldw) matrix with NaN in every column outside the window, or the contiguous copy of the window -> (tensor, ldw, col0)."""
    if contiguous or c.ldw == c.Cin:
        return I.w.to(dev), c.Cin, 0
    w = torch.full((c.Cout, c.ldw), float("nan"))
    w[:, c.col0:c.col0 + c.Cin] = I.w
    return w.to(dev), c.ldw, c.col0


def _packs(L, dev, c, I, contiguous=False):
    """(main, tail) for the wide entries, (pack, None) for x6 / x6gn; built once per case."""
    from caspr_amd import lib
    from caspr_amd.ops import _p, _stream
    key = (c.name, contiguous)
    if key in _PACKS:
        return _PACKS[key]
    w, ldw, col0 = _weight_on_device(c, I, dev, contiguous)

    def pack3(rows0, rows):
        out = torch.empty(L.caspr_bf16x3_packed_bytes(rows, c.Cin), device=dev, dtype=torch.uint8)
        lib.check(L.caspr_pack_weight_bf16x3(_p(w[rows0:]), ldw, rows, col0, c.Cin, _p(out), _stream()), "caspr_pack_weight_bf16x3")
        return out
    if c.entry in ("x6", "x6gn"):
        packs = (pack3(0, c.Cout), None)
    else:
        Cmain = c.Cout - c.Cout % 512
        size, pack = (L.caspr_h3w_packed_bytes, L.caspr_pack_weight_h3w) if c.entry == "h3w" else (L.caspr_x6w_packed_bytes, L.caspr_pack_weight_x6w)
        main = torch.empty(size(Cmain, c.Cin), device=dev, dtype=torch.uint8)
        lib.check(pack(_p(w), ldw, Cmain, col0, c.Cin, _p(main), _stream()), "the wide pack")
        packs = (main, pack3(Cmain, c.Cout - Cmain) if c.Cout > Cmain else None)
    torch.cuda.synchronize()
    w.zero_()               # the NaN columns do not stay behind in the allocator's freed blocks
    _PACKS[key] = packs
    return packs


def _buffers(L, dev, c, I, entries=None):
    """Everything one call of case c reads and writes, by name; pointers as integers (a refusal test moves one)."""
    sl = lambda t: None if t is None else (t if entries is None else t[entries]).contiguous().to(dev)
    x = I.x if entries is None else I.x[entries]
    B, P = x.shape[0], x.shape[1]
    Bs = B // c.pool
    U = SimpleNamespace(B=B, P=P, Bs=Bs)
    U.xbuf = torch.full((B, P, c.Cin + 8), float("nan"))
    U.xbuf[:, :, 4:4 + c.Cin] = x
    U.xbuf = U.xbuf.to(dev)
    U.x = U.xbuf[:, :, 4:4 + c.Cin]
    U.obuf = _sentinel(dev, B, P, c.Cout + 8)
    U.out = U.obuf[:, :, 4:4 + c.Cout]
    U.b, U.bb, U.sc, U.sh, U.gamma, U.beta = I.b if I.b is None else I.b.to(dev), sl(I.bb), sl(I.sc), sl(I.sh), None, None
    U.nb = 0
    if c.G:
        U.gamma, U.beta = I.gamma.to(dev), I.beta.to(dev)
        U.nb = L.caspr_conv_gn_ws_bytes(B, P, c.Cout)
        assert U.nb == B * (P // 128) * c.Cout * 16
        U.ws = _sentinel(dev, (U.nb + GUARD) // 4)
        U.scale, U.shift, U.pmax = (_sentinel(dev, Bs + 2, c.Cout) for _ in range(3))
        U.mean, U.rstd = (_sentinel(dev, Bs + 2, c.G) for _ in range(2))
    return U


def _ptr(t, row=0):
    return 0 if t is None else (t[row:].data_ptr() if row else t.data_ptr())


def _args(c, U, packs, piece=None, g=None, n_cu=256):
    """The named argument list of case c's entry (of one piece of it); pointers as integers, the stream left out."""
    a = {}
    if c.entry in ("x6", "x6gn"):
        a["wpk"] = _ptr(packs[0])
    else:
        a["wpk_main"], a["wpk_tail"] = _ptr(packs[0]), _ptr(packs[1])
    a.update(bias=_ptr(U.b), bbias=_ptr(U.bb), X=U.x.data_ptr(), ldx=c.Cin + 8, in_scale=_ptr(U.sc), in_shift=_ptr(U.sh),
             in_relu=int(c.in_relu), in_relu_from=c.relu_from, Y=U.out.data_ptr() if c.write else 0, ldy=c.Cout + 8, B=U.B, P=U.P, Cin=c.Cin, Cout=c.Cout)
    if c.entry == "x6":
        a["act"] = c.act
        return "caspr_conv1x1_bf16x6_f32", a
    if c.entry == "part":
        m0, m1, with_tail = piece
        g = c.g if g is None else g
        a.update(mt_begin=m0, mt_end=m1, with_tail=with_tail, reserve_cus=n_cu - g if g else 0, ws=_ptr(U.ws), ws_bytes=U.nb)
        return "caspr_conv1x1_x6w_part_f32", a
    a["G"] = c.G
    if c.pool > 1:
        a["pool"] = c.pool
    if c.G:
        a.update(gamma=_ptr(U.gamma), beta=_ptr(U.beta), eps=C.EPS, scale=_ptr(U.scale, 1), shift=_ptr(U.shift, 1), pmax=_ptr(U.pmax, 1),
                 mean=_ptr(U.mean, 1), rstd=_ptr(U.rstd, 1), ws=_ptr(U.ws), ws_bytes=U.nb)
    else:
        a.update(gamma=0, beta=0, eps=0.0, scale=0, shift=0, pmax=0, mean=0, rstd=0, ws=0, ws_bytes=0)
    pooled = "_pooled" if c.pool > 1 else ""
    return {"x6gn": "caspr_conv1x1_gn%s_bf16x6_f32" % pooled, "x6w": "caspr_conv1x1_x6w%s_f32" % pooled, "h3w": "caspr_conv1x1_h3w%s_f32" % pooled}[c.entry], a


_POINTERS = {"wpk", "wpk_main", "wpk_tail", "bias", "bbias", "X", "in_scale", "in_shift", "Y", "gamma", "beta", "scale", "shift", "pmax", "mean", "rstd", "ws"}


def _invoke(L, name, a, x=None):
    """The entry `name` on the named arguments -> its return code."""
    from caspr_amd.ops import _stream, _conv_h3_launch
    vals = [ctypes.c_void_p(v) if k in _POINTERS else v for k, v in a.items()]
    if "h3w" in name:
        with _conv_h3_launch(x) as word:
            return getattr(L, name)(*vals, word, _stream())
    return getattr(L, name)(*vals, _stream())


def _finalize_args(c, U):
    return dict(ws=_ptr(U.ws), ws_bytes=U.nb, B=U.B, P=U.P, Cout=c.Cout, G=c.G, g_begin=0, g_end=c.G, pool=c.pool, gamma=_ptr(U.gamma), beta=_ptr(U.beta),
                eps=C.EPS, scale=_ptr(U.scale, 1), shift=_ptr(U.shift, 1), pmax=_ptr(U.pmax, 1), mean=_ptr(U.mean, 1), rstd=_ptr(U.rstd, 1))


def _surroundings_untouched(c, U):
    bits = U.obuf.view(torch.int32)
    outside = torch.cat([bits[:, :, :4], bits[:, :, 4 + c.Cout:]], dim=2)
    bad = int((outside != SENTINEL).sum())
    assert bad == 0, "%s: %d elements outside columns [0, %d) were written" % (c.name, bad, c.Cout)
    if c.write:
        assert int((bits[:, :, 4:4 + c.Cout] == SENTINEL).sum()) == 0, "%s: output elements were not written" % c.name
    else:
        assert _is_sentinel(U.obuf), "%s: Y = NULL and the output buffer was written" % c.name
    if c.G:
        assert _is_sentinel(U.ws[U.nb // 4:]), "%s: the bytes behind the workspace were written" % c.name
        assert int((U.ws[:U.nb // 4].view(torch.int32) == SENTINEL).sum()) == 0, "%s: partials were not written" % c.name
        for nm in ("scale", "shift", "pmax", "mean", "rstd"):
            t = getattr(U, nm)
            assert _is_sentinel(t[0]) and _is_sentinel(t[-1]), "%s: rows around %s were written" % (c.name, nm)
            assert int((t[1:-1].view(torch.int32) == SENTINEL).sum()) == 0, "%s: %s was not written" % (c.name, nm)


def _run(L, dev, c, I, entries=None, pieces=None, g=None, contiguous=False):
    """Case c (optionally a slice of its entries, other pieces, another grid, the contiguous pack) -> y | None, partials, scale, shift, pmax,
    mean, rstd; the surroundings of every output checked."""
    from caspr_amd import lib
    packs = _packs(L, dev, c, I, contiguous)
    U = _buffers(L, dev, c, I, entries)
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    for piece in ((pieces or c.pieces) if c.entry == "part" else [None]):
        name, a = _args(c, U, packs, piece, g, n_cu)
        lib.check(_invoke(L, name, a, U.x), name)
    if c.entry == "part":
        lib.check(_invoke(L, "caspr_conv_gn_finalize_f32", _finalize_args(c, U)), "caspr_conv_gn_finalize_f32")
    torch.cuda.synchronize()
    _surroundings_untouched(c, U)
    R = SimpleNamespace(y=U.out.clone() if c.write else None, part=None, scale=None, shift=None, pmax=None, mean=None, rstd=None)
    if c.G:
        R.part = U.ws[:U.nb // 4].clone()
        R.scale, R.shift, R.pmax, R.mean, R.rstd = (getattr(U, nm)[1:-1].clone() for nm in ("scale", "shift", "pmax", "mean", "rstd"))
    U.xbuf.zero_()          # the NaN pads do not stay behind in the allocator's freed blocks for the tests that follow
    return R


def _same(tag, got, want, fields=("y", "part", "scale", "shift", "pmax", "mean", "rstd")):
    for f in fields:
        a, b = getattr(got, f), getattr(want, f)
        assert (a is None) == (b is None), "%s: %s" % (tag, f)
        if a is not None:
            exact("%s:%s" % (tag, f), a, b)


def _worst(route, name, share, what):
    key = "conv_bf16x6:worst:" + route
    if share >= REPORT.get(key, {}).get("share_of_bound", -1.0):
        REPORT[key] = {"share_of_bound": share, "case": name, "of": what}


def _against_f64(c, got):
    """Every output of one run against the case's f64 reference, at the project's bounds; the shares per instantiation."""
    W = C.want(c.name)
    tag = "conv_bf16x6:" + c.name
    if c.write:
        for l in c.plan:                      # the columns of each launch, for the report
            cols = slice(l.c0, l.c0 + l.C)
            _worst(l.inst, c.name, C.distance(got.y[:, :, cols].cpu(), W.y[:, :, cols]) / W.tol_y, "y")
        record(tag + ":y", got.y, W.y, W.tol_y)
    if c.G:
        applied = C.apply(W.y, got.scale.cpu(), got.shift.cpu())
        for l in c.plan:
            _worst(l.inst, c.name, C.distance(applied[:, :, l.c0:l.c0 + l.C], W.want[:, :, l.c0:l.c0 + l.C]) / C.APPLY_TOL, "applied normalisation")
        record(tag + ":apply", applied, W.want, C.APPLY_TOL)
        record(tag + ":mean", got.mean, W.mean, 2e-6 * max(1.0, float(W.mean.abs().max())))
        record(tag + ":rstd", got.rstd, W.rstd, 5e-6 * float(W.rstd.max()))
        record(tag + ":pmax", got.pmax, W.pmax, C.APPLY_TOL + 2 * W.tol_y)


@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_case_against_f64(L, dev, name):
    """Every case of the table: the result against f64, the surroundings of every output untouched, and a repeat of the call bit for bit."""
    c, I = C.BY_NAME[name], C.inputs(name)
    got = _run(L, dev, c, I)
    _against_f64(c, got)
    _same("conv_bf16x6:%s:repeat" % name, _run(L, dev, c, I), got)


# ---------------------------------------------------------------------------------------------
# bit for bit
# ---------------------------------------------------------------------------------------------
def _one_per_route(pred):
    """The first case per (entry, set of instantiations) among those pred admits."""
    seen, out = set(), []
    for c in C.CASES:
        key = (c.entry, tuple(l.inst for l in c.plan), c.plan[0].nk)
        if pred(c) and key not in seen:
            seen.add(key)
            out.append(c.name)
    return out


@pytest.mark.parametrize("name", list(dict.fromkeys(_one_per_route(lambda c: c.B >= 2 and c.pool == 1) +
                                                     [c.name for c in C.CASES if c.group in ("stream", "nblk") and c.B >= 2])))
def test_a_batch_entry_alone_is_the_entry_inside_the_batch(L, dev, name):
    """Entry b of the call has the bits of the one-entry call on it (its own bbias / in_scale / in_shift rows): output, partials and
    statistics -- on the wide kernel also when one workgroup walks through several entries."""
    c, I = C.BY_NAME[name], C.inputs(name)
    whole = _run(L, dev, c, I)
    Pt = c.P // 128
    for b in sorted({0, c.B - 1}):
        one = _run(L, dev, c, I, entries=slice(b, b + 1))
        tag = "conv_bf16x6:%s:entry%d" % (name, b)
        if c.write:
            exact(tag + ":y", one.y, whole.y[b:b + 1])
        if c.G:
            exact(tag + ":part", one.part.view(1, Pt * c.Cout * 4), whole.part.view(c.B, Pt * c.Cout * 4)[b:b + 1])
            for f in ("scale", "shift", "pmax", "mean", "rstd"):
                exact("%s:%s" % (tag, f), getattr(one, f), getattr(whole, f)[b:b + 1])


PART = [c.name for c in C.CASES if c.entry == "part"]


@pytest.mark.parametrize("name", PART)
def test_pieces_and_grids_are_the_whole_call(L, dev, name):
    """The case's pieces on its grid of g workgroups, the one-piece call on the full grid and the one-call entry (caspr_conv1x1_x6w_f32 /
    _pooled_f32) agree bit for bit: y, partials, scale, shift, pmax, mean, rstd."""
    c, I = C.BY_NAME[name], C.inputs(name)
    mine = _run(L, dev, c, I)
    whole = _run(L, dev, c, I, pieces=[(0, c.Cout // 512, 1)], g=0)
    _same("conv_bf16x6:%s:vs_one_piece_full_grid" % name, mine, whole)
    one_call = SimpleNamespace(**{**vars(c), "entry": "x6w", "pieces": None, "g": 0, "name": c.name + ":one_call"})
    _PACKS[(one_call.name, False)] = _packs(L, dev, c, I)
    _same("conv_bf16x6:%s:vs_one_call" % name, _run(L, dev, one_call, I), whole)


@pytest.mark.parametrize("g", [1, 2, 3, 5])
@pytest.mark.parametrize("Cin", [64, 96, 128])
def test_grid_of_g_workgroups_is_the_full_grid(L, dev, Cin, g):
    """3 entries x 2 channel tiles = 6 tiles of 2 / 3 / 4 chunks on 1, 2, 3 and ntiles - 1 workgroups: y and partials of the full grid."""
    c = next(k for k in C.CASES if k.group == "stream" and k.Cout == 1024 and k.Cin == Cin and k.g == g)
    assert c.plan[0].ntiles == 6 and max(c.plan[0].nmine) == -(-6 // g)
    I = C.inputs(c.name)
    _same("conv_bf16x6:grid%d_of_6_tiles_%d_chunks" % (g, Cin // 32), _run(L, dev, c, I), _run(L, dev, c, I, g=0), ("y", "part"))


def test_an_empty_channel_tile_range_launches_nothing(L, dev):
    """mt_begin == mt_end without the remainder: accepted, nothing launched, nothing written."""
    from caspr_amd import lib
    c = next(k for k in C.CASES if k.group == "pieces" and any(m0 == m1 and not t for m0, m1, t in k.pieces))
    I = C.inputs(c.name)
    U = _buffers(L, dev, c, I)
    for m in (0, 1, 2):
        name, a = _args(c, U, _packs(L, dev, c, I), (m, m, 0))
        lib.check(_invoke(L, name, a), name)
    torch.cuda.synchronize()
    assert _is_sentinel(U.obuf) and _is_sentinel(U.ws)
    U.xbuf.zero_()


@pytest.mark.parametrize("name", [c.name for c in C.CASES if c.group == "pack"])
def test_the_nan_surrounded_pack_is_the_contiguous_one(L, dev, name):
    """The weight as a column window (col0, ldw > col0 + Cin) of a matrix that is NaN everywhere else: the packs, and so the conv's
    result, have the bits of the contiguous copy's."""
    c, I = C.BY_NAME[name], C.inputs(name)
    a, b = _packs(L, dev, c, I), _packs(L, dev, c, I, contiguous=True)
    for i, nm in enumerate(("main", "tail")):
        if a[i] is not None:
            exact("conv_bf16x6:%s:pack_%s" % (name, nm), a[i], b[i])
    _same("conv_bf16x6:%s:contiguous_pack" % name, _run(L, dev, c, I, contiguous=True), _run(L, dev, c, I))


@pytest.mark.parametrize("name", [c.name for c in C.CASES if c.group == "pack"] + [c.name for c in C.CASES if c.group == "relu" and c.relu_from == 24])
def test_through_ops_it_is_the_same_call(ops, L, dev, name):
    """ops.conv1x1 / ops.conv1x1_gn with _X6_MIN_CIN and the wide kernel's thresholds lowered reach the same kernels: the bits of the
    direct call, and conv1x1_gn's y is conv1x1's."""
    c, I = C.BY_NAME[name], C.inputs(name)
    direct = _run(L, dev, c, I)
    w, ldw, col0 = _weight_on_device(c, I, dev, False)
    pw = ops.PackedWeight(w, col0=col0, ncols=c.Cin)
    assert pw.x6_ok and pw.x6_gn_ok and pw.x6w_ok == (c.Cout >= 512)
    U = _buffers(L, dev, c, I)
    kw = dict(bbias=U.bb, in_scale=U.sc, in_shift=U.sh, in_relu=c.in_relu, in_relu_from=c.relu_from)
    assert ops._conv_route(pw, c.B, c.P, c.relu_from) == ("x6w" if c.Cout >= 512 else "x6")
    y = ops.conv1x1(pw, U.b, U.x, **kw)
    gn = ops.conv1x1_gn(pw, U.b, U.x, torch.ones(c.Cout, device=dev) if U.gamma is None else U.gamma,
                        torch.zeros(c.Cout, device=dev) if U.beta is None else U.beta, groups=4, want_max=True, want_moments=True, **kw)
    torch.cuda.synchronize()
    w.zero_()
    U.xbuf.zero_()
    exact("conv_bf16x6:%s:ops_gn_y_is_conv_y" % name, gn[0], y)
    exact("conv_bf16x6:%s:ops_y_is_direct_y" % name, y[:, :, :c.Cout], direct.y)
    if c.G:
        for i, f in ((1, "scale"), (2, "shift"), (3, "mean"), (4, "rstd"), (5, "pmax")):
            exact("conv_bf16x6:%s:ops_%s_is_direct" % (name, f), gn[i], getattr(direct, f))


# ---------------------------------------------------------------------------------------------
# refusals: every CASPR_REQUIRE of conv_x6_launch, conv_gn_x6_impl, conv_x6w_impl and conv_x6w_part_impl, before any launch
# ---------------------------------------------------------------------------------------------
def _refusals(L, dev, c, table):
    """Each (what, message pattern, overrides) of `table` on case c's call: an error through lib.check, every output untouched."""
    from caspr_amd import lib
    I = C.build_inputs(c)
    packs = _packs(L, dev, c, I)
    U = _buffers(L, dev, c, I)
    piece = c.pieces[0] if c.pieces else None
    for what, match, over in table:
        name, a = _args(c, U, packs, piece)
        for k, v in over.items():
            assert k in a, k
            a[k] = a[k] + v[1] if isinstance(v, tuple) else v       # ("+", n): a pointer moved by n bytes
        rc = _invoke(L, name, a, U.x)
        with pytest.raises(lib.CasprHipError, match=match):
            lib.check(rc, what)
        torch.cuda.synchronize()
        outs = [U.obuf] + ([U.ws, U.scale, U.shift, U.pmax, U.mean, U.rstd] if c.G else [])
        assert all(_is_sentinel(t) for t in outs), "%s launched something before it refused" % what
    U.xbuf.zero_()


COMMON = [        # the checks conv_x6_launch, conv_x6w_impl and conv_x6w_part_impl share (messages differ in their prefix only)
    ("Cin % 32 != 0", "Cin %% 32|Cin % 32", dict(Cin=48)),
    ("Cout % 4 != 0", "Cout %% 4|Cout % 4", dict(Cout=None)),
    ("P % 128 != 0", "P %% 128|P % 128", dict(P=100)),
    ("ldx % 4 != 0", "ldx|row strides", dict(ldx=None)),
    ("ldx < Cin", "ldx|row strides", dict(ldx=32)),
    ("ldy < Cout", "ldy|row strides", dict(ldy=None)),
    ("ldy % 4 != 0", "ldy|row strides", dict(ldy=None)),
    ("in_scale without in_shift", "given together", dict(in_shift=0)),
    ("in_shift without in_scale", "given together", dict(in_scale=0)),
    ("X off by one float", "16-byte aligned", dict(X=("+", 4))),
    ("Y off by one float", "16-byte aligned", dict(Y=("+", 4))),
    ("bias off by one float", "16-byte aligned", dict(bias=("+", 4))),
    ("bbias off by one float", "16-byte aligned", dict(bbias=("+", 4))),
    ("in_relu_from = 4", "multiple of 8", dict(in_relu_from=4)),
    ("in_relu_from = -8", "multiple of 8", dict(in_relu_from=-8)),
    ("B = 0", "bad arguments", dict(B=0)),
    ("X = NULL", "bad arguments", dict(X=0)),
]


def _common(c, main="wpk"):
    """COMMON with case c's numbers filled in."""
    fill = {"Cout % 4 != 0": dict(Cout=c.Cout + 2), "ldx % 4 != 0": dict(ldx=c.Cin + 6), "ldy < Cout": dict(ldy=c.Cout - 4), "ldy % 4 != 0": dict(ldy=c.Cout + 6)}
    return [(w, m, dict(fill.get(w, o))) for w, m, o in COMMON] + [("the pack off by one float", "16-byte aligned", {main: ("+", 4)}),
                                                                   ("the pack = NULL", "bad arguments", {main: 0})]


def test_refusals_of_the_256_channel_entry(L, dev):
    c = C.make_case("refused", "x6", 2, 128, 64, 132, True, True, 8, seed=5)
    _refusals(L, dev, c, _common(c) + [
        ("Y = NULL", "Y is NULL", dict(Y=0)),
        ("2^31 tiles", "too many tiles", dict(B=1 << 21, P=128 << 10)),
    ])


def test_refusals_of_the_statistics_entries(L, dev):
    c = C.make_case("refused", "x6gn", 2, 128, 64, 132, True, True, 8, G=4, seed=6)
    _refusals(L, dev, c, [          # conv_gn_x6_impl's own checks (conv_x6_launch's: the test above)
        ("gamma = NULL", "bad arguments", dict(gamma=0)),
        ("G = 0", "bad arguments", dict(G=0)),
        ("ws = NULL", "bad arguments", dict(ws=0)),
        ("G does not divide Cout", "not a multiple of the 5 groups", dict(G=5)),
        ("mean without rstd", "mean / rstd", dict(rstd=0)),
        ("rstd without mean", "mean / rstd", dict(mean=0)),
        ("B beyond the finalize's grid", "B too large", dict(B=65536)),
        ("workspace one byte short", "workspace too small", dict(ws_bytes=2 * 132 * 16 - 1)),
        ("workspace off by one float", "misaligned", dict(ws=("+", 4))),
    ])
    c2 = C.make_case("refused", "x6gn", 4, 128, 64, 132, True, True, 8, G=4, pool=2, seed=7)
    _refusals(L, dev, c2, [("pool = 3 does not divide B = 4", "pool=3 must divide", dict(pool=3)), ("pool = 0", "pool=0 must divide", dict(pool=0)),
                           ("B beyond the finalize's grid, pooled", "B too large", dict(B=65535 * 2 + 2))])


def test_refusals_of_the_512_channel_entries(L, dev):
    c = C.make_case("refused", "x6w", 2, 128, 64, 512 + 20, True, True, 8, G=4, seed=8)
    _refusals(L, dev, c, _common(c, "wpk_main") + [
        ("Cout < 512", "needs >= 512 channels", dict(Cout=508)),
        ("a remainder without its pack", "the bf16x3 pack of the remainder", dict(wpk_tail=0)),
        ("the remainder's pack off by one float", "16-byte aligned", dict(wpk_tail=("+", 4))),
        ("Cin = 32 on the bf16x6 wide entry", "needs Cin", dict(Cin=32)),
        ("2^31 tiles", "too many tiles", dict(B=1 << 21, P=128 << 10)),
        ("gamma = NULL", "bad GroupNorm arguments", dict(gamma=0)),
        ("G does not divide Cout", "bad GroupNorm arguments", dict(G=8)),
        ("mean without rstd", "bad GroupNorm arguments", dict(rstd=0)),
        ("workspace one byte short", "workspace too small", dict(ws_bytes=2 * 532 * 16 - 1)),
        ("workspace off by one float", "workspace too small or misaligned", dict(ws=("+", 4))),
        ("no statistics and Y = NULL", "Y is NULL", dict(G=0, Y=0)),
    ])
    c2 = C.make_case("refused", "x6w", 4, 128, 64, 512 + 20, True, True, 8, G=4, pool=2, seed=9)
    _refusals(L, dev, c2, [("pool = 3 does not divide B = 4", "pool=3 must divide", dict(pool=3)), ("pool = 0", "pool=0 must divide", dict(pool=0)),
                           ("G = 0 on the pooled entry", "G > 0", dict(G=0)),
                           ("B beyond the finalize's grid, pooled", "too many tiles", dict(B=65535 * 2 + 2))])


def test_refusals_of_the_part_entry(L, dev):
    c = C.make_case("refused", "part", 2, 128, 64, 1024 + 20, True, True, 8, G=4, pieces=[(0, 2, 1)], seed=10)
    _refusals(L, dev, c, _common(c, "wpk_main") + [
        ("Cout < 512", "bad arguments", dict(Cout=508)),
        ("a remainder without its pack", "bad arguments", dict(wpk_tail=0)),
        ("the remainder's pack off by one float", "16-byte aligned", dict(wpk_tail=("+", 4))),
        ("Cin = 32 on the bf16x6 wide entry", "needs Cin", dict(Cin=32)),
        ("mt_begin = -1", "channel tiles -1..1 of 2", dict(mt_begin=-1, mt_end=1)),
        ("mt_begin > mt_end", "channel tiles 2..1 of 2", dict(mt_begin=2, mt_end=1)),
        ("mt_end > Cmain / 512", "channel tiles 0..3 of 2", dict(mt_end=3)),
        ("2^31 tiles", "too many tiles", dict(B=1 << 20, P=128 << 10)),
        ("workspace one byte short", "workspace too small", dict(ws_bytes=2 * 1044 * 16 - 1)),
        ("workspace off by one float", "16-byte aligned", dict(ws=("+", 4))),
        ("ws = NULL", "workspace too small", dict(ws=0)),
    ])
