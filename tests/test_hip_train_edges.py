"""Training tier, kernel by kernel at the edges: the encoder's GroupNorm / max / column-sum kernels (gn_stats_train of csrc/gemm.hip,
gn_bwd of csrc/backward.hip, gn_rows, gn_rows_bwd, argmax_points, colsum_batched of csrc/backward_points.hip), the skinny and
in_relu_from routes of conv1x1_wgrad, and the value-only CNF layers (csrc/backward_flow_value.hip), each called directly through
its train_ops wrapper on the cases of tests/train_edge_cases.py (f64 references of the plain operation; test_train_edge_cases.py
checks the cases' input conditions and that the comparisons below refuse subtly wrong variants).

Every comparison is max |hip - f64| / max |f64| per tensor through test_hip_train.rel, recorded under "edges:<case>:<tensor>" in
that module's parity report (train_parity_report.json).  Bounds (train_edge_cases.py): CNF layers 1e-5 forward / 5e-5 gradients; encoder kernels 2e-5
forward, 5e-5 GroupNorm gradients, 1e-4 per-neighbourhood gradients; column sums 1e-5; weight gradients 3e-6.  Index outputs are
compared with torch.equal, fixed-order sums are run twice and compared bitwise, every output buffer wider or longer than its logical
shape is prefilled with a sentinel that must survive outside the logical region (the CNF wrappers document zeros in their padding
rows instead), and every input pad column holds NaN.
"""
import pytest
import torch

import train_edge_cases as E
from test_hip_train import matmul_mode  # noqa: F401  (fixture: both kernel families of the matrix products)
from test_hip_train_kernels import Checks as _Checks

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = 12345.0


class Checks(_Checks):
    prefix = "edges"


def dev(*ts):
    out = [None if t is None else t.to(DEV) for t in ts]
    return out[0] if len(out) == 1 else out


def wide(t, col0=0, extra=4, rows=None, fill=E.NAN):
    """t embedded in a wider (and, with rows, longer) device buffer of `fill`: -> (buffer, the column slice holding t's columns)."""
    C = t.shape[-1]
    buf = E.embed(t, ld=(col0 + C + 3) // 4 * 4 + extra, col0=col0, rows=rows, fill=fill).to(DEV)
    return buf, buf[..., col0:col0 + C]


def sentinel(shape, C, col0=0, extra=4):
    buf = torch.full(tuple(shape) + ((col0 + C + 3) // 4 * 4 + extra,), SENT, device=DEV)
    return buf, buf[..., col0:col0 + C]


def untouched(buf, C, col0=0, fill=SENT):
    """Nothing outside columns col0 .. col0 + C - 1 was written."""
    out = torch.cat([buf[..., :col0], buf[..., col0 + C:]], dim=-1)
    return bool(torch.isnan(out).all()) if fill != fill else bool((out == fill).all())


def errors():
    from caspr_amd.lib import CasprHipError
    return CasprHipError


# ---------------------------------------------------------------------------------------------
# gn_stats_train
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P,C,groups", E.GN_STATS_CASES)
def test_gn_stats_train_edges(B, P, C, groups):
    """Both partial kernels (rows kernel: C = 64, 1024, 16 / 4 groups; per-group kernel: cpg = 12, 100, 256), P on either side of the
    1024-row split and below the row lanes, ldy = C + 4 with NaN pads, a batch entry around 1000, gamma with negative entries and an
    exact zero for pmax.  Each batch entry is compared on its own (the entry around 1000 would hide the others' shift).

    Bound 2e-5, raised for ONE tensor: pmax of the entry around 1000.  pmax = extreme(y) scale + shift adds two numbers of size
    ~1000 |gamma| rstd to a result of size ~1, so f32 leaves ~ulp(1000) = 6e-5 absolute whatever evaluates it.  Measured, relative to
    the entry's largest pmax, over the 14 cases: this kernel 9.2e-6 .. 7.4e-5; the same formula in plain f32 torch on the CPU (the f64
    scale / shift rounded to f32, train_edge_cases.pmax_f32_error) 1.2e-5 .. 1.1e-4, above the kernel's figure in every case -- e.g.
    (3,1,64): 7.4e-5 vs 1.1e-4, (3,3,64): 5.2e-5 vs 6.1e-5, (3,1024,64): 2.1e-5 vs 2.8e-5, (3,1,4096): 2.7e-5 vs 3.6e-5.  Its bound
    is twice that case's f32-CPU figure (train_edge_cases.pmax_bound), at most 2e-4; the other entries stay at 2e-5 (both sides ~1e-7)."""
    from caspr_amd import train_ops as T
    c = E.case_gn_stats(B, P, C, groups)
    _, y = wide(c.y)
    gamma, beta = dev(c.gamma, c.beta)
    runs = [T.gn_stats_train(y, C, gamma, beta, groups=groups, want_max=True) for _ in range(2)]
    ck = Checks("gn_stats[%d,%d,%d,g%d]" % (B, P, C, groups))
    for name, a, b in zip(("scale", "shift", "mean", "rstd", "pmax"), runs[0], runs[1]):
        assert torch.equal(a, b), name + ": two runs differ"
        for e in range(B):
            ck("%s[%d]" % (name, e), a[e], c.want[name][e], E.pmax_bound(c, e) if name == "pmax" and e == B - 1 else E.ENC_FWD)
    ck.done()


def test_gn_stats_train_refusals():
    from caspr_amd import train_ops as T
    for C, ld in ((4160, 4160), (72, 72)):           # cpg = 260 > 256; C not a multiple of the 16 groups
        with pytest.raises(errors()):
            T.gn_stats_train(torch.zeros(1, 8, ld, device=DEV), C, torch.ones(C, device=DEV), torch.zeros(C, device=DEV))
    with pytest.raises(ValueError):                  # ldy % 4 != 0: the wrapper's own row check refuses it before the library sees it
        T.gn_stats_train(torch.zeros(1, 8, 66, device=DEV)[:, :, :64], 64, torch.ones(64, device=DEV), torch.zeros(64, device=DEV))


# ---------------------------------------------------------------------------------------------
# argmax_points, colsum_batched
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P,C,pairs", E.ARGMAX_CASES)
def test_argmax_points_edges(B, P, C, pairs):
    """First index on exact ties: inside a row phase (p, p + 4), across phases with the later phase first (5, 2), across the
    1024-point split (1023, 1024) and (1500, 100); all-equal columns (scale 0) -> 0; a negative scale -> the first row of the
    minimum; per-entry scale; C = 1 and 65 with ldy > C; P = 1."""
    from caspr_amd import train_ops as T
    c = E.case_argmax(B, P, C, pairs)
    _, y = wide(c.y)
    scale, shift = dev(c.scale, c.shift)
    got = [T.argmax_points(y, C, scale, shift) for _ in range(2)]
    assert torch.equal(got[0], got[1])
    assert torch.equal(got[0].cpu(), c.want), "rows that differ: %s" % (torch.nonzero(got[0].cpu() != c.want)[:8].tolist(),)


@pytest.mark.parametrize("C", E.COLSUM_C)
def test_colsum_batched_edges(C):
    """C around the 64-column block, P around the 512-row split, B = 3, NaN in the pad columns."""
    from caspr_amd import train_ops as T
    ck = Checks("colsum[C=%d]" % C)
    for P in E.COLSUM_P:
        c = E.case_colsum(3, P, C, seed=P)
        _, a = wide(c.a)
        got = [T.colsum_batched(a, C) for _ in range(2)]
        assert torch.equal(got[0], got[1])
        ck("P=%d" % P, got[0], c.want, E.COLSUM)
    ck.done()


# ---------------------------------------------------------------------------------------------
# gn_bwd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P,C", E.GN_BWD_SHAPES)
def test_gn_bwd_edges(B, P, C):
    """cpg = 4, 8, 12 (85 row lanes, one idle thread), 100 (10 row lanes), 256; P on either side of the 1024-row split, P below the
    row lanes; dA with and without the ReLU mask, dMax + amax alone into `out` (amax in the last split, in row 0, in the middle),
    both together; accumulate onto non-zero dgamma / dbeta; in place and out of place bit-equal; ldy, ldd, ldo all wider than C and
    different; the moments are the f64 reference's rounded to f32, and once the GPU forward's (gn_stats_train)."""
    from caspr_amd import train_ops as T
    c = E.case_gn_bwd(B, P, C)
    _, y = wide(c.y, extra=4)
    gamma, beta, dmax, amax = dev(c.gamma, c.beta, c.dmax, c.amax)
    mean, rstd = dev(c.mean.float(), c.rstd.float())
    ck = Checks("gn_bwd[%d,%d,%d]" % (B, P, C))

    def run(use_da, use_dmax, relu, mean=mean, rstd=rstd, init=None):
        da = wide(c.da, extra=8)[1] if use_da else None
        obuf, out = sentinel((B, P), C, extra=12)
        dg, db = (torch.full((C,), SENT, device=DEV), torch.full((C,), SENT, device=DEV)) if init is None else dev(*init)
        T.gn_bwd(y, da, C, mean, rstd, gamma, beta, dg, db, relu=relu, accumulate=init is not None,
                 dmax=dmax if use_dmax else None, amax=amax if use_dmax else None, out=out)
        assert untouched(obuf, C), "columns of `out` past C written"
        return out.clone(), dg, db

    for tag, use_da, use_dmax, relu in (("dA,relu", True, False, True), ("dA", True, False, False), ("dMax", False, True, True),
                                        ("dA+dMax,relu", True, True, True)):
        want = E.gn_bwd_want(c, use_da, use_dmax, relu)
        got, again = run(use_da, use_dmax, relu), run(use_da, use_dmax, relu)
        for name, a, b in zip(("dY", "dgamma", "dbeta"), got, again):
            assert torch.equal(a, b), "%s %s: two runs differ" % (tag, name)
            ck("%s:%s" % (tag, name), a, want[name], E.GN_GRAD)
    want = E.gn_bwd_want(c, True, False, True)
    first = run(True, False, True)
    # in place over dA: the same bits, and the pad columns of the dA buffer still hold their NaN
    dbuf, da = wide(c.da, extra=8)
    dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    assert T.gn_bwd(y, da, C, mean, rstd, gamma, beta, dg, db, relu=True) is da
    assert torch.equal(da, first[0]) and torch.equal(dg, first[1]) and torch.equal(db, first[2]), "in place differs from out of place"
    assert untouched(dbuf, C, fill=E.NAN)
    # accumulate
    _, dg, db = run(True, False, True, init=(c.dgamma0, c.dbeta0))
    ck("accumulate:dgamma", dg, want["dgamma"] + c.dgamma0.double(), E.GN_GRAD)
    ck("accumulate:dbeta", db, want["dbeta"] + c.dbeta0.double(), E.GN_GRAD)
    # the GPU forward's moments into the GPU backward
    _, _, gm, gr = T.gn_stats_train(y, C, gamma, beta, groups=c.groups)
    chained = run(True, False, True, mean=gm, rstd=gr)
    for name, a in zip(("dY", "dgamma", "dbeta"), chained):
        ck("chained:" + name, a, want[name], E.GN_GRAD)
    ck.done()


def test_gn_bwd_refusals():
    from caspr_amd import train_ops as T
    c = E.case_gn_bwd(1, 5, 64)
    y, da, gamma, beta, dmax = dev(c.y, c.da, c.gamma, c.beta, c.dmax)
    mean, rstd = dev(c.mean.float(), c.rstd.float())
    dg, db = torch.empty(64, device=DEV), torch.empty(64, device=DEV)
    with pytest.raises(ValueError):
        T.gn_bwd(y, None, 64, mean, rstd, gamma, beta, dg, db, dmax=dmax, amax=dev(c.amax))
    with pytest.raises(errors()):
        T.gn_bwd(y, da, 64, mean, rstd, gamma, beta, dg, db, dmax=dmax)


# ---------------------------------------------------------------------------------------------
# gn_rows / gn_rows_bwd
# ---------------------------------------------------------------------------------------------
def run_gn_rows(ck, tag, c, B, M, chain=False, accumulate=False):
    """One case through gn_rows (dense and max form) and gn_rows_bwd (from dA and from dMax + arg), every output against the case's f64."""
    from caspr_amd import train_ops as T
    ns, C = c.ns, c.C
    _, y = wide(c.y)
    gamma, beta = dev(c.gamma, c.beta)
    tiny = ns * (C // 16) == 1             # one-element groups: xh = 0, dY = 0 and dgamma = 0 identically
    # forward, dense
    f = [T.gn_rows(y, ns, C, gamma, beta, c.relu, eps=c.eps) for _ in range(2)]
    for a, b in zip(f[0][:3], f[1][:3]):
        assert torch.equal(a, b), tag + ": two forward runs differ"
    A, gm, gr, _ = f[0]
    ck(tag + ":A", A, c.want["A"], E.ENC_FWD)
    ck(tag + ":mean", gm, c.want["mean"], E.ENC_FWD)
    ck(tag + ":rstd", gr, c.want["rstd"], E.ENC_FWD)
    # forward, max over the ns rows into a column slice at offset 8 of a wider buffer
    mbuf, mo = sentinel((B, M), C, col0=8)
    _, gm2, gr2, arg = T.gn_rows(y, ns, C, gamma, beta, c.relu, eps=c.eps, maxout=mo)
    assert untouched(mbuf, C, col0=8), tag + ": columns of the maxout buffer outside the slice written"
    assert torch.equal(gm2, gm) and torch.equal(gr2, gr)
    assert torch.equal(arg.cpu(), c.want["arg"]), "%s: arg differs at %s" % (tag, torch.nonzero(arg.cpu() != c.want["arg"])[:8].tolist())
    ck(tag + ":max", mo, c.want["max"], E.ENC_FWD)
    if "dense" not in c.want:
        return
    # backward
    mean, rstd = (gm, gr) if chain else dev(c.want["mean"].float(), c.want["rstd"].float())
    use_arg = arg if chain else dev(c.want["arg"])
    _, dmax = wide(c.dmax, col0=4)
    for mode in ("dense", "dmax"):
        runs = []
        for _ in range(2):
            obuf, out = sentinel(c.y.shape[:2], C)
            init = (c.dgamma0, c.dbeta0) if accumulate else (torch.full((C,), SENT), torch.full((C,), SENT))
            dg, db = dev(*init)
            T.gn_rows_bwd(y, ns, C, gamma, beta, c.relu, mean, rstd, dg, db, da=wide(c.da, extra=8)[1] if mode == "dense" else None,
                          dmax=dmax if mode == "dmax" else None, arg=use_arg if mode == "dmax" else None, out=out, accumulate=accumulate)
            assert untouched(obuf, C), tag + ": columns of dY past C written"
            runs.append((out.clone(), dg, db))
        for a, b in zip(*runs):
            assert torch.equal(a, b), "%s %s: two backward runs differ" % (tag, mode)
        want = c.want[mode]
        add = (c.dgamma0.double(), c.dbeta0.double()) if accumulate else (0.0, 0.0)
        ck("%s:%s:dY" % (tag, mode), runs[0][0], want["dY"], E.ROWS_GRAD, ref=E.dy_scale(c, mode) if tiny else None)
        ck("%s:%s:dgamma" % (tag, mode), runs[0][1], want["dgamma"] + add[0], E.ROWS_GRAD,
           ref=float(want["dbeta"].abs().max()) if tiny and not accumulate else None)
        ck("%s:%s:dbeta" % (tag, mode), runs[0][2], want["dbeta"] + add[1], E.ROWS_GRAD)


@pytest.mark.parametrize("C", E.ROWS_C)
def test_gn_rows_edges(C):
    """All seven instantiations (cpg = 1, 2, 4, 6, 8, 16, 32), ns = 1, 2, 3 (empty row phases), 5 (ragged), 16, 33, one neighbourhood
    and five, ReLU on and off in both directions.  ns = 5, NB = 5 runs chained (the GPU forward's mean / rstd / arg into the GPU
    backward); ns = 3 accumulates onto non-zero dgamma / dbeta."""
    ck = Checks("gn_rows[C=%d]" % C)
    for ns in E.ROWS_NS:
        for NB in E.ROWS_NB:
            for relu in (False, True):
                c = E.small_rows_case(1, NB, ns, C, relu)
                run_gn_rows(ck, "ns=%d,NB=%d,relu=%d" % (ns, NB, relu), c, 1, NB, chain=(ns == 5 and NB == 5), accumulate=(ns == 3))
    ck.done()


@pytest.mark.parametrize("C,ns,dup", E.ROWS_DUP)
def test_gn_rows_repeated_rows(C, ns, dup):
    """Neighbourhoods whose last rows repeat row 0 (the ball query's padding), up to one row repeated ns times, and pairs of equal rows
    whose later one sits in an earlier row phase ((2, 5), (3, 4)): arg is the first
    occurrence, the dMax gradient enters at that row only, the dense gradient matches autograd.  Two batch entries of three
    neighbourhoods: maxout and dmax are column slices of (B, M, .) buffers."""
    ck = Checks("gn_rows_dup[%d,%d,%s]" % (C, ns, dup))
    for relu in (False, True):
        c = E.first_seed(lambda s: E.case_gn_rows(2, 3, ns, C, relu, "lattice" if relu else "normal", dup, s, E.rows_eps(ns, C)), E.rows_case_ok)
        assert not bool(torch.isin(c.want["arg"], torch.tensor(E.repeated_rows(ns, dup), dtype=torch.int32)).any())
        run_gn_rows(ck, "relu=%d" % relu, c, 2, 3)
    ck.done()


@pytest.mark.parametrize("direction,mode,C,ns", [("fwd", "dense", 16, 2), ("fwd", "max", 16, 2), ("bwd", "dense", 16, 2), ("bwd", "dmax", 16, 2),
                                                 ("bwd", "both", 512, 1)])
def test_gn_rows_grid_stride(direction, mode, C, ns):
    """More neighbourhoods than the capped grids have waves (forward: 8192 workgroups x 4, backward: 2048 x 4, + 3): the grid-stride
    loops run, the backward accumulates dgamma / dbeta across a wave's neighbourhoods."""
    from caspr_amd import train_ops as T
    c = E.stride_rows_case(direction, C, ns)
    ck = Checks("gn_rows_stride[%s,%s,%d,%d]" % (direction, mode, C, ns))
    if direction == "fwd":
        y, gamma, beta = dev(c.y, c.gamma, c.beta)
        if mode == "dense":
            A, gm, gr, _ = T.gn_rows(y, ns, C, gamma, beta, True, eps=c.eps)
            ck("A", A, c.want["A"], E.ENC_FWD)
            ck("mean", gm, c.want["mean"], E.ENC_FWD)
            ck("rstd", gr, c.want["rstd"], E.ENC_FWD)
        else:
            mbuf, mo = sentinel((1, c.NB), C, col0=8)
            arg = T.gn_rows(y, ns, C, gamma, beta, True, eps=c.eps, maxout=mo)[3]
            assert untouched(mbuf, C, col0=8)
            assert torch.equal(arg.cpu(), c.want["arg"]), "arg differs at %s" % (torch.nonzero(arg.cpu() != c.want["arg"])[:8].tolist(),)
            ck("max", mo, c.want["max"], E.ENC_FWD)
    else:
        y, gamma, beta = dev(c.y, c.gamma, c.beta)
        mean, rstd = dev(c.want["mean"].float(), c.want["rstd"].float())
        for m in (("dense", "dmax") if mode == "both" else (mode,)):
            runs = []
            for _ in range(2):
                dg, db = torch.full((C,), SENT, device=DEV), torch.full((C,), SENT, device=DEV)
                out = torch.full(tuple(c.y.shape), SENT, device=DEV)
                T.gn_rows_bwd(y, ns, C, gamma, beta, True, mean, rstd, dg, db, da=dev(c.da) if m == "dense" else None,
                              dmax=dev(c.dmax) if m == "dmax" else None, arg=dev(c.want["arg"]) if m == "dmax" else None, out=out)
                runs.append((out, dg, db))
            for name, a, b in zip(("dY", "dgamma", "dbeta"), *runs):
                assert torch.equal(a, b), "%s %s: two runs differ" % (m, name)
                ck("%s:%s" % (m, name), a, c.want[m][name], E.ROWS_GRAD)
    ck.done()


def test_gn_rows_refusals():
    from caspr_amd import train_ops as T
    for C in (48, 24):                                # C / 16 = 3 is not instantiated; 24 is not a multiple of the 16 groups
        y = torch.zeros(1, 8, C, device=DEV)
        g, b = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        with pytest.raises(errors()):
            T.gn_rows(y, 4, C, g, b, True)
        with pytest.raises(errors()):
            T.gn_rows_bwd(y, 4, C, g, b, True, torch.zeros(2, 16, device=DEV), torch.ones(2, 16, device=DEV), torch.empty(C, device=DEV),
                          torch.empty(C, device=DEV), da=torch.zeros(1, 8, C, device=DEV))


# ---------------------------------------------------------------------------------------------
# conv1x1_wgrad: the skinny route and in_relu_from
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P,Cin,Cout", E.WGRAD_SKINNY)
def test_conv1x1_wgrad_skinny(B, P, Cin, Cout):
    """conv1x1_wgrad_skinny_kernel (Cout <= 4, Cin >= 256, Cin % 4 == 0, no input transform, no bias gradient): Cin with a partial
    256-channel chunk, rows that are no multiple of the four waves or of the slab, one row slab and several; plain, accumulate,
    two runs bit-equal.  x carries NaN pad columns."""
    from caspr_amd import train_ops as T
    c = E.case_wgrad_skinny(B, P, Cin, Cout)
    _, x = wide(c.x)
    dy = dev(c.dy)
    ck = Checks("wgrad_skinny[%d,%d,%d,%d]" % (B, P, Cin, Cout))
    runs = [T.conv1x1_wgrad(dy, x, Cin, Cout, torch.full((Cout, Cin), SENT, device=DEV)) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    ck("dW", runs[0], c.want, E.WGRAD)
    acc = T.conv1x1_wgrad(dy, x, Cin, Cout, dev(c.dw0), accumulate=True)
    ck("accumulate", acc, c.want + c.dw0.double(), E.WGRAD)
    ck.done()


@pytest.mark.parametrize("B,P,Cin,Cout,relu_from", E.WGRAD_RELU_FROM)
def test_conv1x1_wgrad_in_relu_from(matmul_mode, B, P, Cin, Cout, relu_from):
    """The three tile kernels with the channels >= in_relu_from of x scale + shift rectified and the ones below passed through
    (the encoder's head: in_relu_from = L), on both kernel families; in_relu_from = Cin rectifies nothing."""
    from caspr_amd import train_ops as T
    c = E.case_wgrad_relu_from(B, P, Cin, Cout, relu_from)
    _, x = wide(c.x)
    dy, sc, sh = dev(c.dy, c.scale, c.shift)
    ck = Checks("wgrad_relu_from[%s,%d,%d,%d,%d,from=%d]" % (matmul_mode, B, P, Cin, Cout, relu_from))
    runs = []
    for _ in range(2):
        dW, db = torch.full((Cout, Cin), SENT, device=DEV), torch.full((Cout,), SENT, device=DEV)
        T.conv1x1_wgrad(dy, x, Cin, Cout, dW, db, in_scale=sc, in_shift=sh, in_relu=True, in_relu_from=relu_from)
        runs.append((dW, db))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    ck("dW", runs[0][0], c.want["dW"], E.WGRAD)
    ck("db", runs[0][1], c.want["db"], E.WGRAD)
    ck.done()


def test_conv1x1_wgrad_in_relu_from_0_is_in_relu(matmul_mode):
    from caspr_amd import train_ops as T
    c = E.case_wgrad_relu_from(2, 300, 132, 260, 0)
    x, dy, sc, sh = dev(c.x, c.dy, c.scale, c.shift)
    a, b = torch.empty(260, 132, device=DEV), torch.empty(260, 132, device=DEV)
    T.conv1x1_wgrad(dy, x, 132, 260, a, None, in_scale=sc, in_shift=sh, in_relu=True, in_relu_from=0)
    T.conv1x1_wgrad(dy, x, 132, 260, b, None, in_scale=sc, in_shift=sh, in_relu=True)
    assert torch.equal(a, b)
    ck = Checks("wgrad_relu_from[%s,from=0]" % matmul_mode)
    ck("dW", a, c.want["dW"], E.WGRAD)
    ck.done()


# ---------------------------------------------------------------------------------------------
# the value-only CNF layers
# ---------------------------------------------------------------------------------------------
def rows128(R):
    return (R + 127) // 128 * 128


@pytest.mark.parametrize("C,n", E.CNF_GRID)
def test_cnf_in_value_edges(C, n):
    """cnf_in_value / _bwd: partial 256-channel chunks (C = 4, 132, 260), n below the four waves, the 32-point blocks of the forward
    (n = 33, 255 .. 300), 1 split (n < 256) and 8 even / uneven splits, one frame and three; the output rows rounded up to 128 with
    zero padding rows; dh a column slice of a wider and longer tensor with NaN around it."""
    from caspr_amd import train_ops as T
    ck = Checks("cnf_in_value[C=%d,n=%d]" % (C, n))
    for frames in (1, 3):
        c = E.case_cnf_in(frames, n, C)
        R, rows = c.R, rows128(c.R)
        y, w0, b, gate, beta = dev(c.y, c.w0, c.b, c.gate, c.beta)
        h = T.cnf_in_value(y, w0, b, gate, beta, n, rows=rows)
        assert tuple(h.shape) == (rows, C) and bool((h[R:] == 0).all()), "padding rows must be zero"
        ck("f=%d:h" % frames, h[:R], c.want["h"], E.FWD)
        _, dh = wide(c.dh, col0=4, rows=rows + 3)
        runs = [T.cnf_in_value_bwd(y, w0, b, gate, beta, dh, n) for _ in range(2)]
        for name, a, a2 in zip(("dy", "dW0", "dgate", "dbeta"), *runs):
            assert torch.equal(a, a2), name + ": two runs differ"
            ck("f=%d:%s" % (frames, name), a, c.want[name], E.GRAD)
    ck.done()


@pytest.mark.parametrize("C,n", E.CNF_GRID)
def test_cnf_act_value_edges(C, n):
    """cnf_act_value and cnf_act_value_bwd from dh and -- the dH == NULL form -- from dzo (>= R, 4) and wo (3, C), on the same grid,
    with z wider and longer than (R, C) (NaN around it) and beta scaled by 40 on a quarter of the channels (the softplus / sigmoid
    tails).  The padding rows of h and dz come back as zeros."""
    from caspr_amd import train_ops as T
    ck = Checks("cnf_act_value[C=%d,n=%d]" % (C, n))
    for frames in (1, 3):
        c = E.case_cnf_act(frames, n, C)
        R, rows = c.R, rows128(c.R) + 2
        z, _ = wide(c.z, rows=rows)
        b, gate, beta, wo = dev(c.b, c.gate, c.beta, c.wo)
        h = T.cnf_act_value(z, b, gate, beta, n)
        assert tuple(h.shape) == (rows, C) and bool((h[R:] == 0).all())
        ck("f=%d:h" % frames, h[:R], c.want["h"], E.FWD)
        _, dh = wide(c.dh, col0=4, rows=rows + 1)
        dzo, _ = wide(c.dzo, extra=0, rows=rows)               # (rows, 4): column 3 and the rows past R hold NaN
        assert dzo.shape[1] == 4
        for key, kw in (("dh", dict(dh=dh)), ("dzo", dict(dzo=dzo, wo=wo))):
            runs = [T.cnf_act_value_bwd(z, b, gate, beta, n, **kw) for _ in range(2)]
            for name, a, a2 in zip(("dZ", "dgate", "dbeta"), *runs):
                assert torch.equal(a, a2), "%s %s: two runs differ" % (key, name)
                if name == "dZ":
                    assert tuple(a.shape) == (rows, C) and bool((a[R:] == 0).all())
                    a = a[:R]
                ck("f=%d:%s:%s" % (frames, key, name), a, c.want[key][name], E.GRAD)
    ck.done()


@pytest.mark.parametrize("n", E.CNF_OUT_N)
def test_cnf_out_value_edges(n):
    """cnf_out_value / _bwd: n below, around and above the 256-thread block, gate / beta the first three columns of (frames, 8)
    tensors, zo (rows >= R, 4) with NaN in column 3 and past R; dzo comes back (rows, 4) with column 3 and the padding rows zero."""
    from caspr_amd import train_ops as T
    ck = Checks("cnf_out_value[n=%d]" % n)
    for frames in (1, 3):
        c = E.case_cnf_out(frames, n)
        R, rows = c.R, rows128(c.R) + 1
        zo, _ = wide(c.zo, extra=0, rows=rows)
        gate, beta = wide(c.gate, extra=4)[1], wide(c.beta, extra=4)[1]
        assert gate.stride(0) == 8 and zo.shape[1] == 4
        b, da = dev(c.b, c.da)
        a = T.cnf_out_value(zo, b, gate, beta, n)
        ck("f=%d:a" % frames, a, c.want["a"], E.FWD)
        runs = [T.cnf_out_value_bwd(da, zo, b, gate, n) for _ in range(2)]
        for name, g, g2 in zip(("dzo", "dgate", "dbeta"), *runs):
            assert torch.equal(g, g2), name + ": two runs differ"
            if name == "dzo":
                assert tuple(g.shape) == (rows, 4) and bool((g[:, 3] == 0).all()) and bool((g[R:] == 0).all())
                g = g[:R, :3]
            ck("f=%d:%s" % (frames, name), g, c.want[name], E.GRAD)
    ck.done()


def test_cnf_value_refusals():
    from caspr_amd import train_ops as T
    bad = (ValueError, errors())
    c = E.case_cnf_act(2, 5, 8)
    z, b, gate, beta, dh = dev(c.z, c.b, c.gate, c.beta, c.dh)
    y = torch.zeros(10, 3, device=DEV)
    with pytest.raises(bad):                           # C % 4 != 0
        T.cnf_in_value(y, torch.zeros(6, 3, device=DEV), torch.zeros(6, device=DEV), torch.ones(2, 6, device=DEV), torch.zeros(2, 6, device=DEV), 5)
    with pytest.raises(bad):
        T.cnf_act_value(z, torch.zeros(6, device=DEV), gate[:, :6].contiguous(), beta[:, :6].contiguous(), 5)
    with pytest.raises(bad):                           # R % n != 0
        T.cnf_in_value(y, torch.zeros(8, 3, device=DEV), b, gate, beta, 3)
    wider = torch.zeros(10, 16, device=DEV)
    with pytest.raises(bad):                           # a slice that is not 16-byte aligned
        T.cnf_act_value_bwd(z, b, gate, beta, 5, dh=wider[:, 1:9])
    with pytest.raises(bad):                           # too few rows
        T.cnf_act_value(z[:9], b, gate, beta, 5)
    with pytest.raises(bad):
        T.cnf_act_value_bwd(z, b, gate, beta, 5, dh=dh[:9])
    with pytest.raises(bad):
        T.cnf_out_value(torch.zeros(9, 4, device=DEV), torch.zeros(3, device=DEV), torch.ones(2, 3, device=DEV), torch.zeros(2, 3, device=DEV), 5)
