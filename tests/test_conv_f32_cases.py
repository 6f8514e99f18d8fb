"""The cases of tests/conv_f32_cases.py, checked on the CPU (no GPU, no marker).

(a) Coverage: the table reaches every instantiation behind caspr_conv1x1_f32 (by f32_route, the dispatcher's mirror), and the
    LDS-tiled kernel plain, fused and row-invariant.
(b) Boundaries: every boundary value of P, Cout and Cin appears on every kernel that accepts it, with the other dimensions ragged.
(c) Conditioning: the same graph in f32 torch on the CPU stays within HALF the case's bound of f64 -- what the GPU test holds a
    kernel to is the kernel's, not the inputs'.
(d) Discrimination: every mutation of the reference that applies to a case is at least 10 bounds away from it.
"""
import pytest
import torch

import conv_f32_cases as C
from test_hip_parity import REPORT

ALL = C.CASES + [C.LARGE]


def test_table_size_and_names():
    assert len(C.CASES) + 1 <= 200, "%d GPU cases" % (len(C.CASES) + 1)
    assert len({c.name for c in ALL}) == len(ALL)
    assert all(c.route in C.ROUTES for c in ALL)


def test_coverage_of_every_instantiation():
    reached = {c.route for c in ALL}
    assert reached == set(C.ROUTES), "not reached: %s" % sorted(set(C.ROUTES) - reached)
    lds = [c for c in C.CASES if c.route == "lds<64>"]
    assert any(not c.fused and not c.ri for c in lds) and any(c.fused and not c.ri for c in lds) and any(c.ri for c in lds)
    assert C.LARGE.route == "lds<128>"
    for route in C.ROUTES:                              # the sigmoid on every instantiation but the large-P one
        assert route == "lds<128>" or any(c.act == 1 and c.route == route for c in C.CASES), route
    for route in ("lds<64>", "stream<true,1>", "stream<true,8>"):    # every in_relu variant on every kernel with the transform
        seen = {(c.in_relu, "0" if c.relu_from == 0 else "4" if c.relu_from == 4 else "Cin" if c.relu_from == c.Cin else "Cin-4")
                for c in C.CASES if c.route == route and c.fused and c.Cin >= 12 and (c.relu_from in (0, 4) or c.relu_from >= c.Cin - 4)}
        assert seen >= {(False, "0"), (True, "0"), (True, "4"), (True, "Cin-4"), (True, "Cin")}, (route, seen)


def test_the_mirror_at_the_dispatchers_thresholds():
    """f32_route on both sides of every condition of caspr_conv1x1_f32 (what the mirror says, spelt out for the reader who compares)."""
    r = C.f32_route
    assert r(16, 512, 512, False, False) == "skinny" and r(17, 512, 512, False, False) == "lds<64>"
    assert r(16, 512, 512, True, False) == "lds<64>" and r(16, 512, 512, False, True) == "lds<64>"
    assert r(127, 64, 64, False, False) == "lds<64>" and r(128, 64, 64, False, False) == "narrow<4>"
    assert [r(128, 8, co, False, False) for co in (16, 17, 32, 33, 48, 64, 65)] == ["narrow<%d>" % n for n in (1, 2, 2, 4, 4, 4, 8)]
    assert r(128, 191, 64, False, False) == "narrow<4>" and r(128, 192, 64, False, False) == "stream<false,8>"
    assert r(128, 188, 64, True, False) == "lds<64>" and r(128, 192, 64, True, False) == "stream<true,8>"
    assert r(128, 192, 16, True, False) == "stream<true,1>" and r(128, 192, 17, False, False) == "stream<false,8>"
    assert r(128, 2048, 64, True, False) == "stream<true,8>" and r(128, 2052, 64, True, False) == "lds<64>"     # the cap on fused widths
    assert r(128, 2052, 64, False, False) == "stream<false,8>" and r(128, 2052, 4, True, False) == "lds<64>"
    assert r(300, 516, 130, False, True) == "lds<64>" and r(300, 8, 5, False, True) == "lds<64>"
    assert r(65535 * 64, 4, 4, True, False) == "lds<64>" and r(65535 * 64 + 1, 4, 4, True, False) == "lds<128>"
    assert r(65535 * 128, 4, 4, True, False) == "lds<128>" and r(C.REFUSED_P, 4, 4, True, False) == "refused"


ACCEPTS = {      # the unfused, unflagged shapes a kernel takes
    "skinny": lambda P, Cin: P <= 16,
    "narrow": lambda P, Cin: P >= 128 and Cin < 192,
    "stream": lambda P, Cin: P >= 128 and Cin >= 192,
    "lds": lambda P, Cin: 16 < P < 128,
}


@pytest.mark.parametrize("kern", C.KERNELS)
def test_boundary_values_on_every_kernel_that_accepts_them(kern):
    mine = [c for c in C.CASES if C.kernel_of(c.route) == kern and not c.fused and not c.ri]
    assert all(ACCEPTS[kern](c.P, c.Cin) for c in mine)
    ragged = {"P": lambda c: c.P % 16 != 0, "Cin": lambda c: c.Cin % 4 != 0, "Cout": lambda c: c.Cout % 4 != 0}
    missing = []
    for dim, values in (("P", C.P_EDGES), ("Cout", C.COUT_EDGES), ("Cin", C.CIN_EDGES + (C.STREAM_K_EDGES if kern == "stream" else ()))):
        for v in values:
            if dim == "P" and not any(ACCEPTS[kern](v, ci) for ci in (37, 197)):
                continue
            if dim == "Cin" and not any(ACCEPTS[kern](p, v) for p in (13, 77, 141)):
                continue
            others = [d for d in ragged if d != dim]
            if not any(getattr(c, dim) == v and all(ragged[d](c) for d in others) for c in mine):
                missing.append((dim, v))
    assert not missing, "%s: no case with the other dimensions ragged at %s" % (kern, missing)


def test_boundary_values_on_the_fused_kernels():
    """What the issue lists for the transform: the LDS-tiled kernel at P in {1, 16, 64, 65} and at P = 129 with Cin in {4, 36, 188};
    stream<true,8> at Cin in {192, 196, 284, 288, 304}; stream<true,1> at Cout in {3, 4, 16} with the sigmoid; the widths around
    GEMM_MAXC on both sides of the cap."""
    fused = [c for c in C.CASES if c.fused and not c.ri]
    have = lambda route, **kw: any(c.route == route and all(getattr(c, k) == v for k, v in kw.items()) for c in fused)
    assert all(have("lds<64>", P=p) for p in (1, 16, 64, 65))
    assert all(have("lds<64>", P=129, Cin=ci) for ci in (4, 36, 188))
    assert all(have("stream<true,8>", Cin=ci) for ci in (192, 196, 284, 288, 304))
    assert all(have("stream<true,1>", Cout=co, act=1) for co in (3, 4, 16))
    assert have("lds<64>", P=64, Cin=2048) and have("lds<64>", P=64, Cin=2052)
    for co, n in ((4, 1), (130, 8)):
        assert have("stream<true,%d>" % n, P=129, Cin=2048, Cout=co)
        assert have("lds<64>", P=129, Cin=2052, Cout=co) and have("lds<64>", P=129, Cin=2080, Cout=co)


@pytest.mark.parametrize("name", [c.name for c in ALL])
def test_conditioning(name):
    c = C.LARGE if name == C.LARGE.name else C.BY_NAME[name]
    I, y64 = C.inputs(name), C.want(name)
    assert bool(torch.isfinite(y64).all())
    err = C.distance(C.reference(c, I, torch.float32), y64)
    half = C.bound(c, y64) / 2
    assert err <= half, "case %s: the f32 evaluation is %.3e from f64 (half the bound: %.2e): change its inputs" % (name, err, half)
    if c.fused:
        neg = float((I.x.double() * I.sc.double().unsqueeze(1) + I.sh.double().unsqueeze(1) < 0).double().mean())
        # roughly half: 0.4 .. 0.6, or 0.3 .. 0.7 where fewer than 64 (entry, channel) pairs set the shifts
        lo, hi = (0.4, 0.6) if c.B * c.Cin >= 64 else (0.3, 0.7)
        assert c.B * c.P * c.Cin < 512 or lo <= neg <= hi, "case %s: %.2f of the transformed inputs are negative" % (name, neg)
        assert bool((I.sc > 0).any()) and bool((I.sc < 0).any())
    if c.act == 1 and c.Cout >= 3:
        pre = C.reference(c, I, mut="no_sigmoid")
        assert float(pre.min()) < -10.0 and float(pre.max()) > 10.0, "case %s: the sigmoid's tails are not met" % name
    if c.B > 1:
        assert float((I.bb[0] - I.bb[1]).abs().min()) > 0.0


def test_discrimination():
    """Every applicable mutation of the reference is at least 10 bounds from it; the smallest ratio goes into the report."""
    worst, weak, count = (float("inf"), None, None), [], 0
    for c in ALL:
        I, y64 = C.inputs(c.name), C.want(c.name)
        b = C.bound(c, y64)
        for mut in C.MUTATIONS:
            if not C.applies(c, mut):
                continue
            count += 1
            ratio = C.distance(C.reference(c, I, mut=mut), y64) / b
            if ratio < 10.0:
                weak.append((c.name, mut, ratio))
            if ratio < worst[0]:
                worst = (ratio, c.name, mut)
    REPORT["conv_f32:discrimination"] = {"mutated_references": count, "smallest_ratio_to_bound": worst[0], "case": worst[1], "mutation": worst[2]}
    print("conv_f32: %d mutated references, smallest distance %.1f bounds (%s, %s)" % ((count,) + worst))
    assert not weak, "mutations closer than 10 bounds: %s" % weak
