"""The cases of tests/conv_bf16x6_cases.py, checked on the CPU (no GPU, no marker).

(a) Table: size, unique names.
(b) Coverage: every instantiation of the three kernels is reached (by x6_plan, the host's mirror), and on each instantiation every class
    the mirror names -- x6: full / half / dead wave; tail: 1 .. 4 live row tiles, a last workgroup with one tile; x6w: 2 / odd / even
    chunk counts, two or more tiles per workgroup, workgroups with different tile counts -- and on each fused instantiation every
    in_relu_from class: before, between, inside and after the 32-k chunks, inside a 16-k step.
(c) Mirror: x6_plan on both sides of each host condition.
(d) Conditioning: the same graph in f32 torch on the CPU stays within HALF the bounds the GPU test uses.
(e) Discrimination: every mutation of the reference that applies to a case is at least 10 bounds away from it in what the GPU test
    observes of that case, and applies to at least one case per kernel.
"""
import pytest
import torch

import conv_bf16x6_cases as C
from test_hip_parity import REPORT


def test_table_size_and_names():
    assert len(C.CASES) <= 200, "%d GPU cases" % len(C.CASES)
    assert len({c.name for c in C.CASES}) == len(C.CASES)
    assert all(c.B * c.P <= 3 * 256 or c.group == "nblk" for c in C.CASES)           # the block-count cases need 7 and 9 point tiles
    assert all(l.inst in C.INSTANTIATIONS for c in C.CASES for l in c.plan)


def _launches(inst):
    return [(c, l) for c in C.CASES for l in c.plan if l.inst == inst]


def test_coverage_of_every_instantiation_and_class():
    missing = []
    for inst in C.INSTANTIATIONS:
        ls = _launches(inst)
        if not ls:
            missing.append((inst, "not reached"))
            continue
        kernel, fused = inst.split("<")[0], "<true" in inst
        have = set()
        for c, l in ls:
            if kernel == "x6":
                have |= l.waves
            elif kernel == "tail":
                have |= {"nrt%d" % l.nrt, "chunks_" + l.chunks} | ({"last_workgroup_one_tile"} if l.last_single else set())
            else:
                have |= {"chunks_" + l.chunks} | ({"nmine>=2"} if max(l.nmine) >= 2 else set()) | ({"nmine_differs"} if len(set(l.nmine)) > 1 else set())
            if fused and c.in_relu:
                have.add(C.relu_class(c.relu_from, c.Cin))
            if fused and not c.in_relu:
                have.add("affine")
        need = {"x6": {"full", "half", "dead"},
                "tail": {"nrt1", "nrt2", "nrt3", "nrt4", "last_workgroup_one_tile", "chunks_two", "chunks_odd"},
                "x6w": {"chunks_two", "chunks_odd", "chunks_even"}}[kernel]
        if inst.endswith(",true>") and kernel == "x6w":          # the part entry (grids of 1, 2, 3, ntiles - 1) always leaves partials
            need |= {"nmine>=2", "nmine_differs"}
        if fused:
            need |= set(C.RELU_CLASSES)
        missing += [(inst, n) for n in sorted(need - have)]
    assert not missing, "not reached: %s" % missing
    # what one instantiation or another has to reach
    tails = [l for c in C.CASES for l in c.plan if l.kernel == "tail"]
    assert {l.chunks for l in tails} >= {"one", "two", "odd"} and any(l.nk == 5 for l in tails)
    x6 = [(c, l) for c in C.CASES for l in c.plan if l.kernel == "x6"]
    assert {l.nblk for c, l in x6 if c.entry == "x6"} >= {1, 3, 7, 9, 18}
    assert {l.nk for c, l in x6} >= {1, 2, 3}
    assert any(l.c0 > 0 and l.C % 256 for c, l in x6), "no ragged last tile behind the 512-channel kernel"
    for kernel in C.KERNELS:                                   # affine without the ReLU on each kernel
        assert any(c.fused and not c.in_relu and kernel in c.kernels for c in C.CASES), kernel
    stream = [c for c in C.CASES if c.group == "stream"]
    for nk in (2, 3, 4):                                       # one workgroup crossing entries and channel tiles, odd and even chunk counts
        assert any(c.g == 1 and c.B == 3 and c.Cout == 1024 and c.Cin == 32 * nk for c in stream), nk
    assert {c.g for c in stream if c.Cout == 1024} == {1, 2, 3, 5} and all(c.plan[0].ntiles == 6 for c in stream if c.Cout == 1024)
    assert any(not c.write for c in C.CASES if "tail" in c.kernels) and any(not c.write for c in C.CASES if c.entry == "x6gn")
    assert any(not c.write for c in C.CASES if "x6w" in c.kernels)
    assert any(any(m0 == m1 for m0, m1, _ in c.pieces) for c in C.CASES if c.pieces)


def test_what_the_issue_lists_is_in_the_table():
    have = lambda **kw: any(all(getattr(c, k) == v for k, v in kw.items()) for c in C.CASES)
    assert all(have(entry="x6", Cin=ci, Cout=co) for ci in (32, 64) for co in C.X6_COUT)
    assert all(have(entry="x6", Cin=96, Cout=co) for co in C.X6_COUT_HALF) and len(C.X6_COUT_HALF) * 2 == len(C.X6_COUT)
    assert have(entry="x6", Cout=132, act=1, fused=False) and have(entry="x6", Cout=132, act=1, fused=True)
    for co in (64, 132, 260, 508):
        assert all(have(entry="x6gn", Cout=co, write=w, fused=f) for w in (False, True) for f in (False, True))
    for ct in C.X6_REMAINDER:
        assert have(entry="x6w", Cin=64, Cout=512 + ct, fused=False, G=0) and have(entry="x6w", Cin=64, Cout=512 + ct, fused=True, G=4)
    assert all(have(entry="x6w", Cin=ci, Cout=512 + ct) for ci in (64, 96, 160) for ct in C.TAIL_COUT)
    assert have(entry="h3w", Cin=32)
    tails = [(c, l) for c in C.CASES for l in c.plan if l.kernel == "tail"]
    assert {c.B * l.Pt for c, l in tails} >= {1, 2, 3}
    assert all(have(entry="x6w", Cin=ci, Cout=co, B=b, P=p) for ci in (64, 96, 128, 160) for co in (512, 1024) for b, p in ((1, 128), (3, 128), (2, 256)))
    for entry, G in (("x6", 0), ("x6gn", 4), ("x6w", 0), ("x6w", 4)):
        assert all(have(group="relu", entry=entry, G=G, in_relu=True, relu_from=k) for k in (0, 8, 16, 24, 32, 40, 88, 96))
        assert have(group="relu", entry=entry, G=G, fused=True, in_relu=False)
    assert all(have(group="pack", entry=e, col0=k) for e in ("x6", "x6w") for k in (0, 4))
    assert all(c.ldw > c.col0 + c.Cin and c.Cout % 256 for c in C.CASES if c.group == "pack")


def test_the_mirror_at_the_hosts_conditions():
    """x6_plan on both sides of every condition of the host wrappers (what the mirror says, spelt out for the reader who compares)."""
    p = C.x6_plan
    kinds = lambda plan: [(l.kernel, l.c0, l.C, l.cstride) for l in plan]
    # conv_x6_launch: Mt = ceil(Cout / 256), Pt = P / 128, one block per (mt, pt, b); cstride = Cout
    a, = p("x6", 3, 384, 64, 260, False, False)
    assert (a.Mt, a.Pt, a.nblk, a.cstride, a.inst) == (2, 3, 18, 260, "x6<false,false>")
    assert p("x6", 1, 128, 32, 256, True, False)[0].Mt == 1 and p("x6gn", 1, 128, 32, 260, True, True)[0].inst == "x6<true,true>"
    # the wave classes: live = co_w < Cout, half = co_w + 64 >= Cout
    w = lambda co: p("x6", 1, 128, 32, co, False, False)[0].waves
    assert w(4) == {"half", "dead"} and w(64) == {"half", "dead"} and w(68) == {"full", "dead"} and w(128) == {"full", "dead"}
    assert w(132) == {"full", "half"} and w(192) == {"full", "half"} and w(196) == {"full"} and w(256) == {"full"}
    assert w(260) == {"full", "half", "dead"} and w(508) == {"full"}
    # conv_x6w_impl: Cmain = Cout - Cout % 512 on the wide kernel; a remainder <= 64 on the tail kernel, above on x6; both with cstride = Cout
    assert kinds(p("x6w", 2, 128, 64, 512, False, False)) == [("x6w", 0, 512, 512)]
    assert kinds(p("x6w", 2, 128, 64, 576, False, False)) == [("x6w", 0, 512, 576), ("tail", 512, 64, 576)]
    assert kinds(p("x6w", 2, 128, 64, 580, False, True)) == [("x6w", 0, 512, 580), ("x6", 512, 68, 580)]
    assert kinds(p("x6w", 2, 128, 64, 1540, True, True)) == [("x6w", 0, 1536, 1540), ("tail", 1536, 4, 1540)]
    assert [l.inst for l in p("x6w", 2, 128, 64, 580, True, False)] == ["x6w<true,false>", "x6<true,false>"]
    assert [l.inst for l in p("h3w", 2, 128, 32, 532, True, True)] == ["tail<true,true>"]
    # conv_x6w_part_impl: always partials; an empty range launches nothing; the remainder only with with_tail
    assert [l.inst for l in p("part", 2, 128, 64, 1060, False, False, [(0, 1, 0), (1, 1, 0), (1, 2, 1)])] == ["x6w<false,true>", "x6w<false,true>", "tail<false,true>"]
    assert kinds(p("part", 2, 128, 64, 1060, False, True, [(1, 1, 0)])) == [] and kinds(p("part", 2, 128, 64, 1060, False, True, [(1, 1, 1)])) == [("tail", 1024, 36, 1060)]
    assert kinds(p("part", 2, 128, 64, 1060, False, True, [(1, 2, 0)])) == [("x6w", 512, 512, 1060)]
    # caspr_conv_x6w_launch: gridDim = min(ntiles, n_cu - reserve_cus), workgroup w takes tiles w, w + G, ...
    n = lambda g, B=3, Mt=2: p("part", B, 128, 64, 512 * Mt, False, True, [(0, Mt, 1)], g)[0].nmine
    assert n(0) == [1] * 6 and n(1) == [6] and n(2) == [3, 3] and n(3) == [2, 2, 2] and n(5) == [2, 1, 1, 1, 1] and n(6) == [1] * 6 and n(7) == [1] * 6
    assert n(4) == [2, 2, 1, 1]
    assert [p("x6w", 1, 128, ci, 512, False, False)[0].chunks for ci in (64, 96, 128, 160, 192)] == ["two", "odd", "even", "odd", "even"]
    # conv_x6tail_launch: two tiles per workgroup, nrt = ceil(Cout / 16)
    t = lambda ct, B=1, P=128, ci=64: p("x6w", B, P, ci, 512 + ct, False, False)[1]
    assert [t(ct).nrt for ct in (4, 16, 20, 32, 36, 48, 52, 64)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert (t(4).nblk, t(4).last_single) == (1, True) and (t(4, 2).nblk, t(4, 2).last_single) == (1, False) and (t(4, 3).nblk, t(4, 3).last_single) == (2, True)
    assert (t(4, 1, 384).nblk, t(4, 1, 384).Pt) == (2, 3)
    assert [t(4, ci=ci).chunks for ci in (32, 64, 96, 128, 160)] == ["one", "two", "odd", "even", "odd"]
    # relu classes
    assert [C.relu_class(k, 96) for k in (0, 8, 16, 24, 32, 40, 88, 96)] == ["before_first_chunk", "inside_step", "inside_chunk", "inside_step",
                                                                              "between_chunks", "inside_step", "inside_step", "after_last_chunk"]


def _f32_shares(c):
    """The f32 torch evaluation of the whole graph (conv; moments, scale / shift, each rounded to f32, applied to the exact output)."""
    I, R = C.inputs(c.name), C.want(c.name)
    y32 = C.conv(c, I, torch.float32)
    sc, sh = C.statistics(c, I, y32) if c.G else (None, None)
    assert y32.dtype == torch.float32 and (sc is None or sc.dtype == torch.float32)
    return C.shares(c, I, R, y32, sc, sh)


@pytest.mark.parametrize("name", [c.name for c in C.CASES])
def test_conditioning(name):
    c = C.BY_NAME[name]
    I, R = C.inputs(name), C.want(name)
    assert bool(torch.isfinite(R.y).all())
    for what, share in _f32_shares(c).items():
        assert share <= 0.5, "case %s: the f32 evaluation's %s is at %.2f of the bound (half allowed): change its inputs" % (name, what, share)
    if c.fused:
        neg = float((I.x.double() * I.sc.double().unsqueeze(1) + I.sh.double().unsqueeze(1) < 0).double().mean())
        assert 0.4 <= neg <= 0.6, "case %s: %.2f of the transformed inputs are negative" % (name, neg)
        assert bool((I.sc > 0).any()) and bool((I.sc < 0).any())
        if c.B > 1:
            assert float((I.sc[0] - I.sc[1]).abs().min()) > 0.0
    if c.act == 1:
        pre = torch.logit(R.y.clamp(1e-12, 1 - 1e-12))
        assert float(pre.min()) < -10.0 and float(pre.max()) > 10.0, "case %s: the sigmoid's tails are not met" % name
    if c.B > 1 and c.bbias:
        assert float((I.bb[0] - I.bb[1]).abs().min()) > 0.0 and float((I.bb[0] - I.bb[-1]).abs().mean()) > 5.0


def test_discrimination():
    """Every applicable mutation of the reference is at least 10 bounds from it in one of the quantities the GPU test observes; each
    applies to at least one case per kernel; the smallest ratio per mutation goes into the report."""
    weak, report = [], {}
    for mut in C.MUTATIONS:
        worst, per_kernel, count = (float("inf"), None), set(), 0
        for c in C.CASES:
            if not C.applies(c, mut):
                continue
            count += 1
            per_kernel |= c.kernels
            ratio = max(C.mutated_shares(c, mut).values())
            if ratio < 10.0:
                weak.append((c.name, mut, ratio))
            if ratio < worst[0]:
                worst = (ratio, c.name)
        assert per_kernel >= set(C.KERNELS), "%s applies to no case of %s" % (mut, sorted(set(C.KERNELS) - per_kernel))
        report[mut] = {"cases": count, "smallest_ratio_to_bound": worst[0], "case": worst[1]}
        print("conv_bf16x6: %-32s %3d cases, smallest distance %.1f bounds (%s)" % ((mut, count) + worst))
    REPORT["conv_bf16x6:discrimination"] = report
    assert not weak, "mutations closer than 10 bounds: %s" % weak
