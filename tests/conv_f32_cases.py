"""The case table, input builders, f64 reference and dispatcher mirror for the edge tests of the f32 pointwise conv
(caspr_conv1x1_f32, csrc/gemm.hip): test_conv_f32_cases.py checks the table on the CPU, test_conv_f32_edges.py runs the kernels on it.
No GPU code is imported.

The entry is four kernels in eleven instantiations -- conv1x1_skinny_kernel, conv1x1_narrow_kernel<1|2|4|8>,
conv1x1_stream_kernel<false|true, 1|8>, conv1x1_kernel<64|128> -- chosen from P, Cin, Cout, the presence of in_scale and
CASPR_CONV_ROW_INVARIANT.  f32_route() restates that choice from the dispatcher's text, quoting its lines.  A release build cannot
report which kernel ran, so the mirror is checked BY READING: whoever changes a condition in caspr_conv1x1_f32 changes it here.

A case is (B, P, Cin, Cout) plus the fused input transform (in_scale / in_shift per entry, in_relu, in_relu_from), the epilogue
(identity / sigmoid) and row_invariant.  inputs(case) are f32 tensors of the logical shapes (the GPU tests embed them in wider
buffers); reference(case, inputs) is the plain operation in f64,

    act( in(x) @ W^T + bias + bbias[b] ),   in(x) = x                                    without in_scale
                                                  = x * in_scale[b] + in_shift[b], and max(., 0) on the channels k >= in_relu_from
                                                    if in_relu,

and MUTATIONS are subtly wrong variants of it that the case's bound has to tell from the reference by a factor of ten.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from test_hip_parity import rnd

GEMM_MAXC = 2048            # gemm.hip:56
ST_DB = 6                   # gemm.hip:300; the narrow / stream threshold is 32 * ST_DB = 192 channels
GRID_MAX = 65535
CONV_TOL = 2e-6             # x max(1, |y|max) on conv outputs (test_hip_parity.test_conv1x1)
SIGMOID_TOL = 2e-6          # after the sigmoid (test_conv1x1_fused_input_and_epilogues)
SIGMOID_SPREAD = 12.0       # bias of a sigmoid case: spread over +-12, both tails

ROUTES = ("skinny", "narrow<1>", "narrow<2>", "narrow<4>", "narrow<8>", "stream<false,1>", "stream<false,8>", "stream<true,1>",
          "stream<true,8>", "lds<64>", "lds<128>")
KERNELS = ("skinny", "narrow", "stream", "lds")


def ceil_div(a, b):
    return (a + b - 1) // b


def f32_route(P, Cin, Cout, fused, row_invariant):
    """The instantiation caspr_conv1x1_f32 launches in a release build (force == 0), condition by condition (gemm.hip line numbers)."""
    if ceil_div(P, 128) > GRID_MAX:                                            # :695  CASPR_REQUIRE(ceil_div(P, 128) <= 65535, ...)
        return "refused"
    if P <= 16 and not fused and not row_invariant:                            # :696
        return "skinny"
    if P >= 128 and Cin < 32 * ST_DB and not fused and not row_invariant:      # :707
        mt16 = ceil_div(Cout, 16)
        return "narrow<%d>" % (8 if mt16 >= 5 else 4 if mt16 >= 3 else mt16)   # :709
    if P >= 128 and Cin >= 32 * ST_DB and (not fused or Cin <= GEMM_MAXC) and not row_invariant:   # :724, with the cap on fused widths
        return "stream<%s,%d>" % ("true" if fused else "false", 1 if Cout <= 16 else 8)            # :734
    return "lds<128>" if ceil_div(P, 64) > GRID_MAX else "lds<64>"             # :745


def kernel_of(route):
    return route.split("<")[0]


def roundup4(n):
    return (n + 3) // 4 * 4


# ---------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------
P_EDGES = (16, 17, 63, 64, 65, 127, 128, 129)
COUT_EDGES = (16, 17, 48, 49, 64, 65, 127, 128, 129)
CIN_EDGES = (191, 192, 193)
STREAM_K_EDGES = (287, 288, 304)      # six masked chunks / no ragged end / a last chunk that is pure padding (ST_DB = 6 chunks of 16)
# ragged bases: P no multiple of 16, Cin no multiple of 4, Cout no multiple of 4; two point tiles where the kernel has tiles
BASE = {"skinny": (13, 37, 21), "narrow": (141, 37, 21), "stream": (141, 197, 21), "lds": (77, 37, 21)}

CASES = []
_names = set()


def _add(group, P, Cin, Cout, fused=False, in_relu=False, relu_from=0, act=0, ri=False, B=2):
    name = "%s:%dx%dx%dx%d" % (group, B, P, Cin, Cout)
    if fused:
        name += ":in%s" % (("relu%d" % relu_from) if in_relu else "affine")
    name += (":sigmoid" if act else "") + (":ri" if ri else "")
    if name in _names:
        return
    _names.add(name)
    assert not fused or Cin % 4 == 0
    assert relu_from % 4 == 0 and 0 <= relu_from <= Cin
    CASES.append(SimpleNamespace(name=name, group=group, B=B, P=P, Cin=Cin, Cout=Cout, fused=fused, in_relu=in_relu, relu_from=relu_from,
                                 act=act, ri=ri, seed=1000 + 16 * len(CASES), route=f32_route(P, Cin, Cout, fused, ri)))


def relu_variants(Cin):
    """in_relu off, and on from channel 0, 4, Cin - 4 and Cin (= nowhere)."""
    out = [(False, 0)]
    for k in (0, 4, Cin - 4, Cin):
        if (True, k) not in out:
            out.append((True, k))
    return out


def _build():
    # 1. the edge matrix: each kernel's ragged base with one dimension at a time on every boundary value the kernel accepts
    for kern, (P, Cin, Cout) in BASE.items():
        for p in (1,) + P_EDGES:
            if kernel_of(f32_route(p, Cin, Cout, False, False)) == kern:
                _add("edge", p, Cin, Cout)
        for co in COUT_EDGES:
            _add("edge", P, Cin, co)
        for ci in CIN_EDGES + STREAM_K_EDGES:
            if kernel_of(f32_route(P, ci, Cout, False, False)) == kern and (kern == "stream" or ci in CIN_EDGES):
                _add("edge", P, ci, Cout)
    for ci in (193,) + STREAM_K_EDGES:                 # the ragged K end of the one-row-tile streaming kernel
        _add("edge", 141, ci, 13)
    for p in (3, 20, 130):                             # one channel in, one out
        _add("edge", p, 1, 1)
    # 2. the fused input transform
    for p in (1, 16, 64, 65):                          # the LDS-tiled kernel: what the skinny kernel would take unfused, the 64-point tile
        for relu, k in relu_variants(36):
            _add("fused", p, 36, 21, True, relu, k)
    for ci in (4, 36, 188):                            # ... and what the narrow kernel would take unfused
        for relu, k in relu_variants(ci):
            _add("fused", 129, ci, 130, True, relu, k)
    for ci in (192, 196, 284, 288, 304):               # stream<true,8>
        for relu, k in relu_variants(ci):
            _add("fused", 141, ci, 130 if ci in (192, 288) else 21, True, relu, k)
    for ci, co in ((196, 3), (1600, 4), (196, 16)):    # stream<true,1>: the T-NOCS regression's shape among them, with its sigmoid
        for relu, k in relu_variants(ci):
            _add("fused", 141, ci, co, True, relu, k, act=1)
    for ci, k in ((2048, 2044), (2052, 0)):            # around GEMM_MAXC: scale / shift from LDS, then from global memory
        _add("wide", 64, ci, 21, True, True, k)
    for ci in (2048, 2052, 2080):                      # 2048 is the streaming kernel's last width, 2052 / 2080 stay on the LDS-tiled kernel
        _add("wide", 129, ci, 4, True, True, 4)
        _add("wide", 129, ci, 130, True, True, ci - 4)
    # 3. the sigmoid epilogue on every instantiation
    for P, Cin, Cout, fused, ri in ((13, 37, 21, False, False), (141, 37, 13, False, False), (141, 37, 21, False, False), (141, 37, 53, False, False),
                                    (141, 37, 130, False, False), (141, 197, 13, False, False), (141, 197, 130, False, False),
                                    (141, 196, 13, True, False), (141, 196, 130, True, False), (77, 37, 130, False, False),
                                    (77, 36, 21, True, False), (141, 197, 21, False, True)):
        _add("sigmoid", P, Cin, Cout, fused, fused, 4 if fused else 0, act=1, ri=ri)
    # 4. row invariance: one set of 300 rows per width (test_conv_f32_edges.py runs its subsets, reversal and re-batching)
    for ci in RI_CIN:
        for co in RI_COUT:
            _add("ri", RI_ROWS, ci, co, ri=True, B=1)
            _add("ri", RI_ROWS, ci, co, True, True, 4, ri=True, B=1)
    # 5. batch-entry invariance: three entries, block counts 6 / 6 / 12 / 12 (no multiple of 8: the XCD renumbering's remainder)
    for P, Cin, Cout, fused in ((13, 37, 21, False), (141, 37, 21, False), (141, 197, 130, False), (77, 37, 130, False),
                                (141, 196, 130, True), (77, 36, 130, True)):
        _add("batch", P, Cin, Cout, fused, fused, 4 if fused else 0, B=3)


RI_ROWS = 300
RI_CIN = (8, 200, 516)
RI_COUT = (5, 130)
RI_P = (1, 5, 16, 17, 64, 65, 128, 129, 300)
_build()
BY_NAME = {c.name: c for c in CASES}

# 7. the large-P route: ceil(P / 64) = 65536 > 65535 -> conv1x1_kernel<128>; fused, or the narrow kernel would take it
LARGE = SimpleNamespace(name="large:1x4194241x4x4:inrelu0", group="large", B=1, P=4_194_241, Cin=4, Cout=4, fused=True, in_relu=True, relu_from=0,
                        act=0, ri=False, seed=90000, route=f32_route(4_194_241, 4, 4, True, False))
REFUSED_P = GRID_MAX * 128 + 1


# ---------------------------------------------------------------------------------------------
# inputs, reference, mutations
# ---------------------------------------------------------------------------------------------
def build_inputs(c):
    """Weights scaled by 1 / sqrt(Cin) (outputs of unit size), a bias, a per-entry bias that differs between entries; fused: in_scale of
    mixed sign with |.| in [0.5, 1.5] and in_shift ~ N(0, 0.5), so that about half of the transformed inputs are negative; a sigmoid
    case's bias is a permutation of an even spread over +-12."""
    s = c.seed
    g = np.random.default_rng(s + 9)
    I = SimpleNamespace(x=rnd(s, c.B, c.P, c.Cin), w=rnd(s + 1, c.Cout, c.Cin, scale=1.0 / np.sqrt(c.Cin)), b=rnd(s + 2, c.Cout, scale=0.3),
                        bb=rnd(s + 3, c.B, c.Cout, scale=0.1) + 0.5 * torch.linspace(-1.0, 1.0, c.B).unsqueeze(1) if c.B > 1
                        else rnd(s + 3, c.B, c.Cout, scale=0.1), sc=None, sh=None)
    if c.act:
        spread = torch.linspace(-SIGMOID_SPREAD, SIGMOID_SPREAD, c.Cout) if c.Cout > 1 else torch.zeros(1)
        I.b = spread[torch.from_numpy(g.permutation(c.Cout))].contiguous()
    if c.fused:
        I.sc = torch.from_numpy((g.uniform(0.5, 1.5, (c.B, c.Cin)) * g.choice([-1.0, 1.0], (c.B, c.Cin))).astype(np.float32))
        I.sh = rnd(s + 5, c.B, c.Cin, scale=0.5)
        # planted: the last channel of every entry's first row transforms to 1 -- it survives the ReLU even in a one-row case
        I.x[:, 0, c.Cin - 1] = (1.0 - I.sh[:, c.Cin - 1]) / I.sc[:, c.Cin - 1]
    return I


@functools.lru_cache(maxsize=None)
def inputs(name):
    return build_inputs(LARGE if name == LARGE.name else BY_NAME[name])


MUTATIONS = ("drop_last_channel", "last_row_is_the_row_before", "entry0_terms_for_all", "relu_from_0", "no_relu", "no_sigmoid", "nan_pad_unmasked")


def applies(c, mut):
    return {"drop_last_channel": True,
            "last_row_is_the_row_before": c.P >= 2,
            "entry0_terms_for_all": c.B >= 2,
            "relu_from_0": c.fused and c.in_relu and c.relu_from > 0,
            "no_relu": c.fused and c.in_relu and c.relu_from < c.Cin,
            "no_sigmoid": c.act == 1,
            "nan_pad_unmasked": True}[mut]             # the GPU tests give every case NaN pad columns


def reference(c, I, dtype=torch.float64, mut=None):
    """The plain operation in `dtype` (f64: the reference; f32: the conditioning control), or one of its MUTATIONS."""
    assert mut is None or mut in MUTATIONS
    t = lambda a: a.to(dtype)
    per_entry = (lambda a: t(a)[:1].expand_as(a)) if mut == "entry0_terms_for_all" else t
    x, w = t(I.x), t(I.w)
    if c.fused:
        x = x * per_entry(I.sc).unsqueeze(1) + per_entry(I.sh).unsqueeze(1)
        if c.in_relu and mut != "no_relu":
            k = 0 if mut == "relu_from_0" else c.relu_from
            x = torch.cat([x[..., :k], torch.relu(x[..., k:])], dim=-1)
    if mut == "drop_last_channel":
        x, w = x[..., :-1], w[:, :-1]
    if mut == "nan_pad_unmasked":                      # the pad column behind Cin meets its zero weight: 0 * NaN
        x = torch.cat([x, torch.full_like(x[..., :1], float("nan"))], dim=-1)
        w = torch.cat([w, torch.zeros_like(w[:, :1])], dim=-1)
    y = x @ w.t() + t(I.b) + per_entry(I.bb).unsqueeze(1)
    if mut == "last_row_is_the_row_before":
        y = torch.cat([y[:, :-1], y[:, -2:-1]], dim=1)
    if c.act == 1 and mut != "no_sigmoid":
        y = torch.sigmoid(y)
    return y


@functools.lru_cache(maxsize=None)
def want(name):
    c = LARGE if name == LARGE.name else BY_NAME[name]
    return reference(c, inputs(name))


def bound(c, y64):
    return SIGMOID_TOL if c.act == 1 else CONV_TOL * max(1.0, float(y64.abs().max()))


def distance(a, b):
    """max |a - b|, a non-finite entry counting as infinitely far."""
    d = (a.double() - b.double()).abs()
    return float(torch.nan_to_num(d, nan=float("inf")).max())
