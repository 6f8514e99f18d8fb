"""The case table, input builders, f64 reference and host mirror for the edge tests of the bf16x6 pointwise convs
(csrc/gemm_bf16x6.hip: conv1x1_bf16x6_kernel, conv1x1_x6tail_kernel; csrc/gemm_bf16x6w.hip: conv1x1_x6w_kernel):
test_conv_bf16x6_cases.py checks the table on the CPU, test_conv_bf16x6_edges.py runs the kernels on it.  No GPU code is imported.

Three kernels in four instantiations <FUSED, STATS> each, behind these entries (the `entry` of a case):

    x6     caspr_conv1x1_bf16x6_f32                                     conv1x1_bf16x6_kernel<F, false>
    x6gn   caspr_conv1x1_gn_bf16x6_f32 / _gn_pooled_ (pool > 1)         conv1x1_bf16x6_kernel<F, true>, Y may be NULL
    x6w    caspr_conv1x1_x6w_f32 / _x6w_pooled_f32 (pool > 1)           conv1x1_x6w_kernel on the first Cout - Cout % 512 channels, the
                                                                        remainder on conv1x1_x6tail_kernel (<= 64) or conv1x1_bf16x6_kernel
    part   caspr_conv1x1_x6w_part_f32 in `pieces` + the finalize        the same, always <F, true>, on a grid of g workgroups
    h3w    caspr_conv1x1_h3w_f32                                        the tail kernel at Cin = 32 (the 512-channel tiles on f16x3)

x6_plan() restates, condition by condition with the source line quoted, which kernels a call launches, on which channel range, with
what cstride / Mt / Pt / block count, and derives the classes a launch belongs to (x6: full / half / dead waves; tail: live row tiles,
chunk count class, a last workgroup holding one tile; x6w: chunk count class, tiles per workgroup).  A release build cannot report
which kernel ran, so the mirror is checked BY READING, as conv_f32_cases.f32_route is: whoever changes a condition in
conv_x6_launch, conv_x6tail_launch, conv_x6w_impl, conv_x6w_part_impl or caspr_conv_x6w_launch changes it here.

reference(case, inputs) is the plain operation in f64,

    act( in(x) @ W[:, col0:col0+Cin]^T + bias + bbias[b] ),   in(x) = x * in_scale[b] + in_shift[b], max(., 0) on channels k >= relu_from,

with the GroupNorm statistics of its (B / pool, pool * P, C) view (F.group_norm), as test_conv_gn_pooled.  MUTATIONS are subtly wrong
variants that the case's bounds have to tell from the reference by a factor of ten.
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from test_hip_parity import rnd

CONV_TOL = 2e-6             # x max(1, |y64|max) on conv outputs (test_conv1x1_bf16x6, test_conv1x1_x6w_kernel)
SIGMOID_TOL = 2e-6          # after the sigmoid
APPLY_TOL = 5e-6            # on the applied normalisation (test_conv_gn_pooled)
SIGMOID_SPREAD = 12.0       # conv_f32_cases.SIGMOID_SPREAD
EPS = 1e-5
X6_TM, X6_TP = 256, 128     # gemm_bf16x6.hip:38-39
CW_TM, CW_TP = 512, 128     # gemm_bf16x6w.hip:28-29
N_CU = 256                  # the MI355X's compute units; every case has fewer tiles, so the full grid is one tile per workgroup

KERNELS = ("x6", "tail", "x6w")
INSTANTIATIONS = tuple("%s<%s,%s>" % (k, f, s) for k in KERNELS for f in ("false", "true") for s in ("false", "true"))


def ceil_div(a, b):
    return (a + b - 1) // b


def _inst(kernel, fused, stats):
    return "%s<%s,%s>" % (kernel, "true" if fused else "false", "true" if stats else "false")


def _x6(c0, C, B, P, Cin, fused, stats, cstride):
    """conv_x6_launch (gemm_bf16x6.hip:712): one workgroup per (channel tile of 256, point tile of 128, entry)."""
    Mt, Pt = ceil_div(C, X6_TM), P // X6_TP                                    # :727
    waves = set()
    for mt in range(Mt):
        for wm in (0, 1):
            co_w = mt * X6_TM + wm * 128                                       # :152
            waves.add("dead" if not co_w < C else "half" if co_w + 64 >= C else "full")      # :153-154, :289-290
    return SimpleNamespace(kernel="x6", inst=_inst("x6", fused, stats), c0=c0, C=C, cstride=cstride, Mt=Mt, Pt=Pt, nblk=Mt * Pt * B,   # :728
                           nk=Cin // 32, waves=waves)


def _tail(c0, C, B, P, Cin, fused, stats, cstride):
    """conv_x6tail_launch (gemm_bf16x6.hip:865): a workgroup holds two (entry, point tile) tiles."""
    Pt = P // X6_TP                                                            # :870
    ntile = B * Pt                                                             # :871
    nk = Cin // 32
    return SimpleNamespace(kernel="tail", inst=_inst("tail", fused, stats), c0=c0, C=C, cstride=cstride, Mt=1, Pt=Pt, nblk=(ntile + 1) // 2,   # :872
                           nk=nk, nrt=(C + 15) >> 4,                           # :455
                           chunks="one" if nk == 1 else "two" if nk == 2 else "odd" if nk % 2 else "even",     # :522-529
                           last_single=ntile % 2 == 1)                         # :450


def _x6w(mt0, mt1, B, P, Cin, fused, stats, cstride, g):
    """caspr_conv_x6w_launch (gemm_bf16x6w.hip:404): channel tiles mt0 .. mt1 - 1 of 512, a persistent grid."""
    Mt, Pt = mt1 - mt0, P // CW_TP                                             # :411
    ntiles = B * Mt * Pt                                                       # :412
    grid = max(1, g if g else N_CU)                                            # :421-422  (reserve_cus = n_cu - g)
    nblk = min(ntiles, grid)                                                   # :423
    nmine = [(ntiles - w + nblk - 1) // nblk for w in range(nblk)]             # :75
    nk = Cin // 32
    return SimpleNamespace(kernel="x6w", inst=_inst("x6w", fused, stats), c0=mt0 * CW_TM, C=Mt * CW_TM, cstride=cstride, Mt=Mt, Pt=Pt, nblk=nblk,
                           nk=nk, chunks="two" if nk == 2 else "odd" if nk % 2 else "even", ntiles=ntiles, nmine=nmine)


def x6_plan(entry, B, P, Cin, Cout, fused, stats, pieces=None, g=0):
    """The launches of one call, in order (the finalize kernel left out).  stats: the call asks for GroupNorm statistics (x6gn; x6w / h3w
    with G > 0); the part entry always leaves partials (gemm_bf16x6.hip:1003, part = ws)."""
    if entry in ("x6", "x6gn"):
        return [_x6(0, Cout, B, P, Cin, fused, entry == "x6gn", Cout)]         # :716  cstride = Cout
    Cmain = Cout - Cout % 512                                                  # :918 / :992
    Ctail = Cout - Cmain
    out = []
    if entry == "part":
        stats = True
    else:
        pieces = [(0, Cmain // 512, 1)]                                        # :937
    for m0, m1, with_tail in pieces:
        if m1 > m0 and entry != "h3w":                                         # :1005 (the one-call entries always launch: Cmain >= 512); h3w: the f16x3 kernel
            out.append(_x6w(m0, m1, B, P, Cin, fused, stats, Cout, g))
        if Ctail and with_tail and Ctail <= 64:                                # :941 / :1011
            out.append(_tail(Cmain, Ctail, B, P, Cin, fused, stats, Cout))
        elif Ctail and with_tail:                                              # :945 / :1014
            out.append(_x6(Cmain, Ctail, B, P, Cin, fused, stats, Cout))
    return out


def relu_class(relu_from, Cin):
    """Where the ReLU switches on, relative to the kernels' granularities (8 channels per piece in x6 / tail, a pair inside a 16-k step in
    x6w, 32-k chunks in all three)."""
    if relu_from == 0:
        return "before_first_chunk"
    if relu_from >= Cin:
        return "after_last_chunk"
    if relu_from % 32 == 0:
        return "between_chunks"
    return "inside_step" if relu_from % 16 else "inside_chunk"


RELU_CLASSES = ("before_first_chunk", "after_last_chunk", "between_chunks", "inside_chunk", "inside_step")

# ---------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------
X6_COUT = (4, 60, 64, 68, 124, 128, 132, 188, 192, 196, 252, 256, 260, 508)
X6_COUT_HALF = (4, 64, 68, 128, 192, 260, 508)
X6_REMAINDER = (68, 252, 256, 260, 508)
TAIL_COUT = (4, 12, 16, 20, 32, 36, 48, 52, 64)
CASES = []


def make_case(group, entry, B, P, Cin, Cout, fused=False, in_relu=False, relu_from=0, bias=True, bbias=True, act=0, G=0, pool=1, write=True,
              pieces=None, g=0, col0=0, ldw=None, seed=0):
    assert relu_from % 8 == 0 and 0 <= relu_from <= Cin and (not in_relu or fused) and (G > 0 or write)
    assert (entry == "x6gn") == (G > 0 and entry in ("x6", "x6gn")) and (entry != "part" or G > 0)
    assert G == 0 or Cout % G == 0
    name = "%s:%s:%dx%dx%dx%d" % (group, entry, B, P, Cin, Cout)
    if fused:
        name += ":in%s" % (("relu%d" % relu_from) if in_relu else "affine")
    name += ("" if bias else ":nobias") + ("" if bbias else ":nobbias") + (":sigmoid" if act else "")
    name += (":G%d" % G if G else "") + (":pool%d" % pool if pool > 1 else "") + ("" if write else ":nowrite")
    name += (":pieces" + "+".join("%d-%d%s" % (a, b, "t" if t else "") for a, b, t in pieces) if pieces else "") + (":g%d" % g if g else "")
    name += ":col%d" % col0 if ldw else ""
    plan = x6_plan(entry, B, P, Cin, Cout, fused, G > 0, pieces, g)
    return SimpleNamespace(name=name, group=group, entry=entry, B=B, P=P, Cin=Cin, Cout=Cout, fused=fused, in_relu=in_relu, relu_from=relu_from,
                           bias=bias, bbias=bbias, act=act, G=G, pool=pool, write=write, pieces=pieces, g=g, col0=col0,
                           ldw=ldw or Cin, seed=seed, plan=plan, kernels={l.kernel for l in plan})


def _add(*args, **kw):
    CASES.append(make_case(*args, seed=2000 + 16 * len(CASES), **kw))


def relu_sweep(Cin):
    return [(False, 0)] + [(True, k) for k in sorted({0, 8, 16, 24, 32, 40, Cin - 8, Cin})]


def _build():
    # 1. conv1x1_bf16x6_kernel through its own entry: every Cout on both sides of a wave class, the smallest K; transform and
    #    biases rotate
    n = 0
    for Cin, couts in ((32, X6_COUT), (64, X6_COUT), (96, X6_COUT_HALF)):
        for co in couts:
            fused = n % 2 == 1
            _add("x6", "x6", 2 if n % 3 else 1, 128, Cin, co, fused, fused, 8 if fused else 0, bias=n % 4 != 2, bbias=n % 4 != 3)
            n += 1
    # ... its block counts nblk = Mt Pt B (the XCD work map: below 8, and no multiple of 8)
    for B, P, co, nblk in ((1, 128, 132, 1), (3, 128, 132, 3), (7, 128, 68, 7), (3, 384, 196, 9), (3, 384, 260, 18)):
        _add("nblk", "x6", B, P, 64, co, True, True, 8)
        assert CASES[-1].plan[0].nblk == nblk
    for fused in (False, True):
        _add("sigmoid", "x6", 2, 128, 64, 132, fused, fused, 8 if fused else 0, act=1)
    # ... with statistics: a group count that divides Cout, with and without the output, with and without the transform
    for co, G in ((64, 16), (132, 4), (260, 4), (508, 4)):
        for write in (True, False):
            for fused in (False, True):
                _add("stats", "x6gn", 2, 128, 32 if co == 64 else 64, co, fused, fused, 8 if fused else 0, G=G, write=write)
    _add("stats", "x6gn", 4, 128, 64, 132, True, True, 8, G=4, pool=2)
    _add("stats", "x6gn", 3, 256, 96, 260, True, True, 0, G=4, pool=3, write=False)
    # 2. ... as the remainder behind the 512-channel kernel: cstride, Y + Cmain, part + Cmain
    for ct in X6_REMAINDER:
        _add("remainder", "x6w", 2, 128, 64, 512 + ct)
        _add("remainder", "x6w", 2, 128, 64, 512 + ct, True, True, 8, G=4)
    _add("remainder", "x6w", 4, 128, 64, 512 + 132, True, True, 16, G=4, pool=2)
    # 3. conv1x1_x6tail_kernel: every live row tile count, chunk counts 2 / 3 / 5 (1 below), 1 .. 3 tiles, the four instantiations and Y = NULL
    n = 0
    for ct in TAIL_COUT:
        for Cin in (64, 96, 160):
            B, P = ((1, 128), (2, 128), (3, 128), (1, 256), (1, 384))[n % 5]
            fused, stats = ((False, False), (True, False), (False, True), (True, True))[n % 4]
            write = not (stats and (n // 4) % 2)
            _add("tail", "x6w", B, P, Cin, 512 + ct, fused, fused, (8, 24, 40)[n % 3] if fused else 0, bias=n % 4 != 1, bbias=n % 4 != 2,
                 G=4 if stats else 0, write=write)
            n += 1
    _add("tail", "x6w", 4, 128, 64, 512 + 48, True, True, 8, G=4, pool=2)
    for fused in (False, True):                      # one chunk: the tile kernel of the f16x3 entry is this kernel too
        _add("tail", "h3w", 3, 128, 32, 512 + 20, fused, fused, 8 if fused else 0)
        _add("tail", "h3w", 3, 128, 32, 512 + 52, fused, fused, 8 if fused else 0, G=4)
    # 4. conv1x1_x6w_kernel on the full grid: chunk counts 2 / 3 / 4 / 5, one and two channel tiles, 1 .. 4 point tiles
    n = 0
    for Cin in (64, 96, 128, 160):
        for co in (512, 1024):
            for B, P in ((1, 128), (3, 128), (2, 256)):
                fused, stats, write = ((False, False, True), (True, False, True), (False, True, True), (True, True, True), (True, True, False))[n % 5]
                _add("x6w", "x6w", B, P, Cin, co, fused, fused, (8, 16, 24, 40)[n % 4] if fused else 0, bias=n % 3 != 1, bbias=n % 3 != 2,
                     G=16 if stats else 0, write=write)
                n += 1
    # ... its persistent stream: g workgroups walk 6 tiles (3 entries x 2 channel tiles) of 2 / 3 / 4 chunks; at g = 1 one workgroup
    #     crosses entries and channel tiles; ntiles - 1 = 5 gives workgroup 0 two tiles and the others one
    for Cin in (64, 96, 128):
        for g in (1, 2, 3, 5):
            fused = (Cin // 32 + g) % 2 == 0
            _add("stream", "part", 3, 128, Cin, 1024, fused, fused, 24 if fused else 0, G=16, pieces=[(0, 2, 1)], g=g)
    _add("stream", "part", 2, 256, 160, 1024 + 20, True, True, 40, G=4, pieces=[(0, 2, 1)], g=3)
    _add("stream", "part", 3, 128, 64, 1024 + 132, True, True, 8, G=4, pieces=[(0, 2, 1)], g=1, write=False)
    # ... in pieces: tile 0 then tile 1; an empty range in between; the remainder with the first piece / on a call of its own
    _add("pieces", "part", 3, 128, 96, 1024 + 36, True, True, 8, G=4, pieces=[(0, 1, 0), (1, 2, 1)], g=2)
    _add("pieces", "part", 3, 128, 64, 1024 + 36, False, G=4, pieces=[(0, 1, 1), (1, 1, 0), (1, 2, 0)], g=1)
    _add("pieces", "part", 2, 128, 64, 1024 + 68, True, True, 8, G=4, pieces=[(0, 2, 0), (2, 2, 1)])
    # 5. in_relu_from on each kernel: 0, 8, 16, 24, 32, 40, Cin - 8, Cin, and affine without the ReLU
    for relu, k in relu_sweep(96):
        _add("relu", "x6", 2, 128, 96, 132, True, relu, k)
        _add("relu", "x6gn", 2, 128, 96, 132, True, relu, k, G=4)
        for G in (0, 4):
            _add("relu", "x6w", 2, 128, 96, 512 + 20, True, relu, k, G=G)    # x6w and the tail kernel
    # 6. packs: the weight a column window of a wider matrix (the GPU test fills the rest with NaN), ragged Cout
    for col0 in (0, 4):
        _add("pack", "x6", 2, 128, 64, 132, True, True, 8, col0=col0, ldw=64 + 12)
        _add("pack", "x6w", 2, 128, 64, 512 + 20, True, True, 8, G=4, col0=col0, ldw=64 + 12)
        _add("pack", "x6w", 2, 128, 64, 512 + 132, col0=col0, ldw=64 + 8)


_build()
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------------------------------------
# inputs, reference, mutations
# ---------------------------------------------------------------------------------------------
def build_inputs(c):
    """Weights scaled by 1 / sqrt(Cin) inside a (Cout, ldw) matrix, a bias, a per-entry bias spread over +-3 (so that a wrong entry's row
    is visible), per-entry in_scale rows of mixed sign with |.| in [0.5, 1.5] that differ between entries, in_shift ~ N(0, 1) (a few
    units); a sigmoid case's bias is a permutation of an even spread over +-12; gamma with every seventh channel negative."""
    s = c.seed
    g = np.random.default_rng(s + 9)
    I = SimpleNamespace(x=rnd(s, c.B, c.P, c.Cin), w_full=rnd(s + 1, c.Cout, c.ldw, scale=1.0 / np.sqrt(c.Cin)), b=None, bb=None, sc=None, sh=None,
                        gamma=None, beta=None)
    I.w = I.w_full[:, c.col0:c.col0 + c.Cin].contiguous()
    if c.bias:
        I.b = rnd(s + 2, c.Cout, scale=0.3)
        if c.act:
            I.b = torch.linspace(-SIGMOID_SPREAD, SIGMOID_SPREAD, c.Cout)[torch.from_numpy(g.permutation(c.Cout))].contiguous()
    if c.bbias:
        I.bb = rnd(s + 3, c.B, c.Cout, scale=0.1) + (3.0 * torch.linspace(-1.0, 1.0, c.B).unsqueeze(1) if c.B > 1 else 0.0)
    if c.fused:
        I.sc = torch.from_numpy((g.uniform(0.5, 1.5, (c.B, c.Cin)) * g.choice([-1.0, 1.0], (c.B, c.Cin))).astype(np.float32))
        I.sh = rnd(s + 5, c.B, c.Cin)
    if c.G:
        I.gamma, I.beta = rnd(s + 6, c.Cout) * 0.2 + 1.0, rnd(s + 7, c.Cout) * 0.1
        I.gamma[::7] *= -1.0
    return I


@functools.lru_cache(maxsize=None)
def inputs(name):
    return build_inputs(BY_NAME[name])


MUTATIONS = ("relu_from_off_by_8", "other_entrys_in_scale", "other_entrys_bbias", "no_bias_on_last_channel_tile", "last_k_chunk_dropped",
             "first_k_chunk_twice", "tile_halves_swapped", "stats_over_127_of_128", "stats_per_entry_then_averaged", "weight_window_shifted")


def last_tile_start(c):
    """The first channel of the last channel tile a kernel of the case's plan works on."""
    last = c.plan[-1]
    tile = CW_TM if last.kernel == "x6w" else X6_TM
    return last.c0 + (ceil_div(last.C, tile) - 1) * tile


def applies(c, mut):
    return {"relu_from_off_by_8": c.fused and c.in_relu,
            "other_entrys_in_scale": c.fused and c.B >= 2,
            "other_entrys_bbias": c.bbias and c.B >= 2,
            "no_bias_on_last_channel_tile": c.bias,
            "last_k_chunk_dropped": True,
            "first_k_chunk_twice": True,
            "tile_halves_swapped": c.write,
            "stats_over_127_of_128": c.G > 0,
            "stats_per_entry_then_averaged": c.G > 0 and c.pool > 1,
            "weight_window_shifted": c.col0 > 0}[mut]


def conv(c, I, dtype=torch.float64, mut=None):
    """The conv's output (B, P, Cout) in `dtype`, or one of its mutations."""
    t = lambda a: a.to(dtype)
    x = t(I.x)
    w = t(I.w_full[:, :c.Cin]) if mut == "weight_window_shifted" else t(I.w)
    if c.fused:
        sc = t(I.sc).roll(1, 0) if mut == "other_entrys_in_scale" else t(I.sc)
        x = x * sc.unsqueeze(1) + t(I.sh).unsqueeze(1)
        if c.in_relu:
            k = c.relu_from
            if mut == "relu_from_off_by_8":
                k = k + 8 if k + 8 <= c.Cin else k - 8
            x = torch.cat([x[..., :k], torch.relu(x[..., k:])], dim=-1)
    if mut == "last_k_chunk_dropped":
        x = torch.cat([x[..., :-32], torch.zeros_like(x[..., -32:])], dim=-1)
    y = x @ w.t()
    if mut == "first_k_chunk_twice":
        y = y + x[..., :32] @ w[:, :32].t()
    if c.bias:
        b = t(I.b).clone()
        if mut == "no_bias_on_last_channel_tile":
            b[last_tile_start(c):] = 0
        y = y + b
    if c.bbias:
        y = y + (t(I.bb).roll(1, 0) if mut == "other_entrys_bbias" else t(I.bb)).unsqueeze(1)
    if mut == "tile_halves_swapped":
        y = y.view(c.B, c.P // 128, 2, 64, c.Cout).flip(2).reshape(c.B, c.P, c.Cout)
    if c.act == 1:
        y = torch.sigmoid(y)
    return y


def moments(y, pool, G):
    """y (B, P, C) -> mean, biased variance (B / pool, G) over pool consecutive entries, in y's precision."""
    B, P, C = y.shape
    m = y.reshape(B // pool, pool * P, G, C // G).transpose(1, 2).reshape(B // pool, G, -1)
    return m.mean(dim=2), m.var(dim=2, unbiased=False)


def scale_shift(mean, var, gamma, beta, G):
    rstd = 1.0 / torch.sqrt(var + EPS)
    sc = gamma * rstd.repeat_interleave(gamma.numel() // G, dim=1)
    return sc, beta - mean.repeat_interleave(gamma.numel() // G, dim=1) * sc


def apply(y64, sc, sh):
    """scale / shift (B / pool, C) broadcast over their pool * P rows of y64 (B, P, C) -> (B, P, C) in f64."""
    B, P, C = y64.shape
    return (y64.view(sc.shape[0], -1, C) * sc.double().unsqueeze(1) + sh.double().unsqueeze(1)).view(B, P, C)


def statistics(c, I, y, mut=None):
    """scale, shift (B / pool, C) of the GroupNorm on y, in y's precision, or a mutation of them."""
    if mut == "stats_over_127_of_128":
        y = y.view(c.B, c.P // 128, 128, c.Cout)[:, :, :127].reshape(c.B, -1, c.Cout)
    if mut == "stats_per_entry_then_averaged":
        m1, v1 = moments(y, 1, c.G)
        mean, var = m1.view(c.B // c.pool, c.pool, c.G).mean(dim=1), v1.view(c.B // c.pool, c.pool, c.G).mean(dim=1)
    else:
        mean, var = moments(y, c.pool, c.G)
    return scale_shift(mean, var, I.gamma.to(y.dtype), I.beta.to(y.dtype), c.G)


@functools.lru_cache(maxsize=None)
def want(name):
    """The f64 reference of a case: y, and with statistics the normalised output, mean, rstd, pmax (computed once, never modified)."""
    c, I = BY_NAME[name], inputs(name)
    y = conv(c, I)
    R = SimpleNamespace(y=y, tol_y=SIGMOID_TOL if c.act == 1 else CONV_TOL * max(1.0, float(y.abs().max())))
    if c.G:
        R.want = F.group_norm(y.view(c.B // c.pool, c.pool * c.P, c.Cout).transpose(1, 2), c.G, I.gamma.double(), I.beta.double(), EPS).transpose(1, 2)
        R.want = R.want.reshape(c.B, c.P, c.Cout)
        R.mean, var = moments(y, c.pool, c.G)
        R.rstd = 1.0 / torch.sqrt(var + EPS)
        R.pmax = R.want.view(c.B // c.pool, c.pool * c.P, c.Cout).max(dim=1)[0]
    return R


def distance(a, b):
    """max |a - b|, a non-finite entry counting as infinitely far."""
    d = (a.double() - b.double()).abs()
    return float(torch.nan_to_num(d, nan=float("inf")).max())


def shares(c, I, R, y, sc=None, sh=None):
    """What the GPU test observes of a result, as shares of its bounds: the output (if written) and the applied normalisation."""
    out = {}
    if c.write:
        out["y"] = distance(y, R.y) / R.tol_y
    if c.G:
        out["apply"] = distance(apply(R.y, sc, sh), R.want) / APPLY_TOL
    return out


def mutated_shares(c, mut):
    I, R = inputs(c.name), want(c.name)
    stat_mut = mut in ("stats_over_127_of_128", "stats_per_entry_then_averaged")
    y = R.y if stat_mut else conv(c, I, mut=mut)
    sc, sh = statistics(c, I, y, mut if stat_mut else None) if c.G else (None, None)
    return shares(c, I, R, y, sc, sh)
