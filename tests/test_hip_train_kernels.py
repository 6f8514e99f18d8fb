"""Training tier, op by op: the CNF's ODE-function kernels (csrc/backward_flow.hip, the act modes of csrc/gemm_bf16x6.hip, the
autograd Functions of caspr_amd/train/flow_grad.py), one CNF block end to end, and the fixed-order scatter / centred grouping of
the encoder backward (csrc/backward_points.hip), each against plain f64 torch on the CPU, element by element.

The references do not reuse the kernels' formulation: the ODE function is the ConcatSquash layer (x W^T + b) gate + beta followed
by softplus (oracle/model.py: odenet), and the tangent / divergence rows come from forward-mode autograd (torch.func.jvp) or, for
the whole block, from the oracle's GRAD_MODE double backward -- never from the closed form sigmoid(a) * ad.  Every check is
max |hip - f64| / max |f64| per tensor, measured and recorded by test_hip_train.rel: every error and its bound land in that
module's JSON report, keyed "kernels:<case>:<tensor>".

The encoder's GroupNorm / max / column-sum kernels, the skinny and in_relu_from routes of conv1x1_wgrad and the value-only CNF layers
(csrc/backward_flow_value.hip) are not covered here: tests/test_hip_train_edges.py runs them one by one at their edges ("edges:" keys).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_train import rel, rnd

pytestmark = pytest.mark.gpu

FWD, GRAD = 1e-5, 5e-5          # starting bounds of every check (relative to the reference tensor's largest entry)


class Checks:
    """Collects every comparison of one test (so that the report holds all of them even when one fails) and asserts at the end."""

    prefix = "kernels"

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def __call__(self, name, got, want, bound, ref=None):
        assert bound <= 2e-4, "no bound above the full-step L2 bound"
        try:
            rel("%s:%s:%s" % (self.prefix, self.tag, name), got, want, bound, ref=ref)
        except AssertionError as e:
            self.bad.append(str(e))

    def done(self):
        assert not self.bad, self.tag + "\n" + "\n".join(self.bad)


# ---------------------------------------------------------------------------------------------
# row layouts of the (2R, C) value | tangent tensors (include/caspr_hip_train.h)
# ---------------------------------------------------------------------------------------------
def split_rows(z, R, blk):
    """(2R, c) rows in layout blk -> values (R, c), tangents (R, c), by point."""
    zz = z.reshape(R // blk, 2, blk, z.shape[-1])
    return zz[:, 0].reshape(R, -1), zz[:, 1].reshape(R, -1)


def join_rows(v, t, blk):
    R, c = v.shape
    return torch.stack([v.reshape(R // blk, blk, c), t.reshape(R // blk, blk, c)], dim=1).reshape(2 * R, c)


def frame_rows(t, n):
    """(frames, C) -> (frames n, C): every point sees its frame's row."""
    return t.repeat_interleave(n, dim=0)


def gated_softplus(z, b, gate, beta, n):
    """ConcatSquash epilogue + softplus on point rows (odenet)."""
    return F.softplus((z + b) * frame_rows(gate, n) + frame_rows(beta, n))


def f64_leaves(*ts):
    return [t.detach().double().requires_grad_(True) for t in ts]


def gpu_leaves(*ts):
    return [t.detach().to("cuda:0").requires_grad_(True) for t in ts]


def hyper(seed, F_, C, scale=0.3):
    return torch.sigmoid(rnd(seed, F_, C, scale=1.5)), rnd(seed + 1, F_, C, scale=scale)


# ---------------------------------------------------------------------------------------------
# A. the CNF layers, one autograd Function at a time
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,n,C,blk", [(1, 64, 512, 32), (3, 100, 512, "R"), (2, 300, 512, "R"), (2, 1024, 512, 32), (3, 96, 132, "R"),
                                            (1, 256, 1280, 32)])
def test_cnf_in_vs_f64(frames, n, C, blk):
    """CnfIn (caspr_cnf_in_f32 / _bwd_f32): forward h and the gradients w.r.t. y, W0, b0, gate, beta.  The cases reach the rows forward
    kernel and the element forward kernel (C = 132, C = 1280 > 1024), the rows backward kernel with 1 split (n < 256), 8 even and 8
    uneven splits (n = 300), the 64-channel backward kernel with a partial last chunk (C = 132), and both row layouts."""
    from caspr_amd.train import flow_grad as FG
    R = frames * n
    blk = R if blk == "R" else blk
    y, e = rnd(1, R, 3), rnd(2, R, 3)
    w0, b0 = rnd(3, C, 3, scale=0.8), rnd(4, C, scale=0.3)
    gate, beta = hyper(5, frames, C)
    dh = rnd(7, 2 * R, C)
    # f64 reference: value = softplus of the ConcatSquash layer, tangent = its jvp along e
    y6, w6, b6, g6, be6 = f64_leaves(y, w0, b0, gate, beta)
    hv6, ht6 = torch.func.jvp(lambda yy: gated_softplus(yy @ w6.t(), b6, g6, be6, n), (y6,), (e.double(),))
    dhv, dht = split_rows(dh.double(), R, blk)
    ((hv6 * dhv).sum() + (ht6 * dht).sum()).backward()
    # HIP
    yd, wd, bd, gd, bed = gpu_leaves(y, w0, b0, gate, beta)
    h = FG.CnfIn.apply(yd, e.to("cuda:0"), wd, bd, gd, bed, n, blk)
    (h * dh.to("cuda:0")).sum().backward()
    ck = Checks("cnf_in[%d,%d,%d,%d]" % (frames, n, C, blk))
    ck("h", h, join_rows(hv6, ht6, blk), FWD)
    for nm, a, b in (("dy", yd, y6), ("dW0", wd, w6), ("db0", bd, b6), ("dgate", gd, g6), ("dbeta", bed, be6)):
        ck(nm, a.grad, b.grad, GRAD)
    ck.done()


@pytest.mark.parametrize("C", [512, 132])
@pytest.mark.parametrize("blk", ["R", 32])
def test_cnf_act_vs_f64(blk, C):
    """CnfAct (caspr_cnf_act_f32 / _bwd_f32), the unfused route's hidden layer, on 3 frames of 96 points: h and the gradients
    w.r.t. Z (value and tangent rows), b, gate, beta.  A quarter of the frames' channels get pre-activations far into the
    softplus tails (|a| up to ~40), where sigmoid_fast / softplus_fast meet their extremes."""
    from caspr_amd.train import flow_grad as FG
    frames, n = 3, 96
    R = frames * n
    blk = R if blk == "R" else blk
    z = rnd(1, 2 * R, C)
    b = rnd(2, C, scale=0.3)
    gate, beta = hyper(3, frames, C)
    beta[:, : C // 4] *= 40.0
    dh = rnd(5, 2 * R, C)
    z6, b6, g6, be6 = f64_leaves(z, b, gate, beta)
    zv6, zt6 = split_rows(z6, R, blk)
    hv6, ht6 = torch.func.jvp(lambda v: gated_softplus(v, b6, g6, be6, n), (zv6,), (zt6,))
    dhv, dht = split_rows(dh.double(), R, blk)
    ((hv6 * dhv).sum() + (ht6 * dht).sum()).backward()
    zd, bd, gd, bed = gpu_leaves(z, b, gate, beta)
    h = FG.CnfAct.apply(zd, bd, gd, bed, n, blk)
    (h * dh.to("cuda:0")).sum().backward()
    ck = Checks("cnf_act[%d,%d]" % (C, blk))
    ck("h", h, join_rows(hv6, ht6, blk), FWD)
    for nm, a, b_ in (("dZ", zd, z6), ("db", bd, b6), ("dgate", gd, g6), ("dbeta", bed, be6)):
        ck(nm, a.grad, b_.grad, GRAD)
    ck.done()


def _fused_inputs(frames, n, widths, seed=0):
    R = frames * n
    x = rnd(seed + 1, 2 * R, widths[0])
    ws, bs, gs, bes = [], [], [], []
    for i in range(len(widths) - 1):
        cin, cout = widths[i], widths[i + 1]
        ws.append(rnd(seed + 10 + i, cout, cin, scale=1.5 / np.sqrt(cin)))
        bs.append(rnd(seed + 20 + i, cout, scale=0.3))
        g, be = hyper(seed + 30 + 2 * i, frames, cout)
        gs.append(g)
        bes.append(be)
    wo = rnd(seed + 50, 3, widths[-1], scale=1.0 / np.sqrt(widths[-1]))
    return x, ws, bs, gs, bes, wo


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("n", [64, 192, 1024])
@pytest.mark.parametrize("kind", ["layer", "layer_out", "hidden"])
def test_cnf_fused_layers_vs_f64(kind, n, frames):
    """The fused route (row layout blk = 32): CnfLayer (caspr_conv1x1_cnf_act_bf16x6_f32 + caspr_cnf_act_bwd_f32), CnfLayerOut
    (+ caspr_cnf_act_bwd_out_f32) and CnfHidden (+ caspr_conv1x1_cnf_act_bwd_bf16x6_f32) at 512 -> 512 and at the narrower 256 -> 128
    that the bf16x6 conv accepts (Cin % 32, Cout % 4, 2n % 128): output rows and the gradients w.r.t. x and every parameter.
    The reference runs the same layers in f64 with the tangent rows as the jvp of the value map."""
    from caspr_amd.train import flow_grad as FG
    R = frames * n
    ck = Checks("cnf_%s[%d,%d]" % (kind, frames, n))
    for wide in ((512, 512), (256, 128)):
        widths = wide if kind != "hidden" else (wide[0], wide[1], wide[1])
        x, ws, bs, gs, bes, wo = _fused_inputs(frames, n, widths)
        L = len(ws)
        tag = "%d-%d:" % wide
        # f64 reference
        x6 = f64_leaves(x)[0]
        P6 = [f64_leaves(*grp) for grp in (ws, bs, gs, bes)]
        wo6 = f64_leaves(wo)[0]
        xv6, xt6 = split_rows(x6, R, 32)

        def f(v):
            for i in range(L):
                v = gated_softplus(v @ P6[0][i].t(), P6[1][i], P6[2][i], P6[3][i], n)
            return v if kind == "layer" else v @ wo6.t()
        ov6, ot6 = torch.func.jvp(f, (xv6,), (xt6,))
        out6 = join_rows(ov6, ot6, 32)
        dout = rnd(60, *out6.shape)
        (out6 * dout.double()).sum().backward()
        # HIP
        xd = gpu_leaves(x)[0]
        Pd = [gpu_leaves(*grp) for grp in (ws, bs, gs, bes)]
        wod = gpu_leaves(wo)[0]
        if kind == "layer":
            out = FG.CnfLayer.apply(xd, Pd[0][0], Pd[1][0], Pd[2][0], Pd[3][0], n)
        elif kind == "layer_out":
            out = FG.CnfLayerOut.apply(xd, Pd[0][0], Pd[1][0], Pd[2][0], Pd[3][0], wod, n)
        else:
            out = FG.CnfHidden.apply(xd, Pd[0][0], Pd[1][0], Pd[2][0], Pd[3][0], Pd[0][1], Pd[1][1], Pd[2][1], Pd[3][1], wod, n)
        (out * dout.to("cuda:0")).sum().backward()
        ck(tag + "out", out, out6, FWD)
        ck(tag + "dx", xd.grad, x6.grad, GRAD)
        for i in range(L):
            for nm, grp in zip(("dW", "db", "dgate", "dbeta"), range(4)):
                ck(tag + "%s%d" % (nm, i), Pd[grp][i].grad, P6[grp][i].grad, GRAD)
        if kind != "layer":
            ck(tag + "dWo", wod.grad, wo6.grad, GRAD)
    ck.done()


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("blk", ["R", 32])
def test_cnf_out_vs_f64(blk, strided):
    """CnfOut (caspr_cnf_out_f32 / _bwd_f32) on 3 frames of 160 points (not a multiple of the 256-thread block): a = dy/dt and
    nd = -e^T (df/dy) e, with gate / beta given contiguously or as column slices of wider tensors (ldg = 11 > 3); gradients
    w.r.t. Zo (value and tangent rows), b, gate, beta."""
    from caspr_amd.train import flow_grad as FG
    frames, n = 3, 160
    R = frames * n
    blk = R if blk == "R" else blk
    zo4 = rnd(1, 2 * R, 4)
    b = rnd(2, 3, scale=0.3)
    wide = 11 if strided else 3
    G, Bt = torch.sigmoid(rnd(3, frames, wide, scale=1.5)), rnd(4, frames, wide, scale=0.3)
    e = rnd(5, R, 3)
    da, dnd = rnd(6, frames, n, 3), rnd(7, frames, n, 1)
    cg, cb = (slice(4, 7), slice(1, 4)) if strided else (slice(0, 3), slice(0, 3))
    # f64: a is the output layer's value map, nd the contraction of its jvp along the tangent rows with e
    zo6, b6, G6, B6 = f64_leaves(zo4, b, G, Bt)
    zv6, zt6 = split_rows(zo6[:, :3], R, blk)
    a6, ad6 = torch.func.jvp(lambda v: (v + b6) * frame_rows(G6[:, cg], n) + frame_rows(B6[:, cb], n), (zv6,), (zt6,))
    nd6 = -(ad6 * e.double()).sum(dim=1, keepdim=True)
    ((a6 * da.double().reshape(R, 3)).sum() + (nd6 * dnd.double().reshape(R, 1)).sum()).backward()
    zod, bd, Gd, Bd = gpu_leaves(zo4, b, G, Bt)
    a, nd = FG.CnfOut.apply(zod[:, :3], bd, Gd[:, cg], Bd[:, cb], e.to("cuda:0"), n, blk)
    ((a * da.to("cuda:0")).sum() + (nd * dnd.to("cuda:0")).sum()).backward()
    ck = Checks("cnf_out[%d,%s]" % (blk, "ldg11" if strided else "ldg3"))
    ck("a", a.reshape(R, 3), a6, FWD)
    ck("nd", nd.reshape(R, 1), nd6, FWD)
    for nm, x_, r_ in (("dZo", zod, zo6), ("db", bd, b6), ("dgate", Gd, G6), ("dbeta", Bd, B6)):
        ck(nm, x_.grad, r_.grad, GRAD)
    ck.done()


# ---------------------------------------------------------------------------------------------
# B. one CNF block end to end against the oracle's differentiable mode
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,BT,n,steps,weights", [
    ("default", 3, 192, 1, "seeded"), ("default", 3, 192, 2, "seeded"),
    ("no_hidden_node", 3, 192, 1, "seeded"), ("no_hidden_node", 3, 192, 2, "seeded"),
    ("no_out_node", 3, 192, 1, "seeded"), ("no_out_node", 3, 192, 2, "seeded"),
    ("unfused", 3, 100, 1, "seeded"), ("unfused", 3, 100, 2, "seeded"),
    ("default", 2, 256, 1, "stress"), ("default", 2, 256, 2, "stress"),
])
def test_cnf_block_vs_f64_oracle(monkeypatch, seeded_sd, stress_sd, route, BT, n, steps, weights):
    """cnf_block_train against oracle.model.cnf_block in GRAD_MODE at f64 (the divergence by double backward, as the reference's
    training step): x_T, logp_T, the gradients w.r.t. x, context, logpx and every parameter of the block (the four layers'
    weights and biases, both hyper networks of each, sqrt_end_time), on each route of the ODE function."""
    from caspr_amd.models import CaSPR
    from caspr_amd.train import flow_grad as FG
    from oracle import model as O
    monkeypatch.setattr(O, "GRAD_MODE", True)
    monkeypatch.setattr(FG, "HIDDEN_NODE", route != "no_hidden_node")
    monkeypatch.setattr(FG, "OUT_NODE", route != "no_out_node")
    sd = seeded_sd if weights == "seeded" else stress_sd
    pre = "point_cnf.chain.1"
    m = CaSPR(cnf_rk4_steps=steps)
    m.load_state_dict(sd)
    block = m.point_cnf.chain[1].to("cuda:0").train()
    assert block.rk4_steps == steps and block.train_T
    zdim = m.cnf_args.zdim
    x, c, lp, e = rnd(1, BT, n, 3, scale=0.7), rnd(2, BT, zdim, scale=0.5), rnd(3, BT, n, 1), rnd(4, BT, n, 3)
    wx, wl = rnd(5, BT, n, 3), rnd(6, BT, n, 1)
    # f64 oracle
    names = [k for k in sd if k.startswith(pre + ".") and not k.endswith("_num_evals")]
    sd6 = {k: sd[k].detach().double().requires_grad_(True) for k in names}
    x6, c6, lp6 = f64_leaves(x, c, lp)
    xT6, lpT6 = O.cnf_block(sd6, pre, x6, c6, lp6, False, "rk4", steps, e.double())
    ((xT6 * wx.double()).sum() + (lpT6 * wl.double()).sum()).backward()
    # HIP
    xd, cd, lpd = gpu_leaves(x, c, lp)
    xT, lpT = FG.cnf_block_train(block, xd, cd, lpd, e.to("cuda:0"))
    ((xT * wx.to("cuda:0")).sum() + (lpT * wl.to("cuda:0")).sum()).backward()
    ck = Checks("cnf_block[%s,%s,%dx%d,rk4=%d]" % (route, weights, BT, n, steps))
    ck("x_T", xT, xT6, FWD)
    ck("logp_T", lpT, lpT6, FWD)
    for nm, a, b in (("dx", xd, x6), ("dcontext", cd, c6), ("dlogpx", lpd, lp6)):
        ck(nm, a.grad, b.grad, GRAD)
    params = dict(block.named_parameters())
    assert sorted(pre + "." + k for k in params) == sorted(names)
    for k, p in params.items():
        assert p.grad is not None, k
        ck("d" + k, p.grad, sd6[pre + "." + k].grad, GRAD)
    ck.done()


# ---------------------------------------------------------------------------------------------
# C. fixed-order scatters and centred grouping
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 61, 512])
@pytest.mark.parametrize("col0", [0, 3])
@pytest.mark.parametrize("form", ["ball_query", "three_interp"])
def test_segment_sum_vs_f64_index_add(form, col0, C):
    """caspr_segment_sum_f32 through train_ops.Segments against f64 index_add: duplicate targets, targets without contributors
    (accumulate=False writes 0 there, accumulate=True leaves dst alone), the unweighted ball-query form (entry e reads source row e)
    and the weighted three-interpolate form (src_rows), columns col0 .. col0 + C of a wider source.  Columns of dst past C are
    never written; two runs give the same bits."""
    from caspr_amd import train_ops as T
    dev = "cuda:0"
    g = np.random.default_rng(100 + C + col0)
    targets, nnz = 203, 1500
    tgt = torch.from_numpy(g.integers(0, 150, nnz).astype(np.int64))        # targets 150.. and the unlucky ones below get nothing
    tgt[:40] = 17                                                          # one heavily shared target
    lds = (col0 + C + 3) // 4 * 4 + 4
    if form == "ball_query":
        src = rnd(101, nnz, lds)
        w, rows = None, torch.arange(nnz)
        seg = T.Segments(tgt.to(dev), targets)
    else:
        src = rnd(101, 400, lds)
        w, rows = rnd(102, nnz).abs(), torch.from_numpy(g.integers(0, 400, nnz).astype(np.int64))
        seg = T.Segments(tgt.to(dev), targets, weight=w.to(dev), src_rows=rows.to(dev))
    contrib = src.double()[rows, col0:col0 + C] * (1.0 if w is None else w.double().unsqueeze(1))
    want = torch.zeros(targets, C, dtype=torch.float64).index_add_(0, tgt, contrib)
    empty = torch.bincount(tgt, minlength=targets) == 0
    assert int(empty.sum()) > 40
    ldd = (C + 3) // 4 * 4 + 4
    init = rnd(103, targets, ldd)
    srcd = src.to(dev)
    ck = Checks("segment_sum[%s,col0=%d,C=%d]" % (form, col0, C))
    outs = {}
    for acc in (False, True):
        runs = []
        for _ in range(2):
            dst = init.clone().to(dev)
            T.segment_sum(srcd, seg, C, dst, col0=col0, accumulate=acc)
            runs.append(dst.cpu())
        assert torch.equal(runs[0], runs[1]), "accumulate=%s: two runs differ" % acc
        got = runs[0]
        outs[acc] = got
        assert torch.equal(got[:, C:], init[:, C:]), "accumulate=%s: columns past C written" % acc
        ref = want + (init[:, :C].double() if acc else 0.0)
        ck("accumulate=%s" % acc, got[:, :C], ref, FWD, ref=float(want.abs().max()) + float(init[:, :C].abs().max()) * acc)
    assert bool((outs[False][empty, :C] == 0).all()), "accumulate=False: a target without contributors is not 0"
    assert torch.equal(outs[True][empty, :C], init[empty, :C]), "accumulate=True: a target without contributors changed"
    ck.done()


def _aug64(p, kind):
    """oracle.augment_input's columns for feat_kind (QUAD: [x2 y2 z2], PAIRS: [xz xy yz]) in f64."""
    from oracle import model as O
    a = O.augment_input(p, quad=True, pairs=True)
    return a[..., {1: slice(3, 6), 2: slice(6, 9), 3: slice(3, 9)}[kind]]


@pytest.mark.parametrize("feat_kind", [0, 1, 2, 3])
def test_group_rows_centred_vs_f64(feat_kind):
    """caspr_group_rows_f32 with centred = 1 (include/caspr_hip_train.h: every row minus its neighbourhood's sample-0 row; with
    feat_kind = CASPR_FEAT_QUAD | CASPR_FEAT_PAIRS the centred features are those of prep_input's augmentation, formed from the
    coordinates) against that rule built in f64 from oracle.augment_input: [xyz_i - xyz_i0 | f(xyz_i) - f(xyz_i0) | 0].
    Coordinates far from the origin make the squares large against their differences.  feat_kind = 0: generic features, f_i - f_i0."""
    from caspr_amd import train_ops as T
    from caspr_amd import ops
    dev = "cuda:0"
    B, n, M, ns = 2, 300, 37, 24
    g = np.random.default_rng(7)
    xyz = torch.from_numpy((g.uniform(-1, 1, (B, n, 3)) + np.array([3.0, -2.0, 5.0])).astype(np.float32))
    idx = torch.from_numpy(g.integers(0, n, (B, M, ns)).astype(np.int32))
    ctr = xyz[:, :M].contiguous()
    if feat_kind:
        kind = (ops.FEAT_QUAD if feat_kind & 1 else 0) | (ops.FEAT_PAIRS if feat_kind & 2 else 0)
        C = 3 * bin(feat_kind).count("1")
        feat = _aug64(xyz.double(), feat_kind).float()
        f64 = _aug64(xyz.double(), feat_kind)
    else:
        kind, C = 0, 13
        feat = rnd(8, B, n, C)
        f64 = feat.double()
    ldf = (C + 3) // 4 * 4
    G = T.group_rows(xyz.to(dev), ctr.to(dev), F.pad(feat, (0, ldf - C)).contiguous().to(dev), C, idx.to(dev), centred=True, feat_kind=kind)
    bi, li = torch.arange(B).view(B, 1, 1), idx.long()
    rows = torch.cat([xyz.double()[bi, li], f64[bi, li]], dim=3)                  # (B, M, ns, 3 + C)
    want = (rows - rows[:, :, :1]).reshape(B, M * ns, 3 + C)
    ck = Checks("group_rows_centred[kind=%d]" % feat_kind)
    got = G.cpu()
    assert bool((got[:, :, 3 + C:] == 0).all()), "pad columns not zero"
    ck("rows", got[:, :, :3 + C], want, FWD)
    ck.done()
