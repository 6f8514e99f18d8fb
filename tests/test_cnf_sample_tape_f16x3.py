"""The sampling solve with the tape on the 128-point f16x3 evaluation (csrc/ode_sample_tape_h3w.hip; train_ops.cnf_sample_tape_h3 /
cnf_sample_tape_h3_frames; config.cnf_tape_split = "f16x3"), on the GPU:

  1  x_0 is the inference kernel's: torch.equal with ops.cnf_rk4(..., w1h=, w2h=, reverse=True) on the same inputs;
  2  the tape against one RK4 step of oracle.model.odefunc in f64, replayed from the stored state (the check of
     tests/test_cnf_sample_grad.py::test_forward_kernel_vs_f64_oracle, its flat bound 1e-5 (1 + |x|max)); frame invariance;
  3  the per-frame form: the uniform entry's bits for an all-S table, a mixed table against single-frame launches, the launch order;
  4  gradients of decode(differentiable=True) under the switch against f64 autograd through oracle.model.point_cnf (loss 1e-5, rel L2
     2e-4 per tensor: the bounds of tests/test_cnf_sample_grad.py::test_gradients_vs_f64_oracle_autograd);
  5  the routes: the 64-point fallback, the switch off, the block's bits against decode()'s block solve, the two decodes at model level;
  6  bit reproducibility;  7  the range guard;  8  fit_latent.

The cases (BT, n, S, weights) are the smallest shapes at which the 128-point geometry can go wrong: one workgroup and one step; several
frames and steps; two workgroups per frame; a partial second workgroup; a workgroup with a single valid column."""
import pytest
import torch

from test_hip_train import REPORT, rel, rnd
from test_cnf_solve_kernels import Weights, base_samples
from test_cnf_sample_grad import PRE, X_TOL, _Checks, _decode_grads, _model, _one_step, _sd64, _sd_for
from test_cnf_sample_grad_frames import _decode_grads as _decode_grads_frames
from test_cnf_f16x3 import _packs, launch_h3

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(1, 128, 1, "seeded"), (3, 128, 4, "stress"), (2, 256, 2, "seeded"), (2, 200, 2, "stress"), (2, 129, 3, "seeded")]
CASE_IDS = ["bt%d-n%d-s%d-%s" % c for c in CASES]
MIXED = (4, 200, [3, 1, 4, 2])           # BT, n, table: unsorted, every count different, a one-step frame, a partial second workgroup
SENTINEL = -12345.5                      # finite, so that torch.equal works on rows the kernel must leave alone


def _flush():
    rel("cnf_sample_tape_h3_flush", torch.zeros(1), torch.zeros(1), 1.0)          # writes REPORT


class _HChecks(_Checks):
    """_Checks.close (|d| <= 1e-5 (1 + |want|max)) recording under cnf_sample_tape_h3:<case>:<tensor>."""

    def close(self, name, got, want):
        super().close(name, got, want)
        REPORT["cnf_sample_tape_h3:%s:%s" % (self.tag, name)] = REPORT.pop("cnf_sample_grad:%s:%s" % (self.tag, name))

    def done(self):
        _flush()
        assert not self.bad, self.tag + "\n" + "\n".join(self.bad)


@pytest.fixture(scope="module")
def weights(seeded_sd, stress_sd):
    dev = torch.device(DEV)
    return {"seeded": _packs(Weights(seeded_sd, dev)), "stress": _packs(Weights(stress_sd, dev))}


def itab(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _args(W, y, hyper):
    g = lambda v: v.to(DEV).contiguous()
    D = W.dev
    t_end = torch.tensor([W.t_end], device=DEV, dtype=torch.float32)
    return (g(y), g(hyper), D["tcol"], D["w0"], D["b0"], W.w1h, D["b1"], W.w2h, D["b2"], D["w3"], D["b3"], t_end)


def _launch(W, y, hyper, steps):
    from caspr_amd import ops
    from caspr_amd import train_ops as T
    out = T.cnf_sample_tape_h3(*_args(W, y, hyper), steps)
    torch.cuda.synchronize()
    ops.check_deferred_errors()
    return out


def _launch_frames(W, y, hyper, table, order=None, sentinel=False):
    from caspr_amd import ops
    from caspr_amd import train_ops as T
    S_alloc, (BT, n, _) = max(table), y.shape
    bufs = [torch.full((S_alloc, 4, BT, n, 3), SENTINEL, device=DEV) for _ in range(2)] if sentinel else [None, None]
    out = T.cnf_sample_tape_h3_frames(*_args(W, y, hyper), itab(table), S_alloc, order, bufs[0], bufs[1])
    torch.cuda.synchronize()
    ops.check_deferred_errors()
    return out


def _inputs(W, seed, BT, n):
    c, y = rnd(seed, BT, 1600), base_samples(seed + 1, BT, n)
    return c, y, W.hyper(c, 3078)


# ---------------------------------------------------------------------------------------------
# 1, 2: the uniform entry
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("BT,n,S,which", CASES, ids=CASE_IDS)
def test_x0_is_the_inference_kernels_bit_for_bit(BT, n, S, which, weights):
    """x_0 of cnf_sample_tape_h3 == ops.cnf_rk4(..., w1h=, w2h=, reverse=True, no MovingBatchNorm) on the same inputs, the same float32
    t_end and the same steps: the reference is the existing inference kernel (cnf_rk4_h3w_kernel)."""
    from caspr_amd import ops
    W = weights[which]
    _, y, hyper = _inputs(W, 9100 + 13 * BT + n + S, BT, n)
    want = launch_h3(W, y, hyper, S, True)
    torch.cuda.synchronize()
    ops.check_deferred_errors()
    gx, ys, ka = _launch(W, y, hyper, S)
    assert gx.shape == (BT, n, 3) and ys.shape == (S, 4, BT, n, 3) == ka.shape
    assert torch.equal(gx, want), "x_0 differs from the inference kernel's in %d values" % int((gx != want).sum())


@pytest.mark.parametrize("BT,n,S,which", CASES, ids=CASE_IDS)
def test_tape_vs_f64_oracle(BT, n, S, which, weights, seeded_sd, stress_sd):
    """ys[0, 0] is the input bit for bit; x(0) against oracle.cnf_block (reverse, RK4, f64); every stored stage input and stage output
    and each next state against the oracle's RK4 step replayed in f64 from the state the kernel stored at that step's beginning; a frame
    launched alone gives the bits it gives inside the batch (x_0, ys, ka)."""
    from oracle import model as O
    sd = {k: v.double() for k, v in (seeded_sd if which == "seeded" else stress_sd).items()}
    W = weights[which]
    c, y, hyper = _inputs(W, 9100 + 13 * BT + n + S, BT, n)
    gx, ys, ka = _launch(W, y, hyper, S)
    ck = _HChecks("bt%d-n%d-s%d-%s" % (BT, n, S, which))
    wx, _ = O.cnf_block(sd, PRE, y.double(), c.double(), None, True, "rk4", S, None)
    ck.close("x_0", gx, wx)
    assert torch.equal(ys[0, 0].cpu(), y), "the first stage input is the block's input"
    t_end = float(sd[PRE + ".sqrt_end_time"]) ** 2
    h = -t_end / S
    ys64 = ys.cpu().double()
    f = lambda t, y_: O.odefunc(sd, PRE + ".odefunc", t, y_, c.double())[0]
    for s in range(S):
        rec = []
        y1 = _one_step(f, ys64[s, 0], t_end + s * h, h, rec)
        ins, ks = rec[0]
        for st in range(4):
            if st > 0:
                ck.close("step%d:stage_in%d" % (s, st + 1), ys[s, st], ins[st])
            ck.close("step%d:a%d" % (s, st + 1), ka[s, st], ks[st])
        ck.close("step%d:next_state" % s, ys[s + 1, 0] if s + 1 < S else gx, y1)
    for k in range(BT):
        alone = _launch(W, y[k:k + 1], hyper[k:k + 1], S)
        for i, (nm, u, v) in enumerate(zip(("x_0", "stage_in", "a"), (gx, ys, ka), alone)):
            ub = u[k:k + 1] if i == 0 else u[:, :, k:k + 1]
            assert torch.equal(ub, v), "frame %d: %s differs alone / in the batch" % (k, nm)
    ck.done()


def test_fewer_than_128_points_are_refused_naming_the_64_point_entry(weights):
    """n < 128: the Python wrapper refuses, and so does the C entry, which names the entry to launch instead."""
    from caspr_amd import lib as _lib
    from caspr_amd import train_ops as T
    from caspr_amd.ops import _p, _stream
    W = weights["seeded"]
    _, y, hyper = _inputs(W, 9190, 1, 127)
    with pytest.raises(ValueError, match="cnf_sample_tape"):
        T.cnf_sample_tape_h3(*_args(W, y, hyper), 1)
    a = _args(W, y, hyper)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, ys, ka = torch.empty(1, 127, 3, device=DEV), torch.empty(1, 4, 1, 127, 3, device=DEV), torch.empty(1, 4, 1, 127, 3, device=DEV)
    with pytest.raises(_lib.CasprHipError, match="caspr_cnf_sample_tape_f32"):
        _lib.check(_lib.load().caspr_cnf_sample_tape_h3_f32(_p(a[0]), _p(a[1]), a[1].stride(0), *[_p(v) for v in a[2:11]], 512, _p(a[11]), 1, _p(word),
                                                            _p(out), _p(ys), _p(ka), 1, 127, _stream()), "caspr_cnf_sample_tape_h3_f32")


# ---------------------------------------------------------------------------------------------
# 3: the per-frame form
# ---------------------------------------------------------------------------------------------
def test_equal_counts_are_the_uniform_entry(weights):
    """A table of all S and no order gives the uniform entry's bits for x_0, ys, ka."""
    BT, n, S = 3, 200, 2
    W = weights["stress"]
    _, y, hyper = _inputs(W, 9201, BT, n)
    got = _launch_frames(W, y, hyper, [S] * BT)
    want = _launch(W, y, hyper, S)
    for nm, u, v in zip(("x_0", "stage_in", "a"), got, want):
        assert u.shape == v.shape and torch.equal(u, v), "%s differs between the table entry and the uniform entry" % nm


def test_mixed_table_rows_positions_and_order(weights):
    """Table (3, 1, 4, 2), n = 200, launched longest first: frame f's x_0 and tape rows are a uniform launch's on f alone at S_f, the
    tape sits at the frame's POSITION of the launch order, ys / ka handed in full of a sentinel still hold it in every row s >= S_f, and
    x_0 does not depend on the order (no order, and the reverse order, give the same bits; their tapes sit at their own positions)."""
    from caspr_amd import ops
    BT, n, table = MIXED
    W = weights["stress"]
    _, y, hyper = _inputs(W, 9211, BT, n)
    order = ops.cnf_steps_order(itab(table))
    perm = [int(v) for v in order.cpu()]
    assert perm == [2, 0, 3, 1]
    gx, ys, ka = _launch_frames(W, y, hyper, table, order, sentinel=True)
    alone = {f: _launch(W, y[f:f + 1], hyper[f:f + 1], table[f]) for f in range(BT)}
    for p, f in enumerate(perm):
        S = table[f]
        ax, ays, aka = alone[f]
        assert torch.equal(gx[f:f + 1], ax), "frame %d: x_0 differs from the uniform launch on it alone" % f
        assert torch.equal(ys[:S, :, p:p + 1], ays) and torch.equal(ka[:S, :, p:p + 1], aka), "frame %d: tape rows differ at position %d" % (f, p)
        for nm, t_ in (("ys", ys), ("ka", ka)):
            assert bool((t_[S:, :, p] == SENTINEL).all()), "position %d (frame %d): %s rows s >= %d were written" % (p, f, nm, S)
    for other in (None, itab(perm[::-1])):
        ox, oys, oka = _launch_frames(W, y, hyper, table, other, sentinel=True)
        assert torch.equal(ox, gx), "x_0 depends on the launch order"
        operm = list(range(BT)) if other is None else perm[::-1]
        for p, f in enumerate(operm):
            S = table[f]
            assert torch.equal(oys[:S, :, p:p + 1], alone[f][1]) and torch.equal(oka[:S, :, p:p + 1], alone[f][2])
            assert bool((oys[S:, :, p] == SENTINEL).all()) and bool((oka[S:, :, p] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------
# 4: gradients
# ---------------------------------------------------------------------------------------------
def _grad_report(tag, m, blocks, x, loss, gy, gz, grads, loss6, y6, z6, sd6):
    bad = []

    def l2(name, got, want):
        err = float((got.cpu().double() - want).norm() / want.norm().clamp_min(1e-12))
        REPORT["cnf_sample_grad_h3:%s:%s" % (tag, name)] = {"rel_l2": err, "ref_l2": float(want.norm()), "bound": 2e-4}
        if not (bool(torch.isfinite(got).all()) and err <= 2e-4):
            bad.append("%s: rel L2 %.3e" % (name, err))
    l2("dL/dy", gy[0], y6.grad)
    l2("dL/dz", gz[0], z6.grad)
    names = [k for k, _ in m.named_parameters() if k.startswith("point_cnf.")]
    assert len(names) == 21 * blocks + 4 and any(k.endswith("sqrt_end_time") for k in names)
    for k in names:
        assert grads[k] is not None, "no gradient for %s" % k
        assert sd6[k].grad is not None, "the oracle has no gradient for %s" % k
        l2(k, grads[k], sd6[k].grad)
    lerr = abs(float(loss) - float(loss6.detach())) / abs(float(loss6.detach()))
    REPORT["cnf_sample_grad_h3:%s:loss" % tag] = {"rel_err": lerr, "loss": float(loss6.detach()), "bound": 1e-5}
    _flush()
    assert lerr <= 1e-5, "loss %.9g vs %.9g" % (float(loss), float(loss6.detach()))
    assert not bad, tag + "\n" + "\n".join(bad)


def _count_h3(monkeypatch, name):
    """Counts the calls of train_ops.<name> (the new wrapper) without changing what it does."""
    from caspr_amd import train_ops as T
    calls, real = [], getattr(T, name)

    def spy(*a, **kw):
        calls.append(a[0].shape[1])
        return real(*a, **kw)
    monkeypatch.setattr(T, name, spy)
    return calls


GRAD_CASES = [c + (1,) for c in CASES] + [(3, 128, 2, "seeded", 2)]


@pytest.mark.parametrize("BT,n,S,which,blocks", GRAD_CASES, ids=["bt%d-n%d-s%d-%s-b%d" % c for c in GRAD_CASES])
def test_gradients_vs_f64_oracle_autograd(BT, n, S, which, blocks, seeded_sd, stress_sd, monkeypatch):
    """The procedure of tests/test_cnf_sample_grad.py::test_gradients_vs_f64_oracle_autograd with ops.CNF_TAPE_SPLIT = "f16x3": loss
    sum(w * x) through the whole reversed flow, the loss at 1e-5 relative, dL/dy, dL/dz and EVERY point_cnf parameter at rel L2 <= 2e-4
    against autograd through oracle.point_cnf in f64; none missing; every block's forward went through the new wrapper."""
    from caspr_amd import ops
    from oracle import model as O
    monkeypatch.setattr(ops, "CNF_TAPE_SPLIT", "f16x3")
    calls = _count_h3(monkeypatch, "cnf_sample_tape_h3")
    sd = _sd_for(which, blocks, seeded_sd, stress_sd)
    seed = 9500 + 13 * BT + n + S
    z, y, w = rnd(seed, 1, BT, 1600), rnd(seed + 1, 1, BT, n, 3, scale=1.3).clamp(-5.0, 5.0), rnd(seed + 2, 1, BT, n, 3)
    monkeypatch.setattr(O, "GRAD_MODE", True)
    sd6 = _sd64(sd)
    y6, z6 = y[0].double().requires_grad_(True), z[0].double().requires_grad_(True)
    x6 = O.point_cnf(sd6, y6, z6, None, True, "rk4", S, blocks=blocks)
    loss6 = (x6 * w[0].double()).sum()
    loss6.backward()
    m = _model(sd, S, blocks)
    x, loss, gy, gz, grads = _decode_grads(m, z, y, w, n)
    ops.check_deferred_errors()
    assert calls == [n] * blocks, "the f16x3 tape launch was not taken by every block: %s" % calls
    _grad_report("bt%d-n%d-s%d-%s-b%d" % (BT, n, S, which, blocks), m, blocks, x, loss, gy, gz, grads, loss6, y6, z6, sd6)


def test_frames_gradients_vs_f64_oracle_autograd(stress_sd, monkeypatch):
    """The (3, 1, 4, 2) table through decode(..., differentiable=True, frame_steps=table) under the switch: the same bounds against
    oracle.point_cnf in f64 run frame by frame at S_f, the losses summed."""
    from caspr_amd import ops
    from oracle import model as O
    monkeypatch.setattr(ops, "CNF_TAPE_SPLIT", "f16x3")
    calls = _count_h3(monkeypatch, "cnf_sample_tape_h3_frames")
    BT, n, table = MIXED
    z, y, w = rnd(9601, 1, BT, 1600), rnd(9602, 1, BT, n, 3, scale=1.3).clamp(-5.0, 5.0), rnd(9603, 1, BT, n, 3)
    monkeypatch.setattr(O, "GRAD_MODE", True)
    sd6 = _sd64(stress_sd)
    y6, z6 = y[0].double().requires_grad_(True), z[0].double().requires_grad_(True)
    loss6 = 0.0
    for f in range(BT):
        x6 = O.point_cnf(sd6, y6[f:f + 1], z6[f:f + 1], None, True, "rk4", table[f], blocks=1)
        loss6 = loss6 + (x6 * w[0, f:f + 1].double()).sum()
    loss6.backward()
    m = _model(stress_sd, 8, 1)
    x, loss, gy, gz, grads = _decode_grads_frames(m, z, y, w, n, itab(table))
    ops.check_deferred_errors()
    assert calls == [n] and int(m.get_nfe()[1]) == 4 * max(table)
    _grad_report("frames-bt%d-n%d-%s" % (BT, n, "".join(map(str, table))), m, 1, x, loss, gy, gz, grads, loss6, y6, z6, sd6)


# ---------------------------------------------------------------------------------------------
# 5: routes
# ---------------------------------------------------------------------------------------------
def test_64_points_fall_back_to_the_bf16x6_launch(stress_sd, monkeypatch):
    """With the switch on and n = 64, decode(differentiable=True) returns the bits it returns with the switch off, and the new wrapper
    is not called."""
    from caspr_amd import ops
    BT, n, S = 2, 64, 2
    m = _model(stress_sd, S)
    z, y = rnd(9701, 1, BT, 1600).to(DEV), rnd(9702, 1, BT, n, 3).to(DEV)
    off = m.decode(z, n, y=y, differentiable=True)[2].detach()
    monkeypatch.setattr(ops, "CNF_TAPE_SPLIT", "f16x3")
    calls = _count_h3(monkeypatch, "cnf_sample_tape_h3")
    on = m.decode(z, n, y=y, differentiable=True)[2].detach()
    assert calls == [] and torch.equal(on, off)


def test_switch_off_never_reaches_the_new_wrappers(stress_sd, monkeypatch):
    from caspr_amd import ops
    from caspr_amd import train_ops as T
    BT, n, S = 2, 128, 2

    def boom(*a, **kw):
        raise AssertionError("an f16x3 tape wrapper was called with cnf_tape_split at its default")
    monkeypatch.setattr(T, "cnf_sample_tape_h3", boom)
    monkeypatch.setattr(T, "cnf_sample_tape_h3_frames", boom)
    assert ops.cnf_tape_split() == "bf16x6"
    m = _model(stress_sd, S)
    z, y = rnd(9711, 1, BT, 1600).to(DEV), rnd(9712, 1, BT, n, 3).to(DEV)
    x = m.decode(z, n, y=y, differentiable=True)[2]
    x.sum().backward()
    x = m.decode(z, n, y=y, frame_steps=itab([2, 1]), differentiable=True)[2]
    assert bool(torch.isfinite(x).all())


def test_switch_on_block_bits_and_model_level_agreement(stress_sd, monkeypatch):
    """Switch on, n = 128: the block node's x equals the block's own inference solve without MovingBatchNorm (ops.cnf_rk4 on the f16x3
    route, as decode() runs it) bit for bit; at model level (MovingBatchNorm in torch against fused into the kernel) the two decodes
    agree within the flat bound; get_nfe() counts 4 S."""
    from caspr_amd import ops
    from caspr_amd.train import flow_grad as FG
    BT, n, S = 3, 128, 4
    m = _model(stress_sd, S)
    monkeypatch.setattr(ops, "CNF_TAPE_SPLIT", "f16x3")
    calls = _count_h3(monkeypatch, "cnf_sample_tape_h3")
    z, y = rnd(9721, 1, BT, 1600).to(DEV), rnd(9722, 1, BT, n, 3).to(DEV)
    block = m.point_cnf.chain[1]
    yb, c = y[0].contiguous(), z[0].contiguous()
    with torch.enable_grad():
        xb = FG.cnf_block_sample_train(block, yb.clone().requires_grad_(True), c)
    assert calls == [n] and xb.grad_fn is not None
    # the same block solve as inference launches it: the kernel's own arguments, no MovingBatchNorm at either end
    (G_lm, Bb_lm, tg_lm, tb_lm, widths), t_end, _, _, wb = FG._block_node_inputs(block, c, yb.device)
    hyper, tcol = FG._hyper_for_kernel(G_lm, Bb_lm, tg_lm, tb_lm, BT, widths)
    w0, b0, w1, b1, w2, b2, w3, b3 = [t_.detach().contiguous() for t_ in wb]
    w1x, w2x = block._weights_x6()
    w1h, w2h = block._weights_h3()
    t32 = float(t_end.detach().float())
    want = ops.cnf_rk4(yb, hyper, tcol, w0, b0, ops.PackedWeight(w1), b1, ops.PackedWeight(w2), b2, w3, b3, t32, S, True, None, None,
                       w1x=w1x, w2x=w2x, w1h=w1h, w2h=w2h)
    ops.check_deferred_errors()
    assert torch.equal(xb.detach(), want), "the block node's x differs from the inference kernel's in %d values" % int((xb.detach() != want).sum())
    xd = m.decode(z, n, y=y, differentiable=True)[2]
    assert int(m.get_nfe()[1]) == 4 * S and xd.grad_fn is not None
    x0 = m.decode(z, n, y=y)[2]
    ck = _HChecks("decode_routes")
    ck.close("x", xd, x0)
    ck.done()


# ---------------------------------------------------------------------------------------------
# 6: reproducibility
# ---------------------------------------------------------------------------------------------
def test_forward_and_backward_are_bit_reproducible(stress_sd, monkeypatch):
    from caspr_amd import ops
    monkeypatch.setattr(ops, "CNF_TAPE_SPLIT", "f16x3")
    BT, n, S = 3, 128, 4
    m = _model(stress_sd, S)
    z, y, w = rnd(51, 1, BT, 1600), rnd(52, 1, BT, n, 3), rnd(53, 1, BT, n, 3)
    xa, la, gya, gza, ga = _decode_grads(m, z, y, w, n)
    xb, lb, gyb, gzb, gb = _decode_grads(m, z, y, w, n)
    assert torch.equal(xa, xb) and torch.equal(la, lb) and torch.equal(gya, gyb) and torch.equal(gza, gzb)
    diff = [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert not diff, "gradients differ between two identical runs: %s" % diff[:5]


# ---------------------------------------------------------------------------------------------
# 7: the range guard
# ---------------------------------------------------------------------------------------------
def test_range_guard(weights):
    """The construction of tests/test_cnf_f16x3.py::test_range_guard (a layer-1 hyper bias of 5000 on ONE frame): that frame's x is NaN,
    the other frames keep their bits, check_deferred_errors raises naming cnf_tape_split="bf16x6", the channel is clean afterwards and a
    following clean launch raises nothing.  An error report through a status word: nothing faults."""
    from caspr_amd import lib as _lib
    from caspr_amd import ops
    from caspr_amd import train_ops as T
    W = weights["seeded"]
    BT, n, steps = 3, 130, 2
    _, y, hyper = _inputs(W, 3400, BT, n)
    clean = _launch(W, y, hyper, steps)
    hot = hyper.clone()
    hot[1, (3 * 512 + 3) + 512 + 7] = 5000.0
    got = T.cnf_sample_tape_h3(*_args(W, y, hot), steps)
    torch.cuda.synchronize()
    with pytest.raises(_lib.CasprHipError, match='cnf_tape_split="bf16x6"'):
        ops.check_deferred_errors()
    ops.check_deferred_errors()                      # reported once: the channel is clean
    assert bool(torch.isnan(got[0][1]).all())
    for f in (0, 2):
        assert torch.equal(got[0][f], clean[0][f]), "frame %d changed beside the frame the guard caught" % f
        assert torch.equal(got[1][:, :, f], clean[1][:, :, f]) and torch.equal(got[2][:, :, f], clean[2][:, :, f])
    again = _launch(W, y, hyper, steps)
    for u, v in zip(again, clean):
        assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------
# 8: fit_latent
# ---------------------------------------------------------------------------------------------
def test_fit_latent_under_the_switch(seeded_sd, monkeypatch):
    """Three Adam steps at BT = 2, n = 128, S = 2 with the switch on: the loss AFTER the third step (one more forward on the same route,
    fit_latent's own loss) is below the first, every value is finite, every forward went through the new launch."""
    from caspr_amd import losses, ops
    from caspr_amd.utils.fit import fit_latent
    monkeypatch.setattr(ops, "CNF_TAPE_SPLIT", "f16x3")
    calls = _count_h3(monkeypatch, "cnf_sample_tape_h3")
    m = _model(seeded_sd, 2)
    z_true, y = rnd(9901, 1, 2, 1600).to(DEV), rnd(9902, 1, 2, 128, 3).to(DEV)
    with torch.no_grad():
        target = m.decode(z_true, 128, y=y)[2].contiguous()
    z_init = z_true + 0.05 * rnd(9904, 1, 2, 1600).to(DEV)
    z, curve = fit_latent(m, target, z_init, 128, steps=3, y=y)
    with torch.enable_grad():
        after = float(losses.chamfer_loss(m.decode(z.clone().requires_grad_(True), 128, y=y, differentiable=True)[2], target).detach())
    torch.cuda.synchronize()
    ops.check_deferred_errors()
    curve = curve + [after]
    REPORT["cnf_sample_grad_h3:fit_latent:loss_curve"] = {"loss": curve}
    _flush()
    assert calls == [128] * 4
    assert len(curve) == 4 and all(c == c and abs(c) != float("inf") for c in curve), curve
    assert curve[-1] < curve[0], curve
    assert bool(torch.isfinite(z).all())
