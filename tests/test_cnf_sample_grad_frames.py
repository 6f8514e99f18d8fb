"""decode(differentiable=True, frame_steps=...): the gradient through the point CNF's SAMPLING solve with an RK4 step count PER FRAME,
each held fixed (train/flow_grad.py: CnfSampleSolveFrames; csrc/ode_sample_tape.hip: caspr_cnf_sample_tape_frames_f32).

Forward = the tape kernel of tests/test_cnf_sample_grad.py with a step table and a launch order: frame order[p] integrates S_f steps of
h_f = -t_end / S_f and writes its tape at POSITION p, rows s < S_f only.  Backward = the reverse sweep on the prefix of positions still
integrating at each step.  Checked here:

  CPU   the sweep's algebra (per-frame h and stage times, the prefix slices, 1 / S_f in dL/dt_end, the un-permutation) against f64
        autograd frame by frame, on a tape whose unwritten rows hold NaN; that the comparison sees a uniform count; the surface;
  GPU   the kernel against the oracle's RK4 in f64 frame by frame with poisoned tapes, equal counts against the uniform entry, a frame
        alone against the batch, every gradient against f64 oracle autograd, the uniform route frame by frame, reproducibility, the
        pilot against the inference route, fit_latent, the refusals.

Bounds are those of tests/test_cnf_sample_grad.py for the same reasons: state-like values 1e-5 x (1 + |x|max); gradients loss 1e-5
relative and rel L2 2e-4 per tensor against f64; 1e-6 rel L2 between the two routes on the same frame (the same kernels on the same
values: only the association of sums differs); 1e-9 relative for the f64 algebra."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import frame_steps_ref as R
from test_cnf_sample_grad import _Checks, _eval_f64, _model, _one_step, _rk4_down, _sd64, _two_block_sd
from test_cnf_solve_kernels import Weights, base_samples
from test_hip_train import REPORT, rel, rnd

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PRE = "point_cnf.chain.1"
TAG = "cnf_sample_grad_frames"
X_TOL = 1e-5


def _flush():
    rel(TAG + "_flush", torch.zeros(1), torch.zeros(1), 1.0)          # writes REPORT


class _FChecks(_Checks):
    """_Checks of tests/test_cnf_sample_grad.py, recorded under this file's prefix."""

    def close(self, name, got, want):
        got, want = got.detach().cpu().double(), want.detach().cpu().double()
        assert got.shape == want.shape, (name, got.shape, want.shape)
        m = float(want.abs().max())
        bound, err = X_TOL * (1.0 + m), float((got - want).abs().max())
        REPORT["%s:%s:%s" % (TAG, self.tag, name)] = {"max_abs_err": err, "bound": bound, "ref_absmax": m}
        if not (bool(torch.isfinite(got).all()) and err <= bound):
            self.bad.append("%s: max abs err %.3e > %.3e" % (name, err, bound))

    def done(self):
        _flush()
        assert not self.bad, self.tag + "\n" + "\n".join(self.bad)


def _order_of(steps):
    """Longest first, ties by ascending frame: what ops.cnf_steps_order returns (tests/frame_steps_ref.py: order)."""
    return torch.sort(steps.cpu(), stable=True, descending=True).indices.to(torch.int32).to(steps.device)


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def _algebra_setup():
    BT, n = 4, 5
    widths, cin = (7, 6, 5, 3), (3, 7, 6, 5)
    gen = torch.Generator().manual_seed(23)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=gen, dtype=torch.float64) * scale)
    wb = [t_ for l in range(4) for t_ in (r(widths[l], cin[l], scale=0.7), r(widths[l], scale=0.3))]
    tot = BT * sum(widths)
    leaves = {"y": r(BT, n, 3), "G_lm": r(tot), "Bb_lm": r(tot, scale=0.5), "tg": r(sum(widths)), "tb": r(sum(widths)), "t_end": r(()).abs() + 0.7}
    for i, t_ in enumerate(wb):
        leaves["wb%d" % i] = t_
    for t_ in leaves.values():
        t_.requires_grad_(True)
    return BT, n, widths, leaves, r(BT, n, 3)


def _frame_lm(v_lm, f, BT, widths):
    """Layer-major tensor over BT frames -> the layer-major tensor of frame f alone."""
    from caspr_amd.train.flow_grad import _layer_views
    return torch.cat([u[f:f + 1].reshape(-1) for u in _layer_views(v_lm, BT, widths)])


def _reference_grads(BT, n, widths, leaves, wy, counts):
    """Autograd through _rk4_down, frame by frame with that frame's count, the losses summed."""
    wbl = [leaves["wb%d" % i] for i in range(8)]
    loss, xs = 0.0, []
    for f in range(BT):
        G, Bb = _frame_lm(leaves["G_lm"], f, BT, widths), _frame_lm(leaves["Bb_lm"], f, BT, widths)
        fn = lambda t, y_, G=G, Bb=Bb: _eval_f64(wbl, t, y_, G, Bb, leaves["tg"], leaves["tb"], 1, n, widths)   # one frame: its time columns are the rows themselves
        x = _rk4_down(fn, leaves["y"][f:f + 1], leaves["t_end"], counts[f])
        xs.append(x)
        loss = loss + (x * wy[f:f + 1]).sum()
    return torch.cat(xs), torch.autograd.grad(loss, list(leaves.values()))


def _tape_frames_restatement(BT, n, widths, seen):
    """caspr_cnf_sample_tape_frames_f32 (train_ops.cnf_sample_tape_frames) restated in plain torch for (BT, n, widths); appends the
    (launch order, counts) of every call to `seen`.  Module level so that tools/flow_grad_diff.py can import it."""
    cols = np.cumsum((0,) + widths)

    def tape_restatement(y, hyper, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, t_end, steps, max_steps, order=None, ys=None, ka=None):
        # as the kernel: position p holds frame order[p], rows s < S_f written, everything else NaN (torch.empty in the wrapper)
        nG = sum(widths)
        counts = [int(v) for v in steps]
        assert max_steps == max(counts), "the tape has max_f S_f step rows"
        perm = list(range(BT)) if order is None else [int(v) for v in order]
        x0 = torch.empty_like(y)
        ys = torch.full((max_steps, 4, BT, n, 3), float("nan"), dtype=y.dtype)
        ka = torch.full((max_steps, 4, BT, n, 3), float("nan"), dtype=y.dtype)
        for p, f in enumerate(perm):
            lm = lambda row: torch.cat([row[cols[l]:cols[l + 1]] for l in range(4)])
            G, Bb, tg, tb = lm(hyper[f, :nG]), lm(hyper[f, nG:]), lm(tcol[:nG]), lm(tcol[nG:])
            rec = []
            fn = lambda t, y_: _eval_f64((w0, b0, w1x, b1, w2x, b2, w3, b3), t, y_, G, Bb, tg, tb, 1, n, widths)
            x0[f:f + 1] = _rk4_down(fn, y[f:f + 1], t_end.reshape(()), counts[f], rec)
            for s, (ins, ks) in enumerate(rec):
                ys[s, :, p] = torch.stack(ins)[:, 0]
                ka[s, :, p] = torch.stack(ks)[:, 0]
        seen.append((perm, counts))
        return x0, ys, ka
    return tape_restatement


def _node_grads(monkeypatch, BT, n, widths, leaves, wy, table, seen):
    """CnfSampleSolveFrames with the tape launch, the order kernel and the per-evaluation rebuild replaced by f64 torch restatements."""
    from caspr_amd.train import flow_grad as FG
    cols = np.cumsum((0,) + widths)
    over_frames = lambda v: torch.cat([v[cols[l]:cols[l + 1]].unsqueeze(0).expand(BT, -1).reshape(-1) for l in range(4)])
    wbl = [leaves["wb%d" % i] for i in range(8)]
    monkeypatch.setattr(FG.T, "cnf_sample_tape_frames", _tape_frames_restatement(BT, n, widths, seen))
    monkeypatch.setattr(FG.ops, "cnf_steps_order", _order_of)
    monkeypatch.setattr(FG, "_cnf_eval_value", _eval_f64)
    x = FG.CnfSampleSolveFrames.apply(leaves["y"], leaves["G_lm"], leaves["Bb_lm"], over_frames(leaves["tg"]), over_frames(leaves["tb"]), leaves["t_end"],
                                      wbl[2], wbl[4], table, 64, widths, *wbl)
    return x, torch.autograd.grad((x * wy).sum(), list(leaves.values()))


def _compare(leaves, got, want):
    bad = []
    for name, g, w in zip(leaves, got, want):
        err = float((g - w).abs().max() / w.abs().max().clamp_min(1e-30))
        if not err <= 1e-9:
            bad.append("%s: %.3e" % (name, err))
    return bad


def test_frames_sweep_algebra_vs_f64_autograd(monkeypatch):
    """Table [3, 1, 2, 3] (unsorted, a tie, a one-step frame), BT = 4, n = 5, widths (7, 6, 5, 3): every gradient of CnfSampleSolveFrames
    (y, the four hyper tensors, t_end, all weights and biases) against autograd through a plain reversed-time RK4 run frame by frame with
    that frame's count, at 1e-9 of the reference's largest entry.  The restated tape is in launch order with NaN in every row a frame
    does not write: a sweep that reads one of them, uses one frame's h for another or drops the 1 / S_f of dL/dt_end is off by order one
    or NaN.  The same comparison against a reference run at the uniform count max S_f fails, so it can tell the two apart."""
    BT, n, widths, leaves, wy = _algebra_setup()
    table = torch.tensor([3, 1, 2, 3], dtype=torch.int32)
    seen = []
    x, got = _node_grads(monkeypatch, BT, n, widths, leaves, wy, table, seen)
    assert seen == [([0, 3, 2, 1], [3, 1, 2, 3])], seen             # launched longest first, stable
    x_ref, want = _reference_grads(BT, n, widths, leaves, wy, [3, 1, 2, 3])
    assert torch.allclose(x, x_ref, rtol=0, atol=1e-12)
    bad = _compare(leaves, got, want)
    assert not bad, "\n".join(bad)
    _, uniform = _reference_grads(BT, n, widths, leaves, wy, [3, 3, 3, 3])
    assert _compare(leaves, got, uniform), "the comparison cannot tell the per-frame counts from the uniform count"


def test_frames_surface(monkeypatch):
    """Header and lib.SIGNATURES agree on the new entry's 23 arguments (tests/test_host_cpu.py then holds the library to both); the
    wrapper and the node exist; decode / reconstruct / fit_latent have the keyword, `differentiable` still last and False; a table entry
    of 0 or above the allowed maximum is refused with its frame; frame_steps without differentiable=True is refused."""
    from caspr_amd import lib
    from caspr_amd import train_ops as T
    from caspr_amd.models import CaSPR
    from caspr_amd.train import flow_grad as FG
    from caspr_amd.utils.fit import fit_latent
    name = "caspr_cnf_sample_tape_frames_f32"
    hdr = open(os.path.join(ROOT, "include", "caspr_hip_train.h")).read()
    m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
    assert m, "%s is not declared in include/caspr_hip_train.h" % name
    assert len(lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1 == 23
    assert len(lib.SIGNATURES[name][1]) == len(lib.SIGNATURES["caspr_cnf_sample_tape_f32"][1]) + 2
    assert callable(T.cnf_sample_tape_frames) and hasattr(FG, "CnfSampleSolveFrames")
    for fn in (CaSPR.decode, CaSPR.reconstruct, fit_latent, FG.cnf_block_sample_train, FG.point_cnf_sample_train):
        assert inspect.signature(fn).parameters["frame_steps"].default is None, fn
    assert inspect.signature(fit_latent).parameters["pilot_every"].default == 1
    for meth in (CaSPR.decode, CaSPR.reconstruct):
        p = list(inspect.signature(meth).parameters.values())[-1]
        assert p.name == "differentiable" and p.default is False, meth
    monkeypatch.setattr(FG.ops, "cnf_steps_order", _order_of)
    tab = lambda v: torch.tensor(v, dtype=torch.int32)
    assert FG._frames_plan(tab([2, 5, 2]), 5)[:2] == ([2, 5, 2], [1, 0, 2])
    with pytest.raises(ValueError, match="frame 1 "):
        FG._frames_plan(tab([2, 0, 2]), 64)
    with pytest.raises(ValueError, match="frame 2 "):
        FG._frames_plan(tab([2, 4, 65]), 64)
    with pytest.raises(ValueError, match="int32"):
        FG._frames_plan(tab([2, 4]).long(), 64)
    mdl = CaSPR()
    z, y = torch.zeros(1, 2, 1600), torch.zeros(1, 2, 8, 3)
    with pytest.raises(ValueError, match="differentiable=True"):
        mdl.decode(z, 8, y=y, frame_steps=tab([2, 2]))
    with pytest.raises(ValueError, match="differentiable=True"):
        mdl.reconstruct(torch.zeros(1, 2, 8, 4), 8, y=y, frame_steps="pilot")
    with pytest.raises(ValueError, match="frame_steps"):
        mdl.decode(z.requires_grad_(True), 8, y=y, frame_steps="ladder", differentiable=True)


# ---------------------------------------------------------------------------------------------
# GPU 1: the kernel
# ---------------------------------------------------------------------------------------------
def itab(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda:0")


def _launch(W, y, hyper, table, order=None, poison=False):
    from caspr_amd import train_ops as T
    g = lambda v: v.to("cuda:0").contiguous()
    D = W.dev
    t_end = torch.tensor([W.t_end], device="cuda:0", dtype=torch.float32)
    S_alloc, (BT, n, _) = max(table), y.shape
    bufs = [torch.full((S_alloc, 4, BT, n, 3), float("nan"), device="cuda:0") for _ in range(2)] if poison else [None, None]
    out = T.cnf_sample_tape_frames(g(y), g(hyper), D["tcol"], D["w0"], D["b0"], W.w1x, D["b1"], W.w2x, D["b2"], D["w3"], D["b3"], t_end,
                                   itab(table), S_alloc, order, bufs[0], bufs[1])
    torch.cuda.synchronize()
    return out


# (weights, BT, n, table): several workgroup rows with an unsorted table, a tie and a one-step frame; two workgroups per frame; a partial
# workgroup; fewer points than a wave owns
CASES = [("stress", 4, 64, [3, 1, 2, 3]), ("seeded", 3, 128, [2, 4, 1]), ("stress", 2, 100, [1, 3]), ("seeded", 2, 8, [2, 1])]
CASE_IDS = ["%s-bt%d-n%d-%s" % (c[0], c[1], c[2], "".join(map(str, c[3]))) for c in CASES]


@pytest.fixture(scope="module")
def weights(seeded_sd, stress_sd):
    dev = torch.device("cuda:0")
    return {"seeded": Weights(seeded_sd, dev), "stress": Weights(stress_sd, dev)}


@pytest.mark.gpu
@pytest.mark.parametrize("ordered", [False, True], ids=["no_order", "longest_first"])
@pytest.mark.parametrize("which,BT,n,table", CASES, ids=CASE_IDS)
def test_frames_kernel_vs_f64_oracle(which, BT, n, table, ordered, weights, seeded_sd, stress_sd):
    """Frame f's x(0) against oracle.cnf_block (reverse, RK4, S_f steps, f64) at the flat bound; every stored stage input and output of
    the steps s < S_f against the oracle's RK4 step replayed in f64 from the stored state; ys / ka handed in full of NaN come back with
    exactly the rows s >= S_f of every POSITION still all NaN and every other row finite."""
    from caspr_amd import ops
    from oracle import model as O
    sd = {k: v.double() for k, v in (seeded_sd if which == "seeded" else stress_sd).items()}
    W = weights[which]
    seed = 9700 + 13 * BT + n
    c, y = rnd(seed, BT, 1600), base_samples(seed + 1, BT, n)
    hyper = W.hyper(c, 3078)
    order = ops.cnf_steps_order(itab(table)) if ordered else None
    perm = list(range(BT)) if order is None else [int(v) for v in order.cpu()]
    if ordered:
        assert perm == [int(v) for v in R.order(torch.tensor(table))]
    gx, ys, ka = _launch(W, y, hyper, table, order, poison=True)
    S_alloc = max(table)
    assert gx.shape == (BT, n, 3) and ys.shape == (S_alloc, 4, BT, n, 3) == ka.shape
    ck = _FChecks("fwd:%s-bt%d-n%d-%s" % (which, BT, n, "ordered" if ordered else "plain"))
    t_end = float(sd[PRE + ".sqrt_end_time"]) ** 2
    ys64 = ys.cpu().double()
    for p, f in enumerate(perm):
        S = table[f]
        for nm, t_ in (("stage_in", ys), ("a", ka)):
            rows = t_[:, :, p]
            assert bool(torch.isfinite(rows[:S]).all()), "position %d (frame %d): a written row of %s is not finite" % (p, f, nm)
            assert bool(torch.isnan(rows[S:]).all()), "position %d (frame %d): %s rows s >= %d were written" % (p, f, nm, S)
        cf = c[f:f + 1].double()
        wx, _ = O.cnf_block(sd, PRE, y[f:f + 1].double(), cf, None, True, "rk4", S, None)
        ck.close("frame%d:x_0" % f, gx[f:f + 1], wx)
        assert torch.equal(ys[0, 0, p].cpu(), y[f]), "the first stage input is the frame's input"
        h = -t_end / S
        fn = lambda t, y_: O.odefunc(sd, PRE + ".odefunc", t, y_, cf)[0]
        for s in range(S):
            rec = []
            y1 = _one_step(fn, ys64[s, 0, p:p + 1], t_end + s * h, h, rec)
            ins, ks = rec[0]
            for st in range(4):
                if st > 0:
                    ck.close("frame%d:step%d:stage_in%d" % (f, s, st + 1), ys[s, st, p:p + 1], ins[st])
                ck.close("frame%d:step%d:a%d" % (f, s, st + 1), ka[s, st, p:p + 1], ks[st])
            ck.close("frame%d:step%d:next_state" % (f, s), ys[s + 1, 0, p:p + 1] if s + 1 < S else gx[f:f + 1], y1)
    ck.done()


@pytest.mark.gpu
def test_equal_counts_are_the_uniform_kernel(weights):
    """A table of all S without an order gives x_0, ys and ka bit for bit those of caspr_cnf_sample_tape_f32 at S: one kernel text."""
    from caspr_amd import train_ops as T
    BT, n, S = 3, 100, 2
    W = weights["stress"]
    c, y = rnd(9801, BT, 1600), base_samples(9802, BT, n)
    hyper = W.hyper(c, 3078)
    got = _launch(W, y, hyper, [S] * BT)
    D = W.dev
    t_end = torch.tensor([W.t_end], device="cuda:0", dtype=torch.float32)
    want = T.cnf_sample_tape(y.to("cuda:0"), hyper.to("cuda:0"), D["tcol"], D["w0"], D["b0"], W.w1x, D["b1"], W.w2x, D["b2"], D["w3"], D["b3"], t_end, S)
    for nm, u, v in zip(("x_0", "stage_in", "a"), got, want):
        assert u.shape == v.shape and torch.equal(u, v), "%s differs between the table entry and the uniform entry" % nm


@pytest.mark.gpu
def test_a_frame_does_not_depend_on_its_batch(weights):
    """Frame f launched alone with [S_f] gives the bits it gives inside the (ordered) batch, in x_0 and in its tape rows."""
    from caspr_amd import ops
    which, BT, n, table = CASES[0]
    W = weights[which]
    c, y = rnd(9811, BT, 1600), base_samples(9812, BT, n)
    hyper = W.hyper(c, 3078)
    order = ops.cnf_steps_order(itab(table))
    gx, ys, ka = _launch(W, y, hyper, table, order)
    for p, f in enumerate(int(v) for v in order.cpu()):
        ax, ays, aka = _launch(W, y[f:f + 1], hyper[f:f + 1], [table[f]])
        assert torch.equal(gx[f:f + 1], ax), "frame %d: x_0 differs alone / in the batch" % f
        assert torch.equal(ys[:table[f], :, p:p + 1], ays) and torch.equal(ka[:table[f], :, p:p + 1], aka), "frame %d: tape rows differ" % f


# ---------------------------------------------------------------------------------------------
# GPU 2: the model surface
# ---------------------------------------------------------------------------------------------
def _decode_grads(m, z, y, w, n, frame_steps):
    """decode(differentiable=True, frame_steps=...) forward + backward of sum(w * x) -> (x, loss, dL/dy, dL/dz, {parameter: gradient})."""
    m.zero_grad()
    zd, yd = z.to("cuda:0").requires_grad_(True), y.to("cuda:0").requires_grad_(True)
    x = m.decode(zd, n, y=yd, frame_steps=frame_steps, differentiable=True)[2]
    loss = (x * w.to("cuda:0")).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters() if k.startswith("point_cnf.")}
    return x.detach(), loss.detach(), yd.grad.detach().clone(), zd.grad.detach().clone(), grads


GRAD_CASES = [c + (1,) for c in CASES] + [("seeded", 3, 64, [2, 1, 2], 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("which,BT,n,table,blocks", GRAD_CASES, ids=[i + "-b1" for i in CASE_IDS] + ["seeded-bt3-n64-212-b2"])
def test_frames_gradients_vs_f64_oracle_autograd(which, BT, n, table, blocks, seeded_sd, stress_sd, monkeypatch):
    """Loss sum(w * x) through the whole reversed flow (MBN, CNF x blocks, MBN) with the table: the loss at 1e-5 relative, dL/dy, dL/dz
    and EVERY point_cnf parameter (none may be missing) at rel L2 <= 2e-4 against autograd through oracle.point_cnf in f64 run frame by
    frame at S_f, the losses summed: the bounds of tests/test_cnf_sample_grad.py::test_gradients_vs_f64_oracle_autograd."""
    from oracle import model as O
    sd = seeded_sd if which == "seeded" else stress_sd
    sd = _two_block_sd(sd) if blocks == 2 else sd
    seed = 9900 + 13 * BT + n
    z, y, w = rnd(seed, 1, BT, 1600), rnd(seed + 1, 1, BT, n, 3, scale=1.3).clamp(-5.0, 5.0), rnd(seed + 2, 1, BT, n, 3)
    monkeypatch.setattr(O, "GRAD_MODE", True)
    sd6 = _sd64(sd)
    y6, z6 = y[0].double().requires_grad_(True), z[0].double().requires_grad_(True)
    loss6 = 0.0
    for f in range(BT):
        x6 = O.point_cnf(sd6, y6[f:f + 1], z6[f:f + 1], None, True, "rk4", table[f], blocks=blocks)
        loss6 = loss6 + (x6 * w[0, f:f + 1].double()).sum()
    loss6.backward()
    m = _model(sd, 8, blocks)
    x, loss, gy, gz, grads = _decode_grads(m, z, y, w, n, itab(table))
    assert int(m.get_nfe()[1]) == 4 * max(table) * blocks
    tag = "grad:%s-bt%d-n%d-b%d" % (which, BT, n, blocks)
    bad = []

    def l2(name, got, want):
        err = float((got.cpu().double() - want).norm() / want.norm().clamp_min(1e-12))
        REPORT["%s:%s:%s" % (TAG, tag, name)] = {"rel_l2": err, "ref_l2": float(want.norm()), "bound": 2e-4}
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
    REPORT["%s:%s:loss" % (TAG, tag)] = {"rel_err": lerr, "loss": float(loss6.detach()), "bound": 1e-5}
    _flush()
    assert lerr <= 1e-5, "loss %.9g vs %.9g" % (float(loss), float(loss6.detach()))
    assert not bad, tag + "\n" + "\n".join(bad)


@pytest.mark.gpu
def test_frames_route_equals_the_uniform_route_frame_by_frame(stress_sd):
    """Frame f's dL/dy_f and dL/dz_f from the table route equal, at rel L2 <= 1e-6, those of the uniform route run on frame f alone with
    cnf_rk4_steps = S_f (the same kernels on the same values; only the association of sums differs)."""
    which, BT, n, table = CASES[0]
    z, y, w = rnd(9951, 1, BT, 1600), rnd(9952, 1, BT, n, 3, scale=1.3), rnd(9953, 1, BT, n, 3)
    _, _, gy, gz, _ = _decode_grads(_model(stress_sd, 8), z, y, w, n, itab(table))
    bad = []
    for f in range(BT):
        mu = _model(stress_sd, table[f])
        mu.zero_grad()
        zd, yd = z[:, f:f + 1].to("cuda:0").requires_grad_(True), y[:, f:f + 1].to("cuda:0").requires_grad_(True)
        xu = mu.decode(zd, n, y=yd, differentiable=True)[2]
        (xu * w[:, f:f + 1].to("cuda:0")).sum().backward()
        for nm, got, want in (("dL/dy", gy[:, f:f + 1], yd.grad), ("dL/dz", gz[:, f:f + 1], zd.grad)):
            err = float((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-30))
            REPORT["%s:vs_uniform:frame%d:%s" % (TAG, f, nm)] = {"rel_l2": err, "bound": 1e-6}
            if not err <= 1e-6:
                bad.append("frame %d %s: rel L2 %.3e" % (f, nm, err))
    _flush()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_frames_forward_and_backward_are_bit_reproducible(stress_sd):
    """Two forward + backward runs with the table [3, 1, 2, 3]: identical bits in the output and in every gradient (fixed sweep order,
    index assignments over unique indices, no atomics)."""
    which, BT, n, table = CASES[0]
    m = _model(stress_sd, 8)
    z, y, w = rnd(9961, 1, BT, 1600), rnd(9962, 1, BT, n, 3), rnd(9963, 1, BT, n, 3)
    xa, la, gya, gza, ga = _decode_grads(m, z, y, w, n, itab(table))
    xb, lb, gyb, gzb, gb = _decode_grads(m, z, y, w, n, itab(table))
    assert torch.equal(xa, xb) and torch.equal(la, lb) and torch.equal(gya, gyb) and torch.equal(gza, gzb)
    diff = [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert not diff, "gradients differ between two identical runs: %s" % diff[:5]


def _pilot_inputs():
    """B T = 4 frames of 128 points: frames 0, 1, 4, 5 of the rule test of tests/test_cnf_frame_steps.py (contexts rnd(11, 6, 1600) scaled
    by 0.25, 0.5, 1.5, 2.0; base_samples(12, 6, 64) as the 64 pilot points), 64 more points behind them."""
    pick = [0, 1, 4, 5]
    z = (rnd(11, 6, 1600) * torch.tensor([0.25, 0.5, 1.0, 1.0, 1.5, 2.0]).view(6, 1))[pick]
    y = torch.cat([base_samples(12, 6, 64)[pick], base_samples(14, 4, 64)], dim=1)
    return z.view(1, 4, 1600).contiguous(), y.view(1, 4, 128, 3).contiguous()


def test_pilot_inputs_give_distinct_counts_in_f64(stress_sd):
    """The f64 solve of the pilot test's inputs through tests/frame_steps_ref.py: ladder chooses at least two distinct counts, so the GPU
    test below shows something."""
    from test_cnf_solve_kernels import block_params, cnf_solve_f64, hyper_of, mbn_of, solve_args
    sd = {k: v.double() for k, v in stress_sd.items()}
    P = block_params(sd)
    z, y = _pilot_inputs()
    hyper, yp = hyper_of(P, z[0].double()), y[0, :, :64].double()
    solve = lambda S: cnf_solve_f64(yp, hyper, *solve_args(P), P["t_end"], S, True, mbn_of(sd, 2), mbn_of(sd, 0))[0]
    with torch.no_grad():
        steps, capped, _, _ = R.ladder(solve, 4, 1e-5, 1.2, 64)
    assert [int(s) for s in steps] == [28, 32, 41, 32] and int(capped.sum()) == 0, steps


@pytest.mark.gpu
def test_pilot_counts_are_the_inference_route_s(stress_sd):
    """decode(differentiable=True, frame_steps="pilot") on a uniform model: the counts are bit for bit those a cnf_steps="frame" model's
    inference decode chooses for the same (y, z); x is within the flat bound of that result; get_nfe() counts pilot + 4 max S_f; x has a
    grad_fn; last_frame_steps is set; and a cnf_steps="frame" model takes the keyword too."""
    from caspr_amd import ops
    z, y = _pilot_inputs()
    z, y = z.to("cuda:0"), y.to("cuda:0")
    mf = _model(stress_sd, 8, cnf_steps="frame", cnf_steps_points=64)
    with torch.no_grad():
        xi = mf.decode(z, 128, y=y)[2]
    want = mf.last_frame_steps[0].clone()
    m = _model(stress_sd, 8, cnf_steps_points=64)
    x = m.decode(z.clone().requires_grad_(True), 128, y=y, frame_steps="pilot", differentiable=True)[2]
    steps, order, info = m.last_frame_steps
    S = [int(s) for s in steps]
    REPORT["%s:pilot:steps" % TAG] = S
    assert len(set(S)) >= 2, "the pilot chose one count for every frame (%s): the test shows nothing" % S
    assert torch.equal(steps, want) and torch.equal(order, mf.last_frame_steps[1])
    assert int(m.get_nfe()[1]) == 4 * int(info["pilot_steps"].max()) + 4 * max(S)
    assert x.grad_fn is not None
    ck = _FChecks("pilot")
    ck.close("x_vs_inference", x, xi)
    xf = mf.decode(z.clone().requires_grad_(True), 128, y=y, frame_steps="pilot", differentiable=True)[2]
    assert xf.grad_fn is not None and torch.equal(xf.detach(), x.detach()) and torch.equal(mf.last_frame_steps[0], want)
    blk = m.point_cnf.chain[1]
    assert blk.frame_steps is None and blk.frame_order is None and blk._hyper is None and blk._count_evals and not blk._narrow
    ops.check_deferred_errors()
    ck.done()


@pytest.mark.gpu
def test_fit_latent_with_the_pilot(stress_sd, monkeypatch):
    """fit_latent(frame_steps="pilot", pilot_every=2), 3 iterations, B T = 2, n = 64: three finite losses, the pilot ran at iterations 0
    and 2 only, and z moved."""
    from caspr_amd import ops
    from caspr_amd.utils.fit import fit_latent
    m = _model(stress_sd, 8)
    z0 = rnd(9971, 1, 2, 1600).to("cuda:0")
    target = rnd(9972, 1, 2, 64, 3, scale=0.3).to("cuda:0")
    y = rnd(9973, 1, 2, 64, 3).to("cuda:0")
    calls, real = [], ops.cnf_frame_steps
    monkeypatch.setattr(ops, "cnf_frame_steps", lambda *a, **k: calls.append(1) or real(*a, **k))
    zf, losses = fit_latent(m, target, z0, 64, steps=3, lr=1e-2, y=y, frame_steps="pilot", pilot_every=2)
    assert len(losses) == 3 and all(np.isfinite(v) for v in losses), losses
    assert len(calls) == 2, "the pilot ran %d times" % len(calls)
    assert zf.shape == z0.shape and not torch.equal(zf, z0) and bool(torch.isfinite(zf).all())
    try:
        ops.check_deferred_errors()
    except ops.CasprAccuracyError:
        pass                                    # a capped frame of these random latents is not this test's subject


@pytest.mark.gpu
def test_frames_refusals(seeded_sd):
    """A dopri5 model refuses frame_steps; a table entry of 0 or above cnf_steps_max, a table of the wrong length or dtype and frame_steps
    without differentiable=True raise ValueError; a cnf_steps="frame" model without the keyword still refuses, naming it."""
    BT, n = 2, 64
    z, y = rnd(9981, 1, BT, 1600).to("cuda:0").requires_grad_(True), rnd(9982, 1, BT, n, 3).to("cuda:0")
    with pytest.raises(ValueError, match="dopri5"):
        _model(seeded_sd, 2, cnf_method="dopri5").decode(z, n, y=y, frame_steps=itab([2, 2]), differentiable=True)
    m = _model(seeded_sd, 2)
    with pytest.raises(ValueError, match="frame 1 "):
        m.decode(z, n, y=y, frame_steps=itab([2, 0]), differentiable=True)
    with pytest.raises(ValueError, match="frame 0 "):
        m.decode(z, n, y=y, frame_steps=itab([65, 2]), differentiable=True)
    for bad in (itab([2, 2, 2]), itab([2, 2]).long(), itab([2, 2]).cpu()):
        with pytest.raises(ValueError):
            m.decode(z, n, y=y, frame_steps=bad, differentiable=True)
    with pytest.raises(ValueError, match="differentiable=True"):
        m.decode(z, n, y=y, frame_steps=itab([2, 2]))
    with pytest.raises(ValueError, match="frame_steps"):
        _model(seeded_sd, 2, cnf_steps="frame").decode(z, n, y=y, differentiable=True)
    x = m.decode(z, n, y=y, frame_steps=itab([2, 1]), differentiable=True)[2]
    assert x.grad_fn is not None and [int(s) for s in m.last_frame_steps[0]] == [2, 1]
