"""decode(differentiable=True) / reconstruct(differentiable=True): the gradient through the point CNF's SAMPLING solve
(train/flow_grad.py: CnfSampleSolve, point_cnf_sample_train; csrc/ode_sample_tape.hip, csrc/backward_flow_value.hip).

Forward = caspr_cnf_sample_tape_f32: fixed-step RK4 from t_end down to 0 in one launch that writes every evaluation's (BT,n,3) stage
input and stage output.  Backward = a hand-written reverse sweep that rebuilds one evaluation at a time on value rows.  Checked here:

  CPU   the reverse sweep's RK4 algebra for the reversed time axis against f64 autograd through a plain reversed-time RK4, with the two
        HIP-backed pieces replaced by f64 torch restatements; the header / signature surface;
  GPU   the forward kernel against the oracle's RK4 in f64 (final state, every stored stage input / output, partial workgroups, frame
        invariance), decode's two routes against each other, every gradient against f64 oracle autograd, ragged frames against the
        same points embedded in whole workgroups, bit reproducibility, the tape's size, reconstruct end to end, the refusals.

Bounds: state-like values 1e-5 x (1 + |x|max) (the project's flat bound); gradients as tests/test_hip_train.py::
test_full_step_all_flow_parameters_vs_f64_oracle (loss 1e-5, rel L2 2e-4 per tensor; the f32 evaluation of the oracle's graph sits at
<= 9e-7 on these weights); ragged-frame equality 1e-6 rel L2 (the same kernels on the same values: only the association of the
per-frame sums differs, n x 2^-24 relative at most).
"""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_train import REPORT, rel, rnd

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
X_TOL = 1e-5
PRE = "point_cnf.chain.1"
NEW_ENTRIES = ("caspr_cnf_sample_tape_f32", "caspr_cnf_value_splits", "caspr_cnf_in_value_f32", "caspr_cnf_in_value_bwd_f32", "caspr_cnf_act_value_f32",
               "caspr_cnf_act_value_bwd_f32", "caspr_cnf_act_value_bwd_out_f32", "caspr_cnf_out_value_f32", "caspr_cnf_out_value_bwd_f32")


def _flush():
    rel("cnf_sample_grad_flush", torch.zeros(1), torch.zeros(1), 1.0)          # writes REPORT


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def _eval_f64(wb, t, y, G_lm, Bb_lm, tg_lm, tb_lm, BT, n, widths):
    """The ODE function without the Hutchinson term, as flow_grad._cnf_eval_value computes it, in plain torch: gated layers
    (W h + b) * sigmoid(G + t tg) + (Bb + t tb), softplus after all but the last."""
    from caspr_amd.train.flow_grad import _layer_views
    gates = _layer_views(torch.sigmoid(G_lm + t * tg_lm), BT, widths)
    betas = _layer_views(Bb_lm + t * tb_lm, BT, widths)
    hv = y
    for l in range(len(widths)):
        pre = F.linear(hv, wb[2 * l], wb[2 * l + 1]) * gates[l].unsqueeze(1) + betas[l].unsqueeze(1)
        hv = F.softplus(pre) if l + 1 < len(widths) else pre
    return hv


def _rk4_down(f, y, t_end, steps, record=None):
    """Classic RK4 from t_end down to 0: h = -t_end / steps, stage times t_end + (s + c_i) h."""
    h = -t_end / steps
    for s in range(steps):
        t = t_end + h * s
        ins = [y]
        k1 = f(t, y)
        ins.append(y + 0.5 * h * k1)
        k2 = f(t + 0.5 * h, ins[1])
        ins.append(y + 0.5 * h * k2)
        k3 = f(t + 0.5 * h, ins[2])
        ins.append(y + h * k3)
        k4 = f(t + h, ins[3])
        if record is not None:
            record.append((ins, (k1, k2, k3, k4)))
        y = y + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return y


def _tape_restatement(BT, n, widths):
    """caspr_cnf_sample_tape_f32 (train_ops.cnf_sample_tape) restated in plain torch for (BT, n, widths): _rk4_down of _eval_f64 that
    records every stage input and output.  Module level so that tools/flow_grad_diff.py can import it."""
    cols = np.cumsum((0,) + widths)

    def tape_restatement(y, hyper, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, t_end, steps):
        # hyper (BT, [gate l0..l3 | bias l0..l3]) and tcol as the kernel reads them -> back to layer-major
        nG = sum(widths)
        lm = lambda m: torch.cat([m[:, cols[l]:cols[l + 1]].reshape(-1) for l in range(4)])
        G, Bb = lm(hyper[:, :nG]), lm(hyper[:, nG:])
        tg, tb = lm(tcol[:nG].unsqueeze(0).expand(BT, -1)), lm(tcol[nG:].unsqueeze(0).expand(BT, -1))
        rec = []
        f = lambda t, y_: _eval_f64((w0, b0, w1x, b1, w2x, b2, w3, b3), t, y_, G, Bb, tg, tb, BT, n, widths)
        x0 = _rk4_down(f, y, t_end.reshape(()), steps, rec)
        return x0, torch.stack([torch.stack(ins) for ins, _ in rec]), torch.stack([torch.stack(ks) for _, ks in rec])
    return tape_restatement


def test_reverse_sweep_algebra_vs_f64_autograd(monkeypatch):
    """CnfSampleSolve with caspr_cnf_sample_tape_f32 and the per-evaluation rebuild replaced by f64 torch restatements: what is left is
    the node's own arithmetic -- the hyper / tcol assembly for the kernel, the RK4 reverse algebra on the reversed time axis, the
    accumulation.  Every gradient (y, the four layer-major hyper tensors, t_end, all weights and biases) against autograd through a
    plain reversed-time RK4 of the same function at 1e-9: a wrong sign of h, a dropped start-time or stage-time term of dL/dt_end or a
    stage input read from the wrong slot are errors of order one here."""
    from caspr_amd.train import flow_grad as FG
    BT, n, S = 2, 5, 3
    widths = (7, 6, 5, 3)
    cin = (3, 7, 6, 5)
    gen = torch.Generator().manual_seed(11)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=gen, dtype=torch.float64) * scale)
    wb = [t_ for l in range(4) for t_ in (r(widths[l], cin[l], scale=0.7), r(widths[l], scale=0.3))]
    tot = BT * sum(widths)
    leaves = {"y": r(BT, n, 3), "G_lm": r(tot), "Bb_lm": r(tot, scale=0.5), "tg": r(sum(widths)), "tb": r(sum(widths)), "t_end": r(()).abs() + 0.7}
    for i, t_ in enumerate(wb):
        leaves["wb%d" % i] = t_
    for t_ in leaves.values():
        t_.requires_grad_(True)
    wbl = [leaves["wb%d" % i] for i in range(8)]
    # the time columns are one row per layer, repeated over the frames (_hyper_layer_major builds them so; the kernel reads one row)
    cols = np.cumsum((0,) + widths)
    over_frames = lambda v: torch.cat([v[cols[l]:cols[l + 1]].unsqueeze(0).expand(BT, -1).reshape(-1) for l in range(4)])
    L = dict(leaves, tg_lm=over_frames(leaves["tg"]), tb_lm=over_frames(leaves["tb"]))
    wy = r(BT, n, 3)

    monkeypatch.setattr(FG.T, "cnf_sample_tape", _tape_restatement(BT, n, widths))
    monkeypatch.setattr(FG, "_cnf_eval_value", _eval_f64)
    x = FG.CnfSampleSolve.apply(L["y"], L["G_lm"], L["Bb_lm"], L["tg_lm"], L["tb_lm"], L["t_end"], wbl[2], wbl[4], S, widths, *wbl)
    got = torch.autograd.grad((x * wy).sum(), list(leaves.values()))
    f = lambda t, y_: _eval_f64(wbl, t, y_, L["G_lm"], L["Bb_lm"], over_frames(leaves["tg"]), over_frames(leaves["tb"]), BT, n, widths)
    x2 = _rk4_down(f, L["y"], L["t_end"], S)
    want = torch.autograd.grad((x2 * wy).sum(), list(leaves.values()))
    assert torch.allclose(x, x2, rtol=0, atol=1e-12)
    bad = []
    for name, g, w in zip(leaves, got, want):
        err = float((g - w).abs().max() / w.abs().max().clamp_min(1e-30))
        if not err <= 1e-9:
            bad.append("%s: %.3e" % (name, err))
    assert not bad, "\n".join(bad)


def test_new_entries_are_declared_bound_and_built():
    """The new C entries appear in include/caspr_hip_train.h and lib.SIGNATURES with the argument counts of their declarations
    (tests/test_host_cpu.py::test_library_exports_every_declared_symbol then holds the library to them), the two new sources are
    registered with the build -- the tape kernel with the unroll flag of the kernel it was copied from -- and the public keyword exists."""
    import inspect
    from caspr_amd import lib
    from caspr_amd import train_ops as T
    from caspr_amd.csrc import build
    from caspr_amd.models import CaSPR
    from caspr_amd.train import flow_grad as FG
    hdr = open(os.path.join(ROOT, "include", "caspr_hip_train.h")).read()
    for name in NEW_ENTRIES:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, "%s is not declared in include/caspr_hip_train.h" % name
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
    assert len(lib.SIGNATURES["caspr_cnf_sample_tape_f32"][1]) == 21
    assert "ode_sample_tape.hip" in build.SOURCES and "backward_flow_value.hip" in build.SOURCES
    assert build.EXTRA["ode_sample_tape.hip"] == build.EXTRA["ode_train_fwd.hip"]
    assert "cnf.py:70-128" in hdr and "caspr.py:262" in hdr
    for fn in ("cnf_sample_tape", "cnf_in_value", "cnf_in_value_bwd", "cnf_act_value", "cnf_act_value_bwd", "cnf_out_value", "cnf_out_value_bwd"):
        assert callable(getattr(T, fn)), fn
    assert all(hasattr(FG, nm) for nm in ("CnfSampleSolve", "point_cnf_sample_train", "_hyper_layer_major"))
    for meth in (CaSPR.decode, CaSPR.reconstruct):
        p = list(inspect.signature(meth).parameters.values())[-1]
        assert p.name == "differentiable" and p.default is False, meth


def test_differentiable_refuses_the_cpu_and_no_grad():
    """No silent fallback: CPU tensors and grad mode off are refused with the reason."""
    from caspr_amd.models import CaSPR
    m = CaSPR()
    z, y = torch.zeros(1, 1, 1600), torch.zeros(1, 1, 8, 3)
    with pytest.raises(ValueError, match="GPU"):
        m.decode(z, 8, y=y, differentiable=True)
    with torch.no_grad(), pytest.raises(ValueError, match="no_grad"):
        m.decode(z, 8, y=y, differentiable=True)


# ---------------------------------------------------------------------------------------------
# GPU 1: the forward kernel against the oracle's RK4 in f64
# ---------------------------------------------------------------------------------------------
class _Checks:
    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def close(self, name, got, want):
        """|d| <= 1e-5 (1 + |want|max)."""
        got, want = got.detach().cpu().double(), want.detach().cpu().double()
        assert got.shape == want.shape, (name, got.shape, want.shape)
        m = float(want.abs().max())
        bound = X_TOL * (1.0 + m)
        err = float((got - want).abs().max())
        REPORT["cnf_sample_grad:%s:%s" % (self.tag, name)] = {"max_abs_err": err, "bound": bound, "ref_absmax": m}
        if not (bool(torch.isfinite(got).all()) and err <= bound):
            self.bad.append("%s: max abs err %.3e > %.3e" % (name, err, bound))

    def done(self):
        _flush()
        assert not self.bad, self.tag + "\n" + "\n".join(self.bad)


def _launch(W, y, hyper, steps):
    from caspr_amd import train_ops as T
    g = lambda v: v.to("cuda:0").contiguous()
    D = W.dev
    t_end = torch.tensor([W.t_end], device="cuda:0", dtype=torch.float32)
    out = T.cnf_sample_tape(g(y), g(hyper), D["tcol"], D["w0"], D["b0"], W.w1x, D["b1"], W.w2x, D["b2"], D["w3"], D["b3"], t_end, steps)
    torch.cuda.synchronize()
    return out


# (BT, n, S, weights): one workgroup; several frames and steps; two workgroups per frame; a partial workgroup; fewer points than a wave owns
CASES = [(1, 64, 1, "seeded"), (3, 64, 4, "stress"), (2, 128, 2, "seeded"), (2, 100, 2, "stress"), (2, 8, 3, "seeded")]
CASE_IDS = ["bt%d-n%d-s%d-%s" % c for c in CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("BT,n,S,which", CASES, ids=CASE_IDS)
def test_forward_kernel_vs_f64_oracle(BT, n, S, which, seeded_sd, stress_sd):
    """x(0) against oracle.cnf_block (reverse, RK4, f64); ys[0,0] is the input bit for bit; every stored stage input and stage output
    against the oracle's RK4 step replayed in f64 from the state the kernel stored at that step's beginning; a frame launched alone
    gives the bits it gives inside the batch."""
    from oracle import model as O
    from test_cnf_solve_kernels import Weights, base_samples
    sd32 = seeded_sd if which == "seeded" else stress_sd
    sd = {k: v.double() for k, v in sd32.items()}
    W = Weights(sd32, torch.device("cuda:0"))
    seed = 9000 + 13 * BT + n + S
    c, y = rnd(seed, BT, 1600), base_samples(seed + 1, BT, n)
    hyper = W.hyper(c, 3078)
    gx, ys, ka = _launch(W, y, hyper, S)
    assert gx.shape == (BT, n, 3) and ys.shape == (S, 4, BT, n, 3) and ka.shape == (S, 4, BT, n, 3)
    ck = _Checks("fwd:bt%d-n%d-s%d-%s" % (BT, n, S, which))
    wx, _ = O.cnf_block(sd, PRE, y.double(), c.double(), None, True, "rk4", S, None)
    ck.close("x_0", gx, wx)
    assert torch.equal(ys[0, 0].cpu(), y), "the first stage input is the block's input"
    t_end = float(sd[PRE + ".sqrt_end_time"]) ** 2
    h = -t_end / S
    ys64 = ys.cpu().double()
    f = lambda t, y_: O.odefunc(sd, PRE + ".odefunc", t, y_, c.double())[0]
    for s in range(S):
        rec = []
        # one RK4 step of the oracle's function from the STORED state, on the reversed time axis (t_end + s h downwards)
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


def _one_step(f, y, t, h, record):
    """One classic RK4 step of size h (any sign) from (t, y); records (stage inputs, stage outputs)."""
    ins = [y]
    k1 = f(t, y)
    ins.append(y + 0.5 * h * k1)
    k2 = f(t + 0.5 * h, ins[1])
    ins.append(y + 0.5 * h * k2)
    k3 = f(t + 0.5 * h, ins[2])
    ins.append(y + h * k3)
    k4 = f(t + h, ins[3])
    record.append((ins, (k1, k2, k3, k4)))
    return y + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)


# ---------------------------------------------------------------------------------------------
# GPU 2-8: the model surface
# ---------------------------------------------------------------------------------------------
def _model(sd, steps, blocks=1, latent_steps=2, **kw):
    from caspr_amd.models import CaSPR
    m = CaSPR(cnf_rk4_steps=steps, latent_rk4_steps=latent_steps, cnf_blocks=blocks, check_tol=None, **kw)
    m.load_state_dict(sd)
    return m.to("cuda:0").eval()


def _two_block_sd(sd):
    """The checkpoint surface of a two-block flow [MBN, CNF, CNF, MBN] from a one-block state dict: the second block is the first with
    every tensor scaled a little (different dynamics, same conditioning), the closing MovingBatchNorm moves to chain.3."""
    out = {k: v.clone() for k, v in sd.items() if not k.startswith("point_cnf.chain.2.")}
    for k, v in sd.items():
        if k.startswith("point_cnf.chain.1."):
            out[k.replace("chain.1.", "chain.2.")] = (v * 0.9).clone() if v.is_floating_point() and not k.endswith("_num_evals") else v.clone()
        elif k.startswith("point_cnf.chain.2."):
            out[k.replace("chain.2.", "chain.3.")] = v.clone()
    return out


def _sd_for(which, blocks, seeded_sd, stress_sd):
    sd = seeded_sd if which == "seeded" else stress_sd
    return _two_block_sd(sd) if blocks == 2 else sd


_SKIP = ("running_mean", "running_var", "step", "_num_evals")


def _sd64(sd):
    return {k: (v.detach().clone().double().requires_grad_(True) if v.is_floating_point() and not k.endswith(_SKIP) else
                (v.double() if v.is_floating_point() else v)) for k, v in sd.items()}


def _decode_grads(m, z, y, w, n):
    """decode(differentiable=True) forward + backward of sum(w * x) -> (x, loss, dL/dy, dL/dz, {parameter name: gradient})."""
    m.zero_grad()
    zd = z.to("cuda:0").requires_grad_(True)
    yd = y.to("cuda:0").requires_grad_(True)
    x = m.decode(zd, n, y=yd, differentiable=True)[2]
    loss = (x * w.to("cuda:0")).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters() if k.startswith("point_cnf.")}
    return x.detach(), loss.detach(), yd.grad.detach().clone(), zd.grad.detach().clone(), grads


@pytest.mark.gpu
def test_decode_routes_agree_and_count_evaluations(stress_sd):
    """decode(differentiable=True)'s x against the default decode()'s (the 128-point inference kernel, MovingBatchNorm fused into it)
    within the flat bound; get_nfe() reports 4 S; the result carries a grad_fn, the default's does not."""
    BT, n, S = 3, 100, 4
    m = _model(stress_sd, S)
    z, y = rnd(31, 1, BT, 1600).to("cuda:0"), rnd(32, 1, BT, n, 3).to("cuda:0")
    xd = m.decode(z, n, y=y, differentiable=True)[2]
    assert m.get_nfe()[1] == 4 * S and xd.grad_fn is not None
    x0 = m.decode(z, n, y=y)[2]
    assert x0.grad_fn is None and not x0.requires_grad
    ck = _Checks("decode_routes")
    ck.close("x", xd, x0)
    ck.done()


GRAD_CASES = [c + (1,) for c in CASES] + [(3, 64, 2, "seeded", 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("BT,n,S,which,blocks", GRAD_CASES, ids=["bt%d-n%d-s%d-%s-b%d" % c for c in GRAD_CASES])
def test_gradients_vs_f64_oracle_autograd(BT, n, S, which, blocks, seeded_sd, stress_sd, monkeypatch):
    """Loss sum(w * x) through the whole reversed flow (MBN, CNF x blocks, MBN): the loss at 1e-5 relative, dL/dy, dL/dz and EVERY
    point_cnf parameter (sqrt_end_time and both MovingBatchNorms' weight / bias included; none may be missing) at rel L2 <= 2e-4 against
    autograd through oracle.point_cnf in f64."""
    from oracle import model as O
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
    tag = "grad:bt%d-n%d-s%d-%s-b%d" % (BT, n, S, which, blocks)
    bad = []

    def l2(name, got, want):
        err = float((got.cpu().double() - want).norm() / want.norm().clamp_min(1e-12))
        REPORT["cnf_sample_grad:%s:%s" % (tag, name)] = {"rel_l2": err, "ref_l2": float(want.norm())}
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
    REPORT["cnf_sample_grad:%s:loss" % tag] = {"rel_err": lerr, "loss": float(loss6.detach())}
    _flush()
    assert lerr <= 1e-5, "loss %.9g vs %.9g" % (float(loss), float(loss6.detach()))
    assert not bad, tag + "\n" + "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("n,full", [(100, 128), (8, 64)])
def test_ragged_frames_equal_the_same_points_in_whole_workgroups(n, full, stress_sd):
    """What a partial workgroup's clamped columns compute reaches no sum: the gradient of every parameter (and dL/dz, dL/dy) for n points
    equals, at rel L2 <= 1e-6, the gradient of a call with `full` points whose extra points carry zero weight in the loss."""
    BT, S = 2, 2
    m = _model(stress_sd, S)
    z, yf, wf = rnd(41, 1, BT, 1600), rnd(42, 1, BT, full, 3, scale=1.3), rnd(43, 1, BT, full, 3)
    wf[:, :, n:] = 0.0
    _, _, gy_a, gz_a, ga = _decode_grads(m, z, yf[:, :, :n].contiguous(), wf[:, :, :n].contiguous(), n)
    _, _, gy_b, gz_b, gb = _decode_grads(m, z, yf, wf, full)
    bad = []

    def same(name, u, v):
        err = float((u.double() - v.double()).norm() / v.double().norm().clamp_min(1e-30))
        REPORT["cnf_sample_grad:ragged-n%d:%s" % (n, name)] = {"rel_l2": err}
        if not err <= 1e-6:
            bad.append("%s: rel L2 %.3e" % (name, err))
    same("dL/dy", gy_a, gy_b[:, :, :n])
    assert float(gy_b[:, :, n:].abs().max()) == 0.0, "a point without weight in the loss has a gradient"
    same("dL/dz", gz_a, gz_b)
    for k in ga:
        assert ga[k] is not None and gb[k] is not None, k
        same(k, ga[k], gb[k])
    _flush()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_forward_and_backward_are_bit_reproducible(stress_sd):
    """Two forward + backward runs of case (3, 64, 4, stress): identical bits in the output and in every gradient (the reverse sweep and
    every per-frame sum run in a fixed order, no atomics)."""
    BT, n, S = 3, 64, 4
    m = _model(stress_sd, S)
    z, y, w = rnd(51, 1, BT, 1600), rnd(52, 1, BT, n, 3), rnd(53, 1, BT, n, 3)
    xa, la, gya, gza, ga = _decode_grads(m, z, y, w, n)
    xb, lb, gyb, gzb, gb = _decode_grads(m, z, y, w, n)
    assert torch.equal(xa, xb) and torch.equal(la, lb) and torch.equal(gya, gyb) and torch.equal(gza, gzb)
    diff = [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert not diff, "gradients differ between two identical runs: %s" % diff[:5]


@pytest.mark.gpu
def test_tape_is_point_sized(seeded_sd):
    """What CnfSampleSolve saves for its backward: the stage inputs and outputs, S * 4 * BT * n * 24 bytes, plus the four layer-major
    hyper tensors and t_end it already holds -- and nothing with a 512-wide dimension (no layer product, no activation)."""
    from caspr_amd.train import flow_grad as FG
    BT, n, S = 2, 128, 3
    m = _model(seeded_sd, S)
    block = m.point_cnf.chain[1]
    y = rnd(61, BT, n, 3).to("cuda:0").requires_grad_(True)
    c = rnd(62, BT, 1600).to("cuda:0")
    saved = []
    t_end = (block.sqrt_end_time ** 2).detach()
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        G_lm, Bb_lm, tg_lm, tb_lm, widths = FG._hyper_layer_major(block, c)
        before = len(saved)
        wb = [p_ for l in block.odefunc.diffeq.layers for p_ in (l._layer.weight, l._layer.bias)]
        w1x, w2x = block._weights_x6()
        x = FG.CnfSampleSolve.apply(y, G_lm, Bb_lm, tg_lm, tb_lm, t_end, w1x, w2x, S, widths, *wb)
    mine = saved[before:]
    hyper_bytes = 4 * BT * (3 * 512 + 3) * 4 + 4
    total = sum(t.numel() * t.element_size() for t in mine)
    REPORT["cnf_sample_grad:tape_bytes"] = {"saved": total, "tape": S * 4 * BT * n * 24, "hyper_and_t_end": hyper_bytes}
    _flush()
    assert total == S * 4 * BT * n * 24 + hyper_bytes, (total, [tuple(t.shape) for t in mine])
    assert not [tuple(t.shape) for t in mine if 512 in t.shape], "a 512-wide tensor is kept for the backward pass"
    x.sum().backward()
    assert y.grad is not None


@pytest.mark.gpu
def test_reconstruct_end_to_end_vs_f64_oracle(golden, seeded_sd, monkeypatch):
    """reconstruct(differentiable=True) on the golden training batch, loss = sum(w * x_out) + mean |tnocs|, against oracle.reconstruct in
    f64 with its differentiable mode on: the loss at 1e-5, every latent-ODE / CNF / MovingBatchNorm parameter at rel L2 <= 2e-4 (the
    encoder's are skipped as tests/test_hip_train.py::test_full_step_all_flow_parameters_vs_f64_oracle skips them, but must be there
    and finite); the returned x equals the default reconstruct()'s within the flat bound."""
    from oracle import model as O
    S, LS, n = 8, 4, 64
    x_in = torch.from_numpy(golden["train_x"])
    B, Tt = x_in.shape[:2]
    y, w = rnd(71, B, Tt, n, 3), rnd(72, B, Tt, n, 3)
    monkeypatch.setattr(O, "GRAD_MODE", True)
    sd6 = _sd64(seeded_sd)
    _, _, x6, t6 = O.reconstruct(sd6, x_in.double(), y.double(), cnf_steps=S, latent_steps=LS)
    loss6 = (x6 * w.double()).sum() + t6.abs().mean()
    loss6.backward()
    m = _model(seeded_sd, S, latent_steps=LS)
    xd = x_in.to("cuda:0")
    _, _, xo, tn = m.reconstruct(xd, num_points=n, y=y.to("cuda:0"), differentiable=True)
    loss = (xo * w.to("cuda:0")).sum() + tn.abs().mean()
    loss.backward()
    torch.cuda.synchronize()
    rel("sample_e2e_loss", loss.detach().reshape(1), loss6.detach().reshape(1), 1e-5)
    cnt, bad = 0, []
    for name, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        if name.startswith("encoder."):
            continue
        want = sd6[name.replace("latent_ode.solver.ode_func", "latent_ode.ode_func")].grad
        assert want is not None, name
        err = float((p.grad.detach().cpu().double() - want).norm() / want.norm().clamp_min(1e-12))
        REPORT["sample_e2e_grad_l2:" + name] = {"rel_l2": err, "ref_l2": float(want.norm())}
        cnt += 1
        if not err <= 2e-4:
            bad.append("%s: rel L2 %.3e" % (name, err))
    with torch.no_grad():
        x_plain = m.reconstruct(xd, num_points=n, y=y.to("cuda:0"))[2]
    ck = _Checks("e2e")
    ck.close("x_vs_default_reconstruct", xo, x_plain)
    ck.done()
    assert cnt >= 30, cnt
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_refusals_and_the_default_is_untouched(seeded_sd, monkeypatch):
    """differentiable=True under no_grad, with cnf_method="dopri5", with cnf_steps="frame" and with the bf16x6 CNF kernels switched off
    each raise ValueError; decode() without the keyword returns the bits of the inference call it has always made."""
    from caspr_amd import ops
    BT, n = 2, 128
    z, y = rnd(81, 1, BT, 1600).to("cuda:0"), rnd(82, 1, BT, n, 3).to("cuda:0")
    m = _model(seeded_sd, 2)
    with torch.no_grad(), pytest.raises(ValueError, match="no_grad"):
        m.decode(z, n, y=y, differentiable=True)
    with pytest.raises(ValueError, match="dopri5"):
        _model(seeded_sd, 2, cnf_method="dopri5").decode(z, n, y=y, differentiable=True)
    with pytest.raises(ValueError, match="frame"):
        _model(seeded_sd, 2, cnf_steps="frame").decode(z, n, y=y, differentiable=True)
    with monkeypatch.context() as mp, pytest.raises(ValueError, match="CNF_BF16X6"):
        mp.setattr(ops, "CNF_BF16X6", False)
        m.decode(z, n, y=y, differentiable=True)
    with torch.no_grad():
        got = m.decode(z, n, y=y)[2]
        want = m.point_cnf(y[0], z[0], reverse=True)
    assert torch.equal(got[0], want)
    got_g = m.decode(z, n, y=y)[2]                     # grad mode on, keyword left at its default: the same launch, detached
    assert torch.equal(got_g[0], want) and got_g.grad_fn is None
