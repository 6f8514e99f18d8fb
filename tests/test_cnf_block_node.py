"""config.train_cnf_block_node: a point-CNF block trained as ONE autograd node (train/flow_grad.py: CnfBlockSolve).

Forward = caspr_cnf_train_fwd_f32 (csrc/ode_train_fwd.hip): the fixed-step RK4 solve with the Hutchinson divergence in one launch that
writes the (BT,n,3) point state of every evaluation and no layer product.  Backward = a hand-written reverse sweep that rebuilds one
evaluation's tape at a time.  Checked here:

  CPU   the reverse sweep's RK4 algebra (stage cotangents, dL/dt_end through the step size AND the stage times, the order of the stored
        stage inputs) against f64 autograd through a plain RK4, with the two HIP entry points replaced by f64 torch restatements;
  GPU   the forward kernel against the oracle's RK4 in f64 (final state, every stored stage input / output, frame invariance), the
        full training step's gradients against the f64 oracle, peak memory against the taped and the checkpointed routes, bit
        reproducibility, the option switched off, an ineligible shape, sharding.

Bounds: state-like values 1e-5 x (1 + |x|max) (the project's flat bound), log-density-like values 1e-4 x max(1, |logp|max) (the RK4 logp
bound of tests/test_cnf_solve_kernels.py), gradients as tests/test_hip_train.py::test_full_step_all_flow_parameters_vs_f64_oracle
(loss 1e-5, rel L2 2e-4 per tensor).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_train import REPORT, rel, rnd

X_TOL, LP_TOL = 1e-5, 1e-4
PRE = "point_cnf.chain.1"


# ---------------------------------------------------------------------------------------------
# CPU: the reverse sweep's algebra
# ---------------------------------------------------------------------------------------------
def _eval_f64(wb, t, y, G_lm, Bb_lm, tg_lm, tb_lm, e_rows, BT, n, widths):
    """The ODE function with its Hutchinson term, as flow_grad._cnf_eval_fused computes it, in plain torch: gated layers
    (W h + b) * sigmoid(G + t tg) + (Bb + t tb), softplus after all but the last, the tangent J e carried in forward mode."""
    from caspr_amd.train.flow_grad import _layer_views
    gates = _layer_views(torch.sigmoid(G_lm + t * tg_lm), BT, widths)
    betas = _layer_views(Bb_lm + t * tb_lm, BT, widths)
    hv, ht = y, e_rows.reshape(BT, n, 3)
    for l in range(len(widths)):
        w, b = wb[2 * l], wb[2 * l + 1]
        g, be = gates[l].unsqueeze(1), betas[l].unsqueeze(1)
        pre, lin_t = F.linear(hv, w, b) * g + be, F.linear(ht, w) * g
        if l + 1 < len(widths):
            hv, ht = F.softplus(pre), torch.sigmoid(pre) * lin_t
        else:
            hv, ht = pre, lin_t
    return hv, -(ht * e_rows.reshape(BT, n, 3)).sum(-1, keepdim=True)


def _rk4(f, y, lp, h, steps, record=None):
    for s in range(steps):
        t = h * s
        ins = [y]
        k1 = f(t, y)
        ins.append(y + 0.5 * h * k1[0])
        k2 = f(t + 0.5 * h, ins[1])
        ins.append(y + 0.5 * h * k2[0])
        k3 = f(t + 0.5 * h, ins[2])
        ins.append(y + h * k3[0])
        k4 = f(t + h, ins[3])
        if record is not None:
            record.append((ins, (k1, k2, k3, k4)))
        y = y + (h / 6.0) * (k1[0] + 2.0 * k2[0] + 2.0 * k3[0] + k4[0])
        lp = lp + (h / 6.0) * (k1[1] + 2.0 * k2[1] + 2.0 * k3[1] + k4[1])
    return y, lp


def _fwd_restatement(BT, n, widths):
    """caspr_cnf_train_fwd_f32 (train_ops.cnf_train_fwd) restated in plain torch for (BT, n, widths): a plain RK4 of _eval_f64 that
    records every stage input and output.  Module level so that tools/flow_grad_diff.py can import it."""
    cols = np.cumsum((0,) + widths)

    def fwd_restatement(y, logp, e_, hyper, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, t_end, steps):
        # hyper (BT, [gate l0..l3 | bias l0..l3]) and tcol as the kernel reads them -> back to layer-major
        nG = sum(widths)
        lm = lambda m: torch.cat([m[:, cols[l]:cols[l + 1]].reshape(-1) for l in range(4)])
        G, Bb = lm(hyper[:, :nG]), lm(hyper[:, nG:])
        tg, tb = lm(tcol[:nG].unsqueeze(0).expand(BT, -1)), lm(tcol[nG:].unsqueeze(0).expand(BT, -1))
        rec = []
        f = lambda t, y_: _eval_f64((w0, b0, w1x, b1, w2x, b2, w3, b3), t, y_, G, Bb, tg, tb, e_.reshape(-1, 3), BT, n, widths)
        yT, lpT = _rk4(f, y, logp, t_end.reshape(()) / steps, steps, rec)
        ys = torch.stack([torch.stack(ins) for ins, _ in rec])
        ka = torch.stack([torch.stack([k[0] for k in ks]) for _, ks in rec])
        knd = torch.stack([torch.stack([k[1] for k in ks]) for _, ks in rec])
        return yT, lpT, ys, ka, knd
    return fwd_restatement


def test_reverse_sweep_algebra_vs_f64_autograd(monkeypatch):
    """CnfBlockSolve with caspr_cnf_train_fwd_f32 and the per-evaluation training kernels replaced by f64 torch restatements: what is
    left is the node's own arithmetic -- the hyper / tcol assembly for the kernel, the RK4 reverse algebra, the accumulation.  Every
    gradient (x, logpx, the four layer-major hyper tensors, t_end, all weights and biases) against autograd through a plain RK4 of the
    same function at 1e-9: a wrong factor on a stage cotangent, a dropped stage-time term of dL/dt_end or a stage input read from the
    wrong slot are errors of order one here."""
    from caspr_amd.train import flow_grad as FG
    BT, n, S = 2, 5, 3
    widths = (7, 6, 5, 3)
    cin = (3, 7, 6, 5)
    gen = torch.Generator().manual_seed(5)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=gen, dtype=torch.float64) * scale)
    wb = [t_ for l in range(4) for t_ in (r(widths[l], cin[l], scale=0.7), r(widths[l], scale=0.3))]
    tot = BT * sum(widths)
    leaves = {"x": r(BT, n, 3), "logpx": r(BT, n, 1), "G_lm": r(tot), "Bb_lm": r(tot, scale=0.5), "tg": r(sum(widths)), "tb": r(sum(widths)),
              "t_end": r(()).abs() + 0.7}
    for i, t_ in enumerate(wb):
        leaves["wb%d" % i] = t_
    for t_ in leaves.values():
        t_.requires_grad_(True)
    wbl = [leaves["wb%d" % i] for i in range(8)]
    # the time columns are one row per layer, repeated over the frames (cnf_block_train builds them so; the kernel reads one row)
    cols = np.cumsum((0,) + widths)
    over_frames = lambda v: torch.cat([v[cols[l]:cols[l + 1]].unsqueeze(0).expand(BT, -1).reshape(-1) for l in range(4)])
    leaves_lm = dict(leaves, tg_lm=over_frames(leaves["tg"]), tb_lm=over_frames(leaves["tb"]))
    e = r(BT, n, 3)
    wy, wl = r(BT, n, 3), r(BT, n, 1)

    monkeypatch.setattr(FG.T, "cnf_train_fwd", _fwd_restatement(BT, n, widths))
    monkeypatch.setattr(FG, "_cnf_eval_fused", _eval_f64)
    L = leaves_lm
    y, lp = FG.CnfBlockSolve.apply(L["x"], L["logpx"], L["G_lm"], L["Bb_lm"], L["tg_lm"], L["tb_lm"], L["t_end"], e, wbl[2], wbl[4], S, widths, *wbl)
    got = torch.autograd.grad((y * wy).sum() + (lp * wl).sum(), list(leaves.values()))
    f = lambda t, y_: _eval_f64(wbl, t, y_, L["G_lm"], L["Bb_lm"], over_frames(leaves["tg"]), over_frames(leaves["tb"]), e.reshape(-1, 3), BT, n, widths)
    y2, lp2 = _rk4(f, L["x"], L["logpx"], L["t_end"] / S, S)
    want = torch.autograd.grad((y2 * wy).sum() + (lp2 * wl).sum(), list(leaves.values()))
    assert torch.allclose(y, y2, rtol=0, atol=1e-12) and torch.allclose(lp, lp2, rtol=0, atol=1e-12)
    bad = []
    for name, g, w in zip(leaves, got, want):
        err = float((g - w).abs().max() / w.abs().max().clamp_min(1e-30))
        if not err <= 1e-9:
            bad.append("%s: %.3e" % (name, err))
    assert not bad, "\n".join(bad)


def test_option_is_off_by_default_and_read_from_the_environment_only_under_debug():
    from caspr_amd import config as C
    from caspr_amd.train import flow_grad as FG
    assert C.KernelConfig().train_cnf_block_node is False
    with pytest.warns(RuntimeWarning):
        assert C.load({"CASPR_CNF_BLOCK_NODE": "1"}).train_cnf_block_node is False
    assert C.load({"CASPR_CNF_BLOCK_NODE": "1", "CASPR_DEBUG": "1"}).train_cnf_block_node is True
    assert FG.BLOCK_NODE == C.config.train_cnf_block_node


# ---------------------------------------------------------------------------------------------
# GPU 1: the forward kernel against the oracle's RK4 in f64
# ---------------------------------------------------------------------------------------------
class _Checks:
    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def close(self, name, got, want, kind):
        """kind "x": |d| <= 1e-5 (1 + |want|max); kind "lp": |d| <= 1e-4 max(1, |want|max)."""
        got, want = got.detach().cpu().double(), want.detach().cpu().double()
        assert got.shape == want.shape, (name, got.shape, want.shape)
        m = float(want.abs().max())
        bound = X_TOL * (1.0 + m) if kind == "x" else LP_TOL * max(1.0, m)
        err = float((got - want).abs().max())
        REPORT["cnf_block_node:%s:%s" % (self.tag, name)] = {"max_abs_err": err, "bound": bound, "ref_absmax": m}
        if not (bool(torch.isfinite(got).all()) and err <= bound):
            self.bad.append("%s: max abs err %.3e > %.3e" % (name, err, bound))

    def done(self):
        rel("cnf_block_node_flush", torch.zeros(1), torch.zeros(1), 1.0)       # writes REPORT
        assert not self.bad, self.tag + "\n" + "\n".join(self.bad)


def _launch(W, y, lp0, e, hyper, steps):
    from caspr_amd import train_ops as T
    g = lambda v: v.to("cuda:0").contiguous()
    D = W.dev
    t_end = torch.tensor([W.t_end], device="cuda:0", dtype=torch.float32)
    out = T.cnf_train_fwd(g(y), g(lp0), g(e), g(hyper), D["tcol"], D["w0"], D["b0"], W.w1x, D["b1"], W.w2x, D["b2"], D["w3"], D["b3"], t_end, steps)
    torch.cuda.synchronize()
    return out


FWD_CASES = [(1, 64, 1, "seeded"), (3, 1024, 4, "stress"), (20, 64, 8, "stress"), (20, 1024, 1, "seeded"), (1, 1024, 8, "stress"), (3, 64, 4, "seeded"),
             (3, 64, 8, "seeded"), (1, 64, 4, "stress")]


@pytest.mark.gpu
@pytest.mark.parametrize("BT,n,S,which", FWD_CASES, ids=["bt%d-n%d-s%d-%s" % c for c in FWD_CASES])
def test_forward_kernel_vs_f64_oracle(BT, n, S, which, seeded_sd, stress_sd):
    """(x_T, logp_T) against oracle.cnf_block (RK4, f64, same e); every stored stage input and stage output against the oracle's
    RK4 step replayed in f64 from the state the kernel stored at that step's beginning."""
    from oracle import model as O
    from test_cnf_solve_kernels import Weights, base_samples
    sd = {k: v.double() for k, v in (seeded_sd if which == "seeded" else stress_sd).items()}
    W = Weights(seeded_sd if which == "seeded" else stress_sd, torch.device("cuda:0"))
    seed = 7000 + 13 * BT + n + S
    c, y = rnd(seed, BT, 1600), base_samples(seed + 1, BT, n)
    e, lp0 = rnd(seed + 2, BT, n, 3), rnd(seed + 3, BT, n, 1)
    gx, glp, ys, ka, knd = _launch(W, y, lp0, e, W.hyper(c, 3078), S)
    assert ys.shape == (S, 4, BT, n, 3) and ka.shape == (S, 4, BT, n, 3) and knd.shape == (S, 4, BT, n, 1)
    ck = _Checks("fwd:bt%d-n%d-s%d-%s" % (BT, n, S, which))
    wx, wlp = O.cnf_block(sd, PRE, y.double(), c.double(), lp0.double(), False, "rk4", S, e.double())
    ck.close("x_T", gx, wx, "x")
    ck.close("logp_T", glp, wlp, "lp")
    assert torch.equal(ys[0, 0].cpu(), y), "the first stage input is the block's input"
    h = float(sd[PRE + ".sqrt_end_time"]) ** 2 / S
    ys64 = ys.cpu().double()
    for s in range(S):
        rec = []
        f = lambda t, y_: O.odefunc(sd, PRE + ".odefunc", t, y_, c.double(), e.double())
        # one RK4 step of the oracle's function from the STORED state (time offset s h: the gates move in time)
        y1, _ = _rk4(lambda t, y_: f(s * h + t, y_), ys64[s, 0], torch.zeros(BT, n, 1, dtype=torch.float64), h, 1, rec)
        ins, ks = rec[0]
        for st in range(4):
            if st > 0:
                ck.close("step%d:stage_in%d" % (s, st + 1), ys[s, st], ins[st], "x")
            ck.close("step%d:a%d" % (s, st + 1), ka[s, st], ks[st][0], "x")
            ck.close("step%d:nd%d" % (s, st + 1), knd[s, st], ks[st][1], "lp")
        ck.close("step%d:next_state" % s, ys[s + 1, 0] if s + 1 < S else gx, y1, "x")
    ck.done()


@pytest.mark.gpu
def test_forward_kernel_frame_invariance_and_repeat(stress_sd):
    """A frame's outputs (final state and every stored tensor) are bitwise the same alone and inside a batch, and run to run."""
    from test_cnf_solve_kernels import Weights, base_samples
    W = Weights(stress_sd, torch.device("cuda:0"))
    BT, n, S = 5, 128, 2
    c, y = rnd(81, BT, 1600), base_samples(82, BT, n)
    e, lp0 = rnd(83, BT, n, 3), rnd(84, BT, n, 1)
    hyper = W.hyper(c, 3078)
    batch = _launch(W, y, lp0, e, hyper, S)
    again = _launch(W, y, lp0, e, hyper, S)
    names = ("x_T", "logp_T", "stage_in", "a", "nd")
    for nm, u, v in zip(names, batch, again):
        assert torch.equal(u, v), "%s differs between two launches" % nm
    for k in range(BT):
        alone = _launch(W, y[k:k + 1], lp0[k:k + 1], e[k:k + 1], hyper[k:k + 1], S)
        for i, (nm, u, v) in enumerate(zip(names, batch, alone)):
            ub = u[k:k + 1] if i < 2 else u[:, :, k:k + 1]
            assert torch.equal(ub, v), "frame %d: %s differs alone / in the batch" % (k, nm)


# ---------------------------------------------------------------------------------------------
# GPU 2-7: the training step through the node
# ---------------------------------------------------------------------------------------------
class _route:
    """flow_grad.BLOCK_NODE / CHECKPOINT_STEPS set for a `with` block and restored after it."""

    def __init__(self, node, ckpt=False):
        self.want = (node, ckpt)

    def __enter__(self):
        from caspr_amd.train import flow_grad as FG
        self.prev = (FG.BLOCK_NODE, FG.CHECKPOINT_STEPS)
        FG.BLOCK_NODE, FG.CHECKPOINT_STEPS = self.want
        return self

    def __exit__(self, *exc):
        from caspr_amd.train import flow_grad as FG
        FG.BLOCK_NODE, FG.CHECKPOINT_STEPS = self.prev
        return False


def _model(sd, steps, latent_steps=2):
    from caspr_amd.models import CaSPR
    m = CaSPR(cnf_rk4_steps=steps, latent_rk4_steps=latent_steps)
    m.load_state_dict(sd)
    return m.to("cuda:0").train()


def _golden_batch(golden):
    return tuple(torch.from_numpy(golden[k]).to("cuda:0") for k in ("train_x", "train_sp", "train_e"))


def _step(m, x, sp, e, stats=None):
    """One forward + backward from rewound MovingBatchNorm statistics -> (loss tensor, {name: grad}, peak bytes)."""
    if stats is not None:
        m.load_state_dict(stats, strict=False)
    m.zero_grad()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    nll, tl = m(x, sp, e=e)
    loss = 0.01 * nll.sum(2).mean() + 100.0 * tl[:, :, :, :4].mean()
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    return loss.detach().clone(), {n_: (None if p.grad is None else p.grad.detach().clone()) for n_, p in m.named_parameters()}, peak


def _stats(m):
    return {k: v.clone() for k, v in m.state_dict().items() if "running_" in k or k.endswith(".step")}


def _same_bits(ga, gb):
    return [n_ for n_ in ga if (ga[n_] is None) != (gb[n_] is None) or (ga[n_] is not None and not torch.equal(ga[n_], gb[n_]))]


@pytest.mark.gpu
def test_full_step_gradients_through_the_node_vs_f64_oracle(golden, seeded_sd):
    """tests/test_hip_train.py::test_full_step_all_flow_parameters_vs_f64_oracle with the option on, at that test's bounds (loss 1e-5,
    rel L2 2e-4 for every non-encoder parameter: sqrt_end_time and the four hyper networks among them); the node route must have run.
    The distance between node and taped gradients is reported per parameter and gated at the sum of the two oracle bounds (4e-4):
    the two forwards are different kernels (inference-class launch against the training kernels), so no tighter gate."""
    from oracle import model as O
    skip = ("running_mean", "running_var", "step", "_num_evals")
    sd6 = {k: (v.detach().clone().double().requires_grad_(True) if v.is_floating_point() and not k.endswith(skip) else
               (v.double() if v.is_floating_point() else v)) for k, v in seeded_sd.items()}
    x, sp, e = (torch.from_numpy(golden[k]) for k in ("train_x", "train_sp", "train_e"))
    loss6, _, _ = O.training_loss(sd6, x.double(), sp.double(), e.double(), cnf_steps=8, latent_steps=4)
    loss6.backward()
    xd, spd, ed = _golden_batch(golden)
    m = _model(seeded_sd, 8, 4)
    stats = _stats(m)
    cnf = m.point_cnf.chain[1]
    with _route(True):
        loss, g_node, _ = _step(m, xd, spd, ed, stats)
        assert cnf._block_node_used is True
    with _route(False):
        loss_t, g_tape, _ = _step(m, xd, spd, ed, stats)
        assert cnf._block_node_used is False
    rel("node_full64_loss", loss.reshape(1), loss6.detach().reshape(1), 1e-5)
    n, bad = 0, []
    for name, _ in m.named_parameters():
        if name.startswith("encoder."):
            continue
        want = sd6[name.replace("latent_ode.solver.ode_func", "latent_ode.ode_func")].grad
        assert want is not None and g_node[name] is not None, name
        err = float((g_node[name].cpu().double() - want).norm() / want.norm().clamp_min(1e-12))
        vs_tape = float((g_node[name] - g_tape[name]).double().norm() / g_tape[name].double().norm().clamp_min(1e-12))
        REPORT["node_full64_grad_l2:" + name] = {"rel_l2": err, "ref_l2": float(want.norm()), "node_vs_taped_rel_l2": vs_tape}
        n += 1
        if not err <= 2e-4:
            bad.append("%s: rel L2 vs f64 %.3e" % (name, err))
        if not vs_tape <= 4e-4:
            bad.append("%s: node vs taped rel L2 %.3e" % (name, vs_tape))
    rel("node_full64_flush", torch.zeros(1), torch.zeros(1), 1.0)
    assert n >= 30, n
    assert any("sqrt_end_time" in k for k in g_node) and sum("_hyper_" in k for k in g_node) >= 8
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_node_peak_memory_at_8_steps_is_below_the_other_routes_at_2(golden, seeded_sd):
    """The contract: the node keeps ONE evaluation's tape alive, the checkpointed route one step's (four evaluations), the taped route
    all of them -- so the node's peak at S = 8 is below either of the others' at S = 2."""
    x, sp, e = _golden_batch(golden)
    peaks = {}
    for key, steps, node, ckpt in (("node_s8", 8, True, False), ("checkpointed_s2", 2, False, True), ("taped_s2", 2, False, False)):
        m = _model(seeded_sd, steps)
        with _route(node, ckpt):
            _step(m, x, sp, e)          # first call: weight packs, workspaces
            _, _, peaks[key] = _step(m, x, sp, e)
            assert m.point_cnf.chain[1]._block_node_used is node
        del m
        torch.cuda.empty_cache()
    REPORT["cnf_block_node_peak_bytes"] = peaks
    rel("cnf_block_node_peak_flush", torch.zeros(1), torch.zeros(1), 1.0)
    assert peaks["node_s8"] < peaks["checkpointed_s2"], peaks
    assert peaks["node_s8"] < peaks["taped_s2"], peaks


@pytest.mark.gpu
def test_node_steps_are_bit_reproducible(golden, seeded_sd):
    """Two node-mode steps from rewound MovingBatchNorm statistics: torch.equal loss and gradients (the reverse sweep accumulates in a
    fixed order: stage-major within a step, steps descending)."""
    x, sp, e = _golden_batch(golden)
    m = _model(seeded_sd, 4)
    stats = _stats(m)
    with _route(True):
        la, ga, _ = _step(m, x, sp, e, stats)
        lb, gb, _ = _step(m, x, sp, e, stats)
        assert m.point_cnf.chain[1]._block_node_used is True
    assert torch.equal(la, lb)
    bad = _same_bits(ga, gb)
    assert not bad, "gradients differ between two identical node-mode steps: %s" % bad[:5]


@pytest.mark.gpu
def test_option_off_is_untouched_and_flipping_leaves_no_state(golden, seeded_sd):
    """With the flag False the step is today's: loss and gradients torch.equal to a run made before the module attribute was ever
    flipped in this model's life, also after a node-mode step in between."""
    from caspr_amd.train import flow_grad as FG
    x, sp, e = _golden_batch(golden)
    m = _model(seeded_sd, 2)
    stats = _stats(m)
    cnf = m.point_cnf.chain[1]
    with _route(False):
        before = FG.BLOCK_NODE
        l0, g0, _ = _step(m, x, sp, e, stats)
        assert cnf._block_node_used is False
        with _route(True):
            l1, g1, _ = _step(m, x, sp, e, stats)
            assert cnf._block_node_used is True
        assert FG.BLOCK_NODE is before
        l2, g2, _ = _step(m, x, sp, e, stats)
        assert cnf._block_node_used is False
    assert torch.equal(l0, l2)
    bad = _same_bits(g0, g2)
    assert not bad, "the default route changed after the option was flipped on and off: %s" % bad[:5]
    fresh = _model(seeded_sd, 2)        # a model that never saw the option: the same bits again
    with _route(False):
        l3, g3, _ = _step(fresh, x, sp, e)
    assert torch.equal(l0, l3) and not _same_bits(g0, g3)


@pytest.mark.gpu
def test_ineligible_shape_takes_the_taped_route(seeded_sd):
    """n = 96 is not a multiple of 64: the fused-layer kernels do not apply, so with the option on cnf_block_train takes the taped route
    -- bit for bit what it computes with the option off, and the route flag says so."""
    from caspr_amd.train.flow_grad import cnf_block_train
    m = _model(seeded_sd, 2)
    cnf = m.point_cnf.chain[1]
    BT, n = 2, 96
    c = rnd(91, BT, 1600).to("cuda:0")
    e = rnd(93, BT, n, 3).to("cuda:0")
    wy, wl = rnd(94, BT, n, 3).to("cuda:0"), rnd(95, BT, n, 1).to("cuda:0")
    params = [p for p in cnf.parameters()]

    def run(node):
        x = rnd(92, BT, n, 3).to("cuda:0").requires_grad_(True)
        lp = torch.zeros(BT, n, 1, device="cuda:0", requires_grad=True)
        with _route(node):
            y, l = cnf_block_train(cnf, x, c, lp, e)
            used = cnf._block_node_used
        g = torch.autograd.grad((y * wy).sum() + (l * wl).sum(), [x, lp] + params)
        return used, y.detach(), l.detach(), g
    used_on, y_on, l_on, g_on = run(True)
    used_off, y_off, l_off, g_off = run(False)
    assert used_on is False and used_off is False
    assert torch.equal(y_on, y_off) and torch.equal(l_on, l_off)
    assert all(torch.equal(u, v) for u, v in zip(g_on, g_off))


@pytest.mark.gpu
def test_node_sharded_gradient_equals_batch_gradient(seeded_sd):
    """tests/test_hip_train.py::test_sharded_gradient_equals_batch_gradient in node mode, at that test's bound: the gradient over a
    2-sequence batch equals the mean of the two single-sequence gradients."""
    from caspr_amd.train.loop import training_loss
    from caspr_amd.utils.synthetic import dense_sequences
    dev = torch.device("cuda:0")
    x, sp = (t.to(dev) for t in dense_sequences(2, 2, 1024, seed=61))
    e = rnd(7, 4, 1024, 3).to(dev)

    def grads(xs, sps, es):
        m = _model(seeded_sd, 4)
        loss, _, _ = training_loss(m(xs, sps, e=es), 0.01, 100.0)
        loss.backward()
        assert m.point_cnf.chain[1]._block_node_used is True
        return {n: p.grad.detach().clone() for n, p in m.named_parameters()}, float(loss.detach())
    with _route(True):
        g_all, l_all = grads(x, sp, e)
        g0, l0 = grads(x[:1], sp[:1], e[:2])
        g1, l1 = grads(x[1:], sp[1:], e[2:])
    assert abs(l_all - 0.5 * (l0 + l1)) <= 1e-5 * abs(l_all)
    num = den = 0.0
    worst = ("", 0.0)
    for n in g_all:
        avg = 0.5 * (g0[n] + g1[n])
        d, r = float((g_all[n] - avg).norm()), float(avg.norm())
        num, den = num + d * d, den + r * r
        if d > worst[1]:
            worst = (n, d)
    REPORT["node_sharded_grad"] = {"total_rel_l2": (num / den) ** 0.5, "worst": worst[0], "worst_abs_l2": worst[1], "grad_l2": den ** 0.5}
    rel("node_sharded_grad_flush", torch.zeros(1), torch.zeros(1), 1.0)
    assert (num / den) ** 0.5 <= 1e-5 and worst[1] <= 1e-5 * den ** 0.5, REPORT["node_sharded_grad"]
