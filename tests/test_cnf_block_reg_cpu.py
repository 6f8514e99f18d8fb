"""config.train_cnf_block_node_reg on the CPU: CnfBlockSolveReg's reverse sweep with three tapes against f64 autograd through a plain RK4
(the forward entry and the per-evaluation training kernels replaced by f64 torch restatements), the surface of the option (header,
bindings, route table, config, refusal), and the mistakes a port would make (tests/cnf_reg_ref.py's variants) against the bounds the
GPU tests of tests/test_cnf_block_reg.py use on the same cases."""
import os
import re

import numpy as np
import pytest
import torch

import cnf_block_reg_cases as BC
import cnf_reg_ref as RR
from test_cnf_block_node import _eval_f64

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRY = "caspr_cnf_block_reg_fwd_f32"


# ---------------------------------------------------------------------------------------------
# 1. the reverse sweep's algebra with three tapes
# ---------------------------------------------------------------------------------------------
def _eval_reg_f64(wb, t, y, G_lm, Bb_lm, tg_lm, tb_lm, e_rows, BT, n, widths):
    """flow_grad._cnf_eval_fused_reg in plain torch: (a, nd) of test_cnf_block_node._eval_f64, and q = (|a|^2, |J e|^2) with J e taken
    by torch.func.jvp through that function's value path -- not from its tangent recursion."""
    e3 = e_rows.reshape(BT, n, 3)
    a, je = torch.func.jvp(lambda v: _eval_f64(wb, t, v, G_lm, Bb_lm, tg_lm, tb_lm, e_rows, BT, n, widths)[0], (y,), (e3,))
    nd = -(je * e3).sum(-1, keepdim=True)
    return a, nd, torch.stack([(a * a).sum(-1), (je * je).sum(-1)], dim=-1)


def _rk4_reg(f, y, lp, r, h, steps, record=None):
    """Plain RK4 on (y, lp, r) of f(t, y) -> (a, nd, q); record: every step's stage inputs and stage outputs."""
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
        y, lp, r = [v + (h / 6.0) * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]) for i, v in enumerate((y, lp, r))]
    return y, lp, r


def _reg_fwd_restatement(BT, n, widths):
    """caspr_cnf_block_reg_fwd_f32 (train_ops.cnf_block_reg_fwd) restated in plain torch for (BT, n, widths)."""
    cols = np.cumsum((0,) + widths)

    def fwd(y, logp, e_, hyper, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, t_end, steps):
        nG = sum(widths)
        lm = lambda m: torch.cat([m[:, cols[l]:cols[l + 1]].reshape(-1) for l in range(4)])      # kernel columns -> layer-major
        G, Bb = lm(hyper[:, :nG]), lm(hyper[:, nG:])
        tg, tb = lm(tcol[:nG].unsqueeze(0).expand(BT, -1)), lm(tcol[nG:].unsqueeze(0).expand(BT, -1))
        rec = []
        f = lambda t, y_: _eval_reg_f64((w0, b0, w1x, b1, w2x, b2, w3, b3), t, y_, G, Bb, tg, tb, e_.reshape(-1, 3), BT, n, widths)
        yT, lpT, rT = _rk4_reg(f, y, logp, torch.zeros(BT, n, 2, dtype=y.dtype), t_end.reshape(()) / steps, steps, rec)
        ys = torch.stack([torch.stack(ins) for ins, _ in rec])
        ka, knd, kq = [torch.stack([torch.stack([k[i] for k in ks]) for _, ks in rec]) for i in range(3)]
        return yT, lpT, rT, ys, ka, knd, kq
    return fwd


@pytest.mark.parametrize("mode", ["r_in_the_loss", "wr_zero", "r_unused"])
def test_reverse_sweep_algebra_with_three_tapes_vs_f64_autograd(monkeypatch, mode):
    """CnfBlockSolveReg with its forward entry and the per-evaluation kernels replaced by f64 restatements, on the shapes of
    test_cnf_block_node's algebra test (BT = 2, n = 5, S = 3, widths 7-6-5-3): every gradient of <x_T, wx> + <lp_T, wl> + <r_T, wr> --
    x, logpx, the four layer-major hyper tensors, t_end (the <gr, sum_i w_i q_i> term of dL/dh among its parts), all weights and
    biases -- against autograd through the plain RK4 at 1e-9.  The same with wr = 0 and with r_T left out of the loss, where the
    backward takes CnfBlockSolve's two-tape form (_cnf_eval_fused, which is replaced too)."""
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
    cols = np.cumsum((0,) + widths)
    over_frames = lambda v: torch.cat([v[cols[l]:cols[l + 1]].unsqueeze(0).expand(BT, -1).reshape(-1) for l in range(4)])
    L = dict(leaves, tg_lm=over_frames(leaves["tg"]), tb_lm=over_frames(leaves["tb"]))
    e = r(BT, n, 3)
    wy, wl, wr = r(BT, n, 3), r(BT, n, 1), r(BT, n, 2)
    if mode == "wr_zero":
        wr = torch.zeros_like(wr)
    loss = lambda y, lp, rr: (y * wy).sum() + (lp * wl).sum() + (0.0 if mode == "r_unused" else (rr * wr).sum())

    monkeypatch.setattr(FG.T, "cnf_block_reg_fwd", _reg_fwd_restatement(BT, n, widths))
    monkeypatch.setattr(FG, "_cnf_eval_fused_reg", _eval_reg_f64)
    monkeypatch.setattr(FG, "_cnf_eval_fused", _eval_f64)
    y, lp, rT = FG.CnfBlockSolveReg.apply(L["x"], L["logpx"], L["G_lm"], L["Bb_lm"], L["tg_lm"], L["tb_lm"], L["t_end"], e, wbl[2], wbl[4], S, widths, *wbl)
    assert tuple(rT.shape) == (BT, n, 2)
    got = torch.autograd.grad(loss(y, lp, rT), list(leaves.values()))
    f = lambda t, y_: _eval_reg_f64(wbl, t, y_, L["G_lm"], L["Bb_lm"], over_frames(leaves["tg"]), over_frames(leaves["tb"]), e.reshape(-1, 3), BT, n, widths)
    y2, lp2, r2 = _rk4_reg(f, L["x"], L["logpx"], torch.zeros(BT, n, 2, dtype=torch.float64), L["t_end"] / S, S)
    want = torch.autograd.grad(loss(y2, lp2, r2), list(leaves.values()), retain_graph=True)
    assert all(torch.allclose(u, v, rtol=0, atol=1e-12) for u, v in ((y, y2), (lp, lp2), (rT, r2)))
    assert float(r2.detach().min()) > 0
    bad = []
    for name, g, w in zip(leaves, got, want):
        err = float((g - w).abs().max() / w.abs().max().clamp_min(1e-30))
        if not err <= 1e-9:
            bad.append("%s: %.3e" % (name, err))
    assert not bad, "\n".join(bad)
    if mode == "r_in_the_loss":                        # ... and r's cotangent reaches every leaf but logpx
        base = torch.autograd.grad((y2 * wy).sum() + (lp2 * wl).sum(), list(leaves.values()))
        same = [name for name, g, b in zip(leaves, want, base) if torch.equal(g, b)]
        assert same == ["logpx"], same


# ---------------------------------------------------------------------------------------------
# 2. surface
# ---------------------------------------------------------------------------------------------
def test_header_bindings_and_route_table_agree_on_the_entry():
    from caspr_amd import lib, ops
    from caspr_amd.csrc import build
    hdr = open(os.path.join(ROOT, "include", "caspr_hip_train.h")).read()
    src = open(os.path.join(ROOT, "caspr_amd", "csrc", "ode_train_fwd.hip")).read()
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % ENTRY, hdr)
    assert m, "%s is not declared in include/caspr_hip_train.h" % ENTRY
    assert len(m.group(1).split(",")) == 27 and ENTRY in lib.SIGNATURES and len(lib.SIGNATURES[ENTRY][1]) == 27
    sib = lib.SIGNATURES["caspr_cnf_train_fwd_f32"][1]
    assert len(sib) == 25 and lib.SIGNATURES[ENTRY][1][:19] == sib[:19]            # the head, t_end, steps, e, logp_in, logp_out, y_out
    assert re.search(r'extern "C" int %s\s*\(' % ENTRY, src)
    assert not ENTRY.startswith(("caspr_cnf_train_fwd", "caspr_cnf_rk4", "caspr_cnf_dopri5", "caspr_cnf_sample_tape"))
    assert ops._CNF_ENTRY["x6"]["train_fwd_reg"] == ENTRY and ops._CNF_ENTRY["x6"]["train_fwd"] == "caspr_cnf_train_fwd_f32"
    assert "train_fwd_reg" not in ops._CNF_ENTRY["h3"] and "train_fwd_reg" not in ops._CNF_ENTRY["f32"]
    assert build.SOURCES.count("ode_train_fwd.hip") == 1 and len(build.SOURCES) == 25


def test_option_is_off_by_default_and_read_from_the_environment_only_under_debug():
    from caspr_amd import config as C
    from caspr_amd.train import flow_grad as FG
    assert C.KernelConfig().train_cnf_block_node_reg is False
    with pytest.warns(RuntimeWarning):
        assert C.load({"CASPR_CNF_BLOCK_NODE_REG": "1"}).train_cnf_block_node_reg is False
    on = C.load({"CASPR_CNF_BLOCK_NODE_REG": "1", "CASPR_DEBUG": "1"})
    assert on.train_cnf_block_node_reg is True and on.train_cnf_block_node is False
    assert FG.BLOCK_NODE_REG == C.config.train_cnf_block_node_reg


@pytest.mark.parametrize("n", [64, 96])
def test_the_block_node_alone_still_refuses(monkeypatch, n):
    """BLOCK_NODE on, BLOCK_NODE_REG off: the ValueError of before, for a shape the node takes and for one it does not, still naming
    config.train_cnf_checkpoint -- and now the switch that lifts it.  Raised in front of any kernel: CPU tensors get there."""
    from caspr_amd.models import CaSPR
    from caspr_amd.train import flow_grad as FG
    monkeypatch.setattr(FG, "BLOCK_NODE", True)
    monkeypatch.setattr(FG, "BLOCK_NODE_REG", False)
    block = CaSPR().point_cnf.chain[1]
    x = torch.zeros(2, n, 3)
    with pytest.raises(ValueError, match="train_cnf_checkpoint") as ei:
        FG.cnf_block_train(block, x, torch.zeros(2, 1600), torch.zeros(2, n, 1), torch.zeros(2, n, 3), reg=True)
    assert "train_cnf_block_node_reg" in str(ei.value)


# ---------------------------------------------------------------------------------------------
# 3. the bounds of the GPU node test refuse wrong ports
# ---------------------------------------------------------------------------------------------
def relerr(got, want):
    """test_hip_train.rel's measure: max |got - want| / max |want|."""
    return float((got - want).abs().max()) / (float(want.abs().max()) or 1.0)


MARGIN_CASE = (2, 256, 2, "stress")        # the node case picked to carry the 10 x margin for every variant


@pytest.mark.parametrize("variant", RR.VARIANTS_BLOCK)
def test_block_variants_are_refused_by_the_gpu_bounds(seeded_sd, stress_sd, variant):
    """On the cases of test_cnf_block_reg.py::test_node_vs_f64 and with its bounds: |e^T J|^2, q in front of the gate and Euler weights
    move r_T past its bound (1e-4 max(1, |r_T|max)), the dropped factor 2 moves dx, dcontext and a parameter gradient past theirs
    (GRAD_BOUND of the reference tensor's largest entry), on EVERY case; x_T and logp_T stay where they are.  The stress case carries
    the margin: every variant is at least 10 x its bound away there (measured 970 x and more).  The seeded flow is gentle (|r_T|max =
    0.35, below the bound's floor of 1): measured there, in units of the bound, etJ 8.6 at both step counts, euler 12.3 at one step and
    6.1 at two, pre_gate 3900, no2 66 and more -- and more points do not change that (3 x 1024 points: etJ 19.6, euler 7.0 at two steps)."""
    assert MARGIN_CASE in BC.NODE_CASES
    for case in BC.NODE_CASES:
        sd = seeded_sd if case[3] == "seeded" else stress_sd
        _, want = BC.block_want(sd, case)
        _, got = BC.block_want(sd, case, variant)
        assert relerr(got["x_T"], want["x_T"]) <= 1e-12 and relerr(got["logp_T"], want["logp_T"]) <= 1e-12
        r_err = float((got["r_T"] - want["r_T"]).abs().max())
        if variant == "no2":
            assert r_err <= 1e-12 * float(want["r_T"].abs().max())
            grads = {"dx": relerr(got["dx"], want["dx"]), "dcontext": relerr(got["dcontext"], want["dcontext"]),
                     "dparams_max": max(relerr(got["params"][k], want["params"][k]) for k in want["params"])}
            ratio = min(grads.values()) / BC.GRAD_BOUND
        else:
            ratio = r_err / BC.bound("lp", float(want["r_T"].abs().max()))
        print(variant, case, "distance / bound = %.1f" % ratio)
        assert ratio > 1.0, (variant, case, ratio)
        if case == MARGIN_CASE:
            assert ratio >= 10.0, (variant, case, ratio)
