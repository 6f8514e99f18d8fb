"""The f64 reference of the CNF regularisers (tests/cnf_reg_ref.py) against closed forms, its `variant=` mistakes against itself on the
inputs of the GPU tests (tests/test_cnf_reg.py), and the surface of the option: header, bindings, constructor, loss.  CPU only."""
import os
import re

import numpy as np
import pytest
import torch

import cnf_reg_ref as RR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FWD, GRAD = 1e-5, 5e-5          # the bounds of tests/test_cnf_reg.py: what a variant has to exceed to be refused there


def relerr(got, want):
    """test_hip_train.rel's measure: max |got - want| / max |want|."""
    return float((got - want).abs().max()) / (float(want.abs().max()) or 1.0)


# ---------------------------------------------------------------------------------------------
# the reference against closed forms
# ---------------------------------------------------------------------------------------------
def _linear_block(seed=0, width=8, zdim=4):
    """A block whose odenet is affine in y: hyper networks with zero weights (gates sigmoid(bias), no hyper bias, no time dependence)
    and hidden pre-activations above F.softplus's threshold of 20, where it returns its argument (and derivative 1) exactly.
    -> state dict (f64), A (3,3), c (3): odenet(y) = A y + c."""
    g = torch.Generator().manual_seed(seed)
    pre = "blk.odefunc.diffeq.layers."
    dims = [3, width, width, width, 3]
    sd = {"blk.sqrt_end_time": torch.tensor([0.9], dtype=torch.float64)}
    A, c = torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    for l in range(4):
        cin, cout = dims[l], dims[l + 1]
        W = torch.randn(cout, cin, generator=g, dtype=torch.float64) * (0.5 if l == 0 else 0.3 / cin)
        b = torch.full((cout,), 120.0, dtype=torch.float64) if l < 3 else torch.randn(cout, generator=g, dtype=torch.float64)
        gb = torch.randn(cout, generator=g, dtype=torch.float64) * 0.3
        sd[pre + "%d._layer.weight" % l], sd[pre + "%d._layer.bias" % l] = W, b
        sd[pre + "%d._hyper_gate.weight" % l] = torch.zeros(cout, 1 + zdim, dtype=torch.float64)
        sd[pre + "%d._hyper_gate.bias" % l] = gb
        sd[pre + "%d._hyper_bias.weight" % l] = torch.zeros(cout, 1 + zdim, dtype=torch.float64)
        D = torch.diag(torch.sigmoid(gb))
        A, c = D @ W @ A, D @ (W @ c + b)
    return sd, A, c


def test_linear_field_closed_forms():
    """odenet(y) = A y + c: rJ = T |A e|^2 and lp_T = lp - T e^T A e exactly (constant integrands), x_T and rK from RK4's stages written
    out on (A, c) -- none of it through odenet or jvp.  <= 1e-12 relative, and the field is checked to be affine where it is used."""
    from oracle import model as O
    sd, A, c = _linear_block()
    BT, n, steps = 2, 5, 3
    g = torch.Generator().manual_seed(1)
    x, e = [torch.randn(BT, n, 3, generator=g, dtype=torch.float64) for _ in range(2)]
    ctx = torch.randn(BT, 4, generator=g, dtype=torch.float64)
    lp = torch.randn(BT, n, 1, generator=g, dtype=torch.float64)
    tc = torch.cat([torch.full((BT, 1), 0.3, dtype=torch.float64), ctx], dim=1)
    assert relerr(O.odenet(sd, "blk.odefunc.diffeq", tc, x), x @ A.t() + c) <= 1e-13
    xT, lpT, rT = RR.block_ref(sd, "blk", x, ctx, lp, e, steps)
    T = float(sd["blk.sqrt_end_time"]) ** 2
    h = T / steps
    f = lambda y: y @ A.t() + c
    y, rK = x, torch.zeros(BT, n, dtype=torch.float64)
    for _ in range(steps):
        k1 = f(y)
        k2 = f(y + 0.5 * h * k1)
        k3 = f(y + 0.5 * h * k2)
        k4 = f(y + h * k3)
        rK = rK + (h / 6.0) * sum(w * (k * k).sum(-1) for w, k in ((1.0, k1), (2.0, k2), (2.0, k3), (1.0, k4)))
        y = y + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    Ae = e @ A.t()
    assert relerr(xT, y) <= 1e-12
    assert relerr(rT[..., 0], rK) <= 1e-12
    assert relerr(rT[..., 1], T * (Ae * Ae).sum(-1)) <= 1e-12
    assert relerr(lpT, lp - T * (Ae * e).sum(-1, keepdim=True)) <= 1e-12


def test_one_evaluation_against_explicit_jacobian_rows(seeded_sd):
    """On the seeded (non-linear) block: q = (|f|^2, |J e|^2) and nd = -e^T J e of one evaluation with J's rows from
    torch.autograd.functional.jacobian, point by point; the "etJ" variant is |J^T e|^2 of the same matrix."""
    from oracle import model as O
    pre = "point_cnf.chain.1"
    sd6 = {k: v.double() for k, v in seeded_sd.items() if k.startswith(pre + ".")}
    zdim = sd6[pre + ".odefunc.diffeq.layers.0._hyper_gate.weight"].shape[1] - 1
    case = RR.block_case(2, 3, zdim)
    x, c, e = case["x"].double(), case["c"].double(), case["e"].double()
    dy, nd, qk, qj = RR.block_field(sd6, pre, 0.2, x, c, e)
    qj_t = RR.block_field(sd6, pre, 0.2, x, c, e, variant="etJ")[3].detach()
    for f_ in range(2):
        tc = torch.cat([torch.full((1, 1), 0.2, dtype=torch.float64), c[f_:f_ + 1]], dim=1)
        for p in range(3):
            J = torch.autograd.functional.jacobian(lambda v: O.odenet(sd6, pre + ".odefunc.diffeq", tc, v.view(1, 1, 3)).view(3), x[f_, p])
            Je = J @ e[f_, p]
            assert abs(float(qj[f_, p, 0]) - float(Je @ Je)) <= 1e-12 * float(Je @ Je)
            assert abs(float(nd[f_, p, 0]) + float(e[f_, p] @ Je)) <= 1e-12 * max(abs(float(e[f_, p] @ Je)), float(Je @ Je))
            assert abs(float(qk[f_, p, 0]) - float(dy[f_, p] @ dy[f_, p])) <= 1e-12 * float(qk[f_, p, 0])
            etJ = e[f_, p] @ J
            assert abs(float(qj_t[f_, p, 0]) - float(etJ @ etJ)) <= 1e-12 * float(etJ @ etJ)


# ---------------------------------------------------------------------------------------------
# the mistakes a port would make, on the GPU tests' own inputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", RR.VARIANTS_OUT)
def test_epilogue_variants_exceed_the_gpu_bounds(variant):
    """On test_cnf_reg.py's epilogue inputs (3 frames x 160 points): the variant moves q (FWD) or a gradient (GRAD) past the bound."""
    c = RR.out_case(3, 160, False)
    want, got = RR.out_ref_case(c, c["R"]), RR.out_ref_case(c, c["R"], variant)
    errs = {k: relerr(got[k], want[k]) for k in want}
    print(variant, errs)
    if variant == "no2":
        assert errs["a"] == 0 and errs["q"] == 0 and errs["dZo"] > GRAD and errs["dgate"] > GRAD and errs["dbeta"] > GRAD, errs
    else:
        assert errs["q"] > FWD and errs["dZo"] > GRAD, errs


@pytest.fixture(scope="module")
def block_want(seeded_sd):
    zdim = seeded_sd["point_cnf.chain.1.odefunc.diffeq.layers.0._hyper_gate.weight"].shape[1] - 1
    case = RR.block_case(3, 192, zdim)
    return case, RR.block_ref_case(seeded_sd, "point_cnf.chain.1", case, 1)


@pytest.mark.parametrize("variant", RR.VARIANTS_BLOCK)
def test_block_variants_exceed_the_gpu_bounds(seeded_sd, block_want, variant):
    """On test_cnf_reg.py's block inputs (seeded weights, 3 x 192 points, one RK4 step): every variant leaves x_T and logp_T alone and
    moves r_T (FWD) or, for the dropped factor 2, the gradients (GRAD) past the bound."""
    case, want = block_want
    got = RR.block_ref_case(seeded_sd, "point_cnf.chain.1", case, 1, variant)
    errs = {k: relerr(got[k], want[k]) for k in ("x_T", "logp_T", "r_T", "dx", "dcontext")}
    errs["dparams_max"] = max(relerr(got["params"][k], want["params"][k]) for k in want["params"])
    print(variant, errs)
    assert errs["x_T"] <= 1e-12 and errs["logp_T"] <= 1e-12, errs
    if variant == "no2":
        assert errs["r_T"] <= 1e-12 and errs["dx"] > GRAD and errs["dcontext"] > GRAD and errs["dparams_max"] > GRAD, errs
    else:
        assert errs["r_T"] > FWD, errs
        which = 1 if variant == "etJ" else slice(None)
        assert relerr(got["r_T"][..., which], want["r_T"][..., which]) > FWD


# ---------------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_two_entries():
    from caspr_amd import lib
    hdr = open(os.path.join(ROOT, "include", "caspr_hip_train.h")).read()
    src = open(os.path.join(ROOT, "caspr_amd", "csrc", "backward_flow.hip")).read()
    for name, nargs in (("caspr_cnf_out_reg_f32", 14), ("caspr_cnf_out_reg_bwd_f32", 17)):
        m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr)
        assert m, "%s is not declared in include/caspr_hip_train.h" % name
        assert len(m.group(1).split(",")) == nargs
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
        assert re.search(r'extern "C" int %s\s*\(' % name, src)
    # the two entries the new ones stand beside keep their signatures
    assert len(lib.SIGNATURES["caspr_cnf_out_f32"][1]) == 13 and len(lib.SIGNATURES["caspr_cnf_out_bwd_f32"][1]) == 15


def test_caspr_cnf_reg_validation():
    from caspr_amd.models import CaSPR
    assert CaSPR().cnf_reg is False
    assert CaSPR(cnf_reg=True).cnf_reg is True
    with pytest.raises(ValueError, match="pretrain_tnocs"):
        CaSPR(pretrain_tnocs=True, cnf_reg=True)
    with pytest.raises(TypeError):
        CaSPR([0.02, 0.05, 0.1, 0.2, 0.4, 0.8], 512, 1600, 512, 64, False, True, True, 1, True, True)      # keyword-only


def test_training_loss_regulariser_weights():
    """Zero weights, a missing or a None third element: torch.equal to the two-element call.  Non-zero weights: the NLL's reduction of the
    weighted integrals joins `loss` only.  A non-zero weight without the integrals raises."""
    from caspr_amd.train.loop import regulariser_means, training_loss
    g = torch.Generator().manual_seed(0)
    nll, tn, reg = torch.randn(2, 3, 7, generator=g), torch.randn(2, 3, 7, 4, generator=g), torch.rand(2, 3, 7, 2, generator=g)
    base = training_loss((nll, tn), 0.01, 100.0)
    for losses, kw in (((nll, tn, reg), {}), ((nll, tn, None), {}), ((nll, tn, reg), dict(kinetic_weight=0.0, jacobian_weight=0.0)), ((nll, tn), dict(kinetic_weight=0.0))):
        out = training_loss(losses, 0.01, 100.0, **kw)
        assert len(out) == 3 and all(torch.equal(a, b) for a, b in zip(out, base))
    loss, cnf_l, tn_l = training_loss((nll, tn, reg), 0.01, 100.0, kinetic_weight=0.5, jacobian_weight=0.25)
    assert torch.equal(cnf_l, base[1]) and torch.equal(tn_l, base[2])
    want = base[0].double() + 0.01 * (0.5 * reg[..., 0].double() + 0.25 * reg[..., 1].double()).sum(2).mean()
    assert abs(float(loss) - float(want)) <= 1e-6 * abs(float(want))
    for losses in ((nll, tn), (nll, tn, None), (tn,)):
        with pytest.raises(ValueError, match="cnf_reg"):
            training_loss(losses, 0.01, 100.0, jacobian_weight=0.01)
    k, j = regulariser_means((nll, tn, reg))
    assert abs(k - float(reg[..., 0].sum(2).mean())) <= 1e-6 and abs(j - float(reg[..., 1].sum(2).mean())) <= 1e-6
    assert all(np.isnan(v) for v in regulariser_means((nll, tn))) and all(np.isnan(v) for v in regulariser_means((nll, tn, None)))
