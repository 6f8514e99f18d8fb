"""The point CNF's kinetic / Jacobian regularisers on the GPU (opt-in: CaSPR(cnf_reg=True), training_loss(kinetic_weight=, jacobian_weight=)):
the epilogue pair caspr_cnf_out_reg_f32 / _bwd_f32 through CnfOutReg, a block through cnf_block_train(reg=True) on every route that
carries them, and the model and loop on top -- each against the f64 reference of tests/cnf_reg_ref.py (jvp through the ConcatSquash
map per evaluation, oracle.model.rk4_solve on the 4-tuple state per block), whose `variant=` mistakes tests/test_cnf_reg_ref.py shows
to lie outside the bounds used here.  Bit identities guard what must not move: with the option off, or the regulariser out of the
loss, values and gradients are those of the code without it.  Errors land in test_hip_train's report under "reg:<case>:<tensor>".
"""
import copy

import pytest
import torch

import cnf_reg_ref as RR
from test_hip_train import rel, rnd  # noqa: F401  (rel: through Checks)
from test_hip_train_kernels import FWD, GRAD, Checks as _Checks, gpu_leaves

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRE = "point_cnf.chain.1"


class Checks(_Checks):
    prefix = "reg"


def _out_inputs(c):
    zod, bd, Gd, Bd = gpu_leaves(c["zo4"], c["b"], c["G"], c["Bt"])
    return zod, bd, Gd, Bd, c["e"].to(DEV)


def _out_run(fn, c, blk, cots):
    """fn = CnfOut / CnfOutReg on out_case's inputs -> outputs, and the gradients of sum <out_i, cot_i> w.r.t. (zo4, b, G, Bt)."""
    zod, bd, Gd, Bd, e = _out_inputs(c)
    outs = fn.apply(zod[:, :3], bd, Gd[:, c["cg"]], Bd[:, c["cb"]], e, c["n"], blk)
    sum((o * ct.to(DEV)).sum() for o, ct in zip(outs, cots)).backward()
    return outs, [t.grad for t in (zod, bd, Gd, Bd)]


# ---------------------------------------------------------------------------------------------
# A. the epilogue
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,n,blk,strided", [(3, 160, "R", False), (3, 160, "R", True), (3, 160, 32, False), (3, 160, 32, True), (1, 1, "R", False)])
def test_cnf_out_reg_vs_f64(frames, n, blk, strided):
    """CnfOutReg on 3 frames of 160 points (not a multiple of the 256-thread block) in both row layouts, gate / beta contiguous or column
    slices of an ldg = 11 tensor, and on a single point: a, nd, q and the gradients w.r.t. Zo (value and tangent rows), b, gate, beta
    under random cotangents on all three outputs."""
    from caspr_amd.train import flow_grad as FG
    c = RR.out_case(frames, n, strided)
    R = c["R"]
    blk = R if blk == "R" else blk
    want = RR.out_ref_case(c, blk)
    (a, nd, q), grads = _out_run(FG.CnfOutReg, c, blk, (c["da"], c["dnd"], c["dq"]))
    assert tuple(a.shape) == (frames, n, 3) and tuple(nd.shape) == (frames, n, 1) and tuple(q.shape) == (frames, n, 2)
    ck = Checks("cnf_out_reg[%dx%d,%d,%s]" % (frames, n, blk, "ldg11" if strided else "ldg3"))
    ck("a", a.reshape(R, 3), want["a"], FWD)
    ck("nd", nd.reshape(R, 1), want["nd"], FWD)
    ck("q", q.reshape(R, 2), want["q"], FWD)
    for nm, g in zip(("dZo", "db", "dgate", "dbeta"), grads):
        ck(nm, g, want[nm], GRAD)
    ck.done()


@pytest.mark.parametrize("blk,strided", [("R", False), (32, True)])
def test_cnf_out_reg_bit_identities(blk, strided):
    """a, nd of CnfOutReg are CnfOut's bits; with dq = 0 so are dZo, db, dgate, dbeta; two backward runs give the same bits."""
    from caspr_amd.train import flow_grad as FG
    c = RR.out_case(3, 160, strided)
    blk = c["R"] if blk == "R" else blk
    (a0, nd0), g0 = _out_run(FG.CnfOut, c, blk, (c["da"], c["dnd"]))
    (a1, nd1, _), g1 = _out_run(FG.CnfOutReg, c, blk, (c["da"], c["dnd"], torch.zeros_like(c["dq"])))
    assert torch.equal(a0, a1) and torch.equal(nd0, nd1)
    for nm, u, v in zip(("dZo", "db", "dgate", "dbeta"), g0, g1):
        assert torch.equal(u, v), "dq = 0: %s differs from CnfOut.backward's" % nm
    runs = [_out_run(FG.CnfOutReg, c, blk, (c["da"], c["dnd"], c["dq"])) for _ in range(2)]
    for o0, o1 in zip(runs[0][0], runs[1][0]):
        assert torch.equal(o0, o1)
    for nm, u, v in zip(("dZo", "db", "dgate", "dbeta"), runs[0][1], runs[1][1]):
        assert torch.equal(u, v), "two backward runs differ in %s" % nm
    assert not torch.equal(runs[0][1][0], g1[0]), "dq had no effect on dZo"


# ---------------------------------------------------------------------------------------------
# B. one block
# ---------------------------------------------------------------------------------------------
_want = {}


def _block_want(sd, weights, BT, n, steps, zdim):
    key = (weights, BT, n, steps)
    if key not in _want:
        case = RR.block_case(BT, n, zdim)
        _want[key] = (case, RR.block_ref_case(sd, PRE, case, steps))
    return _want[key]


def _block(sd, steps):
    from caspr_amd.models import CaSPR
    m = CaSPR(cnf_rk4_steps=steps)
    m.load_state_dict(sd)
    block = m.point_cnf.chain[1].to(DEV).train()
    assert block.rk4_steps == steps and block.train_T
    return block, m.cnf_args.zdim


def _block_run(block, case, reg, with_r=True):
    """cnf_block_train on block_case's inputs -> outputs, input gradients and parameter gradients of <x_T, wx> + <lp_T, wl> (+ <r_T, wr>)."""
    from caspr_amd.train import flow_grad as FG
    block.zero_grad()
    xd, cd, lpd = gpu_leaves(case["x"], case["c"], case["lp"])
    outs = FG.cnf_block_train(block, xd, cd, lpd, case["e"].to(DEV), reg=True) if reg else FG.cnf_block_train(block, xd, cd, lpd, case["e"].to(DEV))
    assert len(outs) == (3 if reg else 2)
    loss = (outs[0] * case["wx"].to(DEV)).sum() + (outs[1] * case["wl"].to(DEV)).sum()
    if reg and with_r:
        loss = loss + (outs[2] * case["wr"].to(DEV)).sum()
    loss.backward()
    return [o.detach() for o in outs], [xd.grad, cd.grad, lpd.grad], {k: p.grad.detach().clone() for k, p in block.named_parameters()}


@pytest.mark.parametrize("route,BT,n,steps,weights", [
    ("default", 3, 192, 1, "seeded"), ("default", 3, 192, 2, "seeded"), ("no_out_node", 3, 192, 1, "seeded"), ("unfused", 3, 100, 1, "seeded"),
    ("default", 2, 256, 2, "stress"), ("checkpoint", 3, 192, 2, "seeded"),
])
def test_cnf_block_reg_vs_f64(monkeypatch, seeded_sd, stress_sd, route, BT, n, steps, weights):
    """cnf_block_train(reg=True) against cnf_reg_ref.block_ref at f64: x_T, logp_T, r_T and the gradients of
    <x_T, wx> + <logp_T, wl> + <r_T, wr> w.r.t. x, the context, logpx, every block parameter and sqrt_end_time.  Routes: the fused
    layers with CnfOutReg, the epilogue in torch ops (a second opinion on the kernel pair), the unfused layers (n = 100), the stress
    weights, and the per-step checkpointed tape -- which must also equal the taped route bit for bit."""
    from caspr_amd.train import flow_grad as FG
    monkeypatch.setattr(FG, "OUT_NODE", route != "no_out_node")
    monkeypatch.setattr(FG, "CHECKPOINT_STEPS", route == "checkpoint")
    monkeypatch.setattr(FG, "BLOCK_NODE", False)
    sd = seeded_sd if weights == "seeded" else stress_sd
    block, zdim = _block(sd, steps)
    case, want = _block_want(sd, weights, BT, n, steps, zdim)
    (xT, lpT, rT), gin, gpar = _block_run(block, case, True)
    assert tuple(rT.shape) == (BT, n, 2)
    ck = Checks("cnf_block[%s,%s,%dx%d,rk4=%d]" % (route, weights, BT, n, steps))
    ck("x_T", xT, want["x_T"], FWD)
    ck("logp_T", lpT, want["logp_T"], FWD)
    ck("r_T", rT, want["r_T"], FWD)
    for nm, g in zip(("dx", "dcontext", "dlogpx"), gin):
        ck(nm, g, want[nm], GRAD)
    assert sorted(PRE + "." + k for k in gpar) == sorted(want["params"])
    for k, g in gpar.items():
        ck("d" + k, g, want["params"][PRE + "." + k], GRAD)
    if route == "checkpoint":
        monkeypatch.setattr(FG, "CHECKPOINT_STEPS", False)
        outs_t, gin_t, gpar_t = _block_run(block, case, True)
        assert all(torch.equal(u, v) for u, v in zip((xT, lpT, rT), outs_t)), "checkpointed and taped outputs differ"
        assert all(torch.equal(u, v) for u, v in zip(gin, gin_t)), "checkpointed and taped input gradients differ"
        bad = [k for k in gpar if not torch.equal(gpar[k], gpar_t[k])]
        assert not bad, "checkpointed and taped parameter gradients differ: %s" % bad[:5]
    ck.done()


@pytest.mark.parametrize("route,n", [("default", 192), ("no_out_node", 192), ("unfused", 100)])
def test_cnf_block_reg_leaves_the_solve_alone(monkeypatch, seeded_sd, route, n):
    """cnf_block_train(reg=True) returns the x_T and logp_T of reg=False, and with the regulariser left out of the loss the same input and
    parameter gradients, bit for bit."""
    from caspr_amd.train import flow_grad as FG
    monkeypatch.setattr(FG, "OUT_NODE", route != "no_out_node")
    monkeypatch.setattr(FG, "BLOCK_NODE", False)
    block, zdim = _block(seeded_sd, 2)
    case = RR.block_case(3, n, zdim)
    o0, gi0, gp0 = _block_run(block, case, False)
    o1, gi1, gp1 = _block_run(block, case, True, with_r=False)
    assert torch.equal(o0[0], o1[0]) and torch.equal(o0[1], o1[1])
    assert all(torch.equal(u, v) for u, v in zip(gi0, gi1))
    bad = [k for k in gp0 if not torch.equal(gp0[k], gp1[k])]
    assert not bad, "gradients moved although r_T is not in the loss: %s" % bad[:5]


# ---------------------------------------------------------------------------------------------
# C. the model and the loop
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(seeded_sd):
    """2 sequences x 2 frames: 1024 input points for the encoder (its first level samples 1024), 128 sample points for the CNF -- hence
    regress_tnocs=False, whose loss wants as many sample points as input points; every encoder gradient then comes through z."""
    from caspr_amd.utils.synthetic import dense_sequences
    x, sp = dense_sequences(2, 2, 1024, seed=11)
    kw = dict(regress_tnocs=False, cnf_rk4_steps=2, latent_rk4_steps=1, check_tol=None)
    return x.to(DEV), sp[:, :, :128].contiguous().to(DEV), rnd(5, 4, 128, 3).to(DEV), kw


def _model(seeded_sd, kw, **more):
    from caspr_amd.models import CaSPR
    m = CaSPR(**kw, **more)
    m.load_state_dict({k: v for k, v in seeded_sd.items() if k in m.state_dict()})
    return m.to(DEV)


def test_model_returns_the_integrals_and_the_loss_reaches_everything(seeded_sd, small):
    from caspr_amd.train.loop import regulariser_means, training_loss
    x, sp, e, kw = small
    m = _model(seeded_sd, kw, cnf_reg=True).train()
    out = m(x, sp, e=e)
    assert len(out) == 3 and tuple(out[0].shape) == (2, 2, 128) and out[1] is None and tuple(out[2].shape) == (2, 2, 128, 2)
    assert out[2].grad_fn is not None and bool(torch.isfinite(out[2]).all()) and bool((out[2] >= 0).all()) and float(out[2].max()) > 0
    k, j = regulariser_means(out)
    assert k > 0 and j > 0
    loss, cnf_l, _ = training_loss(out, 0.01, 100.0, kinetic_weight=0.01, jacobian_weight=0.01)
    assert float(loss) > float(cnf_l)
    loss.backward()
    flow = {n_: p for n_, p in m.point_cnf.named_parameters()}
    missing = [n_ for n_, p in flow.items() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not missing, "no finite gradient for %s" % missing[:5]
    enc = [(n_, p) for n_, p in m.encoder.named_parameters() if not n_.startswith("conv3")]
    missing = [n_ for n_, p in enc if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not missing, "no finite encoder gradient (through z) for %s" % missing[:5]
    # the regularisers alone reach the block, the encoder and the latent ODE too (not the MovingBatchNorm behind the block)
    m.zero_grad()
    out = m(x, sp, e=e)
    out[2].sum().backward()
    blk = m.point_cnf.chain[1]
    assert float(blk.sqrt_end_time.grad.abs().max()) > 0 and float(m.encoder.conv1.weight.grad.abs().max()) > 0
    assert float(m.point_cnf.chain[0].weight.grad.abs().max()) > 0
    assert m.point_cnf.chain[2].weight.grad is None or float(m.point_cnf.chain[2].weight.grad.abs().max()) == 0
    # the same model without the option: today's 2-tuple, and the same NLL bits
    m2 = _model(seeded_sd, kw).train()
    m3 = _model(seeded_sd, kw, cnf_reg=True).train()
    o2, o3 = m2(x, sp, e=e), m3(x, sp, e=e)
    assert len(o2) == 2 and torch.equal(o2[0], o3[0])


def test_train_step_with_weights_is_bit_reproducible(seeded_sd, small):
    from caspr_amd.train.loop import train_step
    x, sp, e, kw = small
    m = _model(seeded_sd, kw, cnf_reg=True)
    sd0 = copy.deepcopy(m.state_dict())

    def step():
        m.load_state_dict(sd0)
        opt = torch.optim.Adam(m.parameters(), lr=1e-4)
        reg = []
        losses = train_step(m, opt, x, sp, e=e, kinetic_weight=0.01, jacobian_weight=0.01, reg_out=reg)
        return losses, reg, [p.detach().clone() for p in m.parameters()]
    (l0, r0, p0), (l1, r1, p1) = step(), step()
    assert l0 == l1 and r0 == r1 and len(r0) == 2 and all(v == v for v in l0)
    bad = [n_ for (n_, _), u, v in zip(m.named_parameters(), p0, p1) if not torch.equal(u, v)]
    assert not bad, "two steps from the same state differ: %s" % bad[:5]
    assert any(not torch.equal(u, sd0[k]) for (k, _), u in zip(m.named_parameters(), p0)), "the step moved nothing"
    with pytest.raises(ValueError, match="cnf_reg"):                                 # a weight on a model built without the option
        m2 = _model(seeded_sd, kw)
        train_step(m2, torch.optim.Adam(m2.parameters(), lr=1e-4), x, sp, e=e, jacobian_weight=0.01)


def test_no_grad_returns_none_and_the_block_node_refuses(monkeypatch, seeded_sd, small):
    from caspr_amd.train import flow_grad as FG
    x, sp, e, kw = small
    m = _model(seeded_sd, kw, cnf_reg=True).eval()
    with torch.no_grad():
        out = m(x, sp, e=e)
    assert len(out) == 3 and out[2] is None and not out[0].requires_grad and tuple(out[0].shape) == (2, 2, 128)
    monkeypatch.setattr(FG, "BLOCK_NODE", True)
    with pytest.raises(ValueError, match="train_cnf_checkpoint"):
        m(x, sp, e=e)


def test_cnf_out_reg_keeps_cnf_outs_argument_checks():
    """What CnfOut refuses, CnfOutReg refuses with the same words: a column stride in zo, gate or beta, and gate / beta of different row
    strides (the kernels read both with one ldg)."""
    from caspr_amd.train import flow_grad as FG
    c = RR.out_case(3, 160, True)
    zo, b, G, Bt, e = (c[k].to(DEV) for k in ("zo4", "b", "G", "Bt", "e"))
    n, R = c["n"], c["R"]
    bad = [(zo[:, ::2], G[:, c["cg"]], Bt[:, c["cb"]]),         # zo with a column stride of 2
           (zo[:, :3], G[:, 0:6:2], Bt[:, c["cb"]]),                              # gate with a column stride of 2
           (zo[:, :3], G[:, c["cg"]], Bt[:, 0:6:2]),                              # beta with a column stride of 2
           (zo[:, :3], G[:, c["cg"]], Bt[:, c["cb"]].contiguous())]               # row strides 11 and 3
    for zo_, g_, be_ in bad:
        msgs = []
        for fn in (FG.CnfOut, FG.CnfOutReg):
            with pytest.raises(ValueError, match="unit column strides") as ei:
                fn.apply(zo_, b, g_, be_, e, n, R)
            msgs.append(str(ei.value).split(": ", 1)[1])
        assert msgs[0] == msgs[1]


def test_model_with_tnocs_regression_and_regularisers(seeded_sd):
    """The T-NOCS branch beside the option (the reference's default configuration), 1 sequence x 2 frames x 1024 points: the 3-tuple with
    all three elements, a loss that reaches the T-NOCS head, the encoder and every flow parameter."""
    from caspr_amd.train.loop import training_loss
    from caspr_amd.utils.synthetic import dense_sequences
    x, sp = (t.to(DEV) for t in dense_sequences(1, 2, 1024, seed=11))
    m = _model(seeded_sd, dict(cnf_rk4_steps=2, latent_rk4_steps=1, check_tol=None), cnf_reg=True).train()
    out = m(x, sp, e=rnd(5, 2, 1024, 3).to(DEV))
    assert len(out) == 3 and tuple(out[0].shape) == (1, 2, 1024) and tuple(out[1].shape) == (1, 2, 1024, 4) and tuple(out[2].shape) == (1, 2, 1024, 2)
    loss, cnf_l, tn_l = training_loss(out, 0.01, 100.0, kinetic_weight=0.01, jacobian_weight=0.01)
    base = training_loss(out[:2], 0.01, 100.0)
    assert torch.equal(cnf_l, base[1]) and torch.equal(tn_l, base[2]) and float(loss.detach()) > float(base[0].detach())
    loss.backward()
    missing = [n_ for n_, p in m.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not missing, "no finite gradient for %s" % missing[:5]
    assert float(m.encoder.conv3.weight.grad.abs().max()) > 0
