"""config.train_cnf_block_node_reg on the GPU: the kinetic / Jacobian regularisers on the block node (train/flow_grad.py: CnfBlockSolveReg).

Forward = caspr_cnf_block_reg_fwd_f32, the REG instantiation of csrc/ode_train_fwd.hip's kernel: the fixed-step RK4 solve of
CnfBlockSolve that also integrates r' = (|a|^2, |J e|^2) and tapes every evaluation's integrands kq.  Backward = the shared reverse
sweep with three tapes.  Checked here, against the f64 reference of tests/cnf_reg_ref.py (whose `variant=` mistakes
tests/test_cnf_block_reg_cpu.py shows to lie outside the bounds used here):

  the kernel   x_T, logp_T, r_T and every stored kq at a single point, a partial wave, whole workgroups and more than one workgroup per
               frame; its bit identities: the plain launch's bits in everything the plain launch writes, run to run, frame by frame;
  the node     outputs and every gradient of <x_T, wx> + <logp_T, wl> + <r_T, wr>; its bit identities: the reg=False node's x_T and
               logp_T, its gradients when r_T is left out of the loss, run to run; the routing of both switches;
  the model    CaSPR(cnf_reg=True) through train_step with both weights, against the taped route; peak memory against the taped and
               the checkpointed route.

Bounds: tests/cnf_block_reg_cases.py.  Errors land in test_hip_train's report under "block_reg:<case>:<tensor>"."""
import copy

import pytest
import torch

import cnf_block_reg_cases as BC
import cnf_reg_ref as RR
from cnf_block_reg_cases import PRE, Checks
from test_cnf_block_node import _golden_batch
from test_hip_train import REPORT, rnd
from test_hip_train_kernels import gpu_leaves

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TC = (0.0, 0.5, 0.5, 1.0)


class _route:
    """flow_grad.BLOCK_NODE / BLOCK_NODE_REG / CHECKPOINT_STEPS set for a `with` block and restored after it."""

    def __init__(self, node, node_reg, ckpt=False):
        self.want = (node, node_reg, ckpt)

    def __enter__(self):
        from caspr_amd.train import flow_grad as FG
        self.prev = (FG.BLOCK_NODE, FG.BLOCK_NODE_REG, FG.CHECKPOINT_STEPS)
        FG.BLOCK_NODE, FG.BLOCK_NODE_REG, FG.CHECKPOINT_STEPS = self.want
        return self

    def __exit__(self, *exc):
        from caspr_amd.train import flow_grad as FG
        FG.BLOCK_NODE, FG.BLOCK_NODE_REG, FG.CHECKPOINT_STEPS = self.prev
        return False


# ---------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------
def _launch(W, y, lp0, e, hyper, steps, reg=True):
    from caspr_amd import train_ops as T
    g = lambda v: v.to(DEV).contiguous()
    D = W.dev
    t_end = torch.tensor([W.t_end], device=DEV, dtype=torch.float32)
    out = (T.cnf_block_reg_fwd if reg else T.cnf_train_fwd)(g(y), g(lp0), g(e), g(hyper), D["tcol"], D["w0"], D["b0"], W.w1x, D["b1"], W.w2x, D["b2"],
                                                            D["w3"], D["b3"], t_end, steps)
    torch.cuda.synchronize()
    return out


def _kernel_inputs(W, seed, BT, n):
    from test_cnf_solve_kernels import base_samples
    c, y = rnd(seed, BT, 1600), base_samples(seed + 1, BT, n)
    return c, y, rnd(seed + 2, BT, n, 3), rnd(seed + 3, BT, n, 1), W.hyper(c, 3078)


KERNEL_CASES = [(1, 1, 1, "seeded"), (2, 33, 2, "stress"), (3, 64, 2, "seeded"), (2, 96, 1, "stress")]


@pytest.mark.parametrize("BT,n,S,which", KERNEL_CASES, ids=[BC.case_id(c) for c in KERNEL_CASES])
def test_kernel_vs_f64(BT, n, S, which, seeded_sd, stress_sd):
    """A single point, a partial wave and partial workgroup (n = 33), whole workgroups (n = 64), more than one workgroup per frame with a
    partial last one (n = 96): x_T, logp_T, r_T against cnf_reg_ref.block_ref, and every kq[s, st] against cnf_reg_ref.block_field at the
    STORED stage input ys[s, st] and that stage's time.  Measured: r_T 1.7e-7 ... 2.5e-5 (bounds 1.1e-4 ... 3.9e-3), the worst kq at 1.2 % of
    its bound (stress weights, n = 96)."""
    from test_cnf_solve_kernels import Weights
    sd32 = seeded_sd if which == "seeded" else stress_sd
    sd = {k: v.double() for k, v in sd32.items() if k.startswith(PRE + ".") and v.is_floating_point()}
    W = Weights(sd32, torch.device(DEV))
    c, y, e, lp0, hyper = _kernel_inputs(W, 7100 + 13 * BT + n + S, BT, n)
    gx, glp, gr, ys, ka, knd, kq = _launch(W, y, lp0, e, hyper, S)
    assert tuple(gr.shape) == (BT, n, 2) and tuple(kq.shape) == (S, 4, BT, n, 2)
    assert tuple(gx.shape) == (BT, n, 3) and tuple(glp.shape) == (BT, n, 1) and tuple(ys.shape) == (S, 4, BT, n, 3)
    ck = Checks("kernel:" + BC.case_id((BT, n, S, which)))
    with torch.no_grad():
        wx, wlp, wr = RR.block_ref(sd, PRE, y.double(), c.double(), lp0.double(), e.double(), S)
        ck.close("x_T", gx, wx, "x")
        ck.close("logp_T", glp, wlp, "lp")
        ck.close("r_T", gr, wr, "lp")
        h = float(sd[PRE + ".sqrt_end_time"]) ** 2 / S
        ys64 = ys.cpu().double()
        for s in range(S):
            for st in range(4):
                _, _, qk, qj = RR.block_field(sd, PRE, (s + TC[st]) * h, ys64[s, st], c.double(), e.double())
                ck.close("step%d:q%d" % (s, st + 1), kq[s, st], torch.cat([qk, qj], dim=-1), "lp")
    assert bool((kq >= 0).all()) and bool((gr >= 0).all())
    ck.done()


def test_kernel_bit_identities(stress_sd):
    """(5, 128, 2) on the stress weights: what the plain launch writes -- x_T, logp_T, ys, ka, knd -- has the plain launch's bits; two
    launches give the same bits in all seven results; every frame alone gives the bits it has inside the batch."""
    from test_cnf_solve_kernels import Weights
    W = Weights(stress_sd, torch.device(DEV))
    BT, n, S = 5, 128, 2
    c, y, e, lp0, hyper = _kernel_inputs(W, 81, BT, n)
    batch = _launch(W, y, lp0, e, hyper, S)
    plain = _launch(W, y, lp0, e, hyper, S, reg=False)
    names = ("x_T", "logp_T", "r_T", "stage_in", "a", "nd", "q")
    for i, nm in zip((0, 1, 3, 4, 5), ("x_T", "logp_T", "stage_in", "a", "nd")):
        assert torch.equal(batch[i], plain[i - (i > 2)]), "%s differs from the plain launch's" % nm
    again = _launch(W, y, lp0, e, hyper, S)
    for nm, u, v in zip(names, batch, again):
        assert torch.equal(u, v), "%s differs between two launches" % nm
    for k in range(BT):
        alone = _launch(W, y[k:k + 1], lp0[k:k + 1], e[k:k + 1], hyper[k:k + 1], S)
        for i, (nm, u, v) in enumerate(zip(names, batch, alone)):
            ub = u[k:k + 1] if i < 3 else u[:, :, k:k + 1]
            assert torch.equal(ub, v), "frame %d: %s differs alone / in the batch" % (k, nm)


# ---------------------------------------------------------------------------------------------
# the node
# ---------------------------------------------------------------------------------------------
def _block(sd, steps):
    from caspr_amd.models import CaSPR
    m = CaSPR(cnf_rk4_steps=steps)
    m.load_state_dict(sd)
    block = m.point_cnf.chain[1].to(DEV).train()
    assert block.rk4_steps == steps and block.train_T
    return block


def _block_run(block, case, reg, with_r=True):
    """cnf_block_train on block_case's inputs -> outputs, input gradients and parameter gradients of <x_T, wx> + <lp_T, wl> (+ <r_T, wr>),
    and whether the node ran."""
    from caspr_amd.train import flow_grad as FG
    block.zero_grad()
    xd, cd, lpd = gpu_leaves(case["x"], case["c"], case["lp"])
    outs = FG.cnf_block_train(block, xd, cd, lpd, case["e"].to(DEV), reg=True) if reg else FG.cnf_block_train(block, xd, cd, lpd, case["e"].to(DEV))
    assert len(outs) == (3 if reg else 2)
    loss = (outs[0] * case["wx"].to(DEV)).sum() + (outs[1] * case["wl"].to(DEV)).sum()
    if reg and with_r:
        loss = loss + (outs[2] * case["wr"].to(DEV)).sum()
    loss.backward()
    grads = dict({"dx": xd.grad, "dcontext": cd.grad, "dlogpx": lpd.grad}, **{"d" + k: p.grad.detach().clone() for k, p in block.named_parameters()})
    return [o.detach() for o in outs], grads, block._block_node_used


def _differing(ga, gb):
    return [k for k in ga if not torch.equal(ga[k], gb[k])]


@pytest.mark.parametrize("case", BC.NODE_CASES, ids=[BC.case_id(c) for c in BC.NODE_CASES])
def test_node_vs_f64(case, seeded_sd, stress_sd):
    """cnf_block_train(reg=True) with both switches on against cnf_reg_ref.block_ref_case: x_T, logp_T, r_T at the kernel test's bounds,
    and the gradients of <x_T, wx> + <logp_T, wl> + <r_T, wr> w.r.t. x, the context, logpx, every block parameter and sqrt_end_time
    at GRAD_BOUND.  The taped reg=True route runs on the same inputs: its r_T error against f64 is recorded beside the node's, and the
    distance between the two routes per tensor.  Measured: r_T 2.9e-7 / 2.7e-7 / 6.7e-6 (taped route 3.2e-7 / 2.9e-7 / 1.7e-5), the worst
    gradient d sqrt_end_time at 9.8e-6 / 1.1e-5 / 7.7e-6 of GRAD_BOUND = 5e-5, node against taped at most 1.1e-5 rel L2."""
    BT, n, steps, weights = case
    sd = seeded_sd if weights == "seeded" else stress_sd
    block = _block(sd, steps)
    inputs, want = BC.block_want(sd, case)
    with _route(True, True):
        (xT, lpT, rT), grads, used = _block_run(block, inputs, True)
    assert used is True and tuple(rT.shape) == (BT, n, 2)
    assert int(block.odefunc._num_evals) == 4 * steps
    with _route(False, False):
        (xt, lpt, rt), grads_t, used_t = _block_run(block, inputs, True)
    assert used_t is False
    ck = Checks("node:" + BC.case_id(case))
    ck.close("x_T", xT, want["x_T"], "x")
    ck.close("logp_T", lpT, want["logp_T"], "lp")
    ck.close("r_T", rT, want["r_T"], "lp")
    ck.note("r_T:taped_route", max_abs_err=float((rt.cpu().double() - want["r_T"]).abs().max()),
            node_vs_taped_max_abs=float((rT - rt).abs().max()))
    assert sorted(grads) == sorted(["dx", "dcontext", "dlogpx"] + ["d" + k[len(PRE) + 1:] for k in want["params"]])
    for k, g in grads.items():
        ref = want[k] if k in ("dx", "dcontext", "dlogpx") else want["params"][PRE + "." + k[1:]]
        ck(k, g, ref, BC.GRAD_BOUND)
        gt = grads_t[k].double()
        ck.note(k + ":node_vs_taped", rel_l2=float((g.double() - gt).norm() / gt.norm().clamp_min(1e-30)),
                taped_max_rel_err=float((gt.cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)))
    ck.done()


def test_node_bit_identities(seeded_sd):
    """x_T and logp_T of the reg node are the reg=False node's bits; with r_T left out of the loss so are the input and parameter
    gradients; two runs with r in the loss give the same bits; and r in the loss moves the gradients."""
    case = BC.NODE_CASES[1]
    block = _block(seeded_sd, case[2])
    inputs, _ = BC.block_want(seeded_sd, case)
    with _route(True, True):
        o_plain, g_plain, used0 = _block_run(block, inputs, False)
        o_out, g_out, used1 = _block_run(block, inputs, True, with_r=False)
        o_a, g_a, used2 = _block_run(block, inputs, True)
        o_b, g_b, _ = _block_run(block, inputs, True)
    assert used0 is True and used1 is True and used2 is True
    assert torch.equal(o_plain[0], o_out[0]) and torch.equal(o_plain[1], o_out[1])
    assert torch.equal(o_plain[0], o_a[0]) and torch.equal(o_plain[1], o_a[1])
    bad = _differing(g_plain, g_out)
    assert not bad, "gradients moved although r_T is not in the loss: %s" % bad[:5]
    assert all(torch.equal(u, v) for u, v in zip(o_a, o_b))
    bad = _differing(g_a, g_b)
    assert not bad, "two runs with r in the loss differ: %s" % bad[:5]
    same = [k for k in g_a if k != "dlogpx" and torch.equal(g_a[k], g_plain[k])]
    assert not same, "r in the loss left these gradients where they were: %s" % same[:5]


def test_routing_of_the_two_switches(seeded_sd):
    """Both switches on: n = 96 (no multiple of 64) takes the taped reg=True route, bit for bit what both switches off compute; reg=False
    gives the bits of the block-node switch alone."""
    block = _block(seeded_sd, 2)
    zdim = BC.zdim_of(seeded_sd)
    small, full = RR.block_case(2, 96, zdim), RR.block_case(2, 128, zdim)
    with _route(True, True):
        o_on, g_on, used_on = _block_run(block, small, True)
        o_n2, g_n2, used_n2 = _block_run(block, full, False)
    with _route(False, False):
        o_off, g_off, used_off = _block_run(block, small, True)
    with _route(True, False):
        o_n1, g_n1, used_n1 = _block_run(block, full, False)
    assert used_on is False and used_off is False
    assert all(torch.equal(u, v) for u, v in zip(o_on, o_off)) and not _differing(g_on, g_off)
    assert used_n2 is True and used_n1 is True
    assert all(torch.equal(u, v) for u, v in zip(o_n2, o_n1)) and not _differing(g_n2, g_n1)


# ---------------------------------------------------------------------------------------------
# the model and the loop
# ---------------------------------------------------------------------------------------------
def _model(sd, steps, latent_steps=2):
    from caspr_amd.models import CaSPR
    m = CaSPR(cnf_rk4_steps=steps, latent_rk4_steps=latent_steps, cnf_reg=True)
    m.load_state_dict(sd)
    return m.to(DEV)


def test_train_step_on_the_node_vs_the_taped_route(golden, seeded_sd):
    """CaSPR(cnf_reg=True), train_step with kinetic_weight = jacobian_weight = 0.01 on the golden training batch, both switches on
    against both off: losses to 1e-5 relative, every non-encoder gradient within the node-vs-taped bound of the block node's own
    full-step test (4e-4 rel L2), finite positive regulariser means, and two steps from the same state the same bits."""
    from caspr_amd.train.loop import train_step
    x, sp, e = _golden_batch(golden)
    m = _model(seeded_sd, 2)
    sd0 = copy.deepcopy(m.state_dict())

    def step(node):
        m.load_state_dict(sd0)
        opt = torch.optim.Adam(m.parameters(), lr=1e-4)
        reg = []
        with _route(node, node):
            losses = train_step(m, opt, x, sp, e=e, kinetic_weight=0.01, jacobian_weight=0.01, reg_out=reg)
            assert m.point_cnf.chain[1]._block_node_used is node
        return losses, reg, {k: p.grad.detach().clone() for k, p in m.named_parameters()}, [p.detach().clone() for p in m.parameters()]
    l_n, r_n, g_n, p_n = step(True)
    l_b, r_b, g_b, p_b = step(True)
    l_t, r_t, g_t, _ = step(False)
    assert l_n == l_b and r_n == r_b and not _differing(g_n, g_b) and all(torch.equal(u, v) for u, v in zip(p_n, p_b))
    assert len(r_n) == 2 and all(v == v and 0 < v < float("inf") for v in r_n), r_n
    assert abs(l_n[0] - l_t[0]) <= 1e-5 * abs(l_t[0]), (l_n, l_t)
    bad, count = [], 0
    for k in g_n:
        if k.startswith("encoder."):
            continue
        d = float((g_n[k] - g_t[k]).double().norm() / g_t[k].double().norm().clamp_min(1e-12))
        REPORT["block_reg:train_step:node_vs_taped_rel_l2:" + k] = d
        count += 1
        if not d <= 4e-4:
            bad.append("%s: node vs taped rel L2 %.3e" % (k, d))
    REPORT["block_reg:train_step:loss"] = {"node": l_n, "taped": l_t, "reg_means_node": r_n, "reg_means_taped": r_t}
    Checks("train_step").done()
    assert count >= 30 and any("sqrt_end_time" in k for k in g_n)
    assert not bad, "\n".join(bad)


def test_node_reg_peak_memory_at_8_steps_is_below_the_other_reg_routes_at_2(golden, seeded_sd):
    """test_cnf_block_node's memory contract with the regularisers in the loss: the node keeps ONE evaluation's tape alive, the
    checkpointed route one step's, the taped route all of them -- node + reg at S = 8 is below either of the others at S = 2.
    Measured: 790 MB against 891 MB and 1059 MB."""
    from caspr_amd.train.loop import training_loss
    x, sp, e = _golden_batch(golden)

    def step(m):
        m.zero_grad()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        training_loss(m(x, sp, e=e), 0.01, 100.0, kinetic_weight=0.01, jacobian_weight=0.01)[0].backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()
    peaks = {}
    for key, steps, node, ckpt in (("node_reg_s8", 8, True, False), ("checkpointed_reg_s2", 2, False, True), ("taped_reg_s2", 2, False, False)):
        m = _model(seeded_sd, steps).train()
        with _route(node, node, ckpt):
            step(m)                     # first call: weight packs, workspaces
            peaks[key] = step(m)
            assert m.point_cnf.chain[1]._block_node_used is node
        del m
        torch.cuda.empty_cache()
    REPORT["block_reg:peak_bytes"] = peaks
    Checks("peak").done()
    assert peaks["node_reg_s8"] < peaks["checkpointed_reg_s2"], peaks
    assert peaks["node_reg_s8"] < peaks["taped_reg_s2"], peaks
