"""f64 reference of the point CNF's kinetic / Jacobian regularisers (caspr_amd/train/flow_grad.py: CnfOutReg, cnf_block_train(reg=True);
Finlay et al. 2020, "How to train your neural ODE") and the inputs the CPU and GPU tests share.

Nothing here restates the kernels' closed forms.  Per evaluation the tangent of the output layer is torch.func.jvp through the
ConcatSquash map; per block the state (x, lp, rK, rJ) is integrated by oracle.model.rk4_solve with dy from oracle.model.odenet, J e from
torch.func.jvp of odenet in y along e, nd = -(J e . e), rK' = |dy|^2, rJ' = |J e|^2, and T_end = sqrt_end_time^2 kept in the graph.

`variant=` produces the mistakes a port would make, so that the tests can show their comparisons refuse them:
    "etJ"       |e^T J|^2 (reverse mode, RNODE's own estimator) in place of |J e|^2  [block only: per evaluation the output map is diagonal]
    "no2"       the factor 2 dropped in the backward (values unchanged, the squares' gradients halved)
    "pre_gate"  q taken before the output layer's gate: |Zo_v + b|^2 and |Zo_t|^2
    "euler"     r advanced with Euler weights, r + h q(k1), beside an RK4 (x, lp)             [block only]
"""
import torch
import torch.nn.functional as F

from test_hip_train import rnd

VARIANTS_OUT = ("no2", "pre_gate")
VARIANTS_BLOCK = ("etJ", "no2", "pre_gate", "euler")


def _sq(x, variant):
    """sum_j x_j^2 over the last axis; "no2": the same value with half the gradient."""
    s = (x * x).sum(dim=-1)
    return 0.5 * s + 0.5 * s.detach() if variant == "no2" else s


# ---------------------------------------------------------------------------------------------
# one evaluation of the output epilogue
# ---------------------------------------------------------------------------------------------
def out_case(frames, n, strided):
    """Inputs of the epilogue tests (the shapes and seeds of test_hip_train_kernels.test_cnf_out_vs_f64, plus dq): f32 CPU tensors."""
    R = frames * n
    wide = 11 if strided else 3
    cg, cb = (slice(4, 7), slice(1, 4)) if strided else (slice(0, 3), slice(0, 3))
    return {"frames": frames, "n": n, "R": R, "zo4": rnd(1, 2 * R, 4), "b": rnd(2, 3, scale=0.3),
            "G": torch.sigmoid(rnd(3, frames, wide, scale=1.5)), "Bt": rnd(4, frames, wide, scale=0.3), "e": rnd(5, R, 3),
            "da": rnd(6, frames, n, 3), "dnd": rnd(7, frames, n, 1), "dq": rnd(8, frames, n, 2), "cg": cg, "cb": cb}


def out_ref(zv, zt, b, gate_rows, beta_rows, e, variant=None):
    """zv / zt (R, 3) value / tangent rows of the output product by point, gate_rows / beta_rows (R, 3) -> a (R,3), nd (R,1), q (R,2)."""
    a, ad = torch.func.jvp(lambda v: (v + b) * gate_rows + beta_rows, (zv,), (zt,))
    nd = -(ad * e).sum(dim=1, keepdim=True)
    if variant == "pre_gate":
        return a, nd, torch.stack([_sq(zv + b, None), _sq(zt, None)], dim=1)
    return a, nd, torch.stack([_sq(a, variant), _sq(ad, variant)], dim=1)


def out_ref_case(c, blk, variant=None):
    """out_ref on out_case's inputs in row layout blk, with the backward of <a, da> + <nd, dnd> + <q, dq> taken.
    -> {"a", "nd", "q", "dZo" (2R, 4), "db", "dgate", "dbeta"} (gate / beta gradients on the wide tensors)."""
    R, n = c["R"], c["n"]
    zo6, b6, G6, B6 = [t.detach().double().requires_grad_(True) for t in (c["zo4"], c["b"], c["G"], c["Bt"])]
    zz = zo6[:, :3].reshape(R // blk, 2, blk, 3)
    zv, zt = zz[:, 0].reshape(R, 3), zz[:, 1].reshape(R, 3)
    a, nd, q = out_ref(zv, zt, b6, G6[:, c["cg"]].repeat_interleave(n, dim=0), B6[:, c["cb"]].repeat_interleave(n, dim=0), c["e"].double(), variant)
    ((a * c["da"].double().reshape(R, 3)).sum() + (nd * c["dnd"].double().reshape(R, 1)).sum() + (q * c["dq"].double().reshape(R, 2)).sum()).backward()
    return {"a": a.detach(), "nd": nd.detach(), "q": q.detach(), "dZo": zo6.grad, "db": b6.grad, "dgate": G6.grad, "dbeta": B6.grad}


# ---------------------------------------------------------------------------------------------
# one CNF block
# ---------------------------------------------------------------------------------------------
def block_case(BT, n, zdim):
    """Inputs of the block tests (the seeds of test_hip_train_kernels.test_cnf_block_vs_f64_oracle, plus wr): f32 CPU tensors."""
    return {"x": rnd(1, BT, n, 3, scale=0.7), "c": rnd(2, BT, zdim, scale=0.5), "lp": rnd(3, BT, n, 1), "e": rnd(4, BT, n, 3),
            "wx": rnd(5, BT, n, 3), "wl": rnd(6, BT, n, 1), "wr": rnd(7, BT, n, 2)}


def block_field(sd, pre, t, y, c, e, variant=None):
    """The augmented ODE function at time t: -> dy (BT,n,3), nd (BT,n,1), rK' (BT,n,1), rJ' (BT,n,1)."""
    from oracle import model as O
    net = pre + ".odefunc.diffeq"
    tc = torch.cat([torch.ones(y.shape[0], 1, dtype=y.dtype) * t, c.view(y.shape[0], -1)], dim=1)
    dy, je = torch.func.jvp(lambda v: O.odenet(sd, net, tc, v), (y,), (e,))
    nd = -(je * e).sum(dim=-1, keepdim=True)
    if variant == "etJ":                                  # reverse mode: e^T J, one row per point (the points do not interact)
        yy = y if y.requires_grad else y.detach().requires_grad_(True)
        etj = torch.autograd.grad(O.odenet(sd, net, tc, yy), yy, e, create_graph=True)[0]
        return dy, nd, _sq(dy, None).unsqueeze(-1), _sq(etj, None).unsqueeze(-1)
    if variant == "pre_gate":                             # the output layer before its gate and hyper bias
        lp3 = net + ".layers.3"
        gate = torch.sigmoid(F.linear(tc, sd[lp3 + "._hyper_gate.weight"], sd[lp3 + "._hyper_gate.bias"])).unsqueeze(1)
        bias = F.linear(tc, sd[lp3 + "._hyper_bias.weight"]).unsqueeze(1)
        return dy, nd, _sq((dy - bias) / gate, None).unsqueeze(-1), _sq(je / gate, None).unsqueeze(-1)
    return dy, nd, _sq(dy, variant).unsqueeze(-1), _sq(je, variant).unsqueeze(-1)


def block_ref(sd, pre, x, c, lp, e, steps, variant=None):
    """Forward direction, t: 0 -> sqrt_end_time^2 in `steps` RK4 steps on the state (x, lp, rK, rJ), rK(0) = rJ(0) = 0.
    sd: f64 tensors (leaves where gradients are wanted).  -> x_T (BT,n,3), lp_T (BT,n,1), r_T (BT,n,2)."""
    from oracle import model as O
    T_end = sd[pre + ".sqrt_end_time"] ** 2
    zero = torch.zeros_like(lp)
    fn = lambda t, ys: block_field(sd, pre, t, ys[0], c, e, variant)
    if variant != "euler":
        xT, lpT, rK, rJ = O.rk4_solve(fn, (x, lp, zero, zero), 0.0, T_end, steps)
        return xT, lpT, torch.cat([rK, rJ], dim=-1)
    h = T_end / steps
    ys = (x, lp, zero, zero)
    for s in range(steps):
        q = fn(s * h, ys)
        nxt = O.rk4_solve(fn, ys, s * h, (s + 1) * h, 1)
        ys = (nxt[0], nxt[1], ys[2] + h * q[2], ys[3] + h * q[3])
    return ys[0], ys[1], torch.cat([ys[2], ys[3]], dim=-1)


def block_ref_case(sd32, pre, case, steps, variant=None):
    """block_ref on block_case's inputs and the f32 state dict's block `pre`, with the backward of <x_T, wx> + <lp_T, wl> + <r_T, wr>.
    -> {"x_T", "logp_T", "r_T", "dx", "dcontext", "dlogpx", "params": {key: grad}} in f64."""
    names = [k for k in sd32 if k.startswith(pre + ".") and not k.endswith("_num_evals")]
    sd6 = {k: sd32[k].detach().double().requires_grad_(True) for k in names}
    x6, c6, lp6 = [case[k].detach().double().requires_grad_(True) for k in ("x", "c", "lp")]
    xT, lpT, rT = block_ref(sd6, pre, x6, c6, lp6, case["e"].double(), steps, variant)
    ((xT * case["wx"].double()).sum() + (lpT * case["wl"].double()).sum() + (rT * case["wr"].double()).sum()).backward()
    return {"x_T": xT.detach(), "logp_T": lpT.detach(), "r_T": rT.detach(), "dx": x6.grad, "dcontext": c6.grad, "dlogpx": lp6.grad,
            "params": {k: sd6[k].grad for k in names}}
