"""What the CPU and GPU tests of config.train_cnf_block_node_reg share (tests/test_cnf_block_reg_cpu.py, tests/test_cnf_block_reg.py): the
block cases of the node tests, their bounds, the f64 reference of tests/cnf_reg_ref.py computed once per case, and the comparison that
writes into the training parity report under "block_reg:<case>:<tensor>".

Bounds (tests/test_cnf_block_node.py's own): state-like values 1e-5 (1 + |ref|max); logp_T, r_T and the integrands kq the "lp" kind,
1e-4 max(1, |ref|max) -- r and q are built from the same tangent lanes as nd, which carries that bound there.  Gradients through
test_hip_train_kernels.Checks at its starting bound GRAD (5e-5 of the reference tensor's largest entry; its cap is 2e-4)."""
import torch

import cnf_reg_ref as RR
from test_cnf_block_node import LP_TOL, X_TOL
from test_hip_train import REPORT, rel
from test_hip_train_kernels import GRAD, Checks as _Checks

PRE = "point_cnf.chain.1"
NODE_CASES = [(3, 192, 1, "seeded"), (3, 192, 2, "seeded"), (2, 256, 2, "stress")]      # (BT, n, RK4 steps, weights)
GRAD_BOUND = GRAD


def case_id(c):
    return "bt%d-n%d-s%d-%s" % c


def bound(kind, ref_absmax):
    """kind "x": 1e-5 (1 + |ref|max); kind "lp": 1e-4 max(1, |ref|max) -- absolute."""
    return X_TOL * (1.0 + ref_absmax) if kind == "x" else LP_TOL * max(1.0, ref_absmax)


class Checks(_Checks):
    """test_hip_train_kernels.Checks (relative bounds, for the gradients) plus close(): the absolute bounds above, for values."""
    prefix = "block_reg"

    def close(self, name, got, want, kind):
        got, want = got.detach().cpu().double(), want.detach().cpu().double()
        assert got.shape == want.shape, (name, got.shape, want.shape)
        m = float(want.abs().max())
        b, err = bound(kind, m), float((got - want).abs().max())
        REPORT["%s:%s:%s" % (self.prefix, self.tag, name)] = {"max_abs_err": err, "bound": b, "ref_absmax": m}
        if not (bool(torch.isfinite(got).all()) and err <= b):
            self.bad.append("%s: max abs err %.3e > %.3e" % (name, err, b))

    def note(self, name, **figures):
        REPORT["%s:%s:%s" % (self.prefix, self.tag, name)] = figures

    def done(self):
        rel("%s_flush" % self.prefix, torch.zeros(1), torch.zeros(1), 1.0)       # writes REPORT
        super().done()


_want = {}


def zdim_of(sd):
    return sd[PRE + ".odefunc.diffeq.layers.0._hyper_gate.weight"].shape[1] - 1


def block_want(sd, case, variant=None):
    """-> (cnf_reg_ref.block_case, cnf_reg_ref.block_ref_case) of a NODE_CASES entry, computed once and left unchanged."""
    BT, n, steps, weights = case
    key = (weights, BT, n, steps, variant)
    if key not in _want:
        inputs = RR.block_case(BT, n, zdim_of(sd))
        _want[key] = (inputs, RR.block_ref_case(sd, PRE, inputs, steps, variant))
    return _want[key]
