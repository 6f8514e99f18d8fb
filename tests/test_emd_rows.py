"""The row-parallel route of the approximate EMD on the GPU (caspr_amd/csrc/emd.hip: caspr_emd_rows_f32; ops.earth_mover_distance(route="rows"),
ops.EMD_ROUTE) against the route it stands beside ("frame": emd_kernel, one workgroup per frame) and against the f64 oracle.

The design rests on one claim: a row's sum is the same sequential f32 chain on both routes, so the ten levels' ratio vectors -- the tape,
and with it the gradient -- are equal BIT FOR BIT, and only the cost, which is added in another order, may differ in its last bits.  The
shapes are the kernels' edges, two frames each (tests/emd_rows_ref.py: SHAPES): clouds below one workgroup, the 256-row block edge from both
sides, the 1024-point tile edge, both multiplier directions; the inputs are those of tests/test_point_ops_edges.py (uniform [0,1]^3, seed
n + m).  The cost is held to the project's bound for this operator, 1e-4 relative to oracle.model.approx_emd in f64; the restatement of the
route's order in f32 is within 5.9e-7 of f64 on these inputs (tests/test_emd_rows_cases.py)."""
import ctypes
import re

import numpy as np
import pytest
import torch

import emd_rows_ref as R
from oracle import model as O
from test_hip_parity import REPORT, record

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4
_WANT = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    from caspr_amd import ops as _ops
    return _ops


def case(n, m, B=2):
    """-> p (B,n,3), q (B,m,3) on the CPU and the f64 oracle's cost (B,), computed once per shape."""
    key = (n, m, B)
    if key not in _WANT:
        p, q = R.clouds(n, m, B)
        p, q = torch.from_numpy(p), torch.from_numpy(q)
        _WANT[key] = (p, q, O.approx_emd(p.double(), q.double()))
    return _WANT[key]


@pytest.mark.parametrize("n,m", R.SHAPES, ids=["n%d-m%d" % s for s in R.SHAPES])
def test_tape_is_the_frame_routes_and_cost_is_within_the_bound(ops, n, m):
    p, q, want = case(n, m)
    pd, qd = p.to(DEV), q.to(DEV)
    cost_f, tape_f = ops.earth_mover_distance(pd, qd, transpose=False, return_tape=True, route="frame")
    cost_r, tape_r = ops.earth_mover_distance(pd, qd, transpose=False, return_tape=True, route="rows")
    bad = int((tape_r != tape_f).sum())
    REPORT["emd_rows:tape[%d,%d]" % (n, m)] = {"mismatches": bad, "count": tape_f.numel()}
    rel = float((cost_r.cpu().double() / want - 1).abs().max())
    vs = float((cost_r.double() / cost_f.double() - 1).abs().max())
    print("emd_rows[%d,%d]: tape mismatches %d / %d, cost rel to f64 %.3e, to the frame route %.3e" % (n, m, bad, tape_f.numel(), rel, vs))
    assert torch.equal(tape_r, tape_f), "(%d, %d): %d of %d ratio values differ from emd_kernel's" % (n, m, bad, tape_f.numel())
    record("emd_rows:rel[%d,%d]" % (n, m), cost_r.cpu().double() / want, torch.ones_like(want), TOL)
    record("emd_rows:vs_frame[%d,%d]" % (n, m), cost_r.double() / cost_f.double(), torch.ones_like(want), 2e-4)
    cost_plain = ops.earth_mover_distance(pd, qd, transpose=False, route="rows")
    assert torch.equal(cost_plain, cost_r), "the cost without the tape differs from the cost with it"


def test_gradient_is_the_frame_routes(ops):
    from caspr_amd import losses
    p, q, _ = case(37, 64)
    g = torch.tensor([0.75, -1.5], device=DEV)
    grads = {}
    before = ops.EMD_ROUTE
    try:
        for route in ("frame", "rows"):
            ops.EMD_ROUTE = route
            pd, qd = p.to(DEV).requires_grad_(True), q.to(DEV).requires_grad_(True)
            cost = losses.earth_mover_distance(pd, qd, transpose=False)
            (g * cost).sum().backward()
            grads[route] = (pd.grad.clone(), qd.grad.clone(), cost.detach().clone())
    finally:
        ops.EMD_ROUTE = before
    assert float(grads["frame"][0].abs().max()) > 0 and float(grads["frame"][1].abs().max()) > 0
    assert torch.equal(grads["rows"][0], grads["frame"][0]) and torch.equal(grads["rows"][1], grads["frame"][1])
    assert float((grads["rows"][2].double() / grads["frame"][2].double() - 1).abs().max()) <= 2e-4


def test_a_frame_is_a_function_of_the_frame(ops):
    p, q, _ = case(255, 257, B=5)
    pd, qd = p.to(DEV), q.to(DEV)
    batch, tape = ops.earth_mover_distance(pd, qd, transpose=False, return_tape=True, route="rows")
    again, tape2 = ops.earth_mover_distance(pd, qd, transpose=False, return_tape=True, route="rows")
    alone, tape3 = ops.earth_mover_distance(pd[3:4].contiguous(), qd[3:4].contiguous(), transpose=False, return_tape=True, route="rows")
    assert torch.equal(again, batch) and torch.equal(tape2, tape)
    assert torch.equal(alone, batch[3:4]) and torch.equal(tape3, tape[3:4])
    assert torch.equal(ops.earth_mover_distance(pd[3:4].contiguous(), qd[3:4].contiguous(), transpose=False, route="rows"), batch[3:4])


def test_layouts(ops):
    p, q, _ = case(100, 300)
    pd, qd = p.to(DEV), q.to(DEV)
    got = ops.earth_mover_distance(pd, qd, transpose=False, route="rows")
    got_t = ops.earth_mover_distance(pd.transpose(1, 2).contiguous(), qd.transpose(1, 2).contiguous(), route="rows")     # (b,3,n), emd.py:24
    assert torch.equal(got_t, got)
    one = ops.earth_mover_distance(pd[1], qd[1], transpose=False, route="rows")                                          # a 2-D cloud is one frame
    one_t = ops.earth_mover_distance(pd[1].t().contiguous(), qd[1].t().contiguous(), route="rows")
    assert one.shape == (1,) and torch.equal(one, got[1:2]) and torch.equal(one_t, got[1:2])
    before = ops.EMD_ROUTE
    try:
        ops.EMD_ROUTE = "rows"
        assert torch.equal(ops.earth_mover_distance(pd, qd, transpose=False), got)                                       # None: the module's route
    finally:
        ops.EMD_ROUTE = before


def test_evaluation_protocol_follows_the_route(ops):
    from caspr_amd.utils.evaluations import eval_reconstr_frames
    p, q, want = case(300, 300)
    pd, qd = p.to(DEV), q.to(DEV)
    chamfer_f, _ = eval_reconstr_frames(pd, qd)
    before = ops.EMD_ROUTE
    try:
        ops.EMD_ROUTE = "rows"
        chamfer_r, emd_r = eval_reconstr_frames(pd, qd)
        direct = ops.earth_mover_distance(pd, qd, transpose=False, route="rows")
    finally:
        ops.EMD_ROUTE = before
    assert np.array_equal(np.asarray(chamfer_r), np.asarray(chamfer_f))
    assert np.array_equal(np.asarray(emd_r), (direct / 300).cpu().numpy()), "eval_reconstr_frames did not take the rows route"
    record("emd_rows:eval_rel[300,300]", torch.from_numpy(np.asarray(emd_r, dtype=np.float64)) / (want / 300), torch.ones_like(want), TOL)


def test_c_entry_refuses_before_any_launch():
    """A workspace one byte short and B = 65536 are refused on the host with the entry's name; the pointers only have to be non-NULL to
    reach the checks and are never followed."""
    from caspr_amd import lib
    L = lib.load()
    ptr = ctypes.c_void_p(256)
    need = L.caspr_emd_rows_ws_bytes(2, 255, 257)
    assert need >= 2 * (3 * 255 + 2 * 257) * 4
    assert L.caspr_emd_rows_f32(ptr, ptr, 2, 255, 257, ptr, None, ptr, need - 1, None) != 0
    assert "emd_rows: workspace too small" in L.caspr_last_error_string().decode()
    assert L.caspr_emd_rows_f32(ptr, ptr, 65536, 1, 1, ptr, None, ptr, L.caspr_emd_rows_ws_bytes(65536, 1, 1), None) != 0
    assert re.search(r"emd_rows: B=65536.*65535", L.caspr_last_error_string().decode())
    assert L.caspr_emd_rows_f32(ptr, ptr, 1, 0, 1, ptr, None, ptr, 1 << 20, None) != 0
    assert "emd_rows: bad arguments" in L.caspr_last_error_string().decode()
    assert L.caspr_emd_rows_f32(ptr, ptr, 1, 1, 1, None, None, ptr, 1 << 20, None) != 0
    assert "emd_rows: bad arguments" in L.caspr_last_error_string().decode()
