"""The exact EMD (caspr_amd/csrc/emd_exact.hip) on the CPU: the numpy f64 restatement of its auction (tests/emd_exact_ref.py) against the
optimum -- by brute force over all permutations for n <= 7, and by scipy's linear_sum_assignment where scipy imports -- the comparison
functions the GPU test relies on against wrong variants, the host refusals of the new Python entry points, and the declarations.

The bound is derived, not measured (emd_exact_ref.py's header): primal - dual_bound <= n eps, and dual_bound <= optimum <= primal."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import emd_exact_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = 1e-6
SMALL = [(R.uniform, n) for n in (1, 2, 3, 5, 7)] + [(R.clustered, 7), (R.duplicated, 6), (R.permuted, 7)]
LARGER = [(R.uniform, 65), (R.clustered, 64), (R.duplicated, 64), (R.permuted, 63), (R.uniform, 200)]


def _check(p, q, eps, optimum):
    n = p.shape[0]
    assign, prices, info = R.auction(p, q, eps)
    C = R.cost_matrix(p, q)
    assert info[0] == 1 and R.is_permutation(assign)
    primal, dual = R.primal(C, assign), R.dual_bound(C, prices)
    assert primal - dual <= n * eps * (1 + 1e-9), (primal, dual)
    slack = 1e-12 * max(1.0, abs(primal))                 # the f64 summation of 2 n terms, nothing else
    assert dual <= optimum + slack and optimum <= primal + slack, (dual, optimum, primal)
    assert R.certified(C, assign, prices, eps)
    return C, assign, prices


@pytest.mark.parametrize("gen,n", SMALL, ids=["%s-n%d" % (g.__name__, n) for g, n in SMALL])
def test_restatement_against_brute_force(gen, n):
    p, q = gen(n, 4, 10 + n)
    for b in range(4):
        _check(p[b], q[b], EPS, R.brute_force(R.cost_matrix(p[b], q[b])))


@pytest.mark.parametrize("gen,n", LARGER, ids=["%s-n%d" % (g.__name__, n) for g, n in LARGER])
def test_restatement_against_scipy_where_it_imports(gen, n):
    """The extra leg: the brute-force leg above never skips."""
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        pytest.skip("scipy does not import")
    p, q = gen(n, 1, 20 + n)
    C = R.cost_matrix(p[0], q[0])
    r, c = linear_sum_assignment(C)
    _check(p[0], q[0], EPS, float(C[r, c].sum()))


def test_scaled_coordinates_and_eps():
    p, q = R.uniform(7, 1, 5)
    p, q = (p[0] * np.float32(100)).astype(np.float32), (q[0] * np.float32(100)).astype(np.float32)
    _check(p, q, 1e-4, R.brute_force(R.cost_matrix(p, q)))


def test_budget_and_status_of_the_restatement():
    p, q = R.uniform(64, 1, 64064)
    assign, prices, info = R.auction(p[0], q[0], EPS, max_bids=64)
    assert info.tolist() == [0, 1, 1, 64] and (assign == -1).all() and np.isfinite(prices).all()
    assign, prices, info = R.auction(p[0], q[0], EPS, max_bids=64 * 12)
    assert info[0] == 0 and info[3] <= 64 * 12, "the GPU test's mixed batch needs this frame to exhaust 768 bids: %s" % info
    assign, prices, info = R.auction(p[0], p[0], EPS, max_bids=64 * 12)
    assert info[0] == 1 and info[3] <= 640 and (assign == np.arange(64)).all(), info
    one, _, info = R.auction(p[0][:1], q[0][:1], EPS)
    assert one.tolist() == [0] and info[0] == 1


def test_cost_matrix_is_the_kernels_f32_formula():
    p, q = R.uniform(5, 1, 1)
    C = R.cost_matrix(p[0], q[0])
    d = p[0][3].astype(np.float32) - q[0][2].astype(np.float32)
    want = np.sqrt(np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    assert C.dtype == np.float64 and C[3, 2] == float(want)


def test_comparison_functions_reject_wrong_variants():
    """Otherwise the certificate at n eps proves nothing."""
    p, q = R.uniform(7, 1, 77)
    C, assign, prices = _check(p[0], q[0], EPS, R.brute_force(R.cost_matrix(p[0], q[0])))
    n = 7
    swapped = assign.copy()
    swapped[[0, 1]] = swapped[[1, 0]]                    # two rows swapped: still a permutation, no longer within n eps
    assert R.is_permutation(swapped) and not R.certified(C, swapped, prices, EPS)
    assert R.primal(C, swapped) - R.brute_force(C) > n * EPS
    shifted = prices.copy()
    shifted[int(assign[0])] += 0.01                      # prices shifted on one object: its owner is no longer within eps of its best
    assert not R.certified(C, assign, shifted, EPS)
    assert R.dual_bound(C, shifted) <= R.brute_force(C)  # ... while the bound stays a bound (weak duality), merely a looser one
    twice = assign.copy()
    twice[1] = twice[0]                                  # not a permutation
    assert not R.is_permutation(twice) and not R.certified(C, twice, prices, EPS)
    with pytest.raises(ValueError, match="not a permutation"):
        R.primal(C, twice)
    with pytest.raises(ValueError, match="not a permutation"):
        R.primal(C, np.full(n, -1))


def _no_library(monkeypatch):
    from caspr_amd import lib

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(lib, "load", no_library)


def test_ops_entry_refuses_on_the_host(monkeypatch):
    from caspr_amd import ops
    params = inspect.signature(ops.earth_mover_distance_exact).parameters
    assert list(params) == ["xyz1", "xyz2", "transpose", "eps", "max_bids", "return_match"]
    assert params["transpose"].default is True and params["eps"].default == 1e-6 and params["max_bids"].default is None
    assert params["return_match"].default is False
    _no_library(monkeypatch)
    p = torch.zeros(2, 3, 8)
    with pytest.raises(ValueError, match=r"n = 8 and m = 9.*earth_mover_distance \(the approximate EMD\)"):
        ops.earth_mover_distance_exact(p, torch.zeros(2, 3, 9))
    with pytest.raises(ValueError, match=r"n = 8 and m = 9"):
        ops.earth_mover_distance_exact(torch.zeros(8, 3), torch.zeros(9, 3), transpose=False)
    with pytest.raises(ValueError, match=r"n = 2049.*2048"):
        ops.earth_mover_distance_exact(torch.zeros(1, 3, 2049), torch.zeros(1, 3, 2049))
    with pytest.raises(ValueError, match=r"n = 0"):
        ops.earth_mover_distance_exact(torch.zeros(1, 3, 0), torch.zeros(1, 3, 0))
    with pytest.raises(ValueError, match=r"\(b,3,n\)"):
        ops.earth_mover_distance_exact(torch.zeros(2, 8, 3), torch.zeros(2, 8, 3))
    with pytest.raises(ValueError, match=r"same b"):
        ops.earth_mover_distance_exact(p, torch.zeros(3, 3, 8))
    for eps in (0, -1e-6, float("inf"), float("nan"), "1e-6", None, True):
        with pytest.raises(ValueError, match="eps must be positive and finite"):
            ops.earth_mover_distance_exact(p, p, eps=eps)
    for mb in (0, -1, 2 ** 31, 1.5, True):
        with pytest.raises(ValueError, match="max_bids must be an integer"):
            ops.earth_mover_distance_exact(p, p, max_bids=mb)
    with pytest.raises(TypeError, match="xyz2 must be float32"):
        ops.earth_mover_distance_exact(p, p.double())
    with pytest.raises(ValueError, match="xyz1 is on cpu.*no CPU fallback"):
        ops.earth_mover_distance_exact(p, p)


def test_loss_entries_refuse_on_the_host(monkeypatch):
    from caspr_amd import losses
    _no_library(monkeypatch)
    p, q = torch.zeros(2, 8, 3), torch.zeros(2, 9, 3)
    for fn in (losses.emd_exact_loss, lambda a, b, **kw: losses.exact_earth_mover_distance(a, b, transpose=False, **kw)):
        with pytest.raises(ValueError, match=r"has 8 points and (gt|xyz2) has 9: use the approximate EMD"):
            fn(p, q)
        with pytest.raises(ValueError, match=r"(pred|xyz1) is on cpu.*no CPU fallback"):
            fn(p, p)                                                       # the device is checked last: everything else was in order
        with pytest.raises(ValueError, match=r"(gt|xyz2) must be float32, got torch.float64"):
            fn(p, p.double())
        with pytest.raises(ValueError, match=r"(pred|xyz1) must be contiguous"):
            fn(torch.zeros(2, 3, 8).transpose(1, 2), p)
        for eps in (0, -1.0, float("nan"), float("inf"), None):
            with pytest.raises(ValueError, match=r"eps must be positive and finite"):
                fn(p, p, eps=eps)
    with pytest.raises(ValueError, match=r"emd_exact_loss: reduction must be 'mean', 'sum' or 'none', got 'max'"):
        losses.emd_exact_loss(p, p, reduction="max")
    with pytest.raises(ValueError, match=r"emd_exact_loss: pred and gt must both be \(F,N,3\) or \(B,T,N,3\)"):
        losses.emd_exact_loss(p, torch.zeros(3, 8, 3))
    with pytest.raises(ValueError, match=r"exact_earth_mover_distance: xyz1 must be a \(F,3,N\) tensor"):
        losses.exact_earth_mover_distance(p, p)
    with pytest.raises(ValueError, match=r"xyz1 and xyz2 have 2049 points: the exact EMD takes 1 \.\. 2048"):
        losses.exact_earth_mover_distance(torch.zeros(1, 3, 2049), torch.zeros(1, 3, 2049))
    assert list(inspect.signature(losses.exact_earth_mover_distance).parameters) == ["xyz1", "xyz2", "transpose", "eps"]
    assert list(inspect.signature(losses.emd_exact_loss).parameters) == ["pred", "gt", "reduction", "eps"]


def test_gradient_and_evaluation_entries_refuse_on_the_host(monkeypatch):
    from caspr_amd import train_ops
    from caspr_amd.utils import evaluations, fit
    _no_library(monkeypatch)
    assert list(inspect.signature(train_ops.emd_exact_bwd).parameters) == ["p", "q", "assign", "g", "want_p", "want_q"]
    assert list(inspect.signature(evaluations.eval_exact_emd_frames).parameters) == ["pred", "gt", "eps"]
    with pytest.raises(ValueError, match="no CPU fallback"):
        train_ops.emd_exact_bwd(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1))
    with pytest.raises(ValueError, match="no CPU fallback"):
        evaluations.eval_exact_emd_frames(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
    with pytest.raises(ValueError, match="n = 4 and m = 5"):
        evaluations.eval_exact_emd_frames(torch.zeros(1, 4, 3), torch.zeros(1, 5, 3))
    assert sorted(fit.LOSSES) == ["chamfer", "emd"], "fit.LOSSES stays: the exact EMD goes in as a callable"
    assert "loss=losses.emd_exact_loss" in fit.fit_latent.__doc__


def test_entries_are_declared_and_bound():
    from caspr_amd import lib
    from caspr_amd.csrc import build
    inc = os.path.join(ROOT, "include")
    hdr, train = open(os.path.join(inc, "caspr_hip.h")).read(), open(os.path.join(inc, "caspr_hip_train.h")).read()
    for text, entry, ret, nargs, cites in ((hdr, "caspr_emd_exact_ws_bytes", "long", 2, ("emd.py:11-12", "evaluations.py:45-46")),
                                           (hdr, "caspr_emd_exact_f32", "int", 13, ("emd.py:11-12", "evaluations.py:45-46")),
                                           (train, "caspr_emd_exact_bwd_f32", "int", 9, ("emd.py:17-21",))):
        mt = re.search(r"\b%s %s\(([^;]*)\);" % (ret, entry), text)
        assert mt, "%s is not declared in its header" % entry
        assert mt.group(1).count(",") + 1 == nargs
        assert entry in lib.SIGNATURES and len(lib.SIGNATURES[entry][1]) == nargs, entry
        above = text[text.rindex("/*", 0, mt.start()):mt.start()]          # the comment block that ends at the declaration(s)
        assert all(c in above for c in cites), "%s: no reference call site above the declaration" % entry
    above = hdr[hdr.rindex("/*", 0, hdr.index("long caspr_emd_exact_ws_bytes(")):hdr.index("long caspr_emd_exact_ws_bytes(")]
    assert "reference has only the approximation" in above
    assert hdr.index("caspr_emd_rows_f32(") < hdr.index("long caspr_emd_exact_ws_bytes(") < hdr.index("int caspr_emd_exact_f32(") < hdr.index("caspr_pose_ransac_ws_bytes(")
    assert train.index("int caspr_emd_bwd_f32(") < train.index("int caspr_emd_exact_bwd_f32(")
    src = open(os.path.join(ROOT, "caspr_amd", "csrc", "emd_exact.hip")).read()
    assert "emd_exact_kernel" in src and "emd_exact_bwd_kernel" in src
    assert "emd_exact.hip" in build.SOURCES and "-ffp-contract=off" in build.EXTRA["emd_exact.hip"]
    assert lib.SIGNATURES["caspr_emd_exact_f32"][1][4] is __import__("ctypes").c_double
