"""The approximate EMD with a gradient (caspr_amd/losses.py: earth_mover_distance, emd_loss) and latent fitting on it (caspr_amd/utils/fit.py):
caspr_emd_tape_f32 (csrc/emd.hip: emd_kernel<true>), caspr_emd_bwd_f32 (csrc/backward_points.hip: emd_bwd_kernel).

Reference: tests/emd_grad_ref.py -- torch f64 on the CPU, the ten annealing levels as oracle/model.py:approx_emd states them, keeping the
match matrix and the per-level ratios; the gradient by autograd through (match.detach() * dist).sum(), the contract of the reference's
backward (utils/emd.py:17-21: matchcost_backward on the saved match, nothing through approxmatch).  The clouds are seeded, B = 2, uniform
in [0,1)^3 at (n, m) = one point, fewer than a wave with multiL = 1 (truncated) and with rows > columns, the 256-thread block edge,
multiR = 4, the forward's 1024-point tile + 1, and randn at (1100, 700): several LDS tiles with n != m; where n >= 255 seven points
coincide; g has both signs.

Bounds:
  the kernel alone   dp, dq against the f64 closed formula evaluated from THE GPU'S OWN tape: rel L2 <= 1e-5.  An f32 torch evaluation of the
                     same formula from the same tape is 1.3e-7 .. 5.8e-7 from the f64 one on these inputs (measured on the CPU); the bound
                     leaves ~20x for another summation order and is 1e4 x below the nearest wrong variant (0.43, test_reference_refuses_...).
  the tape           sum match * dist in f64 from the GPU tape within 1e-4 relative of the GPU cost (the project's EMD bound,
                     tests/test_hip_parity.py::test_emd_matches_oracle).
  end to end         dp, dq against the f64 reference run from scratch: rel L2 <= 1e-3.  approxmatch is sensitive to f32 rounding: an f32
                     CPU restatement is 3e-8 .. 2.4e-5 from f64 on these shapes; the nearest wrong variant is 0.43 away.
  the norm           |dp_k| <= |g| multiL (1 + 1e-4), |dq_l| <= |g| multiR (1 + 1e-4): row / column sums of the match never exceed the
                     multipliers and every term is a unit vector times its match entry.
Measured on an MI355X: the kernel alone 1.1e-7 .. 5.8e-7, the tape's cost 2.5e-8 .. 1.7e-6, end to end 4.8e-8 .. 2.4e-5 (largest at
(1100, 700), where the f32 CPU restatement is 2.4e-5 from f64 too).
Measured values go to the training parity report (train_parity_report.json, written by test_hip_train.rel) under emd_grad:<case>:<tensor>.
"""
import inspect
import os
import re

import pytest
import torch

import emd_grad_ref as R
from test_hip_train import REPORT, rel, rnd

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KERNEL_TOL = 1e-5
TAPE_TOL = 1e-4
E2E_TOL = 1e-3
SHAPE_IDS = ["n%d-m%d" % s for s in R.SHAPES]
DEV = "cuda:0"


def _flush():
    rel("emd_grad_flush", torch.zeros(1), torch.zeros(1), 1.0)          # writes REPORT


def _l2(bad, case, name, got, want, tol, **extra):
    err = R.rel_l2(got, want)
    REPORT["emd_grad:%s:%s" % (case, name)] = dict({"rel_l2": err, "bound": tol, "ref_l2": float(want.double().norm())}, **extra)
    print("emd_grad:%s:%s rel L2 %.3e (bound %.1e)" % (case, name, err, tol))
    if not (bool(torch.isfinite(got).all()) and err <= tol):
        bad.append("%s %s: rel L2 %.3e > %.1e" % (case, name, err, tol))


def _run(p, q, g, p_grad=True, q_grad=True, transpose=False):
    """losses.earth_mover_distance forward + backward of sum(g cost) -> (cost, dp | None, dq | None) in the (B,N,3) layout."""
    from caspr_amd import losses
    pd, qd = p.to(DEV), q.to(DEV)
    if transpose:
        pd, qd = pd.transpose(1, 2).contiguous(), qd.transpose(1, 2).contiguous()
    pd.requires_grad_(p_grad)
    qd.requires_grad_(q_grad)
    cost = losses.earth_mover_distance(pd, qd, transpose=transpose)
    (g.to(DEV) * cost).sum().backward()
    torch.cuda.synchronize()
    back = (lambda t: None if t is None else (t.transpose(1, 2) if transpose else t))
    return cost.detach(), back(pd.grad), back(qd.grad)


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", R.SHAPES, ids=SHAPE_IDS)
def test_reference_refuses_wrong_variants(n, m):
    """The closed formula of include/caspr_hip_train.h, evaluated in f64 from the reference's own tape, IS the autograd gradient (<= 1e-12
    rel L2) -- and the kernel's bound has teeth: with dq's sign flipped, with the Chamfer-style squared term, without g, with the ratios of
    level i under the kernel of level i + 1, without the level that carries most of the match mass, the same formula misses it by at
    least 100x."""
    p, q, g = R.clouds(n, m)
    _, match, tape, dp, dq = R.reference(n, m)
    fp, fq = R.grads_from_tape(p, q, tape, g)
    assert R.rel_l2(fp, dp) <= 1e-12 and R.rel_l2(fq, dq) <= 1e-12
    assert R.rel_l2(R.match_from_tape(p, q, tape), match) <= 1e-12
    for variant in R.VARIANTS:
        vp, vq = R.grads_from_tape(p, q, tape, g, variant)
        worst = max(R.rel_l2(vp, dp), R.rel_l2(vq, dq))
        assert worst >= 100 * KERNEL_TOL, "%s passes at n=%d m=%d: rel L2 %.3e" % (variant, n, m, worst)


def test_reference_inputs_cover_what_they_claim():
    """g has both signs; seven coincident pairs where n >= 255; the match respects the multipliers (4 at (1024, 256)); the built (5, 3)
    cluster case has an exactly zero match row in f64 and in f32 -- the uniform (5, 3) case has none, with random points some level always
    leaves a kernel value above zero -- and its other rows are not zero."""
    for n, m in R.SHAPES:
        p, q, g = R.clouds(n, m)
        _, match, _, dp, dq = R.reference(n, m)
        multiL, multiR = R.multipliers(n, m)
        assert float(g.min()) < 0.0 < float(g.max())
        assert (n >= 255) == bool((p[:, :min(n, m, 7)] == q[:, :min(n, m, 7)]).all())
        assert float(match.sum(2).max()) <= multiL * (1 + 1e-12) and float(match.sum(1).max()) <= multiR * (1 + 1e-12)
        assert bool(torch.isfinite(dp).all()) and bool(torch.isfinite(dq).all())
    assert R.multipliers(1024, 256) == (1.0, 4.0) and R.multipliers(3, 5) == (1.0, 1.0) and R.multipliers(1025, 1024) == (1.0, 1.0)
    p, q, g = R.cluster_clouds()
    for dtype in (torch.float64, torch.float32):
        rows = R.approx_match(p, q, dtype)[1].sum(2)
        assert bool((rows[:, 4] == 0).all()) and bool((rows[:, :4] > 0.5).all()), rows


def test_new_entries_are_declared_and_bound():
    """caspr_emd_tape_bytes / caspr_emd_tape_f32 in include/caspr_hip.h beside caspr_emd_f32, caspr_emd_bwd_f32 in include/caspr_hip_train.h,
    all in lib.SIGNATURES with the argument counts of their declarations (tests/test_host_cpu.py::test_library_exports_every_declared_symbol
    holds the library to them), each header citing the reference call site; the kernels live in sources the build already lists."""
    from caspr_amd import lib, losses, ops
    from caspr_amd import train_ops as T
    from caspr_amd.csrc import build
    from caspr_amd.utils import fit
    for hdr_name, entry, ret in (("caspr_hip.h", "caspr_emd_tape_bytes", "long"), ("caspr_hip.h", "caspr_emd_tape_f32", "int"),
                                 ("caspr_hip_train.h", "caspr_emd_bwd_f32", "int")):
        hdr = open(os.path.join(ROOT, "include", hdr_name)).read()
        mt = re.search(r"\b%s %s\(([^;]*)\);" % (ret, entry), hdr)
        assert mt, "%s is not declared in include/%s" % (entry, hdr_name)
        assert entry in lib.SIGNATURES and len(lib.SIGNATURES[entry][1]) == mt.group(1).count(",") + 1, entry
        assert "emd.py" in hdr[max(0, mt.start() - 1500):mt.start()], "%s: no reference call site above the declaration" % entry
    assert len(lib.SIGNATURES["caspr_emd_tape_f32"][1]) == 10 and len(lib.SIGNATURES["caspr_emd_bwd_f32"][1]) == 10
    assert len(lib.SIGNATURES["caspr_emd_f32"][1]) == 9, "caspr_emd_f32 keeps its signature"
    csrc = os.path.join(ROOT, "caspr_amd", "csrc")
    emd = open(os.path.join(csrc, "emd.hip")).read()
    assert "emd_kernel<true>" in emd and "emd_kernel<false>" in emd and "emd.hip" in build.SOURCES
    assert "-ffp-contract=off" in build.EXTRA["emd.hip"]
    assert "emd_bwd_kernel" in open(os.path.join(csrc, "backward_points.hip")).read() and "backward_points.hip" in build.SOURCES
    assert inspect.signature(ops.earth_mover_distance).parameters["return_tape"].default is False
    assert list(inspect.signature(losses.earth_mover_distance).parameters) == ["xyz1", "xyz2", "transpose"]
    assert inspect.signature(losses.earth_mover_distance).parameters["transpose"].default is True
    assert callable(T.emd_bwd) and inspect.signature(losses.emd_loss).parameters["reduction"].default == "mean"
    assert inspect.signature(fit.fit_latent).parameters["loss"].default == "chamfer"


def test_refusals_name_the_argument():
    """No silent fallback and no silent copy: a CPU tensor, f64, a non-contiguous tensor, a wrong layout and a mismatched F each raise a
    ValueError that names the argument it is about; the device is looked at last."""
    from caspr_amd import losses
    from caspr_amd.utils.fit import fit_latent
    p, q = torch.zeros(2, 3, 8), torch.zeros(2, 3, 5)                      # the reference's (b,3,n) layout
    with pytest.raises(ValueError, match=r"\bxyz1 is on cpu.*GPU"):
        losses.earth_mover_distance(p, q)
    with pytest.raises(ValueError, match=r"\bxyz2 must be float32"):
        losses.earth_mover_distance(p, q.double())
    with pytest.raises(ValueError, match=r"\bxyz1 must be contiguous"):
        losses.earth_mover_distance(torch.zeros(2, 8, 3).transpose(1, 2), q)
    with pytest.raises(ValueError, match=r"\bxyz2 must be a \(F,3,N\)"):
        losses.earth_mover_distance(p, torch.zeros(2, 5, 4))
    with pytest.raises(ValueError, match=r"\bxyz1 must be a \(F,N,3\)"):
        losses.earth_mover_distance(torch.zeros(2, 4, 8), q, transpose=False)
    with pytest.raises(ValueError, match=r"xyz1 and xyz2 disagree on F"):
        losses.earth_mover_distance(p, torch.zeros(3, 3, 5))
    with pytest.raises(ValueError, match=r"\bxyz1 is on cpu.*GPU"):
        losses.earth_mover_distance(torch.zeros(3, 8), torch.zeros(3, 5))     # a 2-D cloud is one frame, as in emd.py:37-40
    pn, qn = torch.zeros(2, 8, 3), torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match=r"\bpred is on cpu.*GPU"):
        losses.emd_loss(pn, qn)
    with pytest.raises(ValueError, match=r"\bgt must be float32"):
        losses.emd_loss(pn, qn.double())
    with pytest.raises(ValueError, match=r"\bgt must be contiguous"):
        losses.emd_loss(pn.view(1, 2, 8, 3), torch.zeros(1, 2, 3, 5).transpose(2, 3))
    with pytest.raises(ValueError, match=r"pred and gt"):
        losses.emd_loss(pn, torch.zeros(3, 5, 3))
    with pytest.raises(ValueError, match="reduction"):
        losses.emd_loss(pn, qn, reduction="max")
    with pytest.raises(ValueError, match=r"loss must be one of \['chamfer', 'emd'\]"):
        fit_latent(None, qn.view(1, 2, 5, 3), torch.zeros(1, 2, 4), 8, loss="hausdorff")


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """B > 65535 and two NULL outputs are refused by caspr_emd_bwd_f32, a short workspace and a NULL tape by caspr_emd_tape_f32, on the
    host, in front of any launch (the pointers only have to be non-NULL to reach the checks and are never followed); the tape size is
    40 B (n + m) bytes."""
    import ctypes
    from caspr_amd import lib
    L = lib.load()
    ptr = ctypes.c_void_p(256)
    assert L.caspr_emd_tape_bytes(160, 2048, 2048) == 160 * 10 * 4096 * 4
    assert L.caspr_emd_bwd_f32(ptr, ptr, 65536, 1, 1, ptr, ptr, ptr, ptr, None) != 0
    assert re.search(r"emd_bwd: B=65536.*65535", L.caspr_last_error_string().decode())
    assert L.caspr_emd_bwd_f32(ptr, ptr, 1, 1, 1, ptr, ptr, None, None, None) != 0
    assert "d1 and d2" in L.caspr_last_error_string().decode()
    assert L.caspr_emd_tape_f32(ptr, ptr, 1, 1, 1, ptr, ptr, ptr, 8, None) != 0
    assert "workspace too small" in L.caspr_last_error_string().decode()
    assert L.caspr_emd_tape_f32(ptr, ptr, 1, 1, 1, ptr, None, ptr, 1 << 20, None) != 0
    assert "emd_tape: bad arguments" in L.caspr_last_error_string().decode()


# ---------------------------------------------------------------------------------------------
# GPU, per shape
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,m", R.SHAPES, ids=SHAPE_IDS)
def test_cost_bits_tape_and_gradients(n, m):
    """Per shape: (1) the cost of the tape entry and of the autograd Function, in both layouts, is torch.equal to ops.earth_mover_distance;
    (2) dp, dq at rel L2 <= 1e-5 of the f64 closed formula evaluated from the GPU's own tape; (3) sum match * dist rebuilt in f64 from
    that tape within 1e-4 relative of the GPU cost; (4) dp, dq at rel L2 <= 1e-3 of the f64 reference run from scratch, the f32 CPU
    restatement's own distance recorded beside it; (5) everything finite, the coincident pairs included; (6) |dp_k| <= |g| multiL (1 + 1e-4),
    |dq_l| <= |g| multiR (1 + 1e-4); (7) points whose f64 match row (column) is exactly zero have an exactly zero gradient."""
    from caspr_amd import ops
    p, q, g = R.clouds(n, m)
    case, bad = "n%d-m%d" % (n, m), []
    pd, qd = p.to(DEV), q.to(DEV)
    want_cost = ops.earth_mover_distance(pd, qd, transpose=False)
    cost_t, tape = ops.earth_mover_distance(pd, qd, transpose=False, return_tape=True)
    cost_bcn, tape_bcn = ops.earth_mover_distance(pd.transpose(1, 2).contiguous(), qd.transpose(1, 2).contiguous(), return_tape=True)
    cost, dp, dq = _run(p, q, g)
    cost_tr, dp_tr, dq_tr = _run(p, q, g, transpose=True)
    torch.cuda.synchronize()
    # (1)
    assert tape.shape == (R.B, 10, n + m) and tape.dtype == torch.float32 and cost_t.shape == (R.B,)
    assert torch.equal(cost_t, want_cost), "the tape entry's cost differs from caspr_emd_f32: %s vs %s" % (cost_t.tolist(), want_cost.tolist())
    assert torch.equal(cost_bcn, want_cost) and torch.equal(tape_bcn, tape)
    assert torch.equal(cost, want_cost) and torch.equal(cost_tr, want_cost)
    assert torch.equal(dp_tr, dp) and torch.equal(dq_tr, dq), "the (b,3,n) layout changes the gradient"
    # (5)
    assert bool(torch.isfinite(tape).all()) and bool(torch.isfinite(cost).all())
    assert bool(torch.isfinite(dp).all()) and bool(torch.isfinite(dq).all())
    # (2)
    tape64 = tape.cpu().double()
    kp, kq = R.grads_from_tape(p, q, tape64, g)
    _l2(bad, case, "dp_vs_own_tape", dp, kp, KERNEL_TOL)
    _l2(bad, case, "dq_vs_own_tape", dq, kq, KERNEL_TOL)
    # (3)
    cost64 = R.cost_from_tape(p, q, tape64)
    terr = float(((cost64 - cost.cpu().double()).abs() / cost.cpu().double().abs()).max())
    REPORT["emd_grad:%s:cost_from_tape" % case] = {"max_rel_err": terr, "bound": TAPE_TOL, "cost_per_point": float((cost64 / n).mean())}
    print("emd_grad:%s:cost_from_tape rel %.3e" % (case, terr))
    if not terr <= TAPE_TOL:
        bad.append("%s: the cost rebuilt from the tape is %.3e relative from the GPU cost" % (case, terr))
    # (4)
    _, match, _, rp, rq = R.reference(n, m)
    sp, sq = R.restatement_f32(n, m)
    _l2(bad, case, "dp", dp, rp, E2E_TOL, f32_cpu_restatement_rel_l2=R.rel_l2(sp, rp))
    _l2(bad, case, "dq", dq, rq, E2E_TOL, f32_cpu_restatement_rel_l2=R.rel_l2(sq, rq))
    # (6)
    multiL, multiR = R.multipliers(n, m)
    gabs = g.abs()[:, None].double()
    np_, nq_ = dp.cpu().double().norm(dim=2), dq.cpu().double().norm(dim=2)
    REPORT["emd_grad:%s:norm_over_bound" % case] = {"dp": float((np_ / (gabs * multiL)).max()), "dq": float((nq_ / (gabs * multiR)).max())}
    if not bool((np_ <= gabs * multiL * (1 + 1e-4)).all()):
        bad.append("%s: |dp_k| reaches %.6f |g| multiL" % (case, float((np_ / (gabs * multiL)).max())))
    if not bool((nq_ <= gabs * multiR * (1 + 1e-4)).all()):
        bad.append("%s: |dq_l| reaches %.6f |g| multiR" % (case, float((nq_ / (gabs * multiR)).max())))
    # (7)
    zr, zc = match.sum(2) == 0, match.sum(1) == 0
    REPORT["emd_grad:%s:zero_rows" % case] = {"rows": int(zr.sum()), "columns": int(zc.sum())}
    if float(dp.cpu()[zr].abs().sum()) != 0.0 or float(dq.cpu()[zc].abs().sum()) != 0.0:
        bad.append("%s: a point without any match has a gradient" % case)
    _flush()
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------
# GPU, once
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_point_without_match_has_exactly_zero_gradient():
    """The built (5, 3) case of emd_grad_ref.cluster_clouds: p's fifth point has an exactly zero match row in f64; its gradient is exactly
    zero, the four others' is not, and dp, dq hold the kernel's and the end-to-end bounds."""
    p, q, g = R.cluster_clouds()
    _, match, _, rp, rq = R.reference_grads(p, q, g)
    assert bool((match.sum(2)[:, 4] == 0).all())
    from caspr_amd import ops
    _, tape = ops.earth_mover_distance(p.to(DEV), q.to(DEV), transpose=False, return_tape=True)
    _, dp, dq = _run(p, q, g)
    assert float(dp[:, 4].abs().max()) == 0.0, dp[:, 4].tolist()
    assert bool((dp[:, :4].norm(dim=2) > 0).all())
    bad = []
    kp, kq = R.grads_from_tape(p, q, tape.cpu().double(), g)
    _l2(bad, "cluster-n5-m3", "dp_vs_own_tape", dp, kp, KERNEL_TOL)
    _l2(bad, "cluster-n5-m3", "dq_vs_own_tape", dq, kq, KERNEL_TOL)
    _l2(bad, "cluster-n5-m3", "dp", dp, rp, E2E_TOL)
    _l2(bad, "cluster-n5-m3", "dq", dq, rq, E2E_TOL)
    _flush()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_needs_grad_combinations_reproducibility_and_double_backward():
    """(255, 257): with only p or only q requiring grad the other gradient is None and the computed one keeps the bits of the run where
    both do; two backward runs are bit-identical, through autograd and through train_ops.emd_bwd; a tape of another shape is refused; a
    double backward raises."""
    from caspr_amd import losses, ops
    from caspr_amd import train_ops as T
    p, q, g = R.clouds(255, 257)
    _, dp, dq = _run(p, q, g)
    _, dp_only, none_q = _run(p, q, g, q_grad=False)
    _, none_p, dq_only = _run(p, q, g, p_grad=False)
    assert none_q is None and torch.equal(dp_only, dp), "dp changes when q needs no gradient"
    assert none_p is None and torch.equal(dq_only, dq), "dq changes when p needs no gradient"
    _, dp2, dq2 = _run(p, q, g)
    assert torch.equal(dp2, dp) and torch.equal(dq2, dq), "two backward runs differ"
    pd, qd, gd = p.to(DEV), q.to(DEV), g.to(DEV)
    _, tape = ops.earth_mover_distance(pd, qd, transpose=False, return_tape=True)
    a, b = T.emd_bwd(pd, qd, tape, gd), T.emd_bwd(pd, qd, tape, gd)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], dp) and torch.equal(a[1], dq)
    assert T.emd_bwd(pd, qd, tape, gd, want_p=False, want_q=False) == (None, None)
    with pytest.raises(ValueError, match="tape"):
        T.emd_bwd(pd, qd, tape[:, :9].contiguous(), gd)
    pg = pd.clone().requires_grad_(True)
    cost = losses.earth_mover_distance(pg, qd, transpose=False)
    gr, = torch.autograd.grad(cost.sum(), pg, create_graph=True)
    with pytest.raises(RuntimeError):
        gr.sum().backward()


@pytest.mark.gpu
def test_emd_loss_reductions():
    """emd_loss is cost / N of ops.earth_mover_distance reduced by torch, to 1e-6 relative: "none", "sum", "mean", and (B,T,N,3) inputs."""
    from caspr_amd import losses, ops
    p, q, _ = R.clouds(255, 257)
    pd, qd = p.to(DEV), q.to(DEV)
    want = ops.earth_mover_distance(pd, qd, transpose=False) / 255
    close = lambda a, b: bool(((a - b).abs() <= 1e-6 * b.abs()).all())
    per = losses.emd_loss(pd, qd, reduction="none")
    assert per.shape == (R.B,) and close(per, want)
    per4 = losses.emd_loss(pd.view(1, R.B, 255, 3), qd.view(1, R.B, 257, 3), reduction="none")
    assert per4.shape == (1, R.B) and close(per4[0], want)
    assert close(losses.emd_loss(pd, qd, reduction="sum"), want.sum()) and close(losses.emd_loss(pd, qd), want.mean())
    assert close(losses.emd_loss(pd.view(1, R.B, 255, 3), qd.view(1, R.B, 257, 3)), want.mean())
    assert losses.emd_loss(pd, qd).dim() == 0


@pytest.mark.gpu
def test_no_match_matrix_is_allocated():
    """B = 8, n = m = 1024: forward + backward raise torch's peak allocation by less than an eighth of what the eight match matrices
    would take (32 MB; the tape is 0.66 MB, the two gradients 0.2 MB)."""
    from caspr_amd import losses
    Bn, n = 8, 1024
    gen = torch.Generator().manual_seed(R.SEED)
    pd = torch.rand(Bn, n, 3, generator=gen).to(DEV).requires_grad_(True)
    qd = torch.rand(Bn, n, 3, generator=gen).to(DEV).requires_grad_(True)
    losses.earth_mover_distance(pd[:1].detach(), qd[:1].detach(), transpose=False)      # the workspace cache is allocated outside the measurement
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    losses.earth_mover_distance(pd, qd, transpose=False).sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    REPORT["emd_grad:memory:B8-n1024-m1024"] = {"peak_rise_bytes": rise, "bound_bytes": Bn * n * n * 4 // 8, "match_matrices_bytes": Bn * n * n * 4}
    _flush()
    assert rise < Bn * n * n * 4 / 8, rise
    assert bool(torch.isfinite(pd.grad).all()) and bool(torch.isfinite(qd.grad).all())


def _flow_case(seeded_sd):
    from test_cnf_sample_grad import _model
    m = _model(seeded_sd, 2)
    z, y = rnd(9901, 1, 2, 1600).to(DEV), rnd(9902, 1, 2, 128, 3).to(DEV)
    return m, z, y


@pytest.mark.gpu
def test_fit_latent_on_the_emd(seeded_sd):
    """fit_latent(loss="emd"), four Adam steps on the small model and shapes of test_chamfer_grad.py's fit test: every loss finite, the
    last below the first, and every step's recorded loss IS emd_loss of that step's decode -- a callable that forwards to emd_loss and keeps
    what it was given sees the same values, and emd_loss of each kept decode gives them again."""
    from caspr_amd import losses
    from caspr_amd.utils.fit import fit_latent
    m, z_true, y = _flow_case(seeded_sd)
    with torch.no_grad():
        target = m.decode(z_true, 128, y=y)[2].contiguous()
    z_init = z_true + 0.05 * rnd(9904, 1, 2, 1600).to(DEV)
    z, curve = fit_latent(m, target, z_init, 128, steps=4, y=y, loss="emd")
    seen = []

    def spy(x, t):
        seen.append(x.detach().clone())
        return losses.emd_loss(x, t)

    z2, curve2 = fit_latent(m, target, z_init, 128, steps=4, y=y, loss=spy)
    torch.cuda.synchronize()
    REPORT["emd_grad:fit_latent:loss_curve"] = {"loss": curve}
    _flush()
    assert len(curve) == 4 and all(c == c and abs(c) != float("inf") for c in curve), curve
    assert curve2 == curve and torch.equal(z2, z) and len(seen) == 4
    assert [float(losses.emd_loss(x, target)) for x in seen] == curve
    assert curve[-1] < curve[0], curve
    assert not z.requires_grad and not torch.equal(z, z_init)
    assert all(p_.grad is None for p_ in m.parameters())


@pytest.mark.gpu
def test_fit_latent_default_is_the_chamfer_fit(seeded_sd):
    """Without `loss`, fit_latent returns the bits of loss="chamfer": z and every recorded loss."""
    from caspr_amd.utils.fit import fit_latent
    m, z_true, y = _flow_case(seeded_sd)
    with torch.no_grad():
        target = m.decode(z_true, 128, y=y)[2].contiguous()
    z_init = z_true + 0.05 * rnd(9904, 1, 2, 1600).to(DEV)
    za, ca = fit_latent(m, target, z_init, 128, steps=3, y=y)
    zb, cb = fit_latent(m, target, z_init, 128, steps=3, y=y, loss="chamfer")
    assert torch.equal(za, zb) and ca == cb and len(ca) == 3
