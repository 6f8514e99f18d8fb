"""The exact EMD on the GPU (caspr_amd/csrc/emd_exact.hip: caspr_emd_exact_f32, caspr_emd_exact_bwd_f32; ops.earth_mover_distance_exact,
losses.exact_earth_mover_distance / emd_exact_loss, utils.evaluations.eval_exact_emd_frames) held to what can be DERIVED, with no solver in
the loop:

  the certificate   cost64(assign) - dual_bound(C, prices) <= n eps (1 + 1e-9), computed on the CPU in f64 from the kernel's own prices
                    (tests/emd_exact_ref.py: weak duality makes dual_bound a lower bound of the optimum for ANY prices, so this holds
                    the kernel to optimality within n eps);
  the restatement   assign and prices equal the numpy f64 restatement's bit for bit (the arithmetic and the tie rules are fully
                    specified);
  the cost          f32 summation of n non-negative terms: within n 2^-23 cost of the f64 sum over assign;
  the gradient      each component within 4 * 2^-23 |g| of torch autograd in f64 of sum_i |p_i - q[assign[i]]| (a ratio of two f32
                    quantities a few roundings from exact, magnitude <= |g|).
Shapes: n = 1, 2, the 64-lane wave edge from both sides, 255 / 256 (several bidders per wave, more bidders than waves), 2048 (the protocol
size, more bidders than threads in the first round of a phase).  The errors go to the parity report under emd_exact:<case>:<tensor>."""
import ctypes
import re

import numpy as np
import pytest
import torch

import emd_exact_ref as R
from test_hip_parity import REPORT, record, rnd

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-6
U23 = 2.0 ** -23
_CASES = {}

# name -> (generator, n, scale, eps, compare with the CPU restatement bit for bit)
EDGES = dict([("uniform-n%d" % n, (R.uniform, n, 1.0, EPS, True)) for n in (1, 2, 63, 64, 65, 255, 256)] + [
    ("identical-n65", ("identical", 65, 1.0, EPS, True)),
    ("permuted-n255", (R.permuted, 255, 1.0, EPS, True)),
    ("duplicated16-n256", (R.duplicated, 256, 1.0, EPS, False)),     # a price war: tens of thousands of rounds are the GPU's to run
    ("clustered-n256", (R.clustered, 256, 1.0, EPS, True)),
    ("scaled100-n65", (R.uniform, 65, 100.0, 1e-4, True)),
])


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    from caspr_amd import ops as _ops
    return _ops


def clouds(name, B=3):
    """-> p, q (B,n,3) f32 numpy, eps; computed once per case and left unchanged."""
    if (name, B) not in _CASES:
        gen, n, scale, eps, _ = EDGES[name]
        if gen == "identical":
            p = R.uniform(n, B, 1000 + n)[0]
            q = p.copy()
        else:
            p, q = gen(n, B, 1000 + n)
        _CASES[(name, B)] = ((p * np.float32(scale)).astype(np.float32), (q * np.float32(scale)).astype(np.float32), eps)
    return _CASES[(name, B)]


def run(ops, p, q, eps=EPS, **kw):
    out = ops.earth_mover_distance_exact(torch.from_numpy(p).to(DEV), torch.from_numpy(q).to(DEV), transpose=False, eps=eps, return_match=True, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def check_frame(case, b, p, q, eps, cost, assign, prices, info):
    """the permutation, the status, the cost and the certificate of one frame; -> the certificate's gap"""
    n = p.shape[0]
    assert R.is_permutation(assign), "%s frame %d: assign is not a permutation" % (case, b)
    assert info[0] == 1, "%s frame %d: info %s" % (case, b, info)
    C = R.cost_matrix(p, q)
    cost64 = R.primal(C, assign)
    gap = cost64 - R.dual_bound(C, prices)
    print("emd_exact:%s frame %d: cost %.9g, f32 sum off by %.3e (bound %.3e), certificate gap %.3e (bound %.3e), info %s"
          % (case, b, cost64, abs(float(cost) - cost64), n * U23 * cost64, gap, n * eps, info.tolist()))
    assert abs(float(cost) - cost64) <= n * U23 * cost64, "%s frame %d: cost %r vs %r" % (case, b, float(cost), cost64)
    assert gap <= n * eps * (1 + 1e-9), "%s frame %d: certificate gap %.6e > n eps = %.6e" % (case, b, gap, n * eps)
    return gap, cost64


@pytest.mark.parametrize("case", list(EDGES))
def test_edges_hold_the_certificate_and_match_the_restatement(ops, case):
    p, q, eps = clouds(case)
    n = p.shape[1]
    cost, assign, prices, info = run(ops, p, q, eps)
    gaps, costs = zip(*[check_frame(case, b, p[b], q[b], eps, cost[b], assign[b], prices[b], info[b]) for b in range(p.shape[0])])
    REPORT["emd_exact:%s:certificate" % case] = {"max_gap": max(gaps), "bound": n * eps, "rounds": info[:, 2].tolist(), "bids": info[:, 3].tolist()}
    want64 = np.array(costs)
    record("emd_exact:%s:cost" % case, cost.astype(np.float64), want64, n * U23 * float(want64.max()))
    if case.startswith("identical"):
        assert (cost == 0).all() and (assign == np.arange(n)[None, :]).all(), "identical clouds: cost exactly 0 and the identity"
        from caspr_amd import losses
        pd, qd = torch.from_numpy(p).to(DEV).requires_grad_(True), torch.from_numpy(q).to(DEV).requires_grad_(True)
        losses.exact_earth_mover_distance(pd, qd, transpose=False, eps=eps).sum().backward()
        assert float(pd.grad.abs().max()) == 0 and float(qd.grad.abs().max()) == 0, "a coincident pair contributes zero"
    if EDGES[case][4]:
        bad_a = bad_p = 0
        for b in range(p.shape[0]):
            a_ref, p_ref, i_ref = R.auction(p[b], q[b], eps)
            bad_a += int((a_ref != assign[b]).sum())
            bad_p += int((p_ref.view(np.int64) != prices[b].view(np.int64)).sum())
            assert (i_ref == info[b]).all(), "%s frame %d: info %s, the restatement's %s" % (case, b, info[b], i_ref)
        REPORT["emd_exact:%s:assign" % case] = {"mismatches": bad_a, "count": assign.size}
        REPORT["emd_exact:%s:prices" % case] = {"mismatches": bad_p, "count": prices.size}
        assert bad_a == 0 and bad_p == 0, "%s: %d assign and %d price words differ from the restatement's" % (case, bad_a, bad_p)


def test_protocol_size_holds_the_certificate(ops):
    n = 2048
    p = np.stack([R.uniform(n, 1, 2048)[0][0], R.clustered(n, 1, 2049)[0][0]])
    q = np.stack([R.uniform(n, 1, 2048)[1][0], R.clustered(n, 1, 2049)[1][0]])
    cost, assign, prices, info = run(ops, p, q)
    gaps = [check_frame("n2048", b, p[b], q[b], EPS, cost[b], assign[b], prices[b], info[b])[0] for b in range(2)]
    REPORT["emd_exact:n2048:certificate"] = {"max_gap": max(gaps), "bound": n * EPS, "rounds": info[:, 2].tolist(), "bids": info[:, 3].tolist(),
                                             "phases": info[:, 1].tolist()}
    record("emd_exact:n2048:gap", np.array(gaps), np.zeros(2), n * EPS * (1 + 1e-9))


def test_optimum_by_enumeration(ops):
    """n <= 7, 20 random frames in one batch per n: cost64(assign) - brute-force optimum lies in [0, n eps]."""
    worst = 0.0
    for n in (3, 5, 7):
        p, q = R.uniform(n, 20, 70 + n)
        cost, assign, prices, info = run(ops, p, q)
        for b in range(20):
            C = R.cost_matrix(p[b], q[b])
            over = R.primal(C, assign[b]) - R.brute_force(C)
            worst = max(worst, over)
            assert info[b, 0] == 1 and -1e-12 <= over <= n * EPS, "n = %d frame %d: %.3e above the optimum" % (n, b, over)
    record("emd_exact:enumeration:above_optimum", np.array([worst]), np.zeros(1), 7 * EPS)


def test_a_frame_is_a_function_of_the_frame(ops):
    p, q = R.uniform(255, 5, 4242)
    batch = run(ops, p, q)
    again = run(ops, p, q)
    alone = run(ops, p[3:4], q[3:4])
    for name, a, b2, c in zip(("cost", "assign", "prices", "info"), batch, again, alone):
        assert a.tobytes() == b2.tobytes(), "%s differs between two runs" % name
        assert a[3:4].tobytes() == c.tobytes(), "%s of frame 3 differs from the frame alone" % name
    assert (batch[3][:, 0] == 1).all()


def test_the_budget_stops_a_frame_and_reports_it(ops):
    p, q = R.uniform(64, 3, 64064)
    cost, assign, prices, info = run(ops, p, q, max_bids=64)
    print("emd_exact:budget: info %s" % info.tolist())
    assert (info[:, 0] == 0).all() and np.isnan(cost).all() and (assign == -1).all()
    assert (info[:, 3] <= 64).all() and (info[:, 3] >= 1).all() and (info[:, 2] >= 1).all() and (info[:, 1] == 1).all()
    assert np.isfinite(prices).all()
    cost, assign, prices, info = run(ops, p, q)
    assert (info[:, 0] == 1).all() and np.isfinite(cost).all() and all(R.is_permutation(a) for a in assign)
    # a stopped frame beside converged ones: identical clouds need n bids per phase, an ordinary pair more than ten rounds of them
    p2, q2 = p.copy(), q.copy()
    q2[0], q2[2] = p2[0], p2[2]
    cost, assign, prices, info = run(ops, p2, q2, max_bids=64 * 12)
    assert info[:, 0].tolist() == [1, 0, 1], info.tolist()
    assert cost[0] == 0 and cost[2] == 0 and np.isnan(cost[1]) and (assign[1] == -1).all() and info[1, 3] <= 64 * 12
    assert (assign[0] == np.arange(64)).all() and (assign[2] == np.arange(64)).all()


def test_c_entry_refuses_before_any_launch():
    """The pointers only have to be non-NULL to reach the checks and are never followed."""
    from caspr_amd import lib
    L = lib.load()
    ptr = ctypes.c_void_p(256)
    assert L.caspr_emd_exact_ws_bytes(3, 2048) == 0
    ok = dict(B=2, n=64, eps=1e-6, max_bids=1000, cost=ptr, assign=ptr, prices=ptr, info=ptr, ws_bytes=0)

    def call(**kw):
        a = dict(ok, **kw)
        rc = L.caspr_emd_exact_f32(ptr, ptr, a["B"], a["n"], a["eps"], a["max_bids"], a["cost"], a["assign"], a["prices"], a["info"], None, a["ws_bytes"], None)
        assert rc != 0, kw
        return L.caspr_last_error_string().decode()

    for out in ("cost", "assign", "prices", "info"):
        assert "emd_exact: bad arguments" in call(**{out: None})
    assert "emd_exact: bad arguments" in call(n=0)
    assert "emd_exact: bad arguments" in call(B=0)
    assert re.search(r"emd_exact: n=2049.*2048", call(n=2049))
    assert re.search(r"emd_exact: B=65536.*65535", call(B=65536))
    assert "emd_exact: workspace too small" in call(ws_bytes=-1)
    for eps in (0.0, -1.0, float("inf"), float("nan")):
        assert "emd_exact: eps" in call(eps=eps)
    for mb in (0, -5, 2 ** 31):
        assert "emd_exact: max_bids" in call(max_bids=mb)
    assert L.caspr_emd_exact_bwd_f32(ptr, ptr, ptr, ptr, 2, 64, None, None, None) != 0
    assert "emd_exact_bwd: gxyz1 and gxyz2 are both NULL" in L.caspr_last_error_string().decode()
    assert L.caspr_emd_exact_bwd_f32(ptr, ptr, None, ptr, 2, 64, ptr, ptr, None) != 0
    assert "emd_exact_bwd: bad arguments" in L.caspr_last_error_string().decode()
    assert L.caspr_emd_exact_bwd_f32(ptr, ptr, ptr, ptr, 2, 2049, ptr, ptr, None) != 0
    assert re.search(r"emd_exact_bwd: n=2049.*2048", L.caspr_last_error_string().decode())


def test_layouts(ops):
    p, q = R.uniform(63, 2, 6363)
    pd, qd = torch.from_numpy(p).to(DEV), torch.from_numpy(q).to(DEV)
    got = ops.earth_mover_distance_exact(pd, qd, transpose=False)
    assert got.shape == (2,) and got.dtype == torch.float32
    assert torch.equal(ops.earth_mover_distance_exact(pd.transpose(1, 2).contiguous(), qd.transpose(1, 2).contiguous()), got)    # (b,3,n)
    one = ops.earth_mover_distance_exact(pd[1], qd[1], transpose=False)                                                         # one frame
    assert one.shape == (1,) and torch.equal(one, got[1:2])
    assert torch.equal(ops.earth_mover_distance_exact(pd[1].t().contiguous(), qd[1].t().contiguous()), got[1:2])


@pytest.mark.parametrize("n", [1, 65, 256])
def test_gradient(ops, n):
    from caspr_amd import losses
    p, q = R.uniform(n, 2, 500 + n)
    g = torch.tensor([0.75, -1.5], device=DEV)
    _, assign, _, info = ops.earth_mover_distance_exact(torch.from_numpy(p).to(DEV), torch.from_numpy(q).to(DEV), transpose=False, return_match=True)
    assert bool((info[:, 0] == 1).all())
    a = assign.cpu().long()
    p64, q64 = torch.from_numpy(p).double().requires_grad_(True), torch.from_numpy(q).double().requires_grad_(True)
    dist = (p64 - torch.gather(q64, 1, a[:, :, None].expand(-1, -1, 3))).norm(dim=2)
    (g.cpu().double() * dist.sum(dim=1)).sum().backward()
    near = dist.detach() < 1e-6                                       # (B,n) by point of cloud 1; by point of cloud 2 through assign
    near_q = torch.zeros_like(near).scatter_(1, a, near)
    assert float(near.double().mean()) < 0.01
    tol = (4 * U23 * g.abs().cpu().double())[:, None, None]
    got = {}
    for want_p, want_q in ((True, True), (True, False), (False, True)):
        pd, qd = torch.from_numpy(p).to(DEV).requires_grad_(want_p), torch.from_numpy(q).to(DEV).requires_grad_(want_q)
        cost = losses.exact_earth_mover_distance(pd, qd, transpose=False)
        (g * cost).sum().backward()
        for name, t, want, mask in (("gxyz1", pd, p64.grad, near), ("gxyz2", qd, q64.grad, near_q)):
            if t.grad is None:
                assert not t.requires_grad
                continue
            have = t.grad.cpu().double()
            err = ((have - want).abs() / tol)[~mask]
            key = "emd_exact:grad-n%d-%s%s:%s" % (n, "p" if want_p else "", "q" if want_q else "", name)
            REPORT[key] = {"max_err_over_tol": float(err.max()) if err.numel() else 0.0, "tol": float(tol.max()), "excluded": int(mask.sum())}
            print(key, REPORT[key])
            assert bool(torch.isfinite(have).all()) and (err.numel() == 0 or float(err.max()) <= 1.0), key
            assert got.setdefault(name, t.grad.clone()).equal(t.grad), "%s differs between runs" % name
    record("emd_exact:grad-n%d:flush" % n, torch.zeros(1), torch.zeros(1), 1.0)
    pd = torch.from_numpy(p).to(DEV).requires_grad_(True)
    cost = losses.exact_earth_mover_distance(pd, torch.from_numpy(q).to(DEV), transpose=False)
    w = torch.ones(2, device=DEV, requires_grad=True)                 # a weight that asks for the gradient OF the gradient
    gp, = torch.autograd.grad(cost, pd, grad_outputs=w, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gp.sum().backward()


def test_unconverged_frames_get_nan_gradients(ops, monkeypatch):
    from caspr_amd import losses
    p, q = R.uniform(64, 2, 64064)
    monkeypatch.setattr(ops, "EMD_EXACT_BIDS_PER_POINT", 1)
    pd, qd = torch.from_numpy(p).to(DEV).requires_grad_(True), torch.from_numpy(q).to(DEV).requires_grad_(True)
    cost = losses.exact_earth_mover_distance(pd, qd, transpose=False)
    assert bool(torch.isnan(cost).all())
    cost.sum().backward()
    assert bool(torch.isnan(pd.grad).all()) and bool(torch.isnan(qd.grad).all())


def test_loss_reductions_and_evaluation(ops, monkeypatch):
    from caspr_amd import losses
    from caspr_amd.utils.evaluations import eval_exact_emd_frames
    p, q = R.uniform(65, 4, 6565)
    pd, qd = torch.from_numpy(p).to(DEV), torch.from_numpy(q).to(DEV)
    per = ops.earth_mover_distance_exact(pd, qd, transpose=False) / 65
    assert torch.equal(losses.emd_exact_loss(pd, qd, reduction="none"), per)
    assert torch.equal(losses.emd_exact_loss(pd.view(2, 2, 65, 3), qd.view(2, 2, 65, 3), reduction="none"), per.view(2, 2))
    assert torch.equal(losses.emd_exact_loss(pd, qd), per.mean()) and torch.equal(losses.emd_exact_loss(pd, qd, reduction="sum"), per.sum())
    assert torch.equal(losses.exact_earth_mover_distance(pd.transpose(1, 2).contiguous(), qd.transpose(1, 2).contiguous()), per * 65)
    got = eval_exact_emd_frames(pd, qd)
    assert isinstance(got, np.ndarray) and np.array_equal(got, per.cpu().numpy())
    monkeypatch.setattr(ops, "EMD_EXACT_BIDS_PER_POINT", 1)          # the tiny budget: one round
    with pytest.raises(RuntimeError, match=r"eval_exact_emd_frames: .*frame\(s\) \[0, 1, 2, 3\] of 4"):
        eval_exact_emd_frames(pd, qd)


def test_fit_latent_on_the_exact_emd(seeded_sd):
    """fit_latent(loss=losses.emd_exact_loss), four Adam steps on the small model and shapes of test_emd_grad.py's fit test."""
    from caspr_amd import losses
    from caspr_amd.utils.fit import fit_latent
    from test_emd_grad import _flow_case
    m, z_true, y = _flow_case(seeded_sd)
    before = [p_.detach().clone() for p_ in m.parameters()]
    with torch.no_grad():
        target = m.decode(z_true, 128, y=y)[2].contiguous()
    z_init = z_true + 0.05 * rnd(9904, 1, 2, 1600).to(DEV)
    z, curve = fit_latent(m, target, z_init, 128, steps=4, y=y, loss=losses.emd_exact_loss)
    REPORT["emd_exact:fit_latent:loss_curve"] = {"loss": curve}
    record("emd_exact:fit_latent:flush", torch.zeros(1), torch.zeros(1), 1.0)
    assert len(curve) == 4 and all(c == c and abs(c) != float("inf") for c in curve), curve
    assert curve[-1] < curve[0], curve
    assert not z.requires_grad and not torch.equal(z, z_init)
    assert all(p_.grad is None for p_ in m.parameters()) and all(torch.equal(a, b) for a, b in zip(before, m.parameters()))


@pytest.mark.parametrize("case", ["uniform-n256", "clustered-n256"])
def test_distance_of_the_approximation_is_recorded(ops, case):
    """Recorded, not asserted: (approx - exact) / exact for both approximate routes; the only assertion is that both are finite."""
    p, q, eps = clouds(case)
    pd, qd = torch.from_numpy(p).to(DEV), torch.from_numpy(q).to(DEV)
    exact = ops.earth_mover_distance_exact(pd, qd, transpose=False, eps=eps).double()
    for route in ("frame", "rows"):
        gap = ((ops.earth_mover_distance(pd, qd, transpose=False, route=route).double() - exact) / exact).cpu().numpy()
        REPORT["emd_exact:%s:approx_%s_rel_gap" % (case, route)] = {"rel_gap": gap.tolist()}
        print("emd_exact:%s: (approx[%s] - exact) / exact = %s" % (case, route, gap.tolist()))
        assert np.isfinite(gap).all()
    record("emd_exact:%s:approx_flush" % case, torch.zeros(1), torch.zeros(1), 1.0)
