"""Training through the adaptive Dormand-Prince solve of the latent ODE (config.train_latent_dopri5; train/flow_grad.py: LatentSolveDopri5;
include/caspr_hip_train.h: caspr_latent_dopri5_tape_f32, caspr_latent_dopri5_adjoint_f32; csrc/ode_latent_dp5.hip, ode_latent_dp5_adjoint.inc).

The gradient is the one of the forward's own discrete map with its accepted steps held fixed, so the reference is torch autograd in f64
through test_latent_dopri5.replay at the kernel's OWN traced attempts (tests/latent_dp5_grad_ref.py):

  * forward: out, trace and counters of the taping launch are the bits of ops.latent_dopri5 on the same arguments;
  * gradients: dL/dz0 and the eight parameter gradients of L = sum(out * wgt) are within bound = max(3e-5, 4 x |ref32 - ref64|) of the f64
    reference, per tensor, in the measure max |got - want| / |want|max.  3e-5 is what the suite holds the RK4 node to against f64
    (test_hip_train.py: latent_node_vs_f64_*); the second term is the reference's own f32 arithmetic on the same attempts, with the
    margin measure_delta gives f32 against f64 in this family;
  * on the CPU the reference is tied to a central finite difference of replay (f64, frozen dt's), and the comparison is shown to have
    teeth: the same gradient with k7 detached inside the interpolant misses every tensor's bound;
  * the matrix's inputs, run through the oracle's f32 solver on the CPU, hold a rejected attempt, an accepted step with several stamps
    inside, a stamp equal to times[0], a repeated stamp, and no sequence above the 64 steps of the default tape.

Every error and bound lands in the training parity report (train_parity_report.json) under latent_dopri5_grad:<case>:<tensor>.

Three one-line mutations of the reverse sweep (csrc/ode_latent_dp5_adjoint.inc), tried on the GPU once each.  Each makes the same six tests
fail -- test_gradients on all five cases and test_gradients_from_the_repeated_and_first_stamps_alone -- and leaves the forward bits, the
no-attempt case and the bitwise independence / determinism checks passing, as it must (none of them reads a value of the gradient):
  1. the k7 term of the interpolant dropped (the `ab += ...` line removed);
  2. one solution weight changed (LDP_BETA[7][0] doubled in the z_{n+1} combination);
  3. an inside-step stamp's gout sent to z_{n+1} only (`if (tn == t1)` -> `if (true)`).
"""
import functools
import os

import pytest
import torch

import latent_dp5_grad_ref as R
from test_cnf_dopri5 import same_bits
from test_latent_dopri5 import BASE_STAMPS, oracle_run, problem, rel_of, replay, rnd, sequences, stamps, traced, width_name
from test_latent_widths import module, net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (name, weights, tolerance, horizon, first stamp, sequences): the reference tolerance on the seeded weights over more than one workgroup
# (17 = 16 + 1 columns); the stress weights where steps are many and rejected; one sequence alone; two other widths the kernels accept
# (a ragged K chunk and two output row tiles; three output row tiles and 16 hidden row tiles)
CASES = [("seeded-1e-3", "seeded", 1e-3, 1.0, 0.0, 17), ("stress-1e-5", "stress", 1e-5, 3.0, 0.25, 5), ("stress-1e-6", "stress", 1e-6, 3.0, 0.25, 1),
         ("D20H512-1e-6", (20, 512), 1e-6, 3.0, 0.25, 5), ("D33H256-1e-6", (33, 256), 1e-6, 3.0, 0.25, 5)]
SEEDS = {c[0]: 300 + i for i, c in enumerate(CASES)}
SLICED = "seeded-1e-3"            # this case's z0 is a column slice of a wider tensor
SPECIAL = "stress-1e-6"           # ... and this one runs once more with wgt non-zero only at the repeated and the times[0] stamps
SPECIAL_STAMPS = [1, 3, 4]        # BASE_STAMPS: index 1 equals times[0], 3 and 4 repeat


def width_of(which):
    return (64, 512) if isinstance(which, str) else which


def sd_of(which, seeded_sd, stress_sd):
    return {"seeded": seeded_sd, "stress": stress_sd}[which] if isinstance(which, str) else net(*which)


def inputs(case):
    name, which, tol, horizon, t_first, B = case
    D, _ = width_of(which)
    return sequences(SEEDS[name], B, D), stamps(horizon, t_first), rnd(SEEDS[name] + 50, B, len(BASE_STAMPS), D)


def special_wgt(wgt):
    out = torch.zeros_like(wgt)
    out[:, SPECIAL_STAMPS] = wgt[:, SPECIAL_STAMPS]
    return out


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_surface():
    """The two entry points are declared and bound, the source is built, the option is off by default and the tape holds 64 steps."""
    from caspr_amd import lib
    from caspr_amd.config import KernelConfig, load
    from caspr_amd.csrc import build
    from caspr_amd.models.latent_ode_model import LatentODE
    hdr = open(os.path.join(ROOT, "include", "caspr_hip_train.h")).read()
    for sym, nargs in (("caspr_latent_dopri5_tape_f32", 25), ("caspr_latent_dopri5_adjoint_f32", 33)):
        assert sym + "(" in hdr and sym in lib.SIGNATURES and len(lib.SIGNATURES[sym][1]) == nargs, sym
    # the reverse sweep is a text fragment of the solve's translation unit, which is in the list of sources and depends on it
    csrc = os.path.join(ROOT, "caspr_amd", "csrc")
    assert "ode_latent_dp5.hip" in build.SOURCES and '#include "ode_latent_dp5_adjoint.inc"' in open(os.path.join(csrc, "ode_latent_dp5.hip")).read()
    assert os.path.join(csrc, "ode_latent_dp5_adjoint.inc") in [os.path.abspath(d) for d in build.deps()]
    assert 'extern "C" int caspr_latent_dopri5_adjoint_f32(' in open(os.path.join(csrc, "ode_latent_dp5_adjoint.inc")).read()
    assert KernelConfig().train_latent_dopri5 is False
    assert load({"CASPR_DEBUG": "1", "CASPR_TRAIN_LATENT_DP5": "1"}).train_latent_dopri5 is True
    assert LatentODE().train_max_steps == 64


@pytest.mark.parametrize("which,tol,horizon,t_first", [("seeded", 1e-3, 1.0, 0.0), ("stress", 1e-5, 3.0, 0.25)])
def test_reference_is_the_derivative_of_the_frozen_replay(which, tol, horizon, t_first, seeded_sd, stress_sd):
    """grads() against a central finite difference of replay at the same frozen dt's and decisions, f64, on random directions of z0 and of
    one weight: 1e-6 relative (step 1e-6: truncation ~1e-12 x the third derivative, rounding ~1e-16 / 1e-6), and frozen() -- the map from
    the accepted steps alone -- has the same gradient to 1e-10."""
    sd = sd_of(which, seeded_sd, stress_sd)
    z0 = sequences(411, 2)
    rel = rel_of(stamps(horizon, t_first))
    wgt = rnd(412, 2, len(rel), 64).double()
    runs = [replay(*problem(sd, z0[b]), rel, tol, tol) for b in range(2)]
    dts, acc = [r["dts"] for r in runs], [r["accepted"] for r in runs]
    g = R.grads(sd, z0, rel, tol, tol, dts, acc, wgt)
    gf = R.grads(sd, z0, rel, tol, tol, dts, acc, wgt, solve=lambda f, z, b: R.frozen(f, z, rel, dts[b], acc[b]))
    for nm, a, b in zip(R.NAMES, gf, g):
        assert R.err(a, b) <= 1e-10, (nm, R.err(a, b))
    key = "latent_ode.ode_func.dynamics_net.2.weight"

    def loss(dz, dw):
        w = {k: v.double() for k, v in sd.items() if k.startswith("latent_ode.ode_func.dynamics_net")}
        w[key] = w[key] + dw
        tot = 0.0
        with torch.no_grad():
            for b in range(2):
                out = torch.cat(replay(lambda z: R.O.dynamics(w, z), (z0[b].double() + dz[b]).reshape(1, -1), rel, tol, tol, dts=dts[b], decisions=acc[b])["out"], 0)
                tot += float((out * wgt[b]).sum())
        return tot
    eps = 1e-6
    for s in range(3):
        vz, vw = rnd(420 + s, 2, 64).double(), rnd(430 + s, 512, 512).double() / 512 ** 0.5
        for dz, dw, want in ((vz, 0 * vw, float((g[0] * vz).sum())), (0 * vz, vw, float((g[3] * vw).sum()))):
            fd = (loss(eps * dz, eps * dw) - loss(-eps * dz, -eps * dw)) / (2 * eps)
            assert abs(fd - want) <= 1e-6 * max(abs(want), 1e-3), (s, fd, want)


@pytest.mark.parametrize("which,tol,horizon,t_first,B", [("seeded", 1e-3, 1.0, 0.0, 3), ("stress", 1e-5, 3.0, 0.25, 2)])
def test_comparison_has_teeth(which, tol, horizon, t_first, B, seeded_sd, stress_sd):
    """On the oracle's f32 attempts in the kernel's place: the f32 reference is inside every tensor's bound by construction (a factor 4);
    the gradient with k7 detached inside the interpolant is outside every one."""
    sd = sd_of(which, seeded_sd, stress_sd)
    z0 = sequences(441, B)
    rel = rel_of(stamps(horizon, t_first))
    wgt = rnd(442, B, len(rel), 64)
    dts, acc = [], []
    for b in range(B):
        _, _, ratios, d = oracle_run(*problem(sd, z0[b], torch.float32), rel, tol, tol)
        dts.append(d)
        acc.append([r[0] <= 1 for r in ratios])
    g64 = R.grads(sd, z0, rel, tol, tol, dts, acc, wgt)
    g32 = R.grads(sd, z0, rel, tol, tol, dts, acc, wgt, dtype=torch.float32)
    bad = R.grads(sd, z0, rel, tol, tol, dts, acc, wgt, solve=lambda f, z, b: R.frozen(f, z, rel, dts[b], acc[b], detach_k7=True))
    for nm, a32, a64, v in zip(R.NAMES, g32, g64, bad):
        bd = R.bound(a32, a64)
        print("%s %s: f32 %.3e, bound %.3e, k7 detached %.3e" % (which, nm, R.err(a32, a64), bd, R.err(v, a64)))
        assert R.err(a32, a64) <= bd < R.err(v, a64), (nm, R.err(a32, a64), bd, R.err(v, a64))


def test_matrix_exercises_what_it_claims(seeded_sd, stress_sd):
    """The GPU matrix's inputs through the oracle's f32 solver: a rejected attempt, an accepted step with several stamps inside, a stamp
    equal to times[0] and a repeat, and no sequence above the 64 accepted steps of the default tape."""
    assert BASE_STAMPS[1] == BASE_STAMPS[0] and BASE_STAMPS[3] == BASE_STAMPS[4]
    rejected = several = False
    most = 0
    for case in CASES:
        name, which, tol, horizon, t_first, B = case
        sd = sd_of(which, seeded_sd, stress_sd)
        z0, times, _ = inputs(case)
        rel = rel_of(times)
        assert rel[1] == 0.0 and rel[3] == rel[4]
        for b in range(B):
            _, _, ratios, dts = oracle_run(*problem(sd, z0[b], torch.float32), rel, tol, tol)
            acc = [r[0] <= 1 for r in ratios]
            rejected = rejected or not all(acc)
            most = max(most, sum(acc))
            ends, t = [], 0.0
            for d, a in zip(dts, acc):
                if a:
                    t += d
                    ends.append(t)
            several = several or any(sum(1 for x in set(rel) if lo < x < hi) >= 2 for lo, hi in zip([0.0] + ends[:-1], ends))
    assert rejected and several and most <= 64, (rejected, several, most)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lats(dev, seeded_sd, stress_sd):
    from caspr_amd.models import CaSPR
    out = {}
    for name, sd in (("seeded", seeded_sd), ("stress", stress_sd)):
        m = CaSPR(latent_method="dopri5")
        m.load_state_dict(sd)
        out[name] = m.to(dev).eval().latent_ode
    for D, H in ((20, 512), (33, 256)):
        out[(D, H)] = module(D, H, dev, method="dopri5")
    return out


def wb_of(lat):
    return [x for i in (0, 2, 4, 6) for x in (lat.ode_func.dynamics_net[i].weight, lat.ode_func.dynamics_net[i].bias)]


def node(lat, z0, times, tol, wgt, dev, max_steps=64, sliced=False):
    """One forward + backward of the node -> (out, info, [dz0, dw0, db0, .., dw3, db3]) on the CPU."""
    from caspr_amd.train import flow_grad as FG
    if sliced:
        wide = torch.cat([z0, rnd(9, z0.shape[0], 7)], 1).to(dev).requires_grad_(True)
        leaf, z = wide, wide[:, :z0.shape[1]]
    else:
        leaf = z = z0.to(dev).requires_grad_(True)
    wb = wb_of(lat)
    out = FG.LatentSolveDopri5.apply(z, times.to(dev), tol, tol, 1000, max_steps, *wb)
    info = FG.LatentSolveDopri5.last_info
    g = torch.autograd.grad((out * wgt.to(dev)).sum(), [leaf] + wb)
    torch.cuda.synchronize()
    gz = g[0][:, :z0.shape[1]] if sliced else g[0]
    assert not sliced or bool((g[0][:, z0.shape[1]:] == 0).all())
    return out.detach().cpu(), {k: v.cpu() for k, v in info.items()}, [gz.cpu()] + [x.cpu() for x in g[1:]]


@pytest.fixture(scope="module")
def runs(dev, lats, seeded_sd, stress_sd):
    """Every case once: the node's forward and backward, and the f64 / f32 references on the kernel's own traced attempts."""
    from caspr_amd import ops
    ops.check_deferred_errors()
    res = {}
    for case in CASES:
        name, which, tol, horizon, t_first, B = case
        z0, times, wgt = inputs(case)
        out, info, g = node(lats[which], z0, times, tol, wgt, dev, sliced=name == SLICED)
        ops.check_deferred_errors()
        tr = [traced(info, b) for b in range(B)]
        sd, rel = sd_of(which, seeded_sd, stress_sd), rel_of(times)
        ref = functools.partial(reference, sd, z0, rel, tol, tr)
        res[name] = dict(case=case, z0=z0, times=times, wgt=wgt, out=out, info=info, g=g, g64=ref(wgt, torch.float64), g32=ref(wgt, torch.float32), ref=ref)
    return res


def reference(sd, z0, rel, tol, tr, wgt, dtype):
    """R.grads on the traced attempts tr of every sequence."""
    return R.grads(sd, z0, rel, tol, tol, [t["dts"] for t in tr], [t["accepted"] for t in tr], wgt, dtype=dtype)


def compare(tag, g, g32, g64):
    from test_hip_train import rel
    bad = []
    for nm, a, a32, a64 in zip(R.NAMES, g, g32, g64):
        bd = R.bound(a32, a64)
        print("  %s %s: err %.3e, bound %.3e (f32 reference %.3e)" % (tag, nm, R.err(a, a64), bd, R.err(a32, a64)))
        try:
            rel("latent_dopri5_grad:%s:%s" % (tag, nm), a, a64, bd)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_forward_bits(name, runs, lats, dev):
    """out, trace and counters of the taping launch equal ops.latent_dopri5(return_trace=True) under no_grad, bit for bit."""
    from caspr_amd import ops
    r = runs[name]
    _, which, tol, _, _, B = r["case"]
    with torch.no_grad():
        want, winfo = ops.latent_dopri5(r["z0"].to(dev), r["times"].to(dev), tol, tol, lats[which]._weights(), return_trace=True)
    torch.cuda.synchronize()
    assert same_bits(r["out"], want.cpu()) and bool(torch.isfinite(r["out"]).all())
    for k, v in winfo.items():
        assert same_bits(r["info"][k], v.cpu()) if v.dtype.is_floating_point else torch.equal(r["info"][k], v.cpu()), k
    assert int(r["info"]["accepted"].min()) >= 1 and int(r["info"]["accepted"].max()) <= 64


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_gradients(name, runs):
    """dL/dz0 and the eight parameter gradients against the f64 reference on the kernel's own traced attempts, per tensor."""
    r = runs[name]
    compare(name, r["g"], r["g32"], r["g64"])


@pytest.mark.gpu
def test_gradients_from_the_repeated_and_first_stamps_alone(runs, lats, dev):
    """wgt non-zero only at the stamp equal to times[0] and at the two repeated stamps."""
    r = runs[SPECIAL]
    _, which, tol, _, _, _ = r["case"]
    wgt = special_wgt(r["wgt"])
    out, info, g = node(lats[which], r["z0"], r["times"], tol, wgt, dev)
    assert same_bits(out, r["out"])
    compare(SPECIAL + "-special", g, r["ref"](wgt, torch.float32), r["ref"](wgt, torch.float64))


@pytest.mark.gpu
def test_no_attempts(lats, dev):
    """One stamp, and all stamps equal: out is z0, dL/dz0 the summed gout (in f64, rounded once), parameter gradients exactly zero."""
    lat = lats["seeded"]
    z0 = sequences(350, 5)
    for times in (torch.tensor([0.4]), torch.tensor([0.4, 0.4, 0.4])):
        wgt = rnd(351, 5, times.shape[0], 64)
        out, info, g = node(lat, z0, times, 1e-3, wgt, dev)
        assert all(same_bits(out[:, i].contiguous(), z0) for i in range(times.shape[0]))
        assert same_bits(g[0], wgt.double().sum(1).float())
        assert all(bool((x == 0).all()) for x in g[1:])
        assert info["accepted"].tolist() == [0] * 5 and info["nfe"].tolist() == [2] * 5


@pytest.mark.gpu
def test_independence_and_determinism(runs, lats, dev):
    """A sequence's dL/dz0 row has the same bits alone, in the batch of 17 and in another column; two runs give the same parameter bits."""
    r = runs["seeded-1e-3"]
    lat, z0, times, wgt = lats["seeded"], r["z0"], r["times"], r["wgt"]
    _, _, again = node(lat, z0, times, 1e-3, wgt, dev, sliced=True)
    assert all(same_bits(a, b) for a, b in zip(again, r["g"]))
    for b in (3, 16):
        _, _, alone = node(lat, z0[b:b + 1], times, 1e-3, wgt[b:b + 1], dev)
        assert same_bits(alone[0][0], r["g"][0][b]), b
    perm = torch.roll(torch.arange(17), 5)
    _, _, moved = node(lat, z0[perm], times, 1e-3, wgt[perm], dev)
    assert same_bits(moved[0], r["g"][0][perm])


@pytest.mark.gpu
def test_tape_capacity(lats, dev):
    """train_max_steps = 2 on the stress weights: the deferred error names the remedy, the reached rows are finite and the others NaN, and
    a backward through it leaves NaN in the unfinished dL/dz0 rows and finite parameter gradients."""
    from caspr_amd import ops
    from caspr_amd.lib import CasprHipError
    ops.check_deferred_errors()
    z0, times = sequences(360, 5), stamps(3.0, 0.25)
    wgt = rnd(361, 5, len(BASE_STAMPS), 64)
    out, info, g = node(lats["stress"], z0, times, 1e-5, wgt, dev, max_steps=2)
    with pytest.raises(CasprHipError, match="train_max_steps"):
        ops.check_deferred_errors()
    ops.check_deferred_errors()                       # reported once
    assert info["accepted"].tolist() == [2] * 5
    rel = rel_of(times)
    for b in range(5):
        k = int(info["accepted"][b] + info["rejected"][b])
        rows = info["attempts"][b, :k].double()
        reached = float((rows[:, 1] * rows[:, 3]).sum())
        assert reached < rel[-1]
        for i, t in enumerate(rel):
            assert bool(torch.isnan(out[b, i]).all()) == (t > reached) and (t > reached or bool(torch.isfinite(out[b, i]).all())), (b, i, t, reached)
    assert bool(torch.isnan(g[0]).all()) and all(bool(torch.isfinite(x).all()) for x in g[1:])
    out, info, g = node(lats["stress"], z0, times, 1e-5, wgt, dev)      # usable afterwards, with the default tape
    ops.check_deferred_errors()
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(x).all()) for x in g)


@pytest.mark.gpu
def test_model(dev, seeded_sd, monkeypatch):
    """With the switch on CaSPR(latent_method="dopri5") trains: the codes under autograd are the no_grad codes bit for bit, _forward_train
    + backward leaves finite non-zero gradients on the dynamics net and the encoder, get_nfe()[0] is the counters' maximum.  Off: raises."""
    from caspr_amd import ops
    from caspr_amd.models import CaSPR, latent_ode_model as LM
    from caspr_amd.utils.synthetic import dense_sequences
    m = CaSPR(latent_method="dopri5")
    m.load_state_dict(seeded_sd)
    m = m.to(dev).train()
    x, sp = dense_sequences(2, 3, 1024)
    x, sp = x.to(dev), sp.to(dev)
    tt = sp[:, :, 0, 3].contiguous()
    assert LM.TRAIN_DOPRI5 is False
    with pytest.raises(ValueError, match="dopri5"):
        m._forward_train(x, sp)
    monkeypatch.setattr(LM, "TRAIN_DOPRI5", True)
    with torch.no_grad():
        z0, _ = m.encode(x)
        want = m.aggregate_and_solve_latent(z0, tt)
    codes = m.aggregate_and_solve_latent(z0.clone().requires_grad_(True), tt)
    assert codes.requires_grad and same_bits(codes.detach().cpu(), want.cpu())
    assert int(m.get_nfe()[0]) == int(m.latent_ode.last_nfe_per_sequence.max()) >= 8
    m.zero_grad()
    loss = m._forward_train(x, sp)
    sum(l.mean() for l in loss if l is not None).backward()
    ops.check_deferred_errors()
    assert int(m.get_nfe()[0]) == int(m.latent_ode.last_nfe_per_sequence.max()) >= 8
    net_ = m.latent_ode.ode_func.dynamics_net
    enc = next(p for p in m.encoder.parameters() if p.requires_grad)
    for p in (net_[0].weight, net_[6].weight, enc):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
