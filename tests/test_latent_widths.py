"""The latent ODE kernels at every width and batch they accept, against the f64 evaluation of the same map.

caspr_latent_rk4_f32 (one workgroup per 16 sequences: 0 < D <= 64, H <= 512, H % 64 == 0), caspr_latent_rk4_team_f32 and its training
forms _tape / _adjoint (32 workgroups per 16 sequences: D <= 64, H == 512, B <= 64) were run by the suite at D = 64, H = 512 only.
The paths that depend on the width -- the ragged K chunk of layer 0 (KC0 = 2 ceil(D / 32), `d < D` on a partly filled group of four
B-tile rows), RTD = ceil(D / 16) < 4 row tiles of the output layer, RTH < 32 (waves without a row tile), KCH < 32 inside the 4-deep
weight ring, xw = roundup4(D) != D in the tape and the output layer's deltas -- run here.  (The adaptive kernel's widths: the second
route matrix of test_latent_dopri5.py.)

Reference: oracle.model.latent_solve in f64 (size-generic) on weights randn * GAIN / sqrt(fan_in), biases 0.2 randn ON ALL FOUR LAYERS
(init_network_weights zeroes them: a wrong bias row is invisible on every seeded model), z0 = 0.5 randn, horizon 1; for the gradients
f64 torch.autograd through the RK4 map as test_hip_train.py writes it out.  Bounds are the ones the project already holds these
kernels to: |hip - f64| <= 1e-5 max(1, |z|max) (Z_TOL of test_latent_dopri5.py, latent_team_vs_oracle, stress_latent_rk4_*), team
against single-workgroup 5e-6, training 2e-6 / 3e-5 against f64 and 1e-6 / 2e-5 between the two routes (test_hip_train.py), each as
max |got - want| / |want|max (`rel` there).  Where the f32 evaluation of the same map on the CPU (torch) is itself further from f64
than that, 4 x its distance is allowed instead (different association of the K sums, tanhf): both distances are recorded per row
under "latent_widths:" keys of test_hip_parity's JSON report, with the bound in force.

Section 1 needs no GPU: six one-line mutations of the f64 map, each of which must move the last stamp by >= 10 x the bound of section 2
at every (D, H) of the table -- the reference can see what the kernels could get wrong.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import model as O
from test_hip_parity import REPORT, record

PRE = "latent_ode.ode_func.dynamics_net"
GAIN = 1.0                                            # weights randn * GAIN / sqrt(fan_in): section 1 holds at every row (checked on the CPU)
Z_TOL = 1e-5                                          # x max(1, |z|max)
TEAM_VS_SINGLE = 5e-6
DS = (1, 5, 16, 20, 32, 33, 48, 64)
HS = (64, 256, 448, 512)
TIMES = [0.3, 0.3, 0.45, 0.8, 0.8, 1.3]               # a non-zero first stamp, a repeat at the start and one inside; horizon 1
TRAIN_TIMES = [0.2, 0.2, 0.55, 1.0, 1.0]
B_FWD = 5


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def net(D, H, gain=GAIN):
    """f64 state dict of a D -> H -> H -> H -> D dynamics net under the oracle's keys; a function of (D, H, gain) only."""
    seed = 1000 * D + H
    shapes = [(H, D), (H, H), (H, H), (D, H)]
    sd = {}
    for i, (l, (co, ci)) in enumerate(zip((0, 2, 4, 6), shapes)):
        sd["%s.%d.weight" % (PRE, l)] = rnd(seed + 10 * i, co, ci) * gain / math.sqrt(ci)
        sd["%s.%d.bias" % (PRE, l)] = 0.2 * rnd(seed + 10 * i + 1, co)
    # the f32 values ARE the weights: what the kernels are given, exactly representable in the f64 reference
    return {k: v.float().double() for k, v in sd.items()}


def starts(D, B, seed=7):
    return (0.5 * rnd(seed + 100 * D, B, D)).float()


def rel_times(times):
    """The solver's times relative to times[0] in the f32 arithmetic of the kernels (latent_ode_model.py:58), as f64."""
    t = torch.as_tensor(times, dtype=torch.float32)
    return (t - t[0]).double()


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


# ---------------------------------------------------------------------------------------------
# the f64 map with one line changed (section 1); mutation None is oracle.model.dynamics itself
# ---------------------------------------------------------------------------------------------
def late(b):
    """A bias read one row late: row i takes b[i + 1]; the last row reads past the end (zero here)."""
    return torch.cat([b[1:], torch.zeros(1, dtype=b.dtype)])


def applies(mut, D):
    """The output layer's row D - 1 lies in row tile 0 when D <= 16: there `row_tile0` is the unchanged map."""
    return mut != "row_tile0" or D > 16


MUTATIONS = ("last_channel", "ragged_chunk", "hidden_unit", "b0_late", "b3_late", "row_tile0")


def dynamics_mut(sd, z, mut):
    W = [sd["%s.%d.weight" % (PRE, l)] for l in (0, 2, 4, 6)]
    b = [sd["%s.%d.bias" % (PRE, l)] for l in (0, 2, 4, 6)]
    D, H = W[0].shape[1], W[0].shape[0]
    if mut == "last_channel":                          # layer 0 ignores input channel D - 1
        W[0] = W[0].clone()
        W[0][:, D - 1] = 0
    elif mut == "ragged_chunk":                        # layer 0 ignores the whole ragged chunk k >= 16 floor((D - 1) / 16)
        W[0] = W[0].clone()
        W[0][:, 16 * ((D - 1) // 16):] = 0
    elif mut == "b0_late":
        b[0] = late(b[0])
    elif mut == "b3_late":
        b[3] = late(b[3])
    elif mut == "row_tile0":                           # the output layer's row D - 1 computed from row tile 0
        W[3] = W[3].clone()
        W[3][D - 1] = W[3][(D - 1) % 16]
    h = torch.tanh(F.linear(z, W[0], b[0]))
    h = torch.tanh(F.linear(h, W[1], b[1]))
    if mut == "hidden_unit":                           # hidden unit H - 1 of layer 1 is dropped
        h = h.clone()
        h[:, H - 1] = 0
    h = torch.tanh(F.linear(h, W[2], b[2]))
    return F.linear(h, W[3], b[3])


def solve_mut(sd, z0, rel, steps, mut):
    """oracle.model.latent_solve's RK4 loop (rk4_solve per interval) over dynamics_mut."""
    fn = lambda t, ys: (dynamics_mut(sd, ys[0], mut),)
    r = rel.tolist()
    outs, z = [z0], z0
    for k in range(1, len(r)):
        (z,) = O.rk4_solve(fn, (z,), r[k - 1], r[k], steps)
        outs.append(z)
    return torch.stack(outs, dim=1)


_REF = {}


def reference(D, H, B, times, steps, seed=7):
    """-> (sd64, z0 f32 (B, D), f64 solve (B, Tu, D), |f32 on the CPU - f64| max): computed once per key, shared, never written to."""
    key = (D, H, B, tuple(times), steps, seed)
    if key not in _REF:
        sd = net(D, H)
        z0 = starts(D, B, seed)
        rel = rel_times(times)
        w64 = O.latent_solve(sd, z0.double(), rel, "rk4", steps)
        w32 = O.latent_solve(cast(sd, torch.float32), z0, rel.float(), "rk4", steps)
        _REF[key] = (sd, z0, w64, float((w32.double() - w64).abs().max()))
    return _REF[key]


def bound_of(w64, e32, project=Z_TOL):
    return max(project * max(1.0, float(w64.abs().max())), 4.0 * e32)


# ---------------------------------------------------------------------------------------------
# 1. CPU: the reference discriminates
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("D", DS)
def test_reference_discriminates(D, H):
    """Every mutation moves the last stamp by >= 10 x the bound of section 2, at both step counts; the unmutated restatement is the
    oracle's solve to the bit (so the mutations are mutations of THE reference)."""
    for steps in (1, 2):
        sd, z0, w64, e32 = reference(D, H, B_FWD, TIMES, steps)
        rel = rel_times(TIMES)
        assert torch.equal(solve_mut(sd, z0.double(), rel, steps, None), w64)
        bound = bound_of(w64, e32)
        for mut in MUTATIONS:
            if not applies(mut, D):
                continue
            moved = float((solve_mut(sd, z0.double(), rel, steps, mut)[:, -1] - w64[:, -1]).abs().max())
            print("D %d H %d steps %d %s: moved %.3e, bound %.3e, f32-CPU %.3e" % (D, H, steps, mut, moved, bound, e32))
            assert moved >= 10 * bound, "D %d H %d steps %d: mutation %s moves the last stamp by %.3e < 10 x %.3e" % (D, H, steps, mut, moved, bound)


# ---------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _deferred_errors_drained():
    """A team barrier that gave up poisons its output and reports through the deferred channel: raise it in the test that caused it."""
    yield
    if torch.cuda.is_available():
        from caspr_amd import ops
        ops.check_deferred_errors()


_WTS = {}


def weights(D, H, dev):
    """[PackedWeight0, b0, ..., PackedWeight3, b3] of net(D, H) as ops.latent_rk4 takes them; packed once per (D, H)."""
    from caspr_amd import ops
    if (D, H) not in _WTS:
        sd = net(D, H)
        _WTS[(D, H)] = [x for l in (0, 2, 4, 6) for x in (ops.PackedWeight(sd["%s.%d.weight" % (PRE, l)].float().to(dev).contiguous()),
                                                          sd["%s.%d.bias" % (PRE, l)].float().to(dev).contiguous())]
    return _WTS[(D, H)]


def module(D, H, dev, **kw):
    """LatentODE(input_size = D, hidden_size = H) holding net(D, H): the public surface that passes the widths through."""
    from caspr_amd.models.latent_ode_model import LatentODE
    lat = LatentODE(input_size=D, hidden_size=H, **kw)
    sd = net(D, H)
    lat.ode_func.dynamics_net.load_state_dict({k[len(PRE) + 1:]: v.float() for k, v in sd.items()})
    return lat.to(dev).eval()


def run(z0, times, steps, D, H, dev, team):
    from caspr_amd import ops
    t = torch.as_tensor(times, dtype=torch.float32).to(dev)
    with torch.no_grad():
        out = ops.latent_rk4(z0 if z0.is_cuda else z0.to(dev), t, steps, weights(D, H, dev), team=team)
    return out.cpu()


def note(key, **kw):
    REPORT["latent_widths:" + key] = kw
    record("latent_widths:written", 0, 0, 0)            # (writes the report file)


def check(key, got, w64, e32, project=Z_TOL):
    """|hip - f64| against the bound in force; both distances into the report first."""
    bound = bound_of(w64, e32, project)
    err = float((got.double() - w64).abs().max()) if bool(torch.isfinite(got).all()) else float("inf")
    note(key, hip_vs_f64=err, f32_cpu_vs_f64=e32, bound=bound, project_bound=project * max(1.0, float(w64.abs().max())), ref_absmax=float(w64.abs().max()))
    print("%s: |hip - f64| %.3e, |f32 CPU - f64| %.3e, bound %.3e" % (key, err, e32, bound))
    assert err <= bound, "%s: |hip - f64| %.3e > %.3e (|f32 CPU - f64| %.3e)" % (key, err, bound, e32)


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


# ---------------------------------------------------------------------------------------------
# 2. forward RK4, both kernels, against f64
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("D", DS)
def test_forward_against_f64(dev, D, H):
    """The single-workgroup kernel at every (D, H), the team kernel at H = 512 (twice: equal bits), 1 and 2 steps per interval."""
    for steps in (1, 2):
        sd, z0, w64, e32 = reference(D, H, B_FWD, TIMES, steps)
        single = run(z0, TIMES, steps, D, H, dev, team=False)
        assert same_bits(single[:, 0], z0) and same_bits(single[:, 1], z0), "the rows of times[0] are not z0"
        assert same_bits(single[:, 3], single[:, 4]), "a repeated stamp gives different rows"
        check("fwd:single:D%d:H%d:steps%d" % (D, H, steps), single, w64, e32)
        if H != 512:
            continue
        team = run(z0, TIMES, steps, D, H, dev, team=True)
        again = run(z0, TIMES, steps, D, H, dev, team=True)
        assert same_bits(team, again), "the team kernel is not repeatable at D = %d" % D
        assert same_bits(team[:, 0], z0) and same_bits(team[:, 1], z0) and same_bits(team[:, 3], team[:, 4])
        check("fwd:team:D%d:H%d:steps%d" % (D, H, steps), team, w64, e32)
        diff = float((team - single).abs().max())
        note("fwd:team_vs_single:D%d:steps%d" % (D, steps), max_abs_diff=diff, bound=TEAM_VS_SINGLE)
        assert diff <= TEAM_VS_SINGLE, "D %d steps %d: team against single-workgroup %.3e > %.1e" % (D, steps, diff, TEAM_VS_SINGLE)


# ---------------------------------------------------------------------------------------------
# 3. memory edges of the forward kernels
# ---------------------------------------------------------------------------------------------
EDGE_DS = (20, 64)
KERNELS = (("single", False), ("team", True))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,team", KERNELS)
@pytest.mark.parametrize("D", EDGE_DS)
def test_strided_start(dev, D, kernel, team):
    """z0 as the column slice big[:, 3:3+D] of a (B, 71) tensor -- odd row stride, a pointer that is 4-byte aligned only -- whose other
    columns hold 1e30: the bits of the contiguous copy."""
    _, z0, w64, e32 = reference(D, 512, B_FWD, TIMES, 2)
    big = torch.full((B_FWD, 71), 1e30)
    big[:, 3:3 + D] = z0
    view = big.to(dev)[:, 3:3 + D]
    assert view.stride(0) == 71 and view.data_ptr() % 16 == 12
    got = run(view, TIMES, 2, D, 512, dev, team)
    assert same_bits(got, run(z0, TIMES, 2, D, 512, dev, team)), "a strided z0 changes the bits"
    check("edge:strided:%s:D%d" % (kernel, D), got, w64, e32)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,team", KERNELS)
@pytest.mark.parametrize("D", EDGE_DS)
def test_batch_edges(dev, D, kernel, team):
    """B in {1, 15, 16, 17, 33, 64} against f64; the rows of a sequence inside a batch of 17 and of 64 are the bits of that sequence
    solved alone (other columns, other workgroups, ragged last group); an all-NaN sequence among 17 leaves every other row its bits."""
    _, z0, w64, e32 = reference(D, 512, 65, TIMES, 2)
    outs = {}
    for B in (1, 15, 16, 17, 33, 64):
        outs[B] = run(z0[:B], TIMES, 2, D, 512, dev, team)
        check("edge:batch:%s:D%d:B%d" % (kernel, D, B), outs[B], w64[:B], e32)
    alone = [run(z0[b:b + 1], TIMES, 2, D, 512, dev, team) for b in range(64)]
    bad = [(B, b) for B in (17, 64) for b in range(B) if not same_bits(outs[B][b:b + 1], alone[b])]
    assert not bad, "%s kernel, D = %d: (batch, sequence) whose rows differ from the sequence solved alone: %s" % (kernel, D, bad)
    dirty = z0[:17].clone()
    dirty[5] = float("nan")
    got = run(dirty, TIMES, 2, D, 512, dev, team)
    keep = torch.tensor([b for b in range(17) if b != 5])
    assert bool(torch.isnan(got[5]).all()), "the all-NaN sequence has rows that are not NaN"
    assert same_bits(got[keep], outs[17][keep]), "a NaN sequence changes the bits of its batch-mates"


@pytest.mark.gpu
@pytest.mark.parametrize("D", EDGE_DS)
def test_hand_over_at_65_sequences(dev, D):
    """ops.latent_rk4(team=None) with the team kernel on: 64 sequences take the team kernel, 65 the single-workgroup kernel (the team
    entry refuses more than 128 workgroups) -- its bits -- and meet the bound."""
    from caspr_amd import ops
    _, z0, w64, e32 = reference(D, 512, 65, TIMES, 2)
    prev = ops.LATENT_TEAM
    try:
        ops.LATENT_TEAM = True
        auto65, auto64 = run(z0, TIMES, 2, D, 512, dev, None), run(z0[:64], TIMES, 2, D, 512, dev, None)
    finally:
        ops.LATENT_TEAM = prev
    single65, single64, team64 = run(z0, TIMES, 2, D, 512, dev, False), run(z0[:64], TIMES, 2, D, 512, dev, False), run(z0[:64], TIMES, 2, D, 512, dev, True)
    assert not same_bits(single64, team64), "the two kernels give the same bits: the comparison below shows nothing"
    assert same_bits(auto64, team64), "64 sequences did not take the team kernel"
    assert same_bits(auto65, single65), "65 sequences did not take the single-workgroup kernel"
    check("edge:hand_over:D%d:B65" % D, auto65, w64, e32)
    from caspr_amd.lib import CasprHipError
    with pytest.raises(CasprHipError, match="latent_rk4_team: 65 sequences"):
        _team_entry(z0.to(dev), TIMES, 2, D, dev)


def _team_entry(z0, times, steps, D, dev):
    """caspr_latent_rk4_team_f32 itself (ops.latent_rk4 routes B > 64 away from it)."""
    from caspr_amd import lib, ops
    L = lib.load()
    B = z0.shape[0]
    t = torch.as_tensor(times, dtype=torch.float32).to(dev)
    out = torch.empty(B, t.shape[0], D, device=dev)
    ws = torch.zeros(L.caspr_latent_team_ws_bytes(B), device=dev, dtype=torch.uint8)
    ptrs = [ops._p(w.data) if isinstance(w, ops.PackedWeight) else ops._p(w) for w in weights(D, 512, dev)]
    lib.check(L.caspr_latent_rk4_team_f32(ops._p(z0), z0.stride(0), ops._p(t), B, t.shape[0], D, 512, steps, *ptrs, ops._p(out), ops._p(ws), ws.numel(),
                                          ops._stream()), "caspr_latent_rk4_team_f32")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,team", KERNELS)
@pytest.mark.parametrize("D", EDGE_DS)
def test_time_edges(dev, D, kernel, team):
    """One stamp returns z0; all stamps equal: every stamp is z0; a repeat at the end: the last two rows have the same bits."""
    _, z0, _, _ = reference(D, 512, B_FWD, TIMES, 2)
    one = run(z0, [0.7], 2, D, 512, dev, team)
    assert tuple(one.shape) == (B_FWD, 1, D) and same_bits(one[:, 0], z0)
    eq = run(z0, [0.4, 0.4, 0.4], 2, D, 512, dev, team)
    assert all(same_bits(eq[:, i], z0) for i in range(3)), "equal stamps: a row is not z0"
    times = [0.0, 0.5, 1.0, 1.0]
    rep = run(z0, times, 2, D, 512, dev, team)
    assert same_bits(rep[:, 2], rep[:, 3]) and not same_bits(rep[:, 1], rep[:, 2])
    sd = net(D, 512)
    w64 = O.latent_solve(sd, z0.double(), rel_times(times), "rk4", 2)
    w32 = O.latent_solve(cast(sd, torch.float32), z0, rel_times(times).float(), "rk4", 2)
    check("edge:repeat_at_end:%s:D%d" % (kernel, D), rep, w64, float((w32.double() - w64).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("D", EDGE_DS)
def test_equal_stamps_through_the_model(dev, D):
    """LatentODE(input_size = D).solve_at with every stamp equal: z0 at every entry and an evaluation count of 0; with two distinct
    stamps the count is 4 x steps and the values meet the bound (the widths reach the kernels from the public surface)."""
    lat = module(D, 512, dev, rk4_steps=2)
    _, z0, _, _ = reference(D, 512, B_FWD, TIMES, 2)
    zg = z0.to(dev)
    with torch.no_grad():
        out = lat.solve_at(zg, torch.full((B_FWD, 3), 0.6, device=dev)).cpu()
        assert lat.num_evals() == 0
        assert all(same_bits(out[:, i], z0) for i in range(3))
        tt = torch.tensor([[1.0, 0.0, 1.0]]).repeat(B_FWD, 1)
        out = lat.solve_at(zg, tt.to(dev)).cpu()
        assert lat.num_evals() == 4 * 2
    sd = net(D, 512)
    rel = rel_times([0.0, 1.0])
    w64 = O.latent_solve(sd, z0.double(), rel, "rk4", 2)
    w32 = O.latent_solve(cast(sd, torch.float32), z0, rel.float(), "rk4", 2)
    assert same_bits(out[:, 1], z0) and same_bits(out[:, 0], out[:, 2])
    check("edge:solve_at:D%d" % D, out[:, [1, 0]], w64, float((w32.double() - w64).abs().max()))


# ---------------------------------------------------------------------------------------------
# 4. training forms
# ---------------------------------------------------------------------------------------------
TRAIN_STEPS = 2
OUT_RTOL, GRAD_RTOL = 2e-6, 3e-5                       # against f64 (test_hip_train.py: latent_node_vs_f64_*)
ROUTE_OUT_RTOL, ROUTE_GRAD_RTOL = 1e-6, 2e-5           # team against non-team (latent_node_vs_layers_*)
NAMES = ("out", "dz0", "dW0", "db0", "dW1", "db1", "dW2", "db2", "dW3", "db3")
_TRAIN_REF, _TRAIN_GOT = {}, {}


def train_inputs(D, nseq, times):
    return starts(D, nseq, seed=11), rnd(5000 + 10 * D + nseq, nseq, len(times), D).float()


def train_reference(D, H, nseq, times, dtype):
    """torch.autograd on the CPU through the RK4 map (latent_ode_model.py:45-70,139-147 with TRAIN_STEPS steps per interval), the output
    weighted by a fixed random tensor -> [out, dz0, dW0, db0, ..., dW3, db3] in `dtype`."""
    key = (D, H, nseq, tuple(times), dtype)
    if key in _TRAIN_REF:
        return _TRAIN_REF[key]
    sd = net(D, H)
    W = [sd["%s.%d.weight" % (PRE, l)].to(dtype).requires_grad_(True) for l in (0, 2, 4, 6)]
    Bi = [sd["%s.%d.bias" % (PRE, l)].to(dtype).requires_grad_(True) for l in (0, 2, 4, 6)]
    z0, wgt = train_inputs(D, nseq, times)
    z = z0.to(dtype).requires_grad_(True)

    def f(x):
        h = x
        for i in range(4):
            h = h @ W[i].t() + Bi[i]
            if i < 3:
                h = torch.tanh(h)
        return h
    outs, x, tt = [z], z, rel_times(times).to(dtype)
    for k in range(1, tt.shape[0]):
        h = (tt[k] - tt[k - 1]) / TRAIN_STEPS
        for _ in range(TRAIN_STEPS):
            k1 = f(x); k2 = f(x + 0.5 * h * k1); k3 = f(x + 0.5 * h * k2); k4 = f(x + h * k3)
            x = x + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        outs.append(x)
    out = torch.stack(outs, dim=1)
    (out * wgt.to(dtype)).sum().backward()
    _TRAIN_REF[key] = [out.detach(), z.grad] + [g for pair in zip([w.grad for w in W], [b.grad for b in Bi]) for g in pair]
    return _TRAIN_REF[key]


def train_gpu(D, H, nseq, times, team, dev, monkeypatch):
    """flow_grad.LatentSolve.apply on net(D, H) -> ([out, dz0, dW0, ..., db3] on the CPU, the (dy, x) pairs conv1x1_wgrad was given)."""
    from caspr_amd import train_ops
    from caspr_amd.train import flow_grad as FG
    monkeypatch.setattr(FG.LatentSolve, "TEAM", team)
    seen, real = [], train_ops.conv1x1_wgrad

    def spy(dy, x, cin, cout, dw, dbias=None, **kw):
        seen.append((dy.detach().clone(), x.detach().clone(), cin, cout))
        return real(dy, x, cin, cout, dw, dbias, **kw)
    monkeypatch.setattr(train_ops, "conv1x1_wgrad", spy)
    sd = net(D, H)
    wb = [torch.nn.Parameter(sd["%s.%d.%s" % (PRE, l, nm)].float().to(dev)) for l in (0, 2, 4, 6) for nm in ("weight", "bias")]
    z0, wgt = train_inputs(D, nseq, times)
    z = z0.to(dev).requires_grad_(True)
    out = FG.LatentSolve.apply(z, torch.tensor(times, device=dev), TRAIN_STEPS, *wb)
    assert FG.LatentSolve._team_ok(z, wb[0::2], wb[1::2]) == (team and H == 512), "the route asked for is not the one that ran"
    (out * wgt.to(dev)).sum().backward()
    torch.cuda.synchronize()
    return [out.detach().cpu(), z.grad.cpu()] + [p.grad.cpu() for p in wb], seen


def rel_err(got, want):
    """test_hip_train.rel: max |got - want| / |want|max."""
    ref = float(want.abs().max()) or 1.0
    return (float((got.double() - want.double()).abs().max()) / ref) if bool(torch.isfinite(got).all()) else float("inf")


TRAIN_CASES = ([(True, D, 512, n) for D in (5, 20, 33, 48, 64) for n in (3, 17)] + [(False, D, 512, 3) for D in (5, 20, 33, 48, 64)]
               + [(False, 33, 512, 17), (False, 20, 256, 3), (False, 64, 64, 3)])


@pytest.mark.gpu
@pytest.mark.parametrize("team,D,H,nseq", TRAIN_CASES, ids=["%s-D%d-H%d-n%d" % ("team" if c[0] else "layers", c[1], c[2], c[3]) for c in TRAIN_CASES])
def test_training_against_f64_autograd(dev, monkeypatch, team, D, H, nseq):
    """Output, dz0 and the eight parameter gradients of LatentSolve against f64 autograd; the padding columns D .. xw - 1 of the tape's x
    and of the output layer's deltas, as conv1x1_wgrad is handed them, are exactly zero.  team = False at D % 4 != 0 is the route
    through conv1x1_train on rows of D floats: it computes (rows padded to xw) and meets the same bounds."""
    got, seen = train_gpu(D, H, nseq, TRAIN_TIMES, team, dev, monkeypatch)
    _TRAIN_GOT[(team, D, H, nseq)] = got
    w64, w32 = train_reference(D, H, nseq, TRAIN_TIMES, torch.float64), train_reference(D, H, nseq, TRAIN_TIMES, torch.float32)
    bad = []
    for nm, g, a, b in zip(NAMES, got, w64, w32):
        assert g.shape == a.shape, (nm, g.shape, a.shape)
        err, e32 = rel_err(g, a), rel_err(b, a)
        bound = max(OUT_RTOL if nm == "out" else GRAD_RTOL, 4.0 * e32)
        note("train:%s:D%d:H%d:n%d:%s" % ("team" if team else "layers", D, H, nseq, nm), hip_vs_f64=err, f32_cpu_vs_f64=e32, bound=bound,
             project_bound=OUT_RTOL if nm == "out" else GRAD_RTOL, ref_absmax=float(a.abs().max()))
        print("D %d H %d n %d %s %s: %.3e (f32 CPU %.3e, bound %.3e)" % (D, H, nseq, "team" if team else "layers", nm, err, e32, bound))
        if not err <= bound:
            bad.append("%s: %.3e > %.3e (f32 CPU %.3e)" % (nm, err, bound, e32))
    assert not bad, "\n".join(bad)
    xw = (D + 3) // 4 * 4
    assert len(seen) == 4 and [s[2:] for s in seen] == [(D, H), (H, H), (H, H), (H, D)]
    x, d3 = seen[0][1], seen[3][0]
    assert x.shape[-1] == xw and d3.shape[-1] == xw, (x.shape, d3.shape)
    assert float(x[..., :D].abs().max()) > 0 and float(d3[..., :D].abs().max()) > 0
    if xw != D:
        assert float(x[..., D:].abs().max()) == 0.0, "the padding columns of the tape's x are not zero"
        assert float(d3[..., D:].abs().max()) == 0.0, "the padding columns of the output layer's deltas are not zero"


@pytest.mark.gpu
@pytest.mark.parametrize("D", (5, 20, 33, 48, 64))
def test_training_team_against_layers(dev, monkeypatch, D):
    """The one-launch forms against the launch-per-product form of the same node, same inputs (3 sequences, H = 512)."""
    pair = []
    for team in (True, False):
        key = (team, D, 512, 3)
        pair.append(_TRAIN_GOT[key] if key in _TRAIN_GOT else train_gpu(D, 512, 3, TRAIN_TIMES, team, dev, monkeypatch)[0])
    bad = []
    for nm, a, b in zip(NAMES, *pair):
        err, bound = rel_err(a, b), ROUTE_OUT_RTOL if nm == "out" else ROUTE_GRAD_RTOL
        note("train:team_vs_layers:D%d:%s" % (D, nm), max_rel_diff=err, bound=bound)
        if not err <= bound:
            bad.append("%s: %.3e > %.1e" % (nm, err, bound))
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("team,D,H", [(True, 20, 512), (True, 33, 512), (False, 33, 512), (False, 20, 256)])
def test_training_with_equal_stamps(dev, monkeypatch, team, D, H):
    """Every stamp equal: the output is z0 at every stamp, dz0 the sum of the output's gradient over the stamps, every parameter
    gradient exactly zero."""
    times = [0.4, 0.4, 0.4]
    got, _ = train_gpu(D, H, 3, times, team, dev, monkeypatch)
    z0, wgt = train_inputs(D, 3, times)
    assert all(same_bits(got[0][:, i], z0) for i in range(3))
    assert torch.equal(got[1], (wgt[:, 2] + wgt[:, 1]) + wgt[:, 0]), "dz0 is not the sum of the output's gradient (%.3e off)" % float((got[1] - wgt.sum(1)).abs().max())
    for nm, g in zip(NAMES[2:], got[2:]):
        assert float(g.abs().max()) == 0.0, "%s is not zero" % nm


# ---------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(dev):
    """Sizes outside what an entry accepts raise CasprHipError with the entry's own message and launch nothing: every pointer that an
    entry writes through points into one buffer, which keeps its fill."""
    from caspr_amd import lib, ops
    L = lib.load()
    B, Tu = 2, 2
    ro = torch.zeros(1 << 20, device=dev)              # every pointer that is read; large enough for any of the refused sizes
    wr = torch.full((1 << 20,), 7.0, device=dev)       # every pointer that is written
    ws = torch.zeros(L.caspr_latent_team_ws_bytes(B), device=dev, dtype=torch.uint8)
    r, w, s = ops._p(ro), ops._p(wr), ops._stream()
    w8 = [r] * 8

    def rk4(D, H, **kw):
        return L.caspr_latent_rk4_f32(r, 128, r, B, Tu, D, H, 1, *w8, w, s)

    def team(D, H, **kw):
        return L.caspr_latent_rk4_team_f32(r, 128, r, B, Tu, D, H, 1, *w8, w, ops._p(ws), ws.numel(), s)

    def tape(D, H, xw=None):
        return L.caspr_latent_rk4_team_tape_f32(r, 128, r, B, Tu, D, H, 1, *w8, w, w, (D + 3) // 4 * 4 if xw is None else xw, w, w, w, ops._p(ws), ws.numel(), s)

    def adjoint(D, H, xw=None):
        return L.caspr_latent_rk4_team_adjoint_f32(r, r, B, Tu, D, H, 1, r, r, r, r, r, r, r, w, w, w, w, (D + 3) // 4 * 4 if xw is None else xw, w, ops._p(ws),
                                                   ws.numel(), s)

    def dp5(D, H, **kw):
        return L.caspr_latent_dopri5_f32(r, 128, r, B, Tu, D, H, 1e-3, 1e-3, 10, *w8, w, w, w, s)
    entries = [("caspr_latent_rk4_f32", rk4, r"latent_rk4: unsupported sizes D=%d H=%d", False),
               ("caspr_latent_rk4_team_f32", team, r"latent_rk4_team: needs D<=64, H==512 \(got D=%d H=%d\)", True),
               ("caspr_latent_rk4_team_tape_f32", tape, r"latent_rk4_team_tape: needs D<=64, H==512, xw >= D a multiple of 4 \(got D=%d H=%d", True),
               ("caspr_latent_rk4_team_adjoint_f32", adjoint, r"latent_rk4_team_adjoint: needs D<=64, H==512, xw >= D a multiple of 4 \(got D=%d H=%d", True),
               ("caspr_latent_dopri5_f32", dp5, r"latent_dopri5: unsupported sizes D=%d H=%d", False)]
    n = 0
    for name, fn, msg, is_team in entries:
        for D, H in [(65, 512), (64, 576), (64, 96)] + ([(64, 448)] if is_team else []):
            with pytest.raises(lib.CasprHipError, match=msg % (D, H)):
                lib.check(fn(D, H), name)
            n += 1
        if fn in (tape, adjoint):
            for D, xw in [(20, 16), (20, 22), (33, 33), (64, 60)]:          # xw < D, xw % 4 != 0
                with pytest.raises(lib.CasprHipError, match=(msg % (D, 512)) + " xw=%d" % xw):
                    lib.check(fn(D, 512, xw=xw), name)
                n += 1
    assert n == 3 * 5 + 3 + 2 * 4
    torch.cuda.synchronize()
    assert bool((wr == 7.0).all()) and bool((ro == 0.0).all()), "a refused call wrote to its outputs"
    note("refusals", calls=n)
