"""Are the kernels handed the CURRENT weights?  (GPU; the CPU half is tests/test_weight_cache.py.)

Every matrix product reads a derived copy of its parameter -- MFMA-order packs, bf16 / f16 planes, the folded head weight, the
concatenated hyper-network matrix, t_end, the transposed packs of the training tier -- kept in `WeightCache`s next to the modules and in
`train.flow_grad._packed`.  A stale copy passes every kernel test and is wrong for the model.  Here a WARM model `m` (it has run every
entry point on every route below, so every cache holds an entry) has parameters changed, and must then compute, bit for bit, what a second
instance `ref` computes after `ref.load_state_dict(m.state_dict())`, which rebuilds all of `ref`'s caches.  Bitwise comparison is fair:
tests/test_zz_determinism.py and the bit-reproducibility tests of tests/test_hip_train.py establish that two runs give the same bits.

  1. inference, one parameter (or running-statistics buffer) at a time, on every route that has a pack of its own;
  2. training (forward and backward: loss terms and every .grad), one packed tensor at a time;
  3. whole-model writers: Adam, load_state_dict, .cpu() / .to(), `p.data = t`, broadcast_model, `.data` writes + invalidate(), a second
     model in the process; after the load_state_dict pair also tests/test_hip_parity.py's f64-oracle assertions, unchanged;
  4. the control: with the caches frozen at their first build the same harness reports a mismatch behind every cache site.

A change must also MOVE the output (against m's own result before it): a parameter that moves nothing would make its case vacuous.
NO_EFFECT names the exceptions, with the reason.
"""
import collections
import contextlib
import gc

import pytest
import torch
import torch.nn as nn

from caspr_amd.utils.synthetic import dense_sequences

pytestmark = pytest.mark.gpu

SCALE = 1.0 + 2.0 ** -6
# name -> reason from the model's graph.  Never a tensor with two or more dimensions.
_ONE_CHANNEL_GROUPS = ("a per-channel constant in front of a GroupNorm whose groups hold ONE channel (16 channels in 16 groups, pointnet2.py:62: "
                       "[16, 16, 32]) is removed by the normalisation: (x + b) - mean(x + b) = x - mean(x)")
NO_EFFECT = {
    "encoder.local_extract.set_abstractions.0.pointnet_modules.0.conv_layers.0.bias": _ONE_CHANNEL_GROUPS,
    "encoder.local_extract.set_abstractions.0.pointnet_modules.0.conv_layers.1.bias": _ONE_CHANNEL_GROUPS,
}

# conv: (ops.CONV_X6W, ops.CONV_SPLIT, conv products on bf16x6)      cnf: (CNF products on bf16x6, ops.CNF_SPLIT, narrow kernel, num_points)
CONV = {"h3w": (True, "f16x3", True), "x6w": (True, "bf16x6", True), "x6": (False, "bf16x6", True), "f32": (True, "f16x3", False)}
CNF = {"h3": (True, "f16x3", False, 128), "x6": (True, "bf16x6", False, 128), "x6n": (True, "bf16x6", True, 64), "f32": (False, "f16x3", False, 128)}
# commute: feature propagation's first conv on the coarse level (reached from N = 2048 on: the finest level must have twice the rows of
# the one below).  fold: PointNet++'s last layer inside the head's first conv (False: the two layers apart, the recording path).
Route = collections.namedtuple("Route", "conv commute fold cnf N")
DEFAULT = Route("h3w", True, True, "h3", 1024)
CONV_ROUTES = [DEFAULT._replace(conv=c) for c in CONV]
FOLD_ROUTES = [DEFAULT._replace(conv=c, fold=f) for c in CONV for f in (True, False)]
COMMUTE_ROUTES = [DEFAULT._replace(conv=c, commute=k, N=2048) for c in CONV for k in (True, False)]
CNF_ROUTES = [DEFAULT._replace(cnf=c) for c in CNF]
ALL_ROUTES = list(dict.fromkeys(FOLD_ROUTES + COMMUTE_ROUTES + CNF_ROUTES))

LE = "encoder.local_extract."
FLOW = "point_cnf.chain.1.odefunc.diffeq.layers."


def group_of(name):
    p = name.split(".")
    if name.startswith(LE + "set_abstractions."):
        return "sa%s" % p[3]
    if name.startswith(LE + "feature_propagators."):
        return "fp%s" % p[3]
    if name.startswith(LE + "final_layers."):
        return "final"
    if name.startswith("encoder.global_extract."):
        return "global"
    if name.startswith("encoder."):
        return "head"
    if name.startswith("latent_ode."):
        return "latent"
    if name.startswith(FLOW):
        return "flow_l%s" % p[6]
    assert name.startswith("point_cnf."), name
    return "flow_ends"          # both MovingBatchNorms (parameters and running statistics) and sqrt_end_time


GROUPS = (["sa%d" % i for i in range(5)] + ["fp%d" % i for i in range(5)] + ["final", "global", "head", "latent", "flow_ends"]
          + ["flow_l%d" % i for i in range(4)])
GROUP_ROUTES = {"final": FOLD_ROUTES, "global": CONV_ROUTES, "head": FOLD_ROUTES, "latent": [DEFAULT], "flow_ends": CNF_ROUTES}
GROUP_ROUTES.update({"sa%d" % i: [DEFAULT, DEFAULT._replace(conv="f32")] for i in range(5)})      # rows / pre-aggregated route, fused route
GROUP_ROUTES.update({"fp%d" % i: CONV_ROUTES for i in range(4)})
GROUP_ROUTES["fp4"] = COMMUTE_ROUTES
GROUP_ROUTES.update({"flow_l%d" % i: CNF_ROUTES for i in range(4)})
EVERY_ROUTE_1D = {LE + "final_layers.3.bias"}      # enters the folded bias b_fold
DEFAULT_THRESHOLDS = []                            # (ops._X6W_MIN_CIN, ops._X6W_MIN_ROWS) as the `ops` fixture found them


# ---------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _thresholds(ops, min_cin, min_rows):
    """The persistent 512-channel kernel's thresholds.  Read when a PackedWeight is BUILT (x6w_ok) and when a conv is routed."""
    saved = (ops._X6W_MIN_CIN, ops._X6W_MIN_ROWS)
    ops._X6W_MIN_CIN, ops._X6W_MIN_ROWS = min_cin, min_rows
    try:
        yield
    finally:
        ops._X6W_MIN_CIN, ops._X6W_MIN_ROWS = saved


@pytest.fixture(scope="module")
def ops():
    """caspr_amd.ops with the persistent kernel's thresholds lowered so that the (1, 2, 1024) input reaches it on the 512-wide layers
    (as tests/test_hip_parity.py::test_conv1x1_x6w_kernel does); every route switch restored when the module is done."""
    from caspr_amd import ops as _ops
    from caspr_amd.models import pointnet2 as P2
    _ops.check_deferred_errors()
    saved = (_ops.CONV_X6W, _ops.CONV_SPLIT, _ops.CNF_SPLIT, _ops.CONV_BF16X6, _ops.CNF_BF16X6, P2.FP_COMMUTE)
    DEFAULT_THRESHOLDS[:] = [_ops._X6W_MIN_CIN, _ops._X6W_MIN_ROWS]
    try:
        with _thresholds(_ops, 256, 128):
            yield _ops
            _ops.check_deferred_errors()
    finally:
        _ops.CONV_X6W, _ops.CONV_SPLIT, _ops.CNF_SPLIT = saved[:3]
        _ops.set_matmul_mode(conv=saved[3], cnf=saved[4])
        P2.FP_COMMUTE = saved[5]


@contextlib.contextmanager
def _route(ops, model, r):
    from caspr_amd.models import pointnet2 as P2
    from caspr_amd.models.cnf import CNF as CnfBlock
    saved = (ops.CONV_X6W, ops.CONV_SPLIT, ops.CNF_SPLIT, ops.CONV_BF16X6, ops.CNF_BF16X6, P2.FP_COMMUTE)
    blocks = [b for b in model.point_cnf.chain if isinstance(b, CnfBlock)]
    x6w, csplit, conv6 = CONV[r.conv]
    cnf6, fsplit, narrow, _ = CNF[r.cnf]
    ops.CONV_X6W, ops.CONV_SPLIT, ops.CNF_SPLIT, P2.FP_COMMUTE = x6w, csplit, fsplit, r.commute
    ops.set_matmul_mode(conv=conv6, cnf=cnf6)
    model.encoder.record = None if r.fold else []
    for b in blocks:
        b._narrow = narrow
    try:
        yield
    finally:
        ops.CONV_X6W, ops.CONV_SPLIT, ops.CNF_SPLIT, P2.FP_COMMUTE = saved[0], saved[1], saved[2], saved[5]
        ops.set_matmul_mode(conv=saved[3], cnf=saved[4])
        model.encoder.record = None
        for b in blocks:
            b._narrow = False


# ---------------------------------------------------------------------------------------------
# the pair of models, the inputs, the two entry points
# ---------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    """Bit for bit, output by output (torch.equal on the words: -0.0 is not 0.0, and a NaN equals itself)."""
    assert len(a) == len(b)
    return all((u is None and v is None) or (u is not None and v is not None and u.shape == v.shape and torch.equal(_bits(u), _bits(v)))
               for u, v in zip(a, b))


class Pair:
    def __init__(self, ops, dev, seeded_sd, golden):
        from caspr_amd.models import CaSPR
        self.ops, self.dev, self.seeded = ops, dev, seeded_sd
        # the step counts of tests/test_hip_parity.py's `model`: its f64-oracle assertions are run on `m` below
        self.m, self.ref = (CaSPR(cnf_rk4_steps=8, latent_rk4_steps=4, check_tol=None) for _ in range(2))
        for mod in (self.m, self.ref):
            mod.load_state_dict(seeded_sd)
            mod.to(dev).eval()
        self.x, self.ts = {}, None
        for N in (1024, 2048):
            x, sp = dense_sequences(1, 2, N)
            self.x[N], self.ts = x.to(dev), sp[0, :, 0, 3].to(dev)
        y = torch.randn(1, 2, 128, 3, generator=torch.Generator().manual_seed(11))
        self.y = {128: y.to(dev), 64: y[:, :, :64].contiguous().to(dev)}
        self.train_in = tuple(torch.from_numpy(golden[k]).to(dev) for k in ("train_x", "train_sp", "train_e"))
        assert tuple(self.train_in[0].shape) == (1, 2, 1024, 4)
        # warm: every entry point on every route, before any parameter is touched; and m's own results to measure "moved" against
        self.base = {r: self.infer(self.m, r) for r in ALL_ROUTES}
        self.base_train = self.train(self.m)
        self.infer(self.ref, DEFAULT)
        for r, out in self.base.items():
            assert all(bool(torch.isfinite(o).all()) for o in out if o is not None), r
        assert same(self.base_train, self.train(self.m)), "training is not repeatable from the same state: the harness is wrong"
        ops.check_deferred_errors()

    def infer(self, model, r):
        model.eval()
        with _route(self.ops, model, r), torch.no_grad():
            n = CNF[r.cnf][3]
            return tuple(model.reconstruct(self.x[r.N], num_points=n, timestamps=self.ts, y=self.y[n]))

    def train(self, model):
        """Loss terms and every .grad of one training forward + backward.  Buffers (MovingBatchNorm statistics, counters) are put back:
        the call leaves the model as it found it."""
        x, sp, e = self.train_in
        kept = [(b, b.detach().clone()) for b in model.buffers()]
        model.train()
        try:
            model.zero_grad(set_to_none=True)
            nll, tl = model(x, sp, e=e)
            (0.01 * nll.sum(2).mean() + 100.0 * tl[:, :, :, :4].mean()).backward()
            out = (nll.detach(), tl.detach()) + tuple(None if p.grad is None else p.grad.detach().clone() for p in model.parameters())
            model.zero_grad(set_to_none=True)
            return out
        finally:
            model.eval()
            with torch.no_grad():
                for b, v in kept:
                    if not torch.equal(b, v):
                        b.copy_(v)

    def sync_ref(self):
        self.ref.load_state_dict(self.m.state_dict())

    def tensors(self):
        """name -> tensor of m: the 221 parameters and the four running statistics."""
        out = dict(self.m.named_parameters())
        out.update({k: b for k, b in self.m.named_buffers() if k.endswith(("running_mean", "running_var"))})
        return out

    def probe(self, name, routes, training=False):
        """Scale one tensor of m in place (under no_grad), run m and the re-loaded ref.  -> {route: (same as ref, moved against m before)}."""
        t = self.tensors()[name]
        orig = t.detach().clone()
        res = {}
        try:
            with torch.no_grad():
                t.add_(2.0 ** -6) if not bool(t.any()) else t.mul_(SCALE)
            assert not torch.equal(t, orig), name
            self.sync_ref()
            if training:
                got = self.train(self.m)
                res["train"] = (same(got, self.train(self.ref)), not same(got, self.base_train))
            else:
                for r in routes:
                    got = self.infer(self.m, r)
                    res[r] = (same(got, self.infer(self.ref, r)), not same(got, self.base[r]))
        finally:
            with torch.no_grad():
                t.copy_(orig)
        return res

    def reset(self):
        """Back to the seeded weights, whatever a test did to m."""
        self.m.load_state_dict(self.seeded)
        self.m.to(self.dev).eval()

    def check_whole_model(self, what):
        """After a whole-model writer: m against the re-loaded ref on every route of the inference entry point, and in training."""
        self.sync_ref()
        bad = [tuple(r) for r in ALL_ROUTES if not same(self.infer(self.m, r), self.infer(self.ref, r))]
        assert not bad, "%s: reconstruct() differs from a freshly loaded model on %d of %d routes: %s" % (what, len(bad), len(ALL_ROUTES), bad[:4])
        assert same(self.train(self.m), self.train(self.ref)), "%s: the training forward / backward differs from a freshly loaded model" % what
        self.ops.check_deferred_errors()


@pytest.fixture(scope="module")
def pair(ops, seeded_sd, golden):
    assert torch.cuda.is_available(), "the -m gpu tests need a ROCm GPU"
    return Pair(ops, torch.device("cuda:0"), seeded_sd, golden)


@pytest.fixture()
def warm(pair):
    """The pair for a test that rewrites the whole model: m is put back to the seeded weights afterwards."""
    try:
        yield pair
    finally:
        pair.reset()


def _names(pair, group, training=False):
    ts = pair.tensors()
    names = [k for k in ts if group_of(k) == group]
    if training:      # only these are ever packed by the training tier (row_layers, pre_layers, flow_grad._packed, LatentSolve)
        names = [k for k in names if ts[k].dim() >= 2 or k.endswith("sqrt_end_time")]
    return names


def test_every_tensor_has_a_group_and_every_cache_is_warm(pair):
    ts = pair.tensors()
    assert len(ts) == 221 + 4
    assert sorted(set(group_of(k) for k in ts)) == sorted(GROUPS)
    assert not [k for k in NO_EFFECT if ts[k].dim() >= 2], "a weight matrix that moves nothing is a bug, not an exception"
    le = pair.m.encoder.local_extract
    blk = pair.m.point_cnf.chain[1]
    assert {"w", "wx6", "wh3", "t_end"} <= set(blk._cache._store)
    assert {"conv1", "conv2", "conv3"} <= set(pair.m.encoder._cache._store)
    assert "w" in pair.m.latent_ode._cache._store
    assert any(k[0] == "commute" for k in le.feature_propagators[4]._cache._store if isinstance(k, tuple)), "the commute route was not reached"
    assert {0, 3} <= set(le._cache._store)
    assert {"conv1", "conv2", "conv3"} <= set(pair.m.encoder.global_extract._cache._store)
    keys = collections.Counter()
    for sa in le.set_abstractions:
        for pn in sa.pointnet_modules:
            keys.update("rows" if isinstance(k, tuple) else k for k in pn._cache._store)
    assert keys["l0"] and keys["pre"] and keys["rows"], "a set-abstraction route was not reached: %s" % dict(keys)


# ---------------------------------------------------------------------------------------------
# 1. / 2. one tensor at a time
# ---------------------------------------------------------------------------------------------
def _report(pair, group, training):
    stale, unmoved, moved_listed = [], [], []
    for name in _names(pair, group, training):
        t = pair.tensors()[name]
        routes = GROUP_ROUTES[group] if (t.dim() >= 2 or name in EVERY_ROUTE_1D) else [DEFAULT]
        for r, (ok, moved) in pair.probe(name, routes, training).items():
            tag = "%s @ %s" % (name, r if training else "/".join(str(v) for v in r))
            if not ok:
                stale.append(tag)
            if moved == (name in NO_EFFECT):
                (moved_listed if moved else unmoved).append(tag)
    pair.ops.check_deferred_errors()
    assert not stale, "m computes with weights it no longer has (differs from a freshly loaded model): %d cases, %s" % (len(stale), stale[:6])
    assert not unmoved, "the change moved nothing, the case is vacuous: %s" % unmoved[:6]
    assert not moved_listed, "listed in NO_EFFECT but it moves the output: %s" % moved_listed[:6]


@pytest.mark.parametrize("group", GROUPS)
def test_inference_follows_each_parameter(pair, group):
    _report(pair, group, training=False)


@pytest.mark.parametrize("group", GROUPS)
def test_training_follows_each_packed_parameter(pair, group):
    assert _names(pair, group, training=True)
    _report(pair, group, training=True)


def test_odesolver_follows_its_weights(pair, monkeypatch):
    """ODESolver._weights: the one cache site no entry point of the model reaches (the reference-shaped solver module, inference only)."""
    m, ref = pair.m, pair.ref
    z0 = torch.randn(2, m.latent_ode.input_size, generator=torch.Generator().manual_seed(5)).to(pair.dev)
    t = torch.tensor([0.0, 0.4, 1.0], device=pair.dev)
    w = m.latent_ode.ode_func.dynamics_net[2].weight
    orig = w.detach().clone()
    with torch.no_grad():
        base = m.latent_ode.solver(z0, t)
        try:
            w.mul_(SCALE)
            pair.sync_ref()
            got, want = m.latent_ode.solver(z0, t), ref.latent_ode.solver(z0, t)
            assert torch.equal(got, want) and not torch.equal(got, base)
            _freeze_weight_caches(monkeypatch, m)
            w.mul_(SCALE)
            pair.sync_ref()
            assert not torch.equal(m.latent_ode.solver(z0, t), ref.latent_ode.solver(z0, t)), "the control passes a frozen cache"
        finally:
            w.copy_(orig)
    pair.ops.check_deferred_errors()


# ---------------------------------------------------------------------------------------------
# 3. whole-model writers
# ---------------------------------------------------------------------------------------------
def _scaled(sd, names):
    return {k: (v * SCALE if k in names else v.clone()) for k, v in sd.items()}


def test_adam_step(warm):
    m = warm.m
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(2)
    for p in m.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(warm.dev)
    opt.step()
    m.zero_grad(set_to_none=True)
    warm.check_whole_model("Adam step")


def test_load_state_dict_twice_then_f64_oracle(warm, stress_sd, seeded_sd):
    """load_state_dict(stress), a run, load_state_dict(seeded): bitwise against ref, and -- so that "fresh" itself is held to f64 and not
    only to another instance of this code -- tests/test_hip_parity.py's dense reconstruct assertions on m, same oracle, same bounds.
    Under the default thresholds, as that test runs (the packs are rebuilt by the loads, under the thresholds in force then)."""
    from test_hip_parity import _reconstruct_dense_vs_oracle
    m, ops = warm.m, warm.ops
    with _thresholds(ops, *DEFAULT_THRESHOLDS):
        m.load_state_dict(stress_sd)
        r = DEFAULT._replace(cnf="x6")       # (the f16x3 solve states a range for its activations that the stress weights are not held to)
        warm.sync_ref()
        assert same(warm.infer(m, r), warm.infer(warm.ref, r)), "after load_state_dict(stress_sd)"
        assert not same(warm.infer(m, r), warm.base[r])
        m.load_state_dict(seeded_sd)
        warm.sync_ref()
        assert same(warm.infer(m, DEFAULT), warm.infer(warm.ref, DEFAULT)), "after load_state_dict(seeded_sd)"
        assert same(warm.train(m), warm.train(warm.ref))
        with torch.no_grad():
            _reconstruct_dense_vs_oracle(warm.dev, seeded_sd, m, "bf16x6")
    # ... and on every route with the module's thresholds
    m.load_state_dict(stress_sd)
    m.load_state_dict(seeded_sd)
    warm.check_whole_model("load_state_dict(stress_sd), load_state_dict(seeded_sd)")
    assert same(warm.infer(m, DEFAULT), warm.base[DEFAULT]), "the seeded weights no longer give the seeded result"


def test_cpu_round_trip_with_other_weights(warm, seeded_sd):
    m = warm.m
    names = {k for k, _ in m.named_parameters(remove_duplicate=False)}      # (both names of the aliased dynamics net)
    m.cpu()
    m.load_state_dict(_scaled(seeded_sd, names))
    m.to(warm.dev)
    warm.check_whole_model(".cpu(), load_state_dict, .to(device)")
    assert not same(warm.infer(m, DEFAULT), warm.base[DEFAULT])
    # the same with the new values ASSIGNED on the host: no version counter moves, and the device allocator is free to hand the old
    # addresses out again -- unless the caches pin the storages their entries were built from (utils/weight_cache.py)
    m.cpu()
    for p in m.parameters():
        p.data = p.data * SCALE
    m.to(warm.dev)
    warm.check_whole_model(".cpu(), p.data = t, .to(device)")


def test_assign_data_on_every_parameter(warm):
    for p in warm.m.parameters():
        p.data = p.data * SCALE
    warm.check_whole_model("p.data = t")
    assert not same(warm.infer(warm.m, DEFAULT), warm.base[DEFAULT])


def test_broadcast_model_on_device(warm, monkeypatch):
    from caspr_amd.train import loop

    def broadcast(flat, src):
        flat.mul_(SCALE) if flat.is_floating_point() else None

    monkeypatch.setattr(loop.dist, "is_available", lambda: True)
    monkeypatch.setattr(loop.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(loop.dist, "get_world_size", lambda: 2)
    monkeypatch.setattr(loop.dist, "broadcast", broadcast)
    before = warm.m.encoder.conv2.weight.detach().clone()
    loop.broadcast_model(warm.m, 0)
    assert torch.equal(warm.m.encoder.conv2.weight.detach(), before * SCALE)
    warm.check_whole_model("broadcast_model")
    assert not same(warm.infer(warm.m, DEFAULT), warm.base[DEFAULT])


def test_data_writes_then_invalidate(warm):
    """The documented exception: in-place writes through `.data` are invisible (stale: m still gives its old result), invalidate(m)
    makes everything fresh."""
    from caspr_amd.utils.weight_cache import invalidate
    m = warm.m
    w = m.encoder.conv2.weight            # read through its pack only
    # (every plane of that pack exists: a PackedWeight builds its bf16 / f16 planes at their first use, from the tensor it was given --
    # here a view of the parameter -- so planes first used AFTER such a write would hold the new values beside an old f32 pack)
    assert same(warm.infer(m, DEFAULT), warm.base[DEFAULT])
    w.data.mul_(SCALE)
    assert same(warm.infer(m, DEFAULT), warm.base[DEFAULT]), "a write through .data was noticed: the documented rule no longer describes the caches"
    for p in m.parameters():
        if p is not w:
            p.data.mul_(SCALE)
    invalidate(m)
    warm.check_whole_model(".data writes + invalidate()")
    assert not same(warm.infer(m, DEFAULT), warm.base[DEFAULT])


def test_second_model_in_the_process(pair, seeded_sd, stress_sd):
    """What a user's second model meets: the first one's parameters are dead, their ids, addresses and version counters come back."""
    from caspr_amd.models import CaSPR
    from caspr_amd.train import flow_grad as FG

    def build(sd):
        mod = CaSPR(cnf_rk4_steps=2, latent_rk4_steps=2, check_tol=None)
        mod.load_state_dict(sd)
        return mod.to(pair.dev)
    first = build(seeded_sd)
    pair.train(first)
    n_first = len(FG._pack_cache)
    del first
    gc.collect()
    assert len(FG._pack_cache) < n_first, "the dead model's packs are still cached"
    second = build(stress_sd)
    a = pair.train(second)
    FG.drop_packs()
    b = pair.train(second)
    assert same(a, b), "the second model trained on packs that were not its own"
    pair.ops.check_deferred_errors()


# ---------------------------------------------------------------------------------------------
# 4. control: a frozen cache must be reported
# ---------------------------------------------------------------------------------------------
def _freeze_weight_caches(monkeypatch, model):
    """WeightCache.get returns the first build forever -- for `model`'s caches only (ref must stay honest)."""
    from caspr_amd.utils.weight_cache import WeightCache
    mine = {id(v) for mod in model.modules() for v in vars(mod).values() if isinstance(v, WeightCache)}
    real = WeightCache.get

    def get(self, key, sources, build):
        hit = self._store.get(key)
        if id(self) in mine and hit is not None:
            return hit[1]
        return real(self, key, sources, build)
    monkeypatch.setattr(WeightCache, "get", get)


SA = LE + "set_abstractions."
# cache site (module: key) -> a weight behind it, the route on which that site is the one read
SITES = [
    ("CNF: w", FLOW + "0._hyper_gate.weight", DEFAULT),
    ("CNF: wx6", FLOW + "1._layer.weight", DEFAULT._replace(cnf="x6")),
    ("CNF: wh3", FLOW + "2._layer.weight", DEFAULT),
    ("CNF: t_end", "point_cnf.chain.1.sqrt_end_time", DEFAULT),
    ("TPointNet2: conv1", "encoder.conv1.weight", DEFAULT),
    ("TPointNet2: conv1 (the folded layer's weight)", LE + "final_layers.3.weight", DEFAULT),
    ("TPointNet2: conv2", "encoder.conv2.weight", DEFAULT),
    ("TPointNet2: conv3", "encoder.conv3.weight", DEFAULT),
    ("LatentODE: w", "latent_ode.ode_func.dynamics_net.2.weight", DEFAULT),
    ("PointNet2FeatureExtractor: l<n>", SA + "0.pointnet_modules.0.conv_layers.1.weight", DEFAULT),
    ("PointNet2FeatureExtractor: pre", SA + "2.pointnet_modules.0.conv_layers.0.weight", DEFAULT),
    ("PointNet2FeatureExtractor: rows", SA + "4.pointnet_modules.0.conv_layers.1.weight", DEFAULT),
    ("PointNet2FeaturePropagator: (i, cin_pad)", LE + "feature_propagators.1.unit_pointnet.3.weight", DEFAULT),
    ("PointNet2FeaturePropagator: commute", LE + "feature_propagators.4.unit_pointnet.0.weight", DEFAULT._replace(N=2048)),
    ("PointNet2feat: final layer", LE + "final_layers.0.weight", DEFAULT),
    ("PointNetfeat: conv<n>", "encoder.global_extract.conv2.weight", DEFAULT),
]       # (ODESolver: w -- test_odesolver_follows_its_weights)


@pytest.mark.parametrize("site,name,route", SITES, ids=[s[0].replace(" ", "_") for s in SITES])
def test_control_frozen_weight_cache_is_reported(pair, monkeypatch, site, name, route):
    pair.infer(pair.m, route)         # every pack of the route exists, lazily built planes included
    _freeze_weight_caches(monkeypatch, pair.m)
    (ok, moved), = pair.probe(name, [route]).values()
    assert not ok, "%s: the harness passes a cache that never rebuilds" % site
    pair.ops.check_deferred_errors()


def test_control_frozen_flow_grad_packs_are_reported(pair, monkeypatch):
    from caspr_amd.train import flow_grad as FG
    mine = {id(p) for p in pair.m.parameters()}
    real, kept = FG._packed, {}

    def frozen(w, transposed):
        if not isinstance(w, nn.Parameter) or id(w) not in mine:
            return real(w, transposed)
        if (id(w), transposed) not in kept:
            kept[(id(w), transposed)] = real(w, transposed)
        return kept[(id(w), transposed)]
    monkeypatch.setattr(FG, "_packed", frozen)
    pair.train(pair.m)                # the frozen packs: of the seeded weights
    (ok, moved), = pair.probe(FLOW + "1._layer.weight", None, training=True).values()
    assert kept, "the training tier no longer goes through flow_grad._packed: this control checks nothing"
    assert not ok, "the training harness passes packs that never rebuild"
    pair.ops.check_deferred_errors()
