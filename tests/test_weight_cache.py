"""Do the derived weights follow their parameters?  (CPU: no GPU, no library load.)

Every matrix product of the package reads a packed / transposed / folded copy of an nn.Parameter, kept in a `WeightCache` next to the module
(utils/weight_cache.py) or, for the training tier, in `train.flow_grad._packed`.  The kernel tests hold the kernels to f64; these hold the
caches to the parameters: an entry is rebuilt after every way of changing a parameter that the package promises to notice, it is NOT rebuilt
when nothing that enters a pack changed, and it never outlives -- or is mistaken for -- the parameter it was built from.

`ops.PackedWeight` is replaced by a stub that keeps a clone of what it was given, so "fresh" is a plain comparison with the parameter.
tests/test_derived_weights.py asks the same of the real model on the GPU, bit for bit.
"""
import gc
import weakref

import pytest
import torch
import torch.nn as nn


class StubPack:
    """Stands in for ops.PackedWeight: remembers what it was built from."""
    built = 0

    def __init__(self, w2d, col0=0, ncols=None):
        StubPack.built += 1
        self.kept = w2d.clone()


@pytest.fixture()
def ops(monkeypatch):
    from caspr_amd import ops as _ops
    monkeypatch.setattr(_ops, "PackedWeight", StubPack)
    return _ops


@pytest.fixture()
def FG(ops):
    from caspr_amd.train import flow_grad
    return flow_grad


# ---------------------------------------------------------------------------------------------
# 1. lifetime of the training tier's packs
# ---------------------------------------------------------------------------------------------
def test_flow_grad_pack_dies_with_its_parameter(FG):
    gc.collect()
    n0 = len(FG._pack_cache)
    lin = nn.Linear(64, 64)
    a, at = FG._packed(lin.weight, False), FG._packed(lin.weight, True)
    assert FG._packed(lin.weight, False) is a and FG._packed(lin.weight, True) is at, "an unchanged parameter is packed once per orientation"
    assert torch.equal(a.kept, lin.weight.detach()) and torch.equal(at.kept, lin.weight.detach().t())
    assert len(FG._pack_cache) == n0 + 1, "one entry per parameter"
    alive = [weakref.ref(a), weakref.ref(at)]
    del lin, a, at
    gc.collect()
    assert len(FG._pack_cache) == n0, "the entry of a dead parameter stays in flow_grad._pack_cache (%d entries, %d before)" % (len(FG._pack_cache), n0)
    assert all(r() is None for r in alive), "the packs of a dead parameter are still referenced"


def test_flow_grad_pack_is_never_a_dead_parameters(FG):
    """Build, fill, pack and drop the same layer over and over: Python hands out the dead parameter's id again, the allocator its address,
    and the version counters agree.  Every pack must hold the weight it was asked for -- and the loop must actually meet the collision."""
    seen, collisions, wrong = set(), 0, []
    for trial in range(200):
        lin = nn.Linear(64, 64)
        with torch.no_grad():
            lin.weight.fill_(float(trial))
        w = lin.weight
        triple = (id(w), w.data_ptr(), w._version)
        collisions += triple in seen          # every earlier parameter is dead by now
        seen.add(triple)
        pw = FG._packed(w, False)
        if not torch.equal(pw.kept, w.detach()):
            wrong.append((trial, float(pw.kept[0, 0])))
        del lin, w, pw
    assert not wrong, "round -> the dead parameter's value it was handed instead: %s (%d of 200 rounds)" % (wrong[:6], len(wrong))
    assert collisions > 0, "precondition not reached: no round repeated the (id, data_ptr, _version) of a dead parameter in 200 rounds"


def test_flow_grad_packs_temporaries_fresh(FG):
    n0 = len(FG._pack_cache)
    t = torch.randn(8, 8)
    a, b = FG._packed(t, False), FG._packed(t, False)
    assert a is not b and len(FG._pack_cache) == n0
    t.mul_(2.0)
    assert torch.equal(FG._packed(t, True).kept, t.t())


# ---------------------------------------------------------------------------------------------
# 2. what a WeightCache entry notices
# ---------------------------------------------------------------------------------------------
def _layer(seed=0, width=8):
    from caspr_amd.utils.weight_cache import WeightCache
    torch.manual_seed(seed)
    lin = nn.Linear(width, width)
    lin._cache = WeightCache()
    return lin


def _derived(ops, lin):
    """As the model's sites do it: sources and closure look the parameters up at call time."""
    return lin._cache.get("w", [lin.weight, lin.bias], lambda: (ops.PackedWeight(lin.weight.detach()), lin.bias.detach().clone()))


def _is_current(val, lin):
    return torch.equal(val[0].kept, lin.weight.detach().float()) and torch.equal(val[1], lin.bias.detach().float())


def _other_sd():
    return {k: v.clone() for k, v in _layer(1).state_dict().items()}


def _no_grad_mul(lin):
    with torch.no_grad():
        lin.weight.mul_(1.5)
        lin.bias.add_(0.25)


def _step(cls, **kw):
    def change(lin):
        opt = cls(lin.parameters(), lr=0.1, **kw)
        lin.weight.grad, lin.bias.grad = torch.ones_like(lin.weight), torch.ones_like(lin.bias)
        opt.step()
    return change


def _set_data(lin):
    lin.weight.data = torch.full_like(lin.weight, 3.0)
    lin.bias.data = torch.full_like(lin.bias, -1.0)


def _state_dict_write(lin):
    sd = lin.state_dict()
    sd["weight"].mul_(2.0)
    sd["bias"].sub_(1.0)


def _init(lin):
    nn.init.normal_(lin.weight)
    nn.init.constant_(lin.bias, 0.5)


REBUILD = {
    "no_grad_inplace": _no_grad_mul,
    "sgd": _step(torch.optim.SGD, foreach=False), "sgd_foreach": _step(torch.optim.SGD, foreach=True),
    "adam": _step(torch.optim.Adam, foreach=False), "adam_foreach": _step(torch.optim.Adam, foreach=True),
    "load_state_dict": lambda lin: lin.load_state_dict(_other_sd()),
    "load_state_dict_assign": lambda lin: lin.load_state_dict(_other_sd(), assign=True),
    "set_data": _set_data,
    "double_float": lambda lin: lin.double().float(),
    "state_dict_inplace": _state_dict_write,
    "nn_init": _init,
}


@pytest.mark.parametrize("how", sorted(REBUILD))
def test_weight_cache_rebuilds_after(ops, how):
    lin = _layer()
    first = _derived(ops, lin)
    assert _derived(ops, lin) is first and _is_current(first, lin)
    before = (lin.weight.detach().clone(), lin.bias.detach().clone())
    REBUILD[how](lin)
    if how != "double_float":      # (an exact round trip: the values are the same, the storages are not)
        assert not torch.equal(before[0], lin.weight.detach()) and not torch.equal(before[1], lin.bias.detach()), "the change changed nothing"
    second = _derived(ops, lin)
    assert second is not first, "%s: the entry was not rebuilt" % how
    assert _is_current(second, lin), "%s: the rebuilt entry is not the current content" % how
    assert _derived(ops, lin) is second


def test_weight_cache_entry_pins_the_storage_it_was_built_from(ops):
    """A storage that is freed and allocated again between two calls, with new values assigned in between through `p.data = t` (no
    version counter moves): half(), assign, float().  The allocator is free to hand the old address out again -- 3 of 20 rounds did
    on the CPU when this was written -- and (data_ptr, _version, device) would then be what it was.  An entry keeps its sources'
    storages alive, so the address of its signature cannot come back while it can still be hit."""
    stale, reused = [], 0
    for trial in range(100):
        lin = _layer(trial, 64)
        first = _derived(ops, lin)
        ptr = lin.weight.data_ptr()
        lin.half()
        for p in lin.parameters():
            p.data = p.data * 2
        lin.float()
        reused += lin.weight.data_ptr() == ptr
        second = _derived(ops, lin)
        if second is first or not _is_current(second, lin):
            stale.append(trial)
    assert not stale, "the entry of the old values was returned in rounds %s (%d of 100)" % (stale[:8], len(stale))
    assert reused == 0


def _grads(lin):
    lin.weight.grad = torch.ones_like(lin.weight)
    lin.bias.grad = torch.ones_like(lin.bias)
    lin.weight.grad.zero_()
    lin.zero_grad(set_to_none=False)
    lin.zero_grad()


def _toggle(lin):
    for p in lin.parameters():
        p.requires_grad_(False)
    for p in lin.parameters():
        p.requires_grad_(True)


KEEP = {
    "nothing": lambda lin: None,
    "requires_grad": _toggle,
    "grad": _grads,
    "train_eval": lambda lin: lin.train().eval().train(),
}


@pytest.mark.parametrize("how", sorted(KEEP))
def test_weight_cache_keeps_its_entry_after(ops, how):
    lin = _layer()
    first = _derived(ops, lin)
    n = StubPack.built
    KEEP[how](lin)
    assert _derived(ops, lin) is first and StubPack.built == n, "%s: the entry was rebuilt" % how
    assert _is_current(first, lin)


def test_data_inplace_is_stale_until_invalidated(ops, FG):
    """The documented exception (utils/weight_cache.py): a write through `.data` moves neither address nor version.
    What the package promises: the old packs until invalidate(module), the new values afterwards -- in both kinds of cache."""
    from caspr_amd.utils.weight_cache import invalidate
    lin = _layer()
    first, tfirst = _derived(ops, lin), FG._packed(lin.weight, True)
    old = lin.weight.detach().clone()
    lin.weight.data.mul_(2.0)
    lin.bias.data.add_(1.0)
    assert _derived(ops, lin) is first and torch.equal(first[0].kept, old)
    assert FG._packed(lin.weight, True) is tfirst
    invalidate(lin)
    second, tsecond = _derived(ops, lin), FG._packed(lin.weight, True)
    assert second is not first and _is_current(second, lin)
    assert tsecond is not tfirst and torch.equal(tsecond.kept, lin.weight.detach().t())
    assert _derived(ops, lin) is second and FG._packed(lin.weight, True) is tsecond


def test_invalidate_reaches_every_cache_of_a_model(ops):
    """invalidate(model) empties the WeightCache of every submodule that has one (found by type, not by a list of names)."""
    from caspr_amd.models import CaSPR
    from caspr_amd.utils.weight_cache import WeightCache, invalidate
    m = CaSPR()
    caches = [v for mod in m.modules() for v in vars(mod).values() if isinstance(v, WeightCache)]
    assert len(caches) >= 8
    for i, c in enumerate(caches):
        c.get("probe", [], lambda i=i: i)
    invalidate(m.encoder)
    enc = {id(v) for mod in m.encoder.modules() for v in vars(mod).values() if isinstance(v, WeightCache)}
    assert all((len(c._store) == 0) == (id(c) in enc) for c in caches), "invalidate(submodule) clears that submodule's caches and no others"
    invalidate(m)
    assert all(len(c._store) == 0 for c in caches)


# ---------------------------------------------------------------------------------------------
# 3. broadcast_model through a stubbed collective
# ---------------------------------------------------------------------------------------------
class _Replica(nn.Module):
    """The shapes of the real model that matter here: a dynamics net registered under two names (latent_ode_model.py), float buffers,
    an integer buffer (a second dtype) and an empty tensor."""

    def __init__(self):
        super().__init__()
        from caspr_amd.models.latent_ode_model import LatentODE
        self.latent_ode = LatentODE(input_size=8, hidden_size=8)
        self.bn = nn.BatchNorm1d(4)
        self.register_buffer("empty", torch.zeros(0))


def test_broadcast_model_advances_versions(ops, monkeypatch):
    from caspr_amd.train import loop
    from caspr_amd.utils.weight_cache import WeightCache
    torch.manual_seed(3)
    m = _Replica()
    named = list(m.named_parameters(remove_duplicate=False)) + list(m.named_buffers(remove_duplicate=False))
    assert any(k.startswith("latent_ode.solver.ode_func.") for k, _ in named), "the alias this test is about is gone"
    assert all(p.is_leaf and p.requires_grad for p in m.parameters())
    for p in m.parameters():
        p.grad = torch.full_like(p, 7.0)
    uniq = {}
    for k, t in named:
        if t.numel():
            uniq.setdefault(t.data_ptr(), (k, t))
    cache = WeightCache()
    entry = lambda k, t: cache.get(k, [t], lambda: t.detach().clone())
    before = {k: dict(version=t._version, ptr=t.data_ptr(), value=t.detach().clone(), grad=getattr(t, "grad", None), rg=t.requires_grad, entry=entry(k, t))
              for k, t in uniq.values()}
    calls = []

    def broadcast(flat, src):
        calls.append((flat.dtype, flat.numel(), src))
        flat.add_(1)            # what "rank src" holds

    monkeypatch.setattr(loop.dist, "is_available", lambda: True)
    monkeypatch.setattr(loop.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(loop.dist, "get_world_size", lambda: 2)
    monkeypatch.setattr(loop.dist, "broadcast", broadcast)
    loop.broadcast_model(m, 0)
    # one flat collective per dtype, every storage in it once
    want = {}
    for k, t in uniq.values():
        want[t.dtype] = want.get(t.dtype, 0) + t.numel()
    assert sorted(calls, key=str) == sorted(((dt, n, 0) for dt, n in want.items()), key=str)
    for k, t in uniq.values():
        b = before[k]
        assert torch.equal(t.detach(), b["value"] + 1), "%s: not what the collective delivered (written %s)" % (k, "twice" if torch.equal(t.detach(), b["value"] + 2) else "wrong")
        assert t._version > b["version"], "%s: content changed, _version still %d" % (k, t._version)
        assert t._version == b["version"] + 1, "%s: written %d times" % (k, t._version - b["version"])
        assert t.data_ptr() == b["ptr"] and t.requires_grad == b["rg"] and t.is_leaf
        assert getattr(t, "grad", None) is b["grad"]
        if b["grad"] is not None:
            assert torch.equal(b["grad"], torch.full_like(t, 7.0))
        now = entry(k, t)
        assert now is not b["entry"] and torch.equal(now, t.detach()), "%s: a WeightCache entry keyed on it was not rebuilt" % k
    # both names of the aliased net still are one tensor
    assert m.latent_ode.solver.ode_func.dynamics_net[0].weight is m.latent_ode.ode_func.dynamics_net[0].weight
