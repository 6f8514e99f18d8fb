"""Cache of kernel-ready (packed / transposed / concatenated) weights derived from nn.Parameters.

Entries are rebuilt when any source tensor changes storage or is modified in place
(load_state_dict, optimizer steps, .to(device), `p.data = t`, nn.init), detected through (data_ptr, _version, device).

An entry keeps an alias of every storage it was built from.  The address in its signature can therefore not be handed out
again while the entry lives: a storage that is freed and re-allocated between two calls (module.double().float(), .cpu()
followed by .to(device)) comes back at another address even when the version counter did not move in between.

THE `.data` RULE.  In-place writes THROUGH `.data` (`p.data.mul_(d)`, `p.data.copy_(t)`, an EMA or a weight clip written that
way) change neither the address nor `p._version`: they are invisible to every cache of this package, and the kernels go on
reading the packs of the old values (or a mixture: ops.PackedWeight builds its bf16 / f16 planes at their first use, which may
come after the write).  Write under `torch.no_grad()` instead (`p.mul_(d)`, `p.copy_(t)`), or call
`invalidate(module)` after such a write.
"""
import sys


class WeightCache:
    def __init__(self):
        self._store = {}

    def get(self, key, sources, build):
        sig = tuple((t.data_ptr(), t._version, t.device) for t in sources)
        hit = self._store.get(key)
        if hit is not None and hit[0] == sig:
            return hit[1]
        val = build()
        self._store[key] = (sig, val, tuple(t.detach() for t in sources))      # the aliases pin the storages behind `sig`
        return val

    def clear(self):
        self._store.clear()


def invalidate(module):
    """Drop every derived weight under `module`: all WeightCache entries of its submodules and the training tier's packs of its
    parameters (train/flow_grad.py).  The next call of the model rebuilds them from the parameters as they are then.  Needed only
    after in-place writes through `.data` (see the module docstring); every other way of changing a parameter is noticed."""
    for mod in module.modules():
        for v in vars(mod).values():
            if isinstance(v, WeightCache):
                v.clear()
    flow_grad = sys.modules.get(__name__.rsplit(".", 2)[0] + ".train.flow_grad")     # not imported: it holds nothing
    if flow_grad is not None:
        flow_grad.drop_packs(module.parameters())
