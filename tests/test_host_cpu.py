"""CPU-side checks: the C-ABI library loads and exports every symbol include/caspr_hip.h declares,
the host model keeps the reference's surface, the product path refuses to run without a GPU, and the
multi-rank sharding logic is correct under gloo (world_size 2)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_library_exports_every_declared_symbol():
    from caspr_amd import lib
    if not os.path.exists(lib.SO_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build()
    hdr = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("caspr_hip.h", "caspr_hip_train.h"))
    declared = sorted(set(re.findall(r"\b(caspr_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 18
    so = ctypes.CDLL(lib.SO_PATH)
    for name in declared:
        assert hasattr(so, name), "libcaspr_hip.so does not export %s" % name
    assert sorted(lib.SIGNATURES) == declared, "caspr_amd/lib.py and include/*.h disagree"
    L = lib.load()
    assert L.caspr_abi_version() == 1
    assert L.caspr_packed_size(1600, 1600) == 100 * 100 * 256
    assert L.caspr_packed_size(4, 518) == 1 * 34 * 256
    # SURVEY.md 8b "no global state": the production library exports exactly the declared entries -- no caspr_debug_* hook --
    # and never reads the environment (trace hooks / experiment switches exist only in the CASPR_BUILD_DEBUG flavour)
    syms = subprocess.run(["nm", "-D", lib.SO_PATH], capture_output=True, text=True, check=True).stdout.splitlines()
    exported = sorted(l.split()[-1] for l in syms if " T caspr_" in l)
    assert exported == declared, "exported caspr_* symbols differ from include/*.h: %s" % sorted(set(exported) ^ set(declared))
    assert not [l for l in syms if l.split()[-1].split("@")[0] in ("getenv", "secure_getenv")], "the production library must not read the environment"


def test_no_cpu_fallback():
    from caspr_amd import ops
    from caspr_amd.models import CaSPR
    with pytest.raises(ValueError):
        ops.furthest_point_sampling(torch.zeros(1, 8, 3), 4)
    m = CaSPR()
    with pytest.raises(ValueError):
        m.encode(torch.zeros(1, 2, 64, 4))
    with pytest.raises(ValueError):
        m.reconstruct(torch.zeros(1, 2, 64, 4), num_points=16)


def test_model_surface_matches_reference(golden):
    from caspr_amd.models import CaSPR
    from caspr_amd.utils.torch_utils import load_weights, count_params
    m = CaSPR()
    assert [str(k) for k in golden["state_keys"]] == list(m.state_dict().keys())
    assert count_params(m) == 16262189
    for name in ("forward", "encode", "aggregate_and_solve_latent", "gen_latent", "get_nfe", "decode", "reconstruct", "get_nll_loss"):
        assert callable(getattr(m, name))
    assert m.latent_ode.input_size == 64 and m.cnf_args.zdim == 1600 and m.cnf_args.input_dim == 3
    # DataParallel-style checkpoints (module. prefix) load through the reference helper's logic (torch_utils.py:27-44)
    sd = {"module." + k: v + 1 for k, v in m.state_dict().items()}
    load_weights(m, sd)
    assert torch.equal(m.state_dict()["encoder.conv3.bias"], sd["module.encoder.conv3.bias"])
    # pretrain / no-tnocs variants keep the reference's reduced surfaces (caspr.py:55-57, tpointnet2.py:66-68)
    assert all(k.startswith("encoder.") for k in CaSPR(pretrain_tnocs=True).state_dict())
    assert "encoder.conv3.weight" not in CaSPR(regress_tnocs=False).state_dict()
    assert len(CaSPR(cnf_blocks=2).point_cnf.chain) == 4
    with pytest.raises(ValueError):
        CaSPR(radii_list=[0.1, 0.2])


def test_synthetic_generators_are_deterministic(seeded_sd):
    from caspr_amd.utils.synthetic import car_sequences, seeded_state_dict
    a, sa = car_sequences(2, 3, 64, seed=5)
    b, sb = car_sequences(2, 3, 64, seed=5)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    assert a.shape == (2, 3, 64, 4) and float(a[..., 3].max()) == 5.0 and float(sa[..., 3].max()) == 1.0
    assert float((a[..., :3] ** 2).sum(-1).min()) > 1e-3          # the FPS padding guard never triggers
    assert float(sa[..., :3].min()) >= 0.0 and float(sa[..., :3].max()) <= 1.0
    again = seeded_state_dict(seeded_sd, 0)
    assert all(torch.equal(again[k], seeded_sd[k]) for k in seeded_sd)
    assert torch.equal(seeded_sd["latent_ode.ode_func.dynamics_net.0.weight"], seeded_sd["latent_ode.solver.ode_func.dynamics_net.0.weight"])


def test_shard_range_partitions():
    from caspr_amd.utils.sharding import shard_range
    for total in (1, 7, 16, 512):
        for world in (1, 2, 3, 8):
            spans = [shard_range(total, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == total
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1


WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from caspr_amd.utils.sharding import shard_range, max_over_ranks, sum_over_ranks, gather_sharded
from caspr_amd.utils.synthetic import car_sequences
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
B = 5
x, _ = car_sequences(B, 2, 32, seed=3)
lo, hi = shard_range(B, rank, world)
local = x[lo:hi].sum(dim=(1, 2, 3)).view(-1, 1)           # stand-in for a per-sequence result
full = gather_sharded(local, B, rank, world)
assert torch.equal(full, x.sum(dim=(1, 2, 3)).view(-1, 1)), "sharded result differs from the unsharded one"
assert max_over_ranks(rank + 1.5, torch.device("cpu")) == world + 0.5
assert sum_over_ranks(hi - lo, torch.device("cpu")) == B
dist.barrier()
if rank == 0:
    print("SHARD_OK")
'''


def test_two_rank_sharding_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29533", str(script), ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "SHARD_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


TRAIN_WORKER = r'''
import os, sys, torch, torch.nn as nn, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from caspr_amd.train.loop import GradBucket, shard_batch, training_loss
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
torch.manual_seed(0)

class Tiny(nn.Module):          # stand-in with CaSPR.forward's return convention: (per-point nll (B,T,N), per-point tnocs L1 (B,T,N,4))
    def __init__(self):
        super().__init__()
        self.a, self.b = nn.Linear(4, 4), nn.Linear(4, 1)
        self.unused = nn.Parameter(torch.zeros(3))
    def forward(self, x, y):
        return (self.b(torch.tanh(self.a(x))).squeeze(-1) ** 2, (torch.sigmoid(self.a(x)) - y).abs())

B, T, N = 4, 3, 8
x, y = torch.randn(B, T, N, 4), torch.rand(B, T, N, 4)
ref = Tiny()
full, _, _ = training_loss(ref(x, y), 0.01, 100.0)
full.backward()
m = Tiny()
m.load_state_dict(ref.state_dict())
xs, ys = shard_batch(x, y)
assert xs.shape[0] == B // world
loss, _, _ = training_loss(m(xs, ys), 0.01, 100.0)
loss.backward()
bucket = GradBucket(m.parameters())
bucket.all_reduce_mean(weight=xs.shape[0])
for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
    want = q.grad if q.grad is not None else torch.zeros_like(q)
    assert p.grad is not None and torch.allclose(p.grad, want, atol=1e-6, rtol=1e-5), "gradient of %s differs after the all-reduce" % n

# unequal shards (3 sequences -> 2 + 1) and an EMPTY shard (1 sequence -> 1 + 0): train_step on every rank must neither
# deadlock nor diverge, and must apply the single-process step on the global-batch mean (train_utils.py:154,163)
from caspr_amd.train.loop import train_step
for Bg in (3, 1):
    one = Tiny(); one.load_state_dict(ref.state_dict())
    opt1 = torch.optim.Adam(one.parameters(), lr=1e-2)
    opt1.zero_grad()
    l1, _, _ = training_loss(one(x[:Bg], y[:Bg]), 0.01, 100.0)
    l1.backward()
    opt1.step()
    mm = Tiny(); mm.load_state_dict(ref.state_dict())
    optm = torch.optim.Adam(mm.parameters(), lr=1e-2)
    xs, ys = shard_batch(x[:Bg], y[:Bg])
    train_step(mm, optm, xs, ys, 0.01, 100.0, bucket=GradBucket(mm.parameters()))
    for (n, p), (_, q) in zip(mm.named_parameters(), one.named_parameters()):
        assert torch.allclose(p, q, atol=1e-6, rtol=1e-5), "B=%d rank %d: parameter %s differs from the single-process step" % (Bg, rank, n)
dist.barrier()
if rank == 0:
    print("GRAD_OK")
'''


def test_two_rank_gradient_bucket_gloo(tmp_path):
    """Sharded training step: per-rank mean losses + ONE flat all-reduce (mean) give the gradient of the reference's
    global-batch mean (train_utils.py:154,163), including parameters that received no gradient."""
    script = tmp_path / "train_worker.py"
    script.write_text(TRAIN_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29534", str(script), ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "GRAD_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


SEED_WORKER = r'''
import os, sys, torch, torch.nn as nn, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from caspr_amd.train.loop import GradBucket, broadcast_model, shard_batch, train_step
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()

class Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.b = nn.Linear(4, 4), nn.Linear(4, 1)
        self.register_buffer("running_mean", torch.randn(3))       # stands for MovingBatchNorm's statistics
        self.register_buffer("step", torch.zeros(1, dtype=torch.long) + torch.randint(0, 100, (1,)))
    def forward(self, x, y):
        return (self.b(torch.tanh(self.a(x))).squeeze(-1) ** 2, (torch.sigmoid(self.a(x)) - y).abs())

torch.manual_seed(1000 + rank)          # every rank initialises DIFFERENTLY
m = Tiny()
before = [p.detach().clone() for p in m.parameters()]
broadcast_model(m, 0)
def same_everywhere(tensors, what):
    for i, t in enumerate(tensors):
        g = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(g, t.contiguous())
        assert all(torch.equal(g[0], u) for u in g), "%s %d differs between the ranks" % (what, i)
same_everywhere([p.data for p in m.parameters()], "parameter after the broadcast")
same_everywhere([b.data for b in m.buffers()], "buffer after the broadcast")
if rank != 0:
    assert any(not torch.equal(a, p) for a, p in zip(before, m.parameters())), "the broadcast did not change rank %d" % rank
torch.manual_seed(7)                    # the same global batch on every rank, sharded
x, y = torch.randn(4, 3, 8, 4), torch.rand(4, 3, 8, 4)
opt = torch.optim.Adam(m.parameters(), lr=1e-2)
bucket = GradBucket(m.parameters())
for it in range(2):
    xs, ys = shard_batch(x, y)
    train_step(m, opt, xs, ys, 0.01, 100.0, bucket=bucket)
    # the gradients ARE the bucket: views of one flat buffer, no pack / unpack copies
    lo, hi = bucket.flat.data_ptr(), bucket.flat.data_ptr() + bucket.flat.numel() * 4
    assert all(p.grad is not None and lo <= p.grad.data_ptr() < hi for p in m.parameters()), "a gradient left the bucket"
same_everywhere([p.data for p in m.parameters()], "parameter after two steps")
# a caller that drops the gradients (optimizer.zero_grad's default) gets the views back at the next step
opt.zero_grad()
assert all(p.grad is None for p in m.parameters())
train_step(m, opt, *shard_batch(x, y), 0.01, 100.0, bucket=bucket)
assert all(p.grad is not None and lo <= p.grad.data_ptr() < hi for p in m.parameters())
same_everywhere([p.data for p in m.parameters()], "parameter after three steps")
dist.barrier()
if rank == 0:
    print("SEED_OK")
'''


def test_two_ranks_with_different_seeds_train_identical_replicas_gloo(tmp_path):
    """train() broadcasts rank 0's parameters and buffers first; the gradients are views of the flat bucket."""
    script = tmp_path / "seed_worker.py"
    script.write_text(SEED_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29536", str(script), ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "SEED_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


ORACLE_WORKER = r'''
import os, sys, torch, torch.nn as nn, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from oracle import model as O
from caspr_amd.models import CaSPR
from caspr_amd.utils.synthetic import seeded_state_dict, car_sequences
from caspr_amd.train.loop import GradBucket, training_loss, shard_batch
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
torch.set_num_threads(3)


class OracleCaSPR(nn.Module):
    """CaSPR's FULL parameter surface (the 238 state-dict keys of caspr.py, aliases and buffers included) with the CPU oracle's
    differentiable mode as its forward: what the sharded step sees on the GPU box, minus the kernels."""
    def __init__(self, sd):
        super().__init__()
        self.keys = [k for k, v in sd.items() if v.is_floating_point() and not k.endswith(("running_mean", "running_var", "_num_evals", "step"))]
        self.fixed = {k: v for k, v in sd.items() if k not in self.keys}
        self.plist = nn.ParameterList([nn.Parameter(sd[k].clone()) for k in self.keys])

    def forward(self, x, sp, e=None):
        # f32 parameters, f64 arithmetic: on these sparse clouds an f32 forward flips ReLU / max-pool selections with the batch size
        # (1e-2 of the gradient, DESIGN.md section 7), which is not what this test is about
        sd = {k: (v.double() if v.is_floating_point() else v) for k, v in self.fixed.items()}
        sd.update({k: p.double() for k, p in zip(self.keys, self.plist)})
        prev, O.GRAD_MODE = O.GRAD_MODE, True
        try:
            r, t = O.forward_nll(sd, x.double(), sp.double(), e.double(), "rk4", 2, 1)
            return r.float(), t.float()
        finally:
            O.GRAD_MODE = prev


sd = seeded_state_dict(CaSPR().state_dict(), 0)
B, T, N = 2, 2, 96
x, sp = car_sequences(B, T, N, seed=21)
torch.manual_seed(4)
e = torch.randn(B * T, N, 3)

def grads(xs, sps, es, weight=None):
    m = OracleCaSPR(sd)
    bucket = GradBucket(m.parameters()) if weight is not None else None
    if bucket is not None:
        bucket.zero()
    loss, _, _ = training_loss(m(xs, sps, e=es), 0.01, 100.0)
    loss.backward()
    if bucket is not None:
        bucket.all_reduce_mean(weight=weight)
        bucket.drop_untouched()
    return {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in zip(m.keys, m.plist)}

full = grads(x, sp, e)                                  # one process: the whole batch
xs, sps = shard_batch(x, sp)
lo = rank * (B // world)
mine = grads(xs, sps, e[lo * T:(lo + xs.shape[0]) * T], weight=xs.shape[0])
num = den = 0.0
untouched = 0
for k, g in full.items():
    h = mine[k]
    assert (g is None) == (h is None), "parameter %s: touched in one run only" % k
    if g is None:
        untouched += 1
        continue
    num += float((g.double() - h.double()).pow(2).sum())
    den += float(g.double().pow(2).sum())
rel = (num / den) ** 0.5
assert rel <= 1e-4, "rank %d: |sharded - global| / |global| = %.3e" % (rank, rel)
assert untouched >= 8, "the aliases latent_ode.solver.ode_func.* are parameters no loss term reaches: %d untouched" % untouched
dist.barrier()
if rank == 0:
    print("ORACLE_RANKS_OK rel=%.3e untouched=%d" % (rel, untouched))
'''


def test_two_rank_train_step_full_parameter_surface_gloo(tmp_path):
    """CPU twin of tests/test_multi_gpu.py::test_two_rank_train_step_of_the_real_model: CaSPR's full parameter surface with the
    CPU oracle's differentiable mode as the forward, one sequence per rank, backward + ONE flat all-reduce carrying gradients and
    touched-flags -- against the one-process gradient of the two-sequence batch; parameters no loss term reaches (the solver.*
    aliases) end with grad None on every rank."""
    script = tmp_path / "oracle_worker.py"
    script.write_text(ORACLE_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29538", str(script), ROOT], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0 and "ORACLE_RANKS_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_config_reads_the_environment_only_in_debug_mode():
    """Round-4 review: ten A/B switches were read from the environment at import; a stray CASPR_MATMUL=f32 silently changed
    kernels.  Now: defaults unless CASPR_DEBUG=1, and a knob found without it is reported, not obeyed."""
    import warnings
    from caspr_amd import config as C
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        c = C.load({"CASPR_MATMUL": "f32", "CASPR_LATENT_TEAM": "0"})
    assert c == C.KernelConfig() and any("ignored" in str(x.message) for x in w)
    c = C.load({"CASPR_DEBUG": "1", "CASPR_MATMUL": "f32", "CASPR_LATENT_TEAM": "0", "CASPR_EARLY_LATENT": "single", "CASPR_X6W_MIN_CIN": "1024"})
    assert (c.matmul, c.latent_team, c.early_latent, c.early_latent_team, c.x6w_min_cin) == ("f32", False, True, False, 1024)
    with pytest.raises(ValueError):
        C.load({"CASPR_DEBUG": "1", "CASPR_MATMUL": "bf16"})
    a = C.active()
    assert a["matmul"] == {"conv": "bf16x6", "cnf": "bf16x6"} and a["debug_env"] is False and a["sa_lo_parts"] is True


LAUNCH_WORKER = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from caspr_amd.utils.launch import ensure_ranks
from caspr_amd.utils.sharding import max_over_ranks, sum_over_ranks
n = int(sys.argv[2])
rank, local_rank, world = ensure_ranks(n, __file__, sys.argv[1:])      # returns only inside the ranks
assert world == n and "MASTER_PORT" in os.environ
dist.init_process_group("gloo")
assert dist.get_world_size() == n and dist.get_rank() == rank
assert sum_over_ranks(1, torch.device("cpu")) == n and max_over_ranks(rank, torch.device("cpu")) == n - 1
dist.barrier()
if rank == 0:
    print("LAUNCH_OK world=%d" % world)
dist.destroy_process_group()
'''


def test_plain_invocation_starts_its_own_ranks(tmp_path, monkeypatch):
    """`python script.py --gpus N` with WORLD_SIZE unset must become N ranks (bench.py / bench_train.py use the same helper);
    a launcher whose WORLD_SIZE disagrees with --gpus is refused, and so is asking for more ranks than devices."""
    from caspr_amd.utils.launch import ensure_ranks
    script = tmp_path / "launch_worker.py"
    script.write_text(LAUNCH_WORKER)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, str(script), ROOT, "2"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "LAUNCH_OK world=2" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert ensure_ranks(1, "x.py", []) == (0, 0, 1)
    with pytest.raises(RuntimeError):
        ensure_ranks(8, "x.py", [], device_count=lambda: 1)
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(RuntimeError):
        ensure_ranks(8, "x.py", [])
    monkeypatch.setenv("WORLD_SIZE", "4")
    monkeypatch.setenv("RANK", "3")
    monkeypatch.setenv("LOCAL_RANK", "3")
    assert ensure_ranks(4, "x.py", []) == (3, 3, 4)


def test_parameters_the_loss_does_not_reach_keep_grad_none_with_the_bucket():
    """Reference semantics of optimizer.zero_grad() + backward: a parameter no loss term reaches has .grad None and Adam skips it (no
    state, no weight decay).  With the gradients living in GradBucket's views every parameter would have a (zero) gradient tensor and
    weight decay would shrink the unused ones: GradBucket.drop_untouched() hands the None back.  Also: single-process validation
    returns the reference's mean of per-batch means (train_utils.py:226) on a ragged last batch."""
    from caspr_amd.train.loop import GradBucket
    torch.manual_seed(0)
    used, unused = torch.nn.Linear(4, 3), torch.nn.Linear(4, 3)
    params = list(used.parameters()) + list(unused.parameters())
    ref_used, ref_unused = torch.nn.Linear(4, 3), torch.nn.Linear(4, 3)
    ref_used.load_state_dict(used.state_dict())
    ref_unused.load_state_dict(unused.state_dict())
    ref_params = list(ref_used.parameters()) + list(ref_unused.parameters())
    opt = torch.optim.Adam(params, lr=1e-2, weight_decay=0.1)
    ref_opt = torch.optim.Adam(ref_params, lr=1e-2, weight_decay=0.1)
    bucket = GradBucket(params)
    x = torch.randn(5, 4)
    for _ in range(3):
        bucket.zero()
        used(x).pow(2).mean().backward()
        bucket.all_reduce_mean(weight=5)
        bucket.drop_untouched()
        assert all(p.grad is None for p in unused.parameters()) and all(p.grad is not None for p in used.parameters())
        opt.step()
        ref_opt.zero_grad()
        ref_used(x).pow(2).mean().backward()
        ref_opt.step()
    for p, q in zip(params, ref_params):
        assert torch.equal(p.data, q.data)
    assert torch.equal(unused.weight.data, ref_unused.weight.data) and len(opt.state) == 2


def test_training_loss_weights():
    """train_utils.py:151-165: 0.01 * mean_{b,t}(sum_n nll) + 100 * mean(tnocs[..., :4]); pretrain tuple has one entry."""
    from caspr_amd.train.loop import training_loss
    nll, tn = torch.rand(2, 3, 5), torch.rand(2, 3, 5, 4)
    loss, c, t = training_loss((nll, tn), 0.01, 100.0)
    assert torch.allclose(loss, 0.01 * nll.sum(2).mean() + 100.0 * tn.mean())
    loss1, c1, _ = training_loss((tn,), 0.01, 100.0)
    assert torch.allclose(loss1, 100.0 * tn.mean()) and float(c1) == 0.0
    with pytest.raises(ValueError):
        training_loss((nll, tn, tn), 0.01, 100.0)


def test_segments_csr_is_a_stable_inverse_index():
    """train_ops.Segments (host logic of the deterministic scatter-adds): for every target the contributing source rows in
    ascending order, weights permuted alongside; a gather-sum through it equals index_add_."""
    from caspr_amd.train_ops import Segments
    g = np.random.default_rng(4)
    n_targets, nnz, C = 37, 500, 5
    tgt = torch.from_numpy(g.integers(0, n_targets, nnz))
    tgt[tgt == 11] = 12                      # an empty segment
    w = torch.from_numpy(g.normal(0, 1, nnz).astype(np.float32))
    rows = torch.from_numpy(g.integers(0, 200, nnz))
    seg = Segments(tgt, n_targets, weight=w, src_rows=rows)
    assert seg.start[0] == 0 and seg.start[-1] == nnz and seg.start[12] == seg.start[11]
    src = torch.from_numpy(g.normal(0, 1, (200, C)).astype(np.float32))
    got = torch.zeros(n_targets, C)
    for t in range(n_targets):
        e0, e1 = int(seg.start[t]), int(seg.start[t + 1])
        assert (tgt[torch.sort(tgt, stable=True)[1][e0:e1]] == t).all()
        for e in range(e0, e1):
            got[t] += seg.w[e] * src[int(seg.row[e])]
    want = torch.zeros(n_targets, C).index_add_(0, tgt, w.unsqueeze(1) * src[rows])
    assert torch.allclose(got, want, atol=1e-5)
    # default source rows = entry positions; equal targets keep ascending positions (stable sort)
    seg2 = Segments(tgt, n_targets)
    for t in range(n_targets):
        r = seg2.row[int(seg2.start[t]):int(seg2.start[t + 1])]
        assert torch.equal(r, torch.sort(r)[0])


def test_train_loop_cadence_and_resume_on_cpu(tmp_path):
    """train.py:135-190 host logic with a stand-in model (CaSPR.forward's return convention): checkpoint names, BEST on the
    lowest validation loss, and a resumed run that ends bit-identical to the uninterrupted one."""
    import torch.nn as nn
    from caspr_amd.train.loop import train

    class Tiny(nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = nn.Linear(4, 4), nn.Linear(4, 1)

        def forward(self, x, y):
            return (self.b(torch.tanh(self.a(x))).squeeze(-1) ** 2, (torch.sigmoid(self.a(x)) - y).abs())

    torch.manual_seed(0)
    batches = [[(torch.randn(2, 3, 8, 4), torch.rand(2, 3, 8, 4))] for _ in range(3)]
    init = Tiny().state_dict()

    def fresh():
        m = Tiny()
        m.load_state_dict(init)
        return m
    dev = torch.device("cpu")
    m1 = fresh()
    out1 = tmp_path / "full"
    out1.mkdir()
    val = train(m1, batches, batches[:1], dev, str(out1), num_epochs=4, lr=1e-2, save_every=2, log=lambda s: None)
    assert len(val) == 4
    names = sorted(os.listdir(str(out1)))
    assert "BEST_time_model.pth" in names and "time_model_0.pth" in names and "time_model_2.pth" in names and "time_model_1.pth" not in names
    assert list(torch.load(str(out1 / "time_model_2.pth")).keys()) == list(init.keys())      # reference-format weights
    m2 = fresh()
    out2 = tmp_path / "resumed"
    out2.mkdir()
    val2 = train(m2, batches, batches[:1], dev, str(out2), num_epochs=4, lr=1e-2, save_every=2, log=lambda s: None,
                 resume=str(out1 / "resume_2.pth"))
    assert val2 == val
    for k in init:
        assert torch.equal(m1.state_dict()[k], m2.state_dict()[k]), k


def test_bf16x6_split_is_exact_and_six_products_are_f32_accurate():
    """The arithmetic behind csrc/gemm_bf16x6.hip / ode_bf16x6.hip, restated with torch on the CPU: (1) both three-way
    bf16 splits (truncating, as the weight packs; round-to-nearest, as v_cvt_pk_bf16_f32 in the kernels) reproduce every
    f32 value EXACTLY; (2) the six retained partial products, accumulated in f32, are as close to the f64 dot product as a
    plain f32 evaluation."""
    g = torch.Generator().manual_seed(0)
    mag = torch.exp(torch.empty(200000).uniform_(-30.0, 30.0, generator=g))
    x = (torch.randn(200000, generator=g) * mag).float()
    x = torch.cat([x, torch.tensor([0.0, 1.0, -1.0, 3.0e38, 1.1754944e-38, 1e-30, -7.3e-12])])

    def split_rn(v):
        h1 = v.bfloat16().float()
        r1 = v - h1
        h2 = r1.bfloat16().float()
        r2 = r1 - h2
        return h1, h2, r2.bfloat16().float()

    def split_trunc(v):
        def top(u):
            return (u.view(torch.int32) & -65536).view(torch.float32)
        h1 = top(v)
        r1 = v - h1
        h2 = top(r1)
        return h1, h2, top(r1 - h2)

    for split in (split_rn, split_trunc):
        h1, h2, h3 = split(x)
        for h in (h1, h2, h3):
            assert torch.equal(h.bfloat16().float(), h)                       # each part IS a bf16 number
        assert torch.equal(h1.double() + h2.double() + h3.double(), x.double())  # and the three add up exactly

    K, M, N = 512, 64, 96
    w = (torch.randn(M, K, generator=g) / K ** 0.5).float()
    a = torch.nn.functional.softplus(torch.randn(K, N, generator=g)).float()
    ref = w.double() @ a.double()
    w1, w2, w3 = split_trunc(w)
    a1, a2, a3 = split_rn(a)
    six = ((w3 @ a1) + (w2 @ a2) + (w1 @ a3)) + ((w2 @ a1) + (w1 @ a2)) + (w1 @ a1)   # f32 accumulation, smallest terms first
    e6, e32 = float((six.double() - ref).abs().max()), float(((w @ a).double() - ref).abs().max())
    assert e6 <= 1.5 * e32 + 1e-7, (e6, e32)
    three = (w1 @ a1) + (w1 @ a2) + (w2 @ a1)                                  # what "bf16x3" would give: not f32-accurate
    assert float((three.double() - ref).abs().max()) > 3.0 * e32


def _audit(src):
    from caspr_amd.csrc import audit
    obj = os.path.join(ROOT, "caspr_amd", "csrc", src.replace(".hip", ".o"))
    if not (os.path.exists(obj) and audit.tools_present()):
        pytest.skip("needs the in-tree object and the ROCm LLVM tools")
    return audit, obj


def test_cnf_x6w_kernel_keeps_its_accumulator_file_to_itself():
    """cnf_rk4_x6w_kernel (csrc/ode_bf16x6w.hip) manages a0..a255 by hand through inline asm; hipcc must keep out of them and
    must not spill (a scratch reload would also drain the LDS-DMA queue with vmcnt(0)).  The check itself lives in
    caspr_amd/csrc/audit.py and ALSO runs inside build() before the library is linked; here it runs on the in-tree object."""
    audit, obj = _audit("ode_bf16x6w.hip")
    r = audit.audit_cnf_x6w(obj)
    assert r["accvgpr_reads"] == 512 and r["accvgpr_writes"] == 512 and r["mfma_on_acc"] == 384, r


def test_conv_x6w_kernel_keeps_its_accumulator_file_to_itself():
    """The same audit for conv1x1_x6w_kernel (csrc/gemm_bf16x6w.hip, every instantiation)."""
    audit, obj = _audit("gemm_bf16x6w.hip")
    r = audit.audit_conv_x6w(obj)
    assert len(r) >= 4 and all(k["mfma"] == 384 for k in r), r


def test_library_holds_no_packed_f32_instructions(tmp_path):
    """Round 6: the product objects are compiled without v_pk_add / v_pk_mul / v_pk_fma_f32 (csrc/build.py: NO_PACKED_F32; why: audit.audit_no_packed_f32
    and the header of fps_kernel in csrc/point_ops.hip).  Every in-tree object passes the check build() runs before linking, and the check has teeth: the
    index kernels' source compiled WITHOUT the switch -- the compiler's own SLP vectorisation puts packed instructions into it -- is refused."""
    from caspr_amd.csrc import audit, build as B
    if not audit.tools_present():
        pytest.skip("needs the ROCm LLVM tools")
    objs = {s_: os.path.join(ROOT, "caspr_amd", "csrc", s_.replace(".hip", ".o")) for s_ in B.SOURCES}
    if not all(os.path.exists(o) for o in objs.values()):
        pytest.skip("needs the in-tree objects (python -c 'import __graft_entry__ as g; g.build()')")
    assert audit.audit_no_packed_f32(objs) == {s_: 0 for s_ in B.SOURCES}
    src = os.path.join(ROOT, "caspr_amd", "csrc", "point_ops.hip")
    obj = str(tmp_path / "packed.o")
    flags = [f for f in B.FLAGS if f not in B.NO_PACKED_F32] + B.EXTRA["point_ops.hip"]
    r = subprocess.run([B.HIPCC] + flags + ["-c", src, "-o", obj], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-500:]
    with pytest.raises(audit.AuditError, match="packed-f32"):
        audit.audit_no_packed_f32({"point_ops.hip": obj})


def test_build_refuses_a_code_object_whose_accumulator_file_the_compiler_touched(tmp_path):
    """The build-time gate: the same kernel compiled WITHOUT -amdgpu-mfma-vgpr-form (hipcc then parks layer 2's accumulators on top of
    the hand-managed ones) must be rejected by audit_objects -- i.e. build() would not link it."""
    audit, _ = _audit("ode_bf16x6w.hip")
    from caspr_amd.csrc import build as B
    src = os.path.join(ROOT, "caspr_amd", "csrc", "ode_bf16x6w.hip")
    obj = str(tmp_path / "bad.o")
    flags = [f for f in B.EXTRA["ode_bf16x6w.hip"] if f != "-amdgpu-mfma-vgpr-form"]
    flags = [f for i, f in enumerate(flags) if not (f == "-mllvm" and (i + 1 >= len(flags) or flags[i + 1] == "-mllvm" or not flags[i + 1].startswith("-")))]
    r = subprocess.run([B.HIPCC] + B.FLAGS + flags + ["-c", src, "-o", obj], capture_output=True, text=True)
    if r.returncode != 0:
        return          # does not even compile without the flag (register budget): equally not linked
    with pytest.raises(audit.AuditError):
        audit.audit_objects({"ode_bf16x6w.hip": obj})


def test_plan_times_is_the_sorted_unique_mapping_of_the_reference():
    """LatentODE.plan_times (the time-stamp bookkeeping reconstruct() queues ahead of the encoder): solving at ALL B*T sorted stamps
    and gathering (row b, position pos[b, t]) must pick, for every entry, the solution at ITS stamp -- what the reference gets
    from torch.unique(sorted=True, return_inverse=True) (caspr.py:166-176) -- and count the evaluations of the distinct intervals."""
    from caspr_amd.models.latent_ode_model import LatentODE
    lat = LatentODE(input_size=64, hidden_size=512, num_layers=2)
    lat.rk4_steps = 2
    g = torch.Generator().manual_seed(3)
    times = torch.rand(4, 6, generator=g)
    times[1, 2] = times[0, 0]                     # repeats across and inside sequences
    times[2, :] = times[2, 0]
    plan = lat.plan_times(times)
    B, T = times.shape
    assert plan["shape"] == (B, T) and plan["sorted_t"].shape == (B * T,)
    assert bool((plan["sorted_t"][1:] >= plan["sorted_t"][:-1]).all())
    # a "solution" that is just the stamp itself: out[b, k] = sorted_t[k]
    out = plan["sorted_t"].view(1, -1, 1).expand(B, B * T, 1)
    picked = out[plan["rows"], plan["pos"], :][..., 0]
    assert torch.equal(picked, times.float())
    solve_t, time_map = torch.unique(times, sorted=True, return_inverse=True)
    assert torch.equal(solve_t[time_map], picked)
    assert int(plan["evals"]) == 4 * lat.rk4_steps * (solve_t.numel() - 1)


def test_cnf_row_layout_views_match_the_kernel_formula():
    """The (2R, C) tensors of a CNF training solve in the layout blk = 32 (include/caspr_hip_train.h): value row of point p =
    (p / blk) 2 blk + p % blk, tangent row = value row + blk -- the views caspr_amd/train/flow_grad.py takes of them (frames in
    front, blocks of blk value rows | blk tangent rows) address exactly those rows."""
    BT, n, blk, c = 3, 128, 32, 4
    R = BT * n
    z = torch.arange(2 * R * c, dtype=torch.float32).view(2 * R, c)
    zz = z.view(BT, n // blk, 2, blk, c)
    zv, zt = zz[:, :, 0].reshape(R, c), zz[:, :, 1].reshape(R, c)
    p = torch.arange(R)
    vrow = (p // blk) * 2 * blk + p % blk
    assert torch.equal(zv, z[vrow]) and torch.equal(zt, z[vrow + blk])
    # a frame's rows are contiguous: frame f owns rows [2 n f, 2 n (f + 1)) -- what lets the conv treat a frame as a batch entry
    f = p // n
    assert bool(((vrow >= 2 * n * f) & (vrow + blk < 2 * n * (f + 1))).all())


def test_bench_box_calibration_is_optional_and_parses_the_micro_benchmark(tmp_path, monkeypatch):
    """bench.py's config.box: None when tools/micro/mfma_power is not built or fails; otherwise the best rate per operand kind."""
    import importlib.util
    import subprocess
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    real_exists = os.path.exists
    monkeypatch.setattr(os.path, "exists", lambda p: False if p.endswith("mfma_power") else real_exists(p))
    assert bench.box_calibration() is None
    monkeypatch.setattr(os.path, "exists", lambda p: True if p.endswith("mfma_power") else real_exists(p))

    class R:
        stdout = "\n".join(["data 0:    88.44 ms   2428.2 TFLOP/s  (= 2.316 GHz effective at 32 cycles / MFMA)",
                            "data 3:   121.16 ms   1772.4 TFLOP/s  (= 1.690 GHz)", "data 3:   121.77 ms   1763.6 TFLOP/s  (= 1.682 GHz)",
                            "data 7:   117.52 ms   1827.3 TFLOP/s  (= 1.743 GHz)"]) + "\n"
    monkeypatch.setattr(subprocess, "run", lambda *a, **k: R())
    box = bench.box_calibration()
    assert box["bare_mfma_bf16_tflops"] == {"zeros": 2428.2, "random_sign_exponent_mantissa": 1772.4, "bf16x6_operand_planes": 1827.3}
    monkeypatch.setattr(subprocess, "run", lambda *a, **k: (_ for _ in ()).throw(OSError("no such binary")))
    assert bench.box_calibration() is None


def test_bench_dump_outputs_writes_float_arrays_within_the_limit(tmp_path):
    """bench.py --dump-outputs: reconstruct()'s four results as <name>.npy in float32 (float64 kept), None skipped; over the byte limit
    every array keeps the same seeded subset of its rows, the same from call to call."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    g = torch.Generator().manual_seed(0)
    y, x = torch.randn(2, 3, 64, 3, generator=g), torch.randn(2, 3, 64, 3, generator=g)
    tn = torch.randn(2, 3, 64, 4, generator=g, dtype=torch.float64)
    saved = bench.dump_outputs(str(tmp_path / "all"), (y, None, x, tn))
    assert saved == {"y": (2, 3, 64, 3), "x": (2, 3, 64, 3), "tnocs": (2, 3, 64, 4)}
    assert sorted(os.listdir(tmp_path / "all")) == ["tnocs.npy", "x.npy", "y.npy"]
    a = np.load(tmp_path / "all" / "x.npy")
    assert a.dtype == np.float32 and np.array_equal(a, x.numpy())
    assert np.load(tmp_path / "all" / "tnocs.npy").dtype == np.float64
    limit = (4 * (y.numel() + x.numel()) + 8 * tn.numel()) // 4          # a quarter of the total
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), (y, None, x, tn), limit=limit)
    files = sorted(os.listdir(tmp_path / "s1"))
    assert files == ["tnocs.npy", "x.npy", "y.npy"]
    assert sum(os.path.getsize(tmp_path / "s1" / f) - 128 for f in files) <= limit       # 128-byte .npy header
    for f in files:
        a, b = np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f)
        assert a.shape[0] == 2 * 3 * 64 // 4 and np.array_equal(a, b)
    # the sample is a subset of the rows, in order
    xs, rows = np.load(tmp_path / "s1" / "x.npy"), x.numpy().reshape(-1, 3)
    idx = [int(np.flatnonzero((rows == r).all(axis=1))[0]) for r in xs]
    assert idx == sorted(idx) and np.array_equal(rows[idx], xs)


def test_step_count_search_refines_between_powers_of_two():
    """CaSPR.calibrate_rk4_steps' search (models/caspr.py:_first_passing) on a synthetic 4th-order error law: the first passing power of
    two is found, then the counts between the last failing one and it are tried where the law predicts they pass -- and every accepted
    count was VERIFIED by an evaluation (nothing is accepted on the prediction alone)."""
    from caspr_amd.models.caspr import _first_passing, _other_steps
    calls = []

    def law(C, p=4.0):
        def diff_of(S):
            calls.append(S)
            return C / float(S) ** p
        return diff_of
    # the round-5 trained checkpoint: diff(8) = 3.17e-5, diff(16) = 1.79e-6 -> 11 (3.17e-5 (8/11)^4 = 8.9e-6)
    S, diffs = _first_passing(law(3.17e-5 * 8 ** 4), (1, 2, 4, 8, 16, 32), 1e-5)
    assert S == 11 and diffs[11] <= 1e-5 < diffs[8] and 16 in diffs and S in calls
    # a flow that passes at the first candidate, or at adjacent candidates: nothing to refine
    assert _first_passing(law(1e-9), (1, 2, 4), 1e-5)[0] == 1
    assert _first_passing(law(1.5e-5), (1, 2, 4), 1e-5)[0] == 2
    # none passes: the largest candidate, as before
    assert _first_passing(law(1.0), (1, 2, 4), 1e-5)[0] == 4
    # not yet in the asymptotic regime (observed order 2 between the bracketing candidates): the guess follows the OBSERVED order, and a
    # failed guess moves up one count at a time, at most three solves, else the power of two stands
    S2, d2 = _first_passing(law(1e-5 * 12 ** 2 * 0.999, p=2.0), (8, 16), 1e-5)
    assert S2 == 12 and all(d2[k] > 1e-5 for k in d2 if k < 12)
    stubborn = lambda S: 1e-4 if S < 16 else 1e-6          # a cliff: no count below 16 passes
    S3, d3 = _first_passing(stubborn, (8, 16), 1e-5)
    assert S3 == 16 and len([k for k in d3 if 8 < k < 16]) <= 3
    assert _first_passing(law(3.17e-5 * 8 ** 4), (8, 16), 1e-5, refine=False)[0] == 16
    # the guard's comparison partner: half the steps (floor) with the Richardson factor of THAT ratio; S = 1 doubles
    assert _other_steps(8) == (4, 1.0 / 15.0) and _other_steps(1) == (2, 16.0 / 15.0)
    s2, f = _other_steps(11)
    assert s2 == 5 and abs(f - 1.0 / ((11 / 5) ** 4 - 1.0)) < 1e-15
    # the factor recovers e_S exactly under the S^-4 law: e_S' - e_S = diff
    for S_ in (2, 3, 11, 12, 17):
        o, fac = _other_steps(S_)
        e = lambda n: 7.0 / n ** 4
        assert abs(fac * (e(o) - e(S_)) - e(S_)) < 1e-12 * e(S_) + 1e-18
