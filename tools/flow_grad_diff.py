#!/usr/bin/env python
"""Compare the three CNF block nodes of this tree's train/flow_grad.py with another copy's, bit for bit.

    python tools/flow_grad_diff.py OTHER_FLOW_GRAD_PY [--cpu]

OTHER_FLOW_GRAD_PY is another version of caspr_amd/train/flow_grad.py (say, `git show <parent>:caspr_amd/train/flow_grad.py` written to a
file).  It is loaded as a sibling module of this tree's, so both run on the same kernels, wrappers and packed weights; CnfBlockSolve,
CnfSampleSolve and CnfSampleSolveFrames of both then run on identical inputs, and every output and every gradient (y / x / logpx, the
four layer-major hyper tensors, t_end, the weights and biases that require one) is compared with torch.equal.  One table: a row per
tensor, a column per node, `identical` or the number of differing elements and the largest difference over the node's cases.  The exit
status is non-zero on any difference.

--cpu   no GPU: the launches and the evaluations are the f64 restatements of the three *_sweep_algebra_* tests (imported from tests/),
        at those tests' sizes.
default the real nodes on the GPU at the shapes of GRAD_CASES of tests/test_cnf_sample_grad.py and tests/test_cnf_sample_grad_frames.py
        and, for CnfBlockSolve, one frame of 64 points (the smallest _fused_layer_ok takes) at S = 2 and S = 3; stress weights.  Each
        node runs once more with only the weight matrices requiring a gradient."""
import importlib.util
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from caspr_amd import ops  # noqa: E402
from caspr_amd.train import flow_grad as FG  # noqa: E402

NODES = ("CnfBlockSolve", "CnfSampleSolve", "CnfSampleSolveFrames")
HYPER = ("G_lm", "Bb_lm", "tg_lm", "tb_lm")


def load_other(path):
    spec = importlib.util.spec_from_file_location("caspr_amd.train._flow_grad_other", path)     # the name makes `from .. import ops` resolve
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def run(mod, node, L, steps):
    """One node of `mod` forward and backward of sum(w * out) on the leaves L -> {tensor name: value}."""
    hyp, wb = [L[k] for k in HYPER], L["wb"]
    if node == "CnfBlockSolve":
        outs = mod.CnfBlockSolve.apply(L["y"], L["logpx"], *hyp, L["t_end"], L["e"], L["w1x"], L["w2x"], steps, L["widths"], *wb)
        names, leaves = ("x_T", "logp_T"), {"d y": L["y"], "d logpx": L["logpx"]}
    elif node == "CnfSampleSolve":
        outs = (mod.CnfSampleSolve.apply(L["y"], *hyp, L["t_end"], L["w1x"], L["w2x"], steps, L["widths"], *wb),)
        names, leaves = ("x_T",), {"d y": L["y"]}
    else:
        outs = (mod.CnfSampleSolveFrames.apply(L["y"], *hyp, L["t_end"], L["w1x"], L["w2x"], steps, ops.CNF_MAX_TABLE_STEPS, L["widths"], *wb),)
        names, leaves = ("x_T",), {"d y": L["y"]}
    leaves.update({"d " + k: L[k] for k in HYPER + ("t_end",)})
    leaves.update({"d %s%d" % ("wb"[i % 2], i // 2): w for i, w in enumerate(wb) if w.requires_grad})
    grads = torch.autograd.grad(sum((o * w).sum() for o, w in zip(outs, (L["wy"], L["wl"]))), list(leaves.values()))
    return dict(zip(names, (o.detach() for o in outs)), **dict(zip(leaves, grads)))


def cpu_cases(other):
    """The sizes and f64 restatements of the three CPU algebra tests; random f64 leaves."""
    import test_cnf_block_node as TB
    import test_cnf_sample_grad as TS
    import test_cnf_sample_grad_frames as TF
    BT, n, widths, cin = 4, 5, (7, 6, 5, 3), (3, 7, 6, 5)
    FG.T.cnf_train_fwd, FG.T.cnf_sample_tape = TB._fwd_restatement(BT, n, widths), TS._tape_restatement(BT, n, widths)
    FG.T.cnf_sample_tape_frames, ops.cnf_steps_order = TF._tape_frames_restatement(BT, n, widths, []), TF._order_of
    for m in (FG, other):
        m._cnf_eval_fused, m._cnf_eval_value = TB._eval_f64, TS._eval_f64
    gen = torch.Generator().manual_seed(29)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=gen, dtype=torch.float64) * scale).requires_grad_(True)
    over_frames = lambda v: torch.cat([c.unsqueeze(0).expand(BT, -1).reshape(-1) for c in v.split(list(widths))]).detach().requires_grad_(True)
    tot = BT * sum(widths)
    L = {"y": r(BT, n, 3), "logpx": r(BT, n, 1), "e": r(BT, n, 3).detach(), "G_lm": r(tot), "Bb_lm": r(tot, scale=0.5), "tg_lm": over_frames(r(sum(widths))),
         "tb_lm": over_frames(r(sum(widths))), "t_end": (r(()).abs() + 0.7).detach().requires_grad_(True), "widths": widths,
         "wb": [t_ for l in range(4) for t_ in (r(widths[l], cin[l], scale=0.7), r(widths[l], scale=0.3))], "wy": r(BT, n, 3).detach(), "wl": r(BT, n, 1).detach()}
    L["w1x"], L["w2x"] = L["wb"][2], L["wb"][4]
    table = torch.tensor([3, 1, 2, 3], dtype=torch.int32)
    return [("CnfBlockSolve", L, 3), ("CnfSampleSolve", L, 3), ("CnfSampleSolveFrames", L, table)]


def gpu_cases():
    from caspr_amd.models import CaSPR
    from caspr_amd.models.cnf import CNF
    from caspr_amd.utils.synthetic import stress_state_dict
    from test_cnf_sample_grad import GRAD_CASES as UNIFORM
    from test_cnf_sample_grad_frames import GRAD_CASES as FRAMES
    dev = torch.device("cuda:0")
    model = CaSPR(check_tol=None)
    model.load_state_dict(stress_state_dict(CaSPR().state_dict(), 0))
    block = next(b for b in model.to(dev).eval().point_cnf.chain if isinstance(b, CNF))
    layers = block.odefunc.diffeq.layers
    assert all(FG._fused_layer_ok(l, 64) for l in layers[1:3]) and ops.CNF_BF16X6, "the block node's kernels are switched off"
    gen = torch.Generator(device=dev).manual_seed(97)
    r = lambda *s: torch.randn(*s, device=dev, generator=gen)

    def leaves(BT, n):
        with torch.no_grad():
            hyper = FG._hyper_layer_major(block, r(BT, layers[0]._hyper_gate.weight.shape[1] - 1))
            t_end = block.sqrt_end_time * block.sqrt_end_time
        L = {k: v.detach().requires_grad_(True) for k, v in zip(HYPER + ("t_end", "y", "logpx"), hyper[:4] + (t_end, r(BT, n, 3), r(BT, n, 1)))}
        L.update(widths=hyper[4], e=r(BT, n, 3), wy=r(BT, n, 3), wl=r(BT, n, 1), wb=[p_ for l in layers for p_ in (l._layer.weight, l._layer.bias)])
        L["w1x"], L["w2x"] = block._weights_x6()
        return L
    cases = [("CnfBlockSolve", leaves(1, 64), S) for S in (2, 3)]
    cases += [("CnfSampleSolve", leaves(c[0], c[1]), c[2]) for c in UNIFORM]
    cases += [("CnfSampleSolveFrames", leaves(c[1], c[2]), torch.tensor(c[3], dtype=torch.int32, device=dev)) for c in FRAMES]
    return cases, [cases[1], cases[3], cases[-2]], [w for i, w in enumerate(cases[0][1]["wb"]) if i % 2]


def main(argv):
    paths = [a for a in argv if not a.startswith("--")]
    if len(paths) != 1:
        sys.exit(__doc__)
    other = load_other(paths[0])
    if "--cpu" in argv:
        cases = partial = cpu_cases(other)
        biases = [w for i, w in enumerate(cases[0][1]["wb"]) if i % 2]
    else:
        cases, partial, biases = gpu_cases()
    worst, count = {}, dict.fromkeys(NODES, 0)            # (node, tensor) -> [differing elements, largest difference]

    def compare(node, L, steps):
        mine, theirs = run(FG, node, L, steps), run(other, node, L, steps)
        assert list(mine) == list(theirs), (list(mine), list(theirs))
        count[node] += 1
        for k in mine:
            w = worst.setdefault((node, k), [0, 0.0])
            if not torch.equal(mine[k], theirs[k]):
                ne = mine[k] != theirs[k]                  # (NaN differs from NaN here: a NaN is a difference)
                w[0] += int(ne.sum())
                w[1] = max(w[1], float((mine[k].double() - theirs[k].double()).abs()[ne].nan_to_num(nan=float("inf")).max()))
    for case in cases:
        compare(*case)
    for w in biases:                                       # only the weight matrices take a gradient: the sweep's `wsel`
        w.requires_grad_(False)
    for case in partial:
        compare(*case)
    rows = list(dict.fromkeys(k for _, k in worst))
    print(("%-9s" % "tensor" + "".join("  %-24s" % ("%s (%d runs)" % (nd, count[nd])) for nd in NODES)).rstrip())
    for k in rows:
        cell = lambda w: "-" if w is None else "identical" if w[0] == 0 else "%d differ, max %.3e" % tuple(w)
        print(("%-9s" % k + "".join("  %-24s" % cell(worst.get((nd, k))) for nd in NODES)).rstrip())
    bad = sum(1 for w in worst.values() if w[0])
    print("%d tensor(s) differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
