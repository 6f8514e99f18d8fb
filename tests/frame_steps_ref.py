"""Restatement of the per-frame step controller (include/caspr_hip.h: caspr_cnf_steps_update_f32 / caspr_cnf_steps_order;
csrc/cnf_frame_steps.hip) in torch, sharing no code with the kernels or with caspr_amd.ops.

The maxima are taken in the dtype of the solutions (f32 for kernel outputs: what the kernel does; f64 for the CPU solve); everything
after them is IEEE f64 with two correctly rounded square roots, operation by operation as the header states it, so on the same f32
tensors every decision and every statistic equals the kernel's bit for bit."""
import math

import torch

NAN = float("nan")


def update(x_prev, x_cur, P, tol, safety, S_max, steps, capped=None, stats=None):
    """One update after rung P >= 2.  x_prev / x_cur (BT,g,3): the pilot solutions at P/2 and P steps.  steps (BT,) int32 (0 =
    undecided), capped (BT,) int32, stats (BT,4) f64 are NOT modified: -> (steps, next_tab, capped, stats) after the update."""
    BT = x_prev.shape[0]
    steps = steps.clone().cpu()
    capped = torch.zeros(BT, dtype=torch.int32) if capped is None else capped.clone().cpu()
    stats = torch.zeros(BT, 4, dtype=torch.float64) if stats is None else stats.clone().cpu()
    next_tab = torch.zeros(BT, dtype=torch.int32)
    x_prev, x_cur = x_prev.detach().cpu(), x_cur.detach().cpu()
    for f in range(BT):
        if int(steps[f]) != 0:
            continue                              # decided earlier: table entry 0, statistics kept
        diff = x_cur[f] - x_prev[f]               # in the solutions' dtype
        bad = not (bool(torch.isfinite(diff).all()) and bool(torch.isfinite(x_cur[f]).all()))
        d = bound = pred = NAN
        ok = False
        if not bad:
            d = float(diff.abs().max())
            bound = float(tol) * (1.0 + float(x_cur[f].abs().max()))
            e = d / 15.0
            q = (e / bound) if bound != 0.0 else (NAN if e == 0.0 else math.inf)
            pred = (float(P) * math.sqrt(math.sqrt(q))) * float(safety)
            ok = e <= bound
        S, cap = 0, 0
        if ok:
            if P == 2:
                S = 2
            elif pred != pred or pred >= P:
                S = P
            else:
                S = max(int(math.ceil(pred)), P // 2 + 1)
        elif P >= S_max:
            S, cap = S_max, 1
        steps[f], next_tab[f], capped[f] = S, (0 if S else 2 * P), cap
        stats[f] = torch.tensor([d, bound, pred, float(P) if S else 0.0], dtype=torch.float64)
    return steps, next_tab, capped, stats


def ladder(solve, BT, tol, safety, S_max):
    """The whole controller on a solver `solve(S) -> (BT,g,3)` that runs every frame at S steps (the restatement has no need to skip
    decided frames: they are ignored; once every frame is decided the remaining rungs change nothing and are not solved).
    -> (steps, capped, stats, pilot_steps)."""
    steps = torch.zeros(BT, dtype=torch.int32)
    capped, stats = torch.zeros(BT, dtype=torch.int32), torch.zeros(BT, 4, dtype=torch.float64)
    x_prev, P = solve(1), 2
    while P <= S_max and int((steps == 0).sum()):
        x_cur = solve(P)
        steps, _, capped, stats = update(x_prev, x_cur, P, tol, safety, S_max, steps, capped, stats)
        x_prev, P = x_cur, 2 * P
    return steps, capped, stats, (2 * stats[:, 3] - 1).to(torch.int32)


def order(steps):
    """The stable permutation that sorts frames by descending count, ties by ascending frame, by explicit ranking."""
    s = [int(v) for v in steps.cpu()]
    return torch.tensor(sorted(range(len(s)), key=lambda f: (-s[f], f)), dtype=torch.int32)


def guard_ratio(x_S, x_half, S, S_half, tol):
    """The accuracy guard's criterion for one frame: Richardson estimate of the S-step error from the S_half-step solution, over
    tol (1 + max |x_S|).  <= 1 passes."""
    est = float((x_S - x_half).abs().max()) / ((float(S) / float(S_half)) ** 4 - 1.0)
    return est / (float(tol) * (1.0 + float(x_S.abs().max())))
