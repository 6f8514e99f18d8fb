"""The f64 reference of the gradient through the adaptive latent solve (train/flow_grad.py: LatentSolveDopri5): torch autograd through
test_latent_dopri5.replay at GIVEN dt's and decisions.  replay converts only ratios and norms to Python floats, so autograd sees exactly
the frozen-step map -- accepted steps, their interpolants, z0 at the stamps equal to times[0] -- and nothing of the controller.

grads(): dL/dz0 and the eight parameter gradients of L = sum(out * wgt), one sequence at a time, summed over the sequences.
bound(): the tolerance of a float32 implementation against it, per tensor.
frozen(): the same map restated from the accepted steps alone, with one deliberate defect on request (k7 detached inside the interpolant):
what the comparison is shown to catch (tests/test_latent_dopri5_grad.py).
"""
import torch

from oracle import model as O
from test_latent_dopri5 import PRE, dyn_sd, replay

LAYERS = (0, 2, 4, 6)
NAMES = ["dz0"] + ["d%s%d" % (k, i) for i in range(4) for k in ("w", "b")]           # the order grads() returns
FLOOR = 3e-5        # what the suite holds the RK4 node to against f64 (test_hip_train.py: latent_node_vs_f64_*, the same measure)


def params(sd, dtype):
    """The eight dynamics tensors of a state dict as leaves, keyed as oracle.model.dynamics reads them."""
    return {k: v.clone().requires_grad_(True) for k, v in dyn_sd(sd, dtype).items()}


def _ordered(w):
    return [w["%s.%d.%s" % (PRE, l, k)] for l in LAYERS for k in ("weight", "bias")]


def grads(sd, z0, rel, rtol, atol, dts, decisions, wgt, dtype=torch.float64, solve=None):
    """sd: state dict holding the dynamics net; z0 (B,D); rel: the solver's times (test_latent_dopri5.rel_of); dts[b], decisions[b]:
    sequence b's attempts; wgt (B,Tu,D).  -> [dL/dz0 (B,D), dW0, db0, .., dW3, db3] in `dtype`, L = sum(out * wgt).
    solve: what maps (f, z0 row, b) to the (Tu,D) outputs (default: replay at the given attempts)."""
    w = params(sd, dtype)
    f = lambda z: O.dynamics(w, z)
    gz = []
    for b in range(z0.shape[0]):
        z = z0[b].detach().cpu().reshape(1, -1).to(dtype).requires_grad_(True)
        if solve is None:
            out = torch.cat(replay(f, z, rel, rtol, atol, dts=dts[b], decisions=decisions[b])["out"], 0)
        else:
            out = solve(f, z, b)
        (out * wgt[b].detach().cpu().to(dtype)).sum().backward()        # parameter gradients accumulate over the sequences
        gz.append(z.grad.reshape(-1))
    return [torch.stack(gz)] + [p.grad if p.grad is not None else torch.zeros_like(p) for p in _ordered(w)]


def err(got, want):
    """max |got - want| / |want|max: the measure of test_hip_train.rel."""
    ref = float(want.abs().max()) or 1.0
    return float((got.double() - want.double()).abs().max()) / ref


def bound(g32, g64):
    """max(3e-5, 4 x the distance of this reference in f32 from itself in f64) for one tensor: the floor is the RK4 node's bound against
    f64, the factor 4 the margin measure_delta gives f32-against-f64 arithmetic in this test family."""
    return max(FLOOR, 4.0 * err(g32, g64))


def frozen(f, z0, rel, dts, accepted, detach_k7=False):
    """The frozen-step map from the ACCEPTED steps alone, in the dtype of z0 -> (Tu,D).  detach_k7: the defect -- f(z_{n+1}) enters the
    interpolant as a constant."""
    steps = [d for d, a in zip(dts, accepted) if a]
    z, t, f0, out, k = z0, rel[0], f(z0), [z0], 0
    t0s = t1s = t
    interp = None
    for tn in rel[1:]:
        while tn > t1s:
            dt = float(steps[k])
            k += 1
            ks = [f0]
            for brow in O._DP_BETA:
                ks.append(f(z + dt * sum(b * kk for b, kk in zip(brow, ks) if b != 0)))
            znew = z + dt * sum(c * kk for c, kk in zip(O._DP_CSOL, ks) if c != 0)
            zmid = z + dt * sum(c * kk for c, kk in zip(O._DP_CMID, ks) if c != 0)
            fa, fb = f0, (ks[-1].detach() if detach_k7 else ks[-1])
            interp = (2 * dt * (fb - fa) - 8 * (znew + z) + 16 * zmid, dt * (5 * fa - 3 * fb) + 18 * z + 14 * znew - 32 * zmid,
                      dt * (fb - 4 * fa) - 11 * z - 5 * znew + 16 * zmid, dt * fa, z)
            t0s, t1s = t, t + dt
            t, z, f0 = t + dt, znew, ks[-1]
        if interp is None or tn == t1s:
            out.append(z)
        else:
            x = (tn - t0s) / (t1s - t0s)
            A, B, C, D, E = interp
            out.append((((A * x + B) * x + C) * x + D) * x + E)
    return torch.cat(out, 0)
