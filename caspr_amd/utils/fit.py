"""Auto-decoding: fit latent codes to observed point clouds through the differentiable decode (models/caspr.py: decode(differentiable=True))
and the Chamfer loss or the approximate EMD (losses.py).  The reference has no such routine; its decode is differentiable
(caspr.py:204-267 through torchdiffeq) and its metrics are the Chamfer term of evaluations.py:36-44 and the EMD of evaluations.py:45-46,
both differentiable there -- this is the loop a user would write from them."""
import torch

from ..losses import chamfer_loss, emd_loss

LOSSES = {"chamfer": chamfer_loss, "emd": emd_loss}


def fit_latent(model, target, z_init, num_points, steps=100, lr=1e-3, y=None, constant_in_time=False, loss="chamfer", frame_steps=None,
               pilot_every=1):
    """Adam on a copy of z_init (B,T,H) with the model's parameters frozen, minimising
    loss(model.decode(z, y=y, differentiable=True)[2], target), target (B,T,M,3) float32 on the GPU.
    loss: "chamfer" (losses.chamfer_loss, the default), "emd" (losses.emd_loss: a one-to-one transport cost, which does not let the
    samples gather on the target's dense regions as a nearest-neighbour loss does), or a callable (x (B,T,num_points,3), target) -> scalar.
    The EXACT one-to-one transport cost goes in as a callable: fit_latent(..., loss=losses.emd_exact_loss) descends the gradient of the
    optimal assignment itself (emd_loss's goes through a match matrix that meets its marginals only approximately); it needs
    num_points == M <= 2048.
    The base samples are drawn ONCE -- decode's own draw for (num_points, constant_in_time), or the given y (B,T,num_points,3) -- and
    reused at every step, so the loss is a deterministic function of z.  Only dL/dz is asked of autograd: no parameter's .grad or
    requires_grad is touched, and the module's state changes only as decode() itself changes it (the device sampler's draw counter, the
    evaluation counters).
    frame_steps: decode()'s keyword.  None (default): the model's cnf_rk4_steps for every frame, the loop as it always was.  A (B*T,)
    int32 tensor: that table of RK4 step counts at every iteration.  "pilot": the counts are chosen by decode's pilot at iterations 0,
    k, 2k, ... with k = pilot_every, and the last table is reused in between (the latent moves little per Adam step, and a pilot costs
    a ladder of solves); within the iterations that share a table the loss is one differentiable function of z.
    -> (z (B,T,H) detached, [loss of every step, before that step's update])."""
    if z_init.dim() != 3:
        raise ValueError("fit_latent: z_init must be (B,T,H), got %s" % (tuple(z_init.shape),))
    if not callable(loss) and loss not in LOSSES:
        raise ValueError("fit_latent: loss must be one of %s or a callable (x, target) -> scalar, got %r" % (sorted(LOSSES), loss))
    loss_fn = loss if callable(loss) else LOSSES[loss]
    if int(pilot_every) < 1:
        raise ValueError("fit_latent: pilot_every must be a positive number of iterations, got %r" % (pilot_every,))
    B, T, _ = z_init.shape
    z = z_init.detach().clone().requires_grad_(True)
    with torch.no_grad():
        if y is None:
            y = model._base_samples(B, T, num_points, constant_in_time, None, None, None, z)[0]
        y = y.detach().to(z).reshape(B, T, num_points, -1).contiguous()
    opt = torch.optim.Adam([z], lr=lr)
    losses = []
    with torch.enable_grad():
        table = frame_steps
        for it in range(int(steps)):
            if frame_steps is None:
                x = model.decode(z, num_points, y=y, differentiable=True)[2]
            else:
                pilot = isinstance(frame_steps, str) and it % int(pilot_every) == 0
                x = model.decode(z, num_points, y=y, frame_steps=frame_steps if pilot else table, differentiable=True)[2]
                if pilot:
                    table = model.last_frame_steps[0]
            value = loss_fn(x, target)
            z.grad, = torch.autograd.grad(value, [z])
            opt.step()
            losses.append(value.detach())
    return z.detach(), (torch.stack(losses).cpu().tolist() if losses else [])     # one copy at the end, no sync per step
