"""Auto-decoding: fit latent codes to observed point clouds through the differentiable decode (models/caspr.py: decode(differentiable=True))
and the Chamfer loss (losses.py).  The reference has no such routine; its decode is differentiable (caspr.py:204-267 through torchdiffeq)
and its metric is the Chamfer term of evaluations.py:36-44 -- this is the loop a user would write from the two."""
import torch

from ..losses import chamfer_loss


def fit_latent(model, target, z_init, num_points, steps=100, lr=1e-3, y=None, constant_in_time=False):
    """Adam on a copy of z_init (B,T,H) with the model's parameters frozen, minimising
    chamfer_loss(model.decode(z, y=y, differentiable=True)[2], target), target (B,T,M,3) float32 on the GPU.
    The base samples are drawn ONCE -- decode's own draw for (num_points, constant_in_time), or the given y (B,T,num_points,3) -- and
    reused at every step, so the loss is a deterministic function of z.  Only dL/dz is asked of autograd: no parameter's .grad or
    requires_grad is touched, and the module's state changes only as decode() itself changes it (the device sampler's draw counter, the
    evaluation counters).  -> (z (B,T,H) detached, [loss of every step, before that step's update])."""
    if z_init.dim() != 3:
        raise ValueError("fit_latent: z_init must be (B,T,H), got %s" % (tuple(z_init.shape),))
    B, T, _ = z_init.shape
    z = z_init.detach().clone().requires_grad_(True)
    with torch.no_grad():
        if y is None:
            y = model._base_samples(B, T, num_points, constant_in_time, None, None, None, z)[0]
        y = y.detach().to(z).reshape(B, T, num_points, -1).contiguous()
    opt = torch.optim.Adam([z], lr=lr)
    losses = []
    with torch.enable_grad():
        for _ in range(int(steps)):
            x = model.decode(z, num_points, y=y, differentiable=True)[2]
            loss = chamfer_loss(x, target)
            z.grad, = torch.autograd.grad(loss, [z])
            opt.step()
            losses.append(loss.detach())
    return z.detach(), (torch.stack(losses).cpu().tolist() if losses else [])     # one copy at the end, no sync per step
