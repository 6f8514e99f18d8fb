"""Losses on sampled point clouds with hand-written gradients (include/caspr_hip.h: caspr_chamfer_idx_f32, caspr_emd_tape_f32;
include/caspr_hip_train.h: caspr_chamfer_bwd_f32, caspr_emd_bwd_f32).

The reference evaluates reconstructions with the Chamfer term of utils/evaluations.py:36-44 (tk3dv ChamferDistance, which carries its
own CUDA backward).  Here the same term is a differentiable loss on the samples of decode(differentiable=True) /
reconstruct(differentiable=True): auto-decoding (utils/fit.py), fine-tuning the flow on its samples.  The forward keeps the two
nearest-neighbour index vectors (4 bytes per point), never an (n, m) matrix; the backward gathers in a fixed order without float
atomics, so gradients are bit-reproducible.

The approximate EMD of evaluations.py:45-46 (utils/emd.py: an autograd function that saves the (n, m) match matrix) is differentiable the
same way: its forward keeps the ten levels' ratio vectors (40 (n + m) bytes per frame), from which the backward rebuilds every entry of the
match matrix on the fly -- the published matchcost gradient with the match held fixed, nothing through approxmatch -- again without float
atomics.  Same rules as ops.py: float32 contiguous GPU tensors, no CPU fallback.

The EXACT EMD -- the cost of the optimal one-to-one assignment, which the reference does not have and its approximation stands for -- is
exact_earth_mover_distance / emd_exact_loss (caspr_emd_exact_f32: an auction in f64, within n * eps of the optimum with a dual certificate;
caspr_emd_exact_bwd_f32: the gradient with the matching held fixed, which is the true gradient wherever the optimum is unique).  Equal
point counts, n <= 2048; the forward keeps the assignment, 4 n bytes per frame.
"""
import torch
from torch.autograd.function import once_differentiable

from . import ops
from . import train_ops


def _chk_cloud(fn, name, t, channels_first=False):
    """`name` = the argument as the caller wrote it: every refusal says which tensor it is about.  Shape, type and layout first, the
    device last (_chk_gpu), so that what is wrong with a tensor is reported wherever it lives.  channels_first: (F,3,N), the layout
    utils/emd.py takes with transpose=True."""
    if not torch.is_tensor(t) or t.dim() != 3 or t.shape[1 if channels_first else 2] != 3:
        raise ValueError("%s: %s must be a %s tensor, got %s" % (fn, name, "(F,3,N)" if channels_first else "(F,N,3)",
                                                                 tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    if t.dtype != torch.float32:
        raise ValueError("%s: %s must be float32, got %s" % (fn, name, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous (call .contiguous())" % (fn, name))


def _chk_gpu(fn, name, t):
    if not t.is_cuda:
        raise ValueError("%s: %s is on %s: caspr_amd kernels need tensors on the GPU, there is no CPU fallback" % (fn, name, t.device))


class _Chamfer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, q):
        d1, d2, i1, i2 = ops.chamfer_distance(p, q, return_indices=True)
        ctx.save_for_backward(p, q, i1, i2)
        ctx.set_materialize_grads(False)        # an unused distance vector arrives as None -> a NULL pointer, not a tensor of zeros
        return d1, d2

    @staticmethod
    @once_differentiable
    def backward(ctx, g1, g2):
        p, q, i1, i2 = ctx.saved_tensors
        want_p, want_q = ctx.needs_input_grad
        if g1 is None and g2 is None:
            return None, None
        g1 = None if g1 is None else g1.contiguous()
        g2 = None if g2 is None else g2.contiguous()
        return train_ops.chamfer_bwd(p, q, i1, i2, g1, g2, want_p=want_p, want_q=want_q)


def chamfer_distance(p, q):
    """p (F,n,3), q (F,m,3) float32 contiguous GPU tensors -> dist1 (F,n) = min_j |p_i - q_j|^2, dist2 (F,m) = min_i |p_i - q_j|^2: the bits of
    ops.chamfer_distance, differentiable in whichever of p and q requires grad (the other's gradient is not computed).  The gradient
    flows through the nearest neighbour only, the smallest index on ties; a point without a finite candidate has dist = +inf and
    no gradient.  First order only: the backward is once_differentiable, a double backward raises.  The indices themselves:
    ops.chamfer_distance(p, q, return_indices=True)."""
    _chk_cloud("chamfer_distance", "p", p)
    _chk_cloud("chamfer_distance", "q", q)
    if p.shape[0] != q.shape[0]:
        raise ValueError("chamfer_distance: p and q disagree on F: p is %s, q is %s" % (tuple(p.shape), tuple(q.shape)))
    _chk_gpu("chamfer_distance", "p", p)
    _chk_gpu("chamfer_distance", "q", q)
    return _Chamfer.apply(p, q)


def chamfer_loss(pred, gt, reduction="mean"):
    """The Chamfer-L2 of utils.evaluations.eval_reconstr_frames (evaluations.py:36-44) as a loss: per frame
    mean_i dist1 + mean_j dist2.  pred (F,N,3) or (B,T,N,3), gt the same with its own point count.
    reduction: "mean" over the frames (a scalar), "sum", or "none" (the per-frame values, (F,) or (B,T))."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError("chamfer_loss: reduction must be 'mean', 'sum' or 'none', got %r" % (reduction,))
    if not (torch.is_tensor(pred) and torch.is_tensor(gt)) or pred.dim() not in (3, 4) or gt.dim() != pred.dim() or pred.shape[:-2] != gt.shape[:-2]:
        raise ValueError("chamfer_loss: pred and gt must both be (F,N,3) or (B,T,N,3) with the same leading sizes, got pred %s, gt %s"
                         % (tuple(pred.shape) if torch.is_tensor(pred) else type(pred).__name__, tuple(gt.shape) if torch.is_tensor(gt) else type(gt).__name__))
    lead = pred.shape[:-2]
    for name, t in (("pred", pred), ("gt", gt)):            # before the reshape, which would silently copy a strided tensor
        if not t.is_contiguous():
            raise ValueError("chamfer_loss: %s must be contiguous (call .contiguous())" % name)
    p3, g3 = pred.reshape(-1, pred.shape[-2], pred.shape[-1]), gt.reshape(-1, gt.shape[-2], gt.shape[-1])
    _chk_cloud("chamfer_loss", "pred", p3)
    _chk_cloud("chamfer_loss", "gt", g3)
    _chk_gpu("chamfer_loss", "pred", p3)
    _chk_gpu("chamfer_loss", "gt", g3)
    d1, d2 = _Chamfer.apply(p3, g3)
    per_frame = d1.mean(dim=1) + d2.mean(dim=1)
    if reduction == "mean":
        return per_frame.mean()
    if reduction == "sum":
        return per_frame.sum()
    return per_frame.reshape(lead)


class _EMD(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, q):
        p, q = p.contiguous(), q.contiguous()   # emd.py:8-9: the (F,N,3) view of a (F,3,N) input is copied here, as the reference does
        cost, tape = ops.earth_mover_distance(p, q, transpose=False, return_tape=True)
        ctx.save_for_backward(p, q, tape)
        ctx.set_materialize_grads(False)        # an unused cost arrives as None: nothing is launched for it
        return cost

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        p, q, tape = ctx.saved_tensors
        want_p, want_q = ctx.needs_input_grad
        if g is None:
            return None, None
        return train_ops.emd_bwd(p, q, tape, g.contiguous(), want_p=want_p, want_q=want_q)


def earth_mover_distance(xyz1, xyz2, transpose=True):
    """utils.emd.earth_mover_distance (emd.py:24-45) with its signature and layouts: xyz1 (F,3,n), xyz2 (F,3,m) when `transpose` (as the
    reference calls it), else (F,n,3), (F,m,3); a 2-D cloud is one frame.  float32 contiguous GPU tensors -> cost (F,), the bits of
    ops.earth_mover_distance, differentiable in whichever input requires grad (the other's gradient is not computed).  The gradient is
    emd_cuda's matchcost_backward (emd.py:17-21): d cost / d xyz with the match matrix held fixed, nothing through approxmatch; a
    coincident pair contributes zero.  First order only: the backward is once_differentiable, a double backward raises.  The forward
    keeps 40 (n + m) bytes per frame, never the (n, m) match matrix."""
    if torch.is_tensor(xyz1) and xyz1.dim() == 2:
        xyz1 = xyz1.unsqueeze(0)
    if torch.is_tensor(xyz2) and xyz2.dim() == 2:
        xyz2 = xyz2.unsqueeze(0)
    _chk_cloud("earth_mover_distance", "xyz1", xyz1, channels_first=transpose)
    _chk_cloud("earth_mover_distance", "xyz2", xyz2, channels_first=transpose)
    if xyz1.shape[0] != xyz2.shape[0]:
        raise ValueError("earth_mover_distance: xyz1 and xyz2 disagree on F: xyz1 is %s, xyz2 is %s" % (tuple(xyz1.shape), tuple(xyz2.shape)))
    _chk_gpu("earth_mover_distance", "xyz1", xyz1)
    _chk_gpu("earth_mover_distance", "xyz2", xyz2)
    if transpose:
        xyz1, xyz2 = xyz1.transpose(1, 2), xyz2.transpose(1, 2)
    return _EMD.apply(xyz1, xyz2)


def emd_loss(pred, gt, reduction="mean"):
    """The approximate EMD of utils.evaluations.eval_reconstr_frames (evaluations.py:45-46) as a loss: per frame cost / pred.size(-2).
    pred (F,N,3) or (B,T,N,3), gt the same with its own point count.
    reduction: "mean" over the frames (a scalar), "sum", or "none" (the per-frame values, (F,) or (B,T))."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError("emd_loss: reduction must be 'mean', 'sum' or 'none', got %r" % (reduction,))
    if not (torch.is_tensor(pred) and torch.is_tensor(gt)) or pred.dim() not in (3, 4) or gt.dim() != pred.dim() or pred.shape[:-2] != gt.shape[:-2]:
        raise ValueError("emd_loss: pred and gt must both be (F,N,3) or (B,T,N,3) with the same leading sizes, got pred %s, gt %s"
                         % (tuple(pred.shape) if torch.is_tensor(pred) else type(pred).__name__, tuple(gt.shape) if torch.is_tensor(gt) else type(gt).__name__))
    lead = pred.shape[:-2]
    for name, t in (("pred", pred), ("gt", gt)):            # before the reshape, which would silently copy a strided tensor
        if not t.is_contiguous():
            raise ValueError("emd_loss: %s must be contiguous (call .contiguous())" % name)
    p3, g3 = pred.reshape(-1, pred.shape[-2], pred.shape[-1]), gt.reshape(-1, gt.shape[-2], gt.shape[-1])
    _chk_cloud("emd_loss", "pred", p3)
    _chk_cloud("emd_loss", "gt", g3)
    _chk_gpu("emd_loss", "pred", p3)
    _chk_gpu("emd_loss", "gt", g3)
    per_frame = _EMD.apply(p3, g3) / p3.shape[1]
    if reduction == "mean":
        return per_frame.mean()
    if reduction == "sum":
        return per_frame.sum()
    return per_frame.reshape(lead)


def _chk_eps(fn, eps):
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (0.0 < float(eps) < float("inf")):
        raise ValueError("%s: eps must be positive and finite, got %r" % (fn, eps))


class _EMDExact(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, q, eps):
        p, q = p.contiguous(), q.contiguous()   # the (F,N,3) view of a (F,3,N) input is copied here, as _EMD does
        cost, assign, _, _ = ops.earth_mover_distance_exact(p, q, transpose=False, eps=eps, return_match=True)
        ctx.save_for_backward(p, q, assign)
        ctx.set_materialize_grads(False)        # an unused cost arrives as None: nothing is launched for it
        return cost

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        p, q, assign = ctx.saved_tensors
        want_p, want_q = ctx.needs_input_grad[:2]
        if g is None:
            return None, None, None
        return train_ops.emd_exact_bwd(p, q, assign, g.contiguous(), want_p=want_p, want_q=want_q) + (None,)


def exact_earth_mover_distance(xyz1, xyz2, transpose=True, eps=1e-6):
    """The exact EMD of ops.earth_mover_distance_exact with earth_mover_distance's signature and layouts: xyz1, xyz2 (F,3,n) when
    `transpose`, else (F,n,3), the SAME point count n <= 2048 on both sides; a 2-D cloud is one frame.  float32 contiguous GPU tensors ->
    cost (F,), the bits of ops.earth_mover_distance_exact (within n * eps of the optimal one-to-one assignment cost), differentiable in
    whichever input requires grad (the other's gradient is not computed).  The gradient holds the matching fixed -- the true gradient
    wherever the optimum is unique: d cost / d x_i = (x_i - y_assign[i]) / |x_i - y_assign[i]|, the negative of it on the matched point;
    a coincident pair contributes zero.  A frame that exhausts the default bid budget (ops.earth_mover_distance_exact: a target of
    nearly identical points at n >= 1024) has cost NaN and NaN gradients.  First order only: the backward is once_differentiable, a
    double backward raises.  The forward keeps 4 n bytes per frame (the assignment)."""
    if torch.is_tensor(xyz1) and xyz1.dim() == 2:
        xyz1 = xyz1.unsqueeze(0)
    if torch.is_tensor(xyz2) and xyz2.dim() == 2:
        xyz2 = xyz2.unsqueeze(0)
    _chk_cloud("exact_earth_mover_distance", "xyz1", xyz1, channels_first=transpose)
    _chk_cloud("exact_earth_mover_distance", "xyz2", xyz2, channels_first=transpose)
    if xyz1.shape[0] != xyz2.shape[0]:
        raise ValueError("exact_earth_mover_distance: xyz1 and xyz2 disagree on F: xyz1 is %s, xyz2 is %s" % (tuple(xyz1.shape), tuple(xyz2.shape)))
    _chk_counts("exact_earth_mover_distance", "xyz1", "xyz2", xyz1.shape[2 if transpose else 1], xyz2.shape[2 if transpose else 1])
    _chk_eps("exact_earth_mover_distance", eps)
    _chk_gpu("exact_earth_mover_distance", "xyz1", xyz1)
    _chk_gpu("exact_earth_mover_distance", "xyz2", xyz2)
    if transpose:
        xyz1, xyz2 = xyz1.transpose(1, 2), xyz2.transpose(1, 2)
    return _EMDExact.apply(xyz1, xyz2, eps)


def _chk_counts(fn, name1, name2, n, m):
    if n != m:
        raise ValueError("%s: a one-to-one assignment needs equal point counts, %s has %d points and %s has %d: use the approximate EMD "
                         "(earth_mover_distance / emd_loss) for clouds of different sizes" % (fn, name1, n, name2, m))
    if not 1 <= n <= ops.EMD_EXACT_MAX_POINTS:
        raise ValueError("%s: %s and %s have %d points: the exact EMD takes 1 .. %d" % (fn, name1, name2, n, ops.EMD_EXACT_MAX_POINTS))


def emd_exact_loss(pred, gt, reduction="mean", eps=1e-6):
    """The exact EMD as a loss: per frame (optimal one-to-one assignment cost) / N, the scale of evaluations.py:46.
    pred (F,N,3) or (B,T,N,3), gt the same with the SAME point count N <= 2048.
    reduction: "mean" over the frames (a scalar), "sum", or "none" (the per-frame values, (F,) or (B,T)).
    eps: the auction's final increment; a frame's cost is within N * eps of the optimum (losses.exact_earth_mover_distance)."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError("emd_exact_loss: reduction must be 'mean', 'sum' or 'none', got %r" % (reduction,))
    _chk_eps("emd_exact_loss", eps)
    if not (torch.is_tensor(pred) and torch.is_tensor(gt)) or pred.dim() not in (3, 4) or gt.dim() != pred.dim() or pred.shape[:-2] != gt.shape[:-2]:
        raise ValueError("emd_exact_loss: pred and gt must both be (F,N,3) or (B,T,N,3) with the same leading sizes, got pred %s, gt %s"
                         % (tuple(pred.shape) if torch.is_tensor(pred) else type(pred).__name__, tuple(gt.shape) if torch.is_tensor(gt) else type(gt).__name__))
    lead = pred.shape[:-2]
    for name, t in (("pred", pred), ("gt", gt)):            # before the reshape, which would silently copy a strided tensor
        if not t.is_contiguous():
            raise ValueError("emd_exact_loss: %s must be contiguous (call .contiguous())" % name)
    p3, g3 = pred.reshape(-1, pred.shape[-2], pred.shape[-1]), gt.reshape(-1, gt.shape[-2], gt.shape[-1])
    _chk_cloud("emd_exact_loss", "pred", p3)
    _chk_cloud("emd_exact_loss", "gt", g3)
    _chk_counts("emd_exact_loss", "pred", "gt", p3.shape[1], g3.shape[1])
    _chk_gpu("emd_exact_loss", "pred", p3)
    _chk_gpu("emd_exact_loss", "gt", g3)
    per_frame = _EMDExact.apply(p3, g3, eps) / p3.shape[1]
    if reduction == "mean":
        return per_frame.mean()
    if reduction == "sum":
        return per_frame.sum()
    return per_frame.reshape(lead)
