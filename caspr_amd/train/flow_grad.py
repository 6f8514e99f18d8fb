"""Training path of the latent ODE and the point CNF.

The reference back-propagates through torchdiffeq's adjoint (cnf.py:102-110, latent_ode_model.py:98).  This build
integrates with fixed-step RK4, so the training path differentiates the discrete RK4 map itself
(discretise-then-optimise): the gradient is exact for the map the forward pass computes, including d/d(sqrt_end_time)
through the step size and the stage times.

Status (round 1): every matrix product of the path -- the 512x512 layers of the ODE function on value AND tangent
columns (the Hutchinson divergence e^T (df/dy) e is carried as a forward-mode tangent, odefunc.py:13-31), the hyper
networks, the latent dynamics -- runs on the HIP kernels through `LinearRows` (forward: caspr_conv1x1_f32, data
gradient: the same kernel with the transposed packed weight, weight/bias gradient: caspr_conv1x1_wgrad_f32).  The
gated softplus layers (value and tangent rows, forward and backward with the per-frame gate / bias reductions) are the
fused kernels caspr_cnf_act_f32 / caspr_cnf_act_bwd_f32 (`CnfAct`).  torch.autograd records only the small tensors
around them: the (frames, C) gates, the (BT,n,3) RK4 combinations and the 3-channel output layer.  Fusing the
activation into the GEMM epilogue and recomputing instead of storing the layer products is the next step
(DESIGN.md section 7).  No CPU path: everything below requires GPU tensors.

The SAMPLING direction of the point CNF (decode(differentiable=True); cnf.py:70-128 with reverse = True, caspr.py:262) is at the end of the
file: CnfSampleSolve / point_cnf_sample_train, one node per block on value rows only; CnfSampleSolveFrames is the same node with an RK4
step count per frame (decode(differentiable=True, frame_steps=...)).

The three block nodes -- CnfBlockSolve (forward direction, value + divergence), CnfSampleSolve, CnfSampleSolveFrames -- each launch one
taping solve kernel forward and share ONE hand-written reverse sweep, _rk4_reverse_sweep, whose docstring states the RK4 algebra; a
node's backward only describes its variant (outputs, time axis, scalar or per frame) and forms dL/dt_end from what the sweep returns.
CnfBlockSolveReg is CnfBlockSolve with the kinetic / Jacobian regularisers as a third, summed output (config.train_cnf_block_node_reg).
"""
import collections
import functools
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .. import train_ops as T

_pack_cache = {}     # id(parameter) -> (weakref to THAT parameter, {transposed: (signature, PackedWeight, alias of the storage)})


def _packed(w, transposed):
    """PackedWeight of a 2-D weight; cached for nn.Parameters (keyed on storage + version), fresh for temporaries.
    An entry belongs to one parameter OBJECT and dies with it: ids, addresses and version counters all repeat between a dead
    module and the next one built the same way, so the id only finds the entry, the weak reference (`is`) decides, and its
    callback evicts.  (No WeakKeyDictionary: it compares keys with ==, which is element-wise on tensors.)  The alias of the
    storage keeps the address of the signature from being handed out again while the entry lives (utils/weight_cache.py)."""
    def build():
        src = w.detach()
        return ops.PackedWeight((src.t() if transposed else src).contiguous())
    if not isinstance(w, nn.Parameter):
        return build()
    key = id(w)
    ent = _pack_cache.get(key)
    if ent is None or ent[0]() is not w:
        def evict(ref, key=key, cache=_pack_cache):
            cur = cache.get(key)
            if cur is not None and cur[0] is ref:
                del cache[key]
        ent = _pack_cache[key] = (weakref.ref(w, evict), {})
    sig = (w.data_ptr(), w._version, w.device)
    hit = ent[1].get(transposed)
    if hit is not None and hit[0] == sig:
        return hit[1]
    pw = build()
    ent[1][transposed] = (sig, pw, w.detach())
    return pw


def drop_packs(params=None):
    """Forget the cached packs of `params` (an iterable of parameters; None: of every parameter).  utils.weight_cache.invalidate()
    calls it after in-place writes through `.data`, which no signature sees."""
    if params is None:
        _pack_cache.clear()
        return
    for p in params:
        ent = _pack_cache.get(id(p))
        if ent is not None and ent[0]() is p:
            del _pack_cache[id(p)]


def _pad4(x):
    c = x.shape[-1]
    return x.contiguous() if c % 4 == 0 else F.pad(x, (0, (-c) % 4)).contiguous()


class LinearRows(torch.autograd.Function):
    """y = x W^T (+ b) over rows.  x (R, >=Cin) f32 GPU, W (Cout, Cin), b (Cout) | None  ->  (R, Cout)."""

    @staticmethod
    def forward(ctx, x, w, b):
        if not x.is_cuda:
            raise ValueError("LinearRows runs on the GPU only (HIP kernels)")
        cout, cin = w.shape
        xp = _pad4(x[:, :cin]) if x.shape[1] != (cin + 3) // 4 * 4 else x.contiguous()
        y = ops.conv1x1_train(_packed(w, False), None if b is None else b.detach().contiguous(), xp.view(1, xp.shape[0], xp.shape[1]))
        ctx.save_for_backward(xp, w)
        ctx.has_bias = b is not None
        ctx.x_cols = x.shape[1]
        return y.view(xp.shape[0], -1)[:, :cout]

    @staticmethod
    def backward(ctx, dy):
        xp, w = ctx.saved_tensors
        cout, cin = w.shape
        R = xp.shape[0]
        dyp = _pad4(dy)
        dyv = dyp.view(1, R, dyp.shape[1])
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ops.conv1x1_train(_packed(w, True), None, dyv).view(R, -1)
            if dx.shape[1] != cin:
                dx[:, cin:] = 0.0
            if dx.shape[1] != ctx.x_cols:
                dx = dx[:, :ctx.x_cols] if dx.shape[1] > ctx.x_cols else F.pad(dx, (0, ctx.x_cols - dx.shape[1]))
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw = torch.empty(cout, cin, device=xp.device, dtype=torch.float32)
            db = torch.empty(cout, device=xp.device, dtype=torch.float32) if ctx.has_bias else None
            T.conv1x1_wgrad(dyv, xp.view(1, R, xp.shape[1]), cin, cout, dw, db)
        return dx, dw, db


def linear_rows(x, w, b=None):
    return LinearRows.apply(x, w, b)


class CnfAct(torch.autograd.Function):
    """Gated softplus layer on value + tangent rows (caspr_cnf_act_f32 / caspr_cnf_act_bwd_f32).
    z (2R,C) = layer product, b (C), gate / beta (frames, C), n points per frame -> h (2R,C)."""

    @staticmethod
    def forward(ctx, z, b, gate, beta, n, blk):
        from .. import lib as _lib
        from ..ops import _p, _stream
        R2, C = z.shape
        R = R2 // 2
        if not (z.is_cuda and z.stride(1) == 1 and z.stride(0) % 4 == 0):
            raise ValueError("CnfAct: z must be a GPU (2R,C) tensor with unit column stride")
        b, gate, beta = b.detach().contiguous(), gate.detach().contiguous(), beta.detach().contiguous()
        h = torch.empty(R2, C, device=z.device, dtype=torch.float32)
        _lib.check(_lib.load().caspr_cnf_act_f32(_p(z), z.stride(0), _p(b), _p(gate), _p(beta), R, n, C, blk, _p(h), C, _stream()), "caspr_cnf_act_f32")
        ctx.save_for_backward(z, b, gate, beta)
        ctx.n, ctx.blk = n, blk
        return h

    @staticmethod
    def backward(ctx, dh):
        from .. import lib as _lib
        from ..ops import _p, _stream
        z, b, gate, beta = ctx.saved_tensors
        R2, C = z.shape
        R = R2 // 2
        dh = dh.contiguous()
        dz = torch.empty(R2, C, device=z.device, dtype=torch.float32)
        dgate = torch.empty_like(gate)
        dbeta = torch.empty_like(beta)
        _lib.check(_lib.load().caspr_cnf_act_bwd_f32(_p(z), z.stride(0), _p(b), _p(gate), _p(beta), _p(dh), C, R, ctx.n, C, ctx.blk, _p(dz), C,
                                                     _p(dgate), _p(dbeta), _stream()), "caspr_cnf_act_bwd_f32")
        db = (gate * dbeta).sum(dim=0)                                    # d/db = sum_r da*g = sum_f g[f]*dbeta[f]
        return dz, db, dgate, dbeta, None, None


class CnfLayer(torch.autograd.Function):
    """A hidden layer of the ODE function in ONE launch: z = x W^T on the bf16x6 conv kernel with the gated softplus of CnfAct in
    its epilogue (caspr_conv1x1_cnf_act_bf16x6_f32; row layout blk = 32).  x (2R, Cin), W (Cout, Cin), b (Cout), gate / beta
    (frames, Cout) -> h (2R, Cout).  Same values as linear_rows + CnfAct, one pass less over the (2R, Cout) product."""

    @staticmethod
    def forward(ctx, x, w, b, gate, beta, n):
        from .. import lib as _lib
        from ..ops import _p, _stream
        cout, cin = w.shape
        R2 = x.shape[0]
        xp = x.contiguous()
        b, gate, beta = b.detach().contiguous(), gate.detach().contiguous(), beta.detach().contiguous()
        z = torch.empty(R2, cout, device=x.device, dtype=torch.float32)
        h = torch.empty(R2, cout, device=x.device, dtype=torch.float32)
        pw = _packed(w, False)
        with ops.timed("k:conv1x1_bf16x6:%d:%d:%d" % (cin, cout, R2), 2):
            _lib.check(_lib.load().caspr_conv1x1_cnf_act_bf16x6_f32(_p(pw.x3()), _p(b), _p(gate), _p(beta), _p(xp), xp.stride(0), _p(z), cout, _p(h), cout,
                                                                    R2 // (2 * n), n, cin, cout, _stream()), "caspr_conv1x1_cnf_act_bf16x6_f32")
        ctx.save_for_backward(xp, w, z, b, gate, beta)
        ctx.n = n
        return h

    @staticmethod
    def backward(ctx, dh):
        from .. import lib as _lib
        from ..ops import _p, _stream
        xp, w, z, b, gate, beta = ctx.saved_tensors
        cout, cin = w.shape
        R2 = xp.shape[0]
        dh = dh.contiguous()
        dz = torch.empty(R2, cout, device=z.device, dtype=torch.float32)
        dgate, dbeta = torch.empty_like(gate), torch.empty_like(beta)
        _lib.check(_lib.load().caspr_cnf_act_bwd_f32(_p(z), cout, _p(b), _p(gate), _p(beta), _p(dh), cout, R2 // 2, ctx.n, cout, 32, _p(dz), cout,
                                                     _p(dgate), _p(dbeta), _stream()), "caspr_cnf_act_bwd_f32")
        dzv = dz.view(1, R2, cout)
        dx = ops.conv1x1_train(_packed(w, True), None, dzv).view(R2, -1) if ctx.needs_input_grad[0] else None
        dw = torch.empty(cout, cin, device=xp.device, dtype=torch.float32)
        T.conv1x1_wgrad(dzv, xp.view(1, R2, cin), cin, cout, dw, None)
        return dx, dw, (gate * dbeta).sum(dim=0), dgate, dbeta, None


class CnfLayerOut(torch.autograd.Function):
    """The last hidden layer AND the 3-channel output product behind it (odefunc.py:103: no activation there): h = CnfLayer(x),
    zo = h Wo^T.  Backward: the output layer's data gradient dzo Wo is formed inside the activation's backward kernel
    (caspr_cnf_act_bwd_out_f32) instead of being written by a K = 3 conv and read back.
    x (2R, Cin), w (C, Cin), b (C), gate / beta (frames, C), wo (3, C) -> zo (2R, 3)."""

    @staticmethod
    def forward(ctx, x, w, b, gate, beta, wo, n):
        from .. import lib as _lib
        from ..ops import _p, _stream
        cout, cin = w.shape
        R2 = x.shape[0]
        xp = x.contiguous()
        b, gate, beta = b.detach().contiguous(), gate.detach().contiguous(), beta.detach().contiguous()
        z = torch.empty(R2, cout, device=x.device, dtype=torch.float32)
        h = torch.empty(R2, cout, device=x.device, dtype=torch.float32)
        with ops.timed("k:conv1x1_bf16x6:%d:%d:%d" % (cin, cout, R2), 2):
            _lib.check(_lib.load().caspr_conv1x1_cnf_act_bf16x6_f32(_p(_packed(w, False).x3()), _p(b), _p(gate), _p(beta), _p(xp), xp.stride(0), _p(z), cout,
                                                                    _p(h), cout, R2 // (2 * n), n, cin, cout, _stream()), "caspr_conv1x1_cnf_act_bf16x6_f32")
        zo = ops.conv1x1_train(_packed(wo, False), None, h.view(1, R2, cout)).view(R2, -1)
        ctx.save_for_backward(xp, w, z, b, gate, beta, h, wo)
        ctx.n = n
        return zo[:, :wo.shape[0]]

    @staticmethod
    def backward(ctx, dzo):
        from .. import lib as _lib
        from ..ops import _p, _stream
        xp, w, z, b, gate, beta, h, wo = ctx.saved_tensors
        cout, cin = w.shape
        R2 = xp.shape[0]
        dzop = _pad4(dzo)
        dwo = torch.empty(wo.shape[0], cout, device=xp.device, dtype=torch.float32)
        T.conv1x1_wgrad(dzop.view(1, R2, dzop.shape[1]), h.view(1, R2, cout), cout, wo.shape[0], dwo, None)
        dz = torch.empty(R2, cout, device=z.device, dtype=torch.float32)
        dgate, dbeta = torch.empty_like(gate), torch.empty_like(beta)
        woc = wo.detach().contiguous()
        _lib.check(_lib.load().caspr_cnf_act_bwd_out_f32(_p(z), cout, _p(b), _p(gate), _p(beta), _p(dzop), dzop.shape[1], _p(woc), cout, R2 // 2, ctx.n, cout,
                                                         32, _p(dz), cout, _p(dgate), _p(dbeta), _stream()), "caspr_cnf_act_bwd_out_f32")
        dzv = dz.view(1, R2, cout)
        dx = ops.conv1x1_train(_packed(w, True), None, dzv).view(R2, -1) if ctx.needs_input_grad[0] else None
        dw = torch.empty(cout, cin, device=xp.device, dtype=torch.float32)
        T.conv1x1_wgrad(dzv, xp.view(1, R2, cin), cin, cout, dw, None)
        return dx, dw, (gate * dbeta).sum(dim=0), dgate, dbeta, dwo, None


class SplitLayers(torch.autograd.Function):
    """(gate, bias) of all layers of one evaluation, stored LAYER-MAJOR in two 1-D tensors ([layer][frame][channel]) -> the per-layer
    (frames, C_l) tensors as contiguous VIEWS.  The gradient comes back as ONE concatenation per tensor.  (Column slices of a
    (frames, sum C) tensor cost a copy per layer and tensor on the way in and a zero-fill + copy each on the way back: 22
    launches per evaluation.)"""

    @staticmethod
    def forward(ctx, gate_lm, bias_lm, BT, widths):
        outs, off = [], 0
        for w in widths:
            outs.append(gate_lm[off:off + BT * w].view(BT, w))
            off += BT * w
        off = 0
        for w in widths:
            outs.append(bias_lm[off:off + BT * w].view(BT, w))
            off += BT * w
        ctx.BT, ctx.widths = BT, widths
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        L = len(ctx.widths)
        def cat(gs):
            gs = [g.reshape(-1) if g is not None else torch.zeros(ctx.BT * w, device=ref.device, dtype=ref.dtype) for g, w in zip(gs, ctx.widths)]
            return torch.cat(gs)
        ref = next(g for g in grads if g is not None)
        return cat(grads[:L]), cat(grads[L:]), None, None


def _cnf_out_args(who, zo, b, gate, beta):
    """The argument check CnfOut and CnfOutReg share -> b as the kernels read it."""
    if zo.stride(1) != 1 or gate.stride(1) != 1 or beta.stride(1) != 1 or gate.stride(0) != beta.stride(0):
        raise ValueError("%s: unit column strides and a common row stride of gate / beta are required" % who)
    return b.detach().contiguous()


class CnfOut(torch.autograd.Function):
    """Epilogue of the 3-channel output layer (caspr_cnf_out_f32 / _bwd_f32): zo (2R, 3) [a view of the conv's 4-wide rows], b (3),
    gate / beta (frames, 3) [column slices of the all-layer tensors: passed with their row stride], e (R, 3) ->
    a (BT, n, 3) = dy/dt and nd (BT, n, 1) = - e^T (df/dy) e.  One launch each way instead of ~25 element-wise ones."""

    @staticmethod
    def forward(ctx, zo, b, gate, beta, e_rows, n, blk):
        from .. import lib as _lib
        from ..ops import _p, _stream
        R = e_rows.shape[0]
        b = _cnf_out_args("CnfOut", zo, b, gate, beta)
        a = torch.empty(R, 3, device=zo.device, dtype=torch.float32)
        nd = torch.empty(R, 1, device=zo.device, dtype=torch.float32)
        _lib.check(_lib.load().caspr_cnf_out_f32(_p(zo), zo.stride(0), _p(b), _p(gate), _p(beta), gate.stride(0), _p(e_rows), R, n, blk, _p(a), _p(nd),
                                                 _stream()), "caspr_cnf_out_f32")
        ctx.save_for_backward(zo, b, gate, e_rows)
        ctx.n, ctx.blk = n, blk
        return a.view(R // n, n, 3), nd.view(R // n, n, 1)

    @staticmethod
    def backward(ctx, da, dnd):
        from .. import lib as _lib
        from ..ops import _p, _stream
        zo, b, gate, e_rows = ctx.saved_tensors
        R, n = e_rows.shape[0], ctx.n
        frames = R // n
        da, dnd = da.contiguous(), dnd.contiguous()
        dzo = torch.empty(2 * R, 4, device=zo.device, dtype=torch.float32)
        dgate = torch.empty(frames, 3, device=zo.device, dtype=torch.float32)
        dbeta = torch.empty(frames, 3, device=zo.device, dtype=torch.float32)
        _lib.check(_lib.load().caspr_cnf_out_bwd_f32(_p(da), _p(dnd), _p(zo), zo.stride(0), _p(b), _p(gate), gate.stride(0), _p(e_rows), R, n, ctx.blk,
                                                     _p(dzo), _p(dgate), _p(dbeta), _stream()), "caspr_cnf_out_bwd_f32")
        return dzo[:, :3], (gate * dbeta).sum(dim=0), dgate, dbeta, None, None, None


class CnfOutReg(torch.autograd.Function):
    """CnfOut with the integrands of the kinetic and Jacobian regularisers kept (caspr_cnf_out_reg_f32 / _bwd_f32; Finlay et al. 2020,
    "How to train your neural ODE"): same arguments -> a (BT, n, 3), nd (BT, n, 1) [CnfOut's bits] and q (BT, n, 2) with
    q[..., 0] = |a|^2 and q[..., 1] = |J e|^2.  The tangent rows of zo hold J e (forward mode), so the Jacobian term is the estimator
    |J e|^2, not RNODE's |e^T J|^2 (reverse mode); both have expectation |J|_F^2 for e ~ N(0, I).  The backward is first order: the
    cotangent 2 dq1 (J e) joins -dnd e on the tangent rows, which the layers' backward kernels take as any other."""

    @staticmethod
    def forward(ctx, zo, b, gate, beta, e_rows, n, blk):
        from .. import lib as _lib
        from ..ops import _p, _stream
        R = e_rows.shape[0]
        b = _cnf_out_args("CnfOutReg", zo, b, gate, beta)
        a = torch.empty(R, 3, device=zo.device, dtype=torch.float32)
        nd = torch.empty(R, 1, device=zo.device, dtype=torch.float32)
        q = torch.empty(R, 2, device=zo.device, dtype=torch.float32)
        _lib.check(_lib.load().caspr_cnf_out_reg_f32(_p(zo), zo.stride(0), _p(b), _p(gate), _p(beta), gate.stride(0), _p(e_rows), R, n, blk, _p(a),
                                                     _p(nd), _p(q), _stream()), "caspr_cnf_out_reg_f32")
        ctx.save_for_backward(zo, b, gate, beta, e_rows)
        ctx.n, ctx.blk = n, blk
        return a.view(R // n, n, 3), nd.view(R // n, n, 1), q.view(R // n, n, 2)

    @staticmethod
    def backward(ctx, da, dnd, dq):
        from .. import lib as _lib
        from ..ops import _p, _stream
        zo, b, gate, beta, e_rows = ctx.saved_tensors
        R, n = e_rows.shape[0], ctx.n
        frames = R // n
        da, dnd, dq = da.contiguous(), dnd.contiguous(), dq.contiguous()
        dzo = torch.empty(2 * R, 4, device=zo.device, dtype=torch.float32)
        dgate = torch.empty(frames, 3, device=zo.device, dtype=torch.float32)
        dbeta = torch.empty(frames, 3, device=zo.device, dtype=torch.float32)
        _lib.check(_lib.load().caspr_cnf_out_reg_bwd_f32(_p(da), _p(dnd), _p(dq), _p(zo), zo.stride(0), _p(b), _p(gate), _p(beta), gate.stride(0),
                                                         _p(e_rows), R, n, ctx.blk, _p(dzo), _p(dgate), _p(dbeta), _stream()),
                   "caspr_cnf_out_reg_bwd_f32")
        return dzo[:, :3], (gate * dbeta).sum(dim=0), dgate, dbeta, None, None, None


class CnfHidden(torch.autograd.Function):
    """Both hidden layers of the ODE function and the 3-channel output product as ONE node: forward = two fused conv + activation
    launches + the output conv; backward = the output layer's data gradient inside the last layer's activation backward (as
    CnfLayerOut), and the FIRST hidden layer's activation backward in the epilogue of the data-gradient conv that produces its dH
    (caspr_conv1x1_cnf_act_bwd_bf16x6_f32): that dH (2R x C) is never written, one 1 GB pass per evaluation less.
    x (2R, C0), (w1, b1, gate1, beta1), (w2, b2, gate2, beta2), wo (3, C2) -> zo (2R, 3).  Row layout blk = 32."""

    @staticmethod
    def forward(ctx, x, w1, b1, g1, be1, w2, b2, g2, be2, wo, n):
        from .. import lib as _lib
        from ..ops import _p, _stream
        L = _lib.load()
        R2 = x.shape[0]
        xp = x.contiguous()
        b1, g1, be1, b2, g2, be2 = [t.detach().contiguous() for t in (b1, g1, be1, b2, g2, be2)]
        zs, hs, cur = [], [], xp
        for (w, b, g, be) in ((w1, b1, g1, be1), (w2, b2, g2, be2)):
            cout, cin = w.shape
            z = torch.empty(R2, cout, device=x.device, dtype=torch.float32)
            h = torch.empty(R2, cout, device=x.device, dtype=torch.float32)
            with ops.timed("k:conv1x1_bf16x6:%d:%d:%d" % (cin, cout, R2), 2):
                _lib.check(L.caspr_conv1x1_cnf_act_bf16x6_f32(_p(_packed(w, False).x3()), _p(b), _p(g), _p(be), _p(cur), cur.stride(0), _p(z), cout, _p(h), cout,
                                                              R2 // (2 * n), n, cin, cout, _stream()), "caspr_conv1x1_cnf_act_bf16x6_f32")
            zs.append(z)
            hs.append(h)
            cur = h
        zo = ops.conv1x1_train(_packed(wo, False), None, cur.view(1, R2, cur.shape[1])).view(R2, -1)
        ctx.save_for_backward(xp, w1, b1, g1, be1, w2, b2, g2, be2, wo, zs[0], hs[0], zs[1], hs[1])
        ctx.n = n
        return zo[:, :wo.shape[0]]

    @staticmethod
    def backward(ctx, dzo):
        from .. import lib as _lib
        from ..ops import _p, _stream, _workspace
        L = _lib.load()
        xp, w1, b1, g1, be1, w2, b2, g2, be2, wo, z1, h1, z2, h2 = ctx.saved_tensors
        n, R2 = ctx.n, xp.shape[0]
        c1, c0 = w1.shape
        c2 = w2.shape[0]
        dev = xp.device
        dzop = _pad4(dzo)
        dwo = torch.empty(wo.shape[0], c2, device=dev, dtype=torch.float32)
        T.conv1x1_wgrad(dzop.view(1, R2, dzop.shape[1]), h2.view(1, R2, c2), c2, wo.shape[0], dwo, None)
        # last hidden layer: dH = dzo Wo formed inside the activation backward
        dz2 = torch.empty(R2, c2, device=dev, dtype=torch.float32)
        dg2, db2 = torch.empty_like(g2), torch.empty_like(be2)
        woc = wo.detach().contiguous()
        _lib.check(L.caspr_cnf_act_bwd_out_f32(_p(z2), c2, _p(b2), _p(g2), _p(be2), _p(dzop), dzop.shape[1], _p(woc), c2, R2 // 2, n, c2, 32, _p(dz2), c2,
                                               _p(dg2), _p(db2), _stream()), "caspr_cnf_act_bwd_out_f32")
        dw2 = torch.empty(c2, c1, device=dev, dtype=torch.float32)
        T.conv1x1_wgrad(dz2.view(1, R2, c2), h1.view(1, R2, c1), c1, c2, dw2, None)
        # first hidden layer: its activation backward in the epilogue of dz2 W2 (the product that is its dH)
        dz1 = torch.empty(R2, c1, device=dev, dtype=torch.float32)
        dg1, db1 = torch.empty_like(g1), torch.empty_like(be1)
        frames = R2 // (2 * n)
        nbytes = L.caspr_conv1x1_cnf_act_bwd_ws_bytes(frames, n, c1)
        ws = _workspace(nbytes, dev)
        with ops.timed("k:conv1x1_bf16x6:%d:%d:%d" % (c2, c1, R2), 2):
            _lib.check(L.caspr_conv1x1_cnf_act_bwd_bf16x6_f32(_p(_packed(w2, True).x3()), _p(dz2), c2, _p(z1), c1, _p(b1), _p(g1), _p(be1), _p(dz1), c1,
                                                              _p(dg1), _p(db1), _p(ws), ws.numel(), frames, n, c2, c1, _stream()),
                       "caspr_conv1x1_cnf_act_bwd_bf16x6_f32")
        dw1 = torch.empty(c1, c0, device=dev, dtype=torch.float32)
        T.conv1x1_wgrad(dz1.view(1, R2, c1), xp.view(1, R2, c0), c0, c1, dw1, None)
        dx = ops.conv1x1_train(_packed(w1, True), None, dz1.view(1, R2, c1)).view(R2, -1) if ctx.needs_input_grad[0] else None
        return (dx, dw1, (g1 * db1).sum(dim=0), dg1, db1, dw2, (g2 * db2).sum(dim=0), dg2, db2, dwo, None)


def _fused_layer_ok(l, n):
    cout, cin = l._layer.weight.shape
    return ops.CONV_BF16X6 and cin % 32 == 0 and cin >= 64 and cout % 4 == 0 and cout >= 128 and n % 64 == 0


class CnfIn(torch.autograd.Function):
    """First ODE-function layer (3 -> C) fused with gate + softplus on value / tangent rows
    (caspr_cnf_in_f32 / caspr_cnf_in_bwd_f32).  y, e (R,3); w0 (C,3); b0 (C); gate / beta (frames, C) -> h (2R, C)."""

    @staticmethod
    def forward(ctx, y, e, w0, b0, gate, beta, n, blk):
        from .. import lib as _lib
        from ..ops import _p, _stream
        if not y.is_cuda:
            raise ValueError("CnfIn runs on the GPU only (HIP kernels)")
        R, C = y.shape[0], w0.shape[0]
        y, e = y.detach().contiguous(), e.detach().contiguous()
        w0, b0, gate, beta = w0.detach().contiguous(), b0.detach().contiguous(), gate.detach().contiguous(), beta.detach().contiguous()
        h = torch.empty(2 * R, C, device=y.device, dtype=torch.float32)
        _lib.check(_lib.load().caspr_cnf_in_f32(_p(y), _p(e), _p(w0), _p(b0), _p(gate), _p(beta), R, n, C, blk, _p(h), _stream()), "caspr_cnf_in_f32")
        ctx.save_for_backward(y, e, w0, b0, gate, beta)
        ctx.n, ctx.blk = n, blk
        return h

    @staticmethod
    def backward(ctx, dh):
        from .. import lib as _lib
        from ..ops import _p, _stream
        y, e, w0, b0, gate, beta = ctx.saved_tensors
        R, C = y.shape[0], w0.shape[0]
        L = _lib.load()
        ch, ns = L.caspr_cnf_in_bwd_chunk(C), L.caspr_cnf_in_bwd_splits(C, ctx.n)
        frames, chunks = R // ctx.n, (C + ch - 1) // ch
        dh = dh.contiguous()
        dgate = torch.empty(frames, ns, C, device=y.device, dtype=torch.float32)
        dbeta = torch.empty(frames, ns, C, device=y.device, dtype=torch.float32)
        dw_part = torch.empty(frames * ns, C, 3, device=y.device, dtype=torch.float32)
        dy_part = torch.empty(chunks, R, 3, device=y.device, dtype=torch.float32)
        _lib.check(L.caspr_cnf_in_bwd_f32(_p(y), _p(e), _p(w0), _p(b0), _p(gate), _p(beta), _p(dh), R, ctx.n, C, ctx.blk, _p(dgate), _p(dbeta),
                                          _p(dw_part), _p(dy_part), _stream()), "caspr_cnf_in_bwd_f32")
        if ns > 1:
            dgate, dbeta = dgate.sum(dim=1), dbeta.sum(dim=1)
        else:
            dgate, dbeta = dgate[:, 0], dbeta[:, 0]
        return dy_part.sum(dim=0), None, dw_part.sum(dim=0), (gate * dbeta).sum(dim=0), dgate, dbeta, None, None


# ---------------------------------------------------------------------------------------------
# latent ODE (latent_ode_model.py:45-70,139-147): z' = MLP_tanh(z), classic RK4, `steps` per requested interval
# ---------------------------------------------------------------------------------------------
class LatentSolve(torch.autograd.Function):
    """The whole latent RK4 solve as ONE autograd node: a taped forward and a hand-written reverse sweep over the same kernels
    (conv1x1 forward / transposed), with the WEIGHT gradients of all evaluations taken at the end as one product per layer over
    the concatenated rows (the four layers are shared by every evaluation: dW = sum_e d_e^T x_e = [d_1; d_2; ...]^T [x_1; x_2; ...]).
    Node per layer call (`linear_rows`) this was 288 eight-row weight-gradient launches with their slab reductions and 288
    gradient accumulations per step (cfg-3: 72 evaluations x 4 layers); same arithmetic otherwise.
    z0 (B,D), tt (Tu,) device times, steps, then w0, b0, ..., w3, b3 -> (B,Tu,D)."""

    TEAM = True        # the one-launch forms (caspr_latent_rk4_team_tape_f32 / _adjoint_f32) where the shape allows

    @staticmethod
    def _team_ok(z0, ws, bs):
        return (LatentSolve.TEAM and len(ws) == 4 and all(b is not None for b in bs) and z0.shape[0] <= 64 and ws[0].shape[0] == 512
                and ws[1].shape == (512, 512) and ws[2].shape == (512, 512) and ws[3].shape[1] == 512 and ws[0].shape[1] == ws[3].shape[0] <= 64
                and ws[0].shape[1] == z0.shape[1])

    @staticmethod
    def _forward_team(ctx, z0, tt, steps, ws, bs):
        from .. import lib as _lib
        from ..ops import _p, _stream
        L = _lib.load()
        B, D = z0.shape
        Tu = tt.shape[0]
        E, xw = 4 * steps * (Tu - 1), (D + 3) // 4 * 4
        dev = z0.device
        pk = [_packed(w, False) for w in ws]
        bd = [b.detach().contiguous() for b in bs]
        zc = z0.detach().contiguous()
        tape = [torch.zeros(E * B, xw, device=dev, dtype=torch.float32)] + [torch.zeros(E * B, 512, device=dev, dtype=torch.float32) for _ in range(3)]
        out = torch.empty(B, Tu, D, device=dev, dtype=torch.float32)
        ptrs = [p_ for w, b in zip(pk, bd) for p_ in (_p(w.data), _p(b))]
        with ops._team.on(dev) as status:                          # as ops.latent_rk4
            wsb = ops._team_workspace(L.caspr_latent_team_ws_bytes(B), dev)
            with ops.timed("latent_rk4_tape"):
                _lib.check(L.caspr_latent_rk4_team_tape_f32(_p(zc), zc.stride(0), _p(tt), B, Tu, D, 512, int(steps), *ptrs, _p(out), _p(tape[0]), xw,
                                                            _p(tape[1]), _p(tape[2]), _p(tape[3]), _p(wsb), wsb.numel(), _stream()),
                           "caspr_latent_rk4_team_tape_f32")
            status.post(ops._team_words(wsb, B))
        ctx.team, ctx.tape, ctx.tt, ctx.steps, ctx.ws = True, tape, tt, steps, ws
        return out

    @staticmethod
    def _backward_team(ctx, gout):
        from .. import lib as _lib
        from ..ops import _p, _stream
        L = _lib.load()
        tape, tt, steps, ws = ctx.tape, ctx.tt, ctx.steps, ctx.ws
        B, Tu, D = gout.shape
        xw = tape[0].shape[1]
        dev = gout.device
        pkt = [_packed(w, True) for w in ws]
        g = gout.contiguous()
        deltas = [torch.zeros_like(tape[1]) for _ in range(3)] + [torch.zeros_like(tape[0])]
        gz = torch.empty(B, D, device=dev, dtype=torch.float32)
        with ops._team.on(dev) as status:                          # as ops.latent_rk4
            wsb = ops._team_workspace(L.caspr_latent_team_ws_bytes(B), dev)
            with ops.timed("latent_rk4_adjoint"):
                _lib.check(L.caspr_latent_rk4_team_adjoint_f32(_p(g), _p(tt), B, Tu, D, 512, int(steps), _p(pkt[3].data), _p(pkt[2].data), _p(pkt[1].data),
                                                               _p(pkt[0].data), _p(tape[1]), _p(tape[2]), _p(tape[3]), _p(deltas[0]), _p(deltas[1]),
                                                               _p(deltas[2]), _p(deltas[3]), xw, _p(gz), _p(wsb), wsb.numel(), _stream()),
                           "caspr_latent_rk4_team_adjoint_f32")
            status.post(ops._team_words(wsb, B))
        grads = []
        for i in range(4):
            cout, cin = ws[i].shape
            dw = torch.empty(cout, cin, device=dev, dtype=torch.float32)
            db = torch.empty(cout, device=dev, dtype=torch.float32)
            T.conv1x1_wgrad(deltas[i].view(1, deltas[i].shape[0], -1), tape[i].view(1, tape[i].shape[0], -1), cin, cout, dw, db)
            grads += [dw, db]
        ctx.tape = None
        return (gz, None, None) + tuple(grads)

    @staticmethod
    def forward(ctx, z0, tt, steps, *wb):
        ws, bs = wb[0::2], wb[1::2]
        ctx.single = tt.shape[0] == 1
        if ctx.single:          # one time stamp: nothing to integrate (odeint returns the initial state, latent_ode_model.py:58-66)
            ctx.ws, ctx.has_b = ws, [b is not None for b in bs]
            return z0.detach().unsqueeze(1).clone()
        if LatentSolve._team_ok(z0, ws, bs):
            return LatentSolve._forward_team(ctx, z0, tt, steps, ws, bs)
        ctx.team = False
        pk = [_packed(w, False) for w in ws]
        bd = [b.detach().contiguous() for b in bs]
        B = z0.shape[0]
        tape = []

        def f(z):
            a = [_pad4(z)]                             # rows of roundup4(D) floats, zero-filled: conv1x1 takes row strides that are multiples of 4
            for i in range(4):
                y = ops.conv1x1_train(pk[i], bd[i], a[-1].view(1, B, -1)).view(B, -1)[:, :ws[i].shape[0]]
                a.append(torch.tanh(y) if i < 3 else y)
            tape.append(a[:4])
            return a[4]
        outs, z, hs = [z0], z0.detach(), []
        for k in range(1, tt.shape[0]):
            h = (tt[k] - tt[k - 1]) / steps
            hh = (h, 0.5 * h, h / 3.0, h / 6.0)         # 0-dim device tensors, made once per interval: one fused launch per RK4 combination
            for _ in range(steps):
                k1 = f(z)
                k2 = f(torch.addcmul(z, k1, hh[1]))
                k3 = f(torch.addcmul(z, k2, hh[1]))
                k4 = f(torch.addcmul(z, k3, hh[0]))
                z = torch.addcmul(z, torch.add(k1 + k4, k2 + k3, alpha=2.0), hh[3])
                hs.append(hh)
            outs.append(z)
        ctx.tape, ctx.hs, ctx.steps, ctx.ws = tape, hs, steps, ws
        ctx.has_b = [b is not None for b in bs]
        return torch.stack(outs, dim=1)

    @staticmethod
    def backward(ctx, gout):
        if ctx.single:
            zeros = [g for w, hb in zip(ctx.ws, ctx.has_b) for g in (torch.zeros_like(w), torch.zeros(w.shape[0], device=w.device, dtype=w.dtype) if hb else None)]
            return (gout[:, 0].contiguous(), None, None) + tuple(zeros)
        if ctx.team:
            return LatentSolve._backward_team(ctx, gout)
        tape, hs, steps, ws = ctx.tape, ctx.hs, ctx.steps, ctx.ws
        pkt = [_packed(w, True) for w in ws]
        B = gout.shape[0]
        deltas, inputs = [[] for _ in range(4)], [[] for _ in range(4)]

        def fb(a, g):                              # a = (x, h1, h2, h3) of one evaluation, g = dL/d f(x) -> dL/dx
            for i in (3, 2, 1, 0):
                d = _pad4(g) if i == 3 else torch.ops.aten.tanh_backward(g, a[i + 1])    # tanh' from the layer's stored output: one launch
                deltas[i].append(d)
                inputs[i].append(a[i])
                g = ops.conv1x1_train(pkt[i], None, d.view(1, B, -1)).view(B, -1)[:, :ws[i].shape[1]]
            return g
        Tu = gout.shape[1]
        gz = gout[:, Tu - 1].clone()
        e = len(tape)
        for k in range(Tu - 1, 0, -1):
            for st in range(steps):
                h, h2, h3, h6 = hs[(k - 1) * steps + (steps - 1 - st)]
                a1, a2, a3, a4 = tape[e - 4], tape[e - 3], tape[e - 2], tape[e - 1]
                e -= 4
                g6, g3z = h6 * gz, h3 * gz
                g4 = fb(a4, g6)
                g3 = fb(a3, torch.addcmul(g3z, g4, h))
                g2 = fb(a2, torch.addcmul(g3z, g3, h2))
                g1 = fb(a1, torch.addcmul(g6, g2, h2))
                gz = gz + (g4 + g3) + (g2 + g1)
            gz = gz + gout[:, k - 1]
        grads = []
        for i in range(4):
            d, x = torch.cat(deltas[i], dim=0), torch.cat(inputs[i], dim=0)
            cout, cin = ws[i].shape
            dw = torch.empty(cout, cin, device=d.device, dtype=torch.float32)
            db = torch.empty(cout, device=d.device, dtype=torch.float32) if ctx.has_b[i] else None
            T.conv1x1_wgrad(_pad4(d).view(1, d.shape[0], -1), _pad4(x).view(1, x.shape[0], -1), cin, cout, dw, db)
            grads += [dw, db]
        ctx.tape = None
        return (gz, None, None) + tuple(grads)


class LatentSolveDopri5(torch.autograd.Function):
    """The ADAPTIVE latent solve (LatentODE(method="dopri5"); latent_ode_model.py:45-70,85-99, where the reference trains through
    odeint_adjoint on dopri5) as one autograd node: forward = train_ops.latent_dopri5_tape, the launch and the bits of
    ops.latent_dopri5 plus (z_n, dt_n) of every accepted step; backward = train_ops.latent_dopri5_adjoint, one launch, then one
    weight-gradient product per layer over all evaluations' rows, as LatentSolve._backward_team.
    The gradient is the one of the forward's own discrete map with its accepted step sequence held fixed: every dt, stage time,
    interpolation abscissa and accept / reject decision is a constant, rejected attempts and the initial-step selection contribute
    nothing.  Left out: the dependence of the step sizes on z0 and the parameters (the sensitivity of the discretisation error, of the
    order of the tolerance) -- the reference's continuous adjoint never differentiates its controller either.
    z0 (B,D), tt (Tu,) ascending device times, rtol, atol, max_attempts, max_steps, then w0, b0, ..., w3, b3 -> (B,Tu,D).
    One stamp, or all stamps equal: the launch makes no attempt (two evaluations, the initial-step selection's, as in inference); the
    output is z0 at every stamp, dL/dz0 the sum of gout over the stamps (in f64, rounded once), the parameter gradients exactly zero.
    The stamps' values are never read on the host; with one stamp the backward skips its launch.
    Backward memory: B (1 + 6 max_steps) rows x (3 H + 2 roundup4(D)) floats x 2, freed after the products: about 39 MB at B = 8 and
    315 MB at B = 64 for max_steps = 64, H = 512.  The accepted count is not read on the host to shrink it.
    `info` of the last forward (trace views and counters, device tensors) is left in LatentSolveDopri5.last_info."""

    last_info = None

    @staticmethod
    def forward(ctx, z0, tt, rtol, atol, max_attempts, max_steps, *wb):
        ws, bs = wb[0::2], wb[1::2]
        if any(b is None for b in bs):
            raise ValueError("LatentSolveDopri5: the dynamics net's four layers carry biases (latent_ode_model.py:139-147)")
        ctx.ws = ws
        ctx.single = tt.shape[0] == 1
        pk = [_packed(w, False) for w in ws]
        bd = [b.detach().contiguous() for b in bs]
        wts = [x for w, b in zip(pk, bd) for x in (w, b)]
        out, info, tape = T.latent_dopri5_tape(z0.detach(), tt, rtol, atol, wts, max_attempts=max_attempts, max_steps=max_steps)
        LatentSolveDopri5.last_info = info
        ctx.tape, ctx.wts = tape, wts
        return out

    @staticmethod
    def backward(ctx, gout):
        ws = ctx.ws
        if ctx.single:
            zeros = [g for w in ws for g in (torch.zeros_like(w), torch.zeros(w.shape[0], device=w.device, dtype=w.dtype))]
            return (gout[:, 0].contiguous(), None, None, None, None, None) + tuple(zeros)
        pkt = [_packed(w, True) for w in (ws[3], ws[2], ws[1], ws[0])]
        gz, inputs, deltas = T.latent_dopri5_adjoint(gout.contiguous(), ctx.tape, ctx.wts, pkt)
        grads = []
        for i in range(4):
            cout, cin = ws[i].shape
            dw = torch.empty(cout, cin, device=gz.device, dtype=torch.float32)
            db = torch.empty(cout, device=gz.device, dtype=torch.float32)
            T.conv1x1_wgrad(deltas[i].view(1, deltas[i].shape[0], -1), inputs[i].view(1, inputs[i].shape[0], -1), cin, cout, dw, db)
            grads += [dw, db]
        ctx.tape = ctx.wts = None
        return (gz, None, None, None, None, None) + tuple(grads)


def latent_solve_layers(lat, z0, times):
    """The same solve with one autograd node per layer call (`linear_rows`) and torch.autograd's own reverse sweep: what
    LatentSolve is checked against (tests/test_hip_train.py)."""
    lin = [lat.ode_func.dynamics_net[i] for i in (0, 2, 4, 6)]

    def f(z):
        h = z
        for i, l in enumerate(lin):
            h = linear_rows(h, l.weight, l.bias)
            if i < 3:
                h = torch.tanh(h)
        return h
    outs, z, tt = [z0], z0, times.detach().float()
    for k in range(1, tt.shape[0]):
        h = (tt[k] - tt[k - 1]) / lat.rk4_steps
        for _ in range(lat.rk4_steps):
            k1 = f(z)
            k2 = f(z + 0.5 * h * k1)
            k3 = f(z + 0.5 * h * k2)
            k4 = f(z + h * k3)
            z = z + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        outs.append(z)
    return torch.stack(outs, dim=1)


from ..config import config as _cfg     # (A/B timing and debugging switches: caspr_amd/config.py, environment only under CASPR_DEBUG=1)
OUT_NODE = _cfg.train_cnf_out_node          # False: the output layer's epilogue in torch element-wise ops
HIDDEN_NODE = _cfg.train_cnf_hidden_node    # False: CnfLayer + CnfLayerOut
LATENT_NODE = _cfg.train_latent_node        # False: the per-layer form
CHECKPOINT_STEPS = _cfg.train_cnf_checkpoint   # True: the CNF's tape per RK4 step, recomputed in the backward pass (cnf_block_train)
BLOCK_NODE = _cfg.train_cnf_block_node      # True: a CNF block as one autograd node (CnfBlockSolve) where the shape allows; wins over CHECKPOINT_STEPS
BLOCK_NODE_REG = _cfg.train_cnf_block_node_reg   # True (with BLOCK_NODE): cnf_block_train(reg=True) on the node too (CnfBlockSolveReg) instead of refusing


def latent_solve_train(lat, z0, times):
    """z0 (B,D) differentiable, times (Tu,) ascending -> (B,Tu,D); first output is z0 itself.  lat.method "dopri5" (with
    config.train_latent_dopri5, which LatentODE checks): the adaptive solve's node, LatentSolveDopri5."""
    tt = times.detach().float()
    wb = []
    for i in (0, 2, 4, 6):
        l = lat.ode_func.dynamics_net[i]
        wb += [l.weight, l.bias]
    if lat.method == "dopri5":
        out = LatentSolveDopri5.apply(z0, tt.contiguous(), lat.rtol, lat.atol, lat.max_attempts, lat.train_max_steps, *wb)
        info = LatentSolveDopri5.last_info
        lat.last_nfe_per_sequence = info["nfe"]           # measured, as LatentODE.solve_dopri5: element-wise device ops, no host read
        lat.ode_func._num_evals.mul_(0).add_(info["nfe"].max().to(lat.ode_func._num_evals.dtype))
        return out
    if LATENT_NODE:
        out = LatentSolve.apply(z0, tt, lat.rk4_steps, *wb)
    else:
        out = latent_solve_layers(lat, z0, times)
    lat.ode_func._num_evals.fill_(4 * lat.rk4_steps * max(tt.shape[0] - 1, 0))
    return out


# ---------------------------------------------------------------------------------------------
# point CNF block (cnf.py:70-128, odefunc.py:119-142, diffeq_layers.py:83-90)
# ---------------------------------------------------------------------------------------------
def _layer_views(v_lm, BT, widths):
    """Layer-major 1-D tensor ([layer][frame][channel]) -> the per-layer (BT, C_l) views."""
    outs, off = [], 0
    for w in widths:
        outs.append(v_lm[off:off + BT * w].view(BT, w))
        off += BT * w
    return outs


def _cnf_eval_fused(wb, t, y, G_lm, Bb_lm, tg_lm, tb_lm, e_rows, BT, n, widths):
    """One evaluation of the ODE function on the training kernels in the fused-layer row layout (blk = 32): the nodes `func` of
    cnf_block_train runs by default.  wb = (w0, b0, ..., w3, b3); y (BT,n,3) -> a (BT,n,3), nd (BT,n,1)."""
    w0, b0, w1, b1, w2, b2, w3, b3 = wb
    parts = SplitLayers.apply(torch.sigmoid(G_lm + t * tg_lm), Bb_lm + t * tb_lm, BT, widths)
    h = CnfIn.apply(y.reshape(BT * n, 3), e_rows, w0, b0, parts[0], parts[4], n, 32)
    z = CnfHidden.apply(h, w1, b1, parts[1], parts[5], w2, b2, parts[2], parts[6], w3, n)
    return CnfOut.apply(z, b3, parts[3], parts[7], e_rows, n, 32)


def _cnf_eval_fused_reg(wb, t, y, G_lm, Bb_lm, tg_lm, tb_lm, e_rows, BT, n, widths):
    """_cnf_eval_fused with CnfOutReg at its end: the same nodes up to the output product -> a (BT,n,3), nd (BT,n,1) [its bits] and
    q (BT,n,2) = (|a|^2, |J e|^2), the regularisers' integrands.  What CnfBlockSolveReg's reverse sweep rebuilds and differentiates."""
    w0, b0, w1, b1, w2, b2, w3, b3 = wb
    parts = SplitLayers.apply(torch.sigmoid(G_lm + t * tg_lm), Bb_lm + t * tb_lm, BT, widths)
    h = CnfIn.apply(y.reshape(BT * n, 3), e_rows, w0, b0, parts[0], parts[4], n, 32)
    z = CnfHidden.apply(h, w1, b1, parts[1], parts[5], w2, b2, parts[2], parts[6], w3, n)
    return CnfOutReg.apply(z, b3, parts[3], parts[7], e_rows, n, 32)


def _hyper_layer_major(block, context):
    """The four hyper networks of a CNF block for every frame, as both block nodes (CnfBlockSolve, CnfSampleSolve) and the taped route
    take them: the context columns once per solve through `linear_rows` (constant over the solve; this is where dL/d context and the
    hyper networks' gradients flow), the time column per evaluation.  All four layers' gate / bias rows live in layer-major 1-D tensors
    ([layer][frame][channel]) so that the per-evaluation time update is one element-wise launch for all layers and the per-layer
    (BT, C_l) tensors are contiguous views.  context (BT, zdim) -> G_lm, Bb_lm, tg_lm, tb_lm, widths."""
    BT = context.shape[0]
    c = context.contiguous()
    G, Bb, tg, tb, widths = [], [], [], [], []
    for l in block.odefunc.diffeq.layers:
        wg, wb = l._hyper_gate.weight, l._hyper_bias.weight
        G.append(linear_rows(c, wg[:, 1:].contiguous(), l._hyper_gate.bias))
        Bb.append(linear_rows(c, wb[:, 1:].contiguous(), None))
        tg.append(wg[:, 0])
        tb.append(wb[:, 0])
        widths.append(wg.shape[0])
    G_lm, Bb_lm = torch.cat([g.reshape(-1) for g in G]), torch.cat([b_.reshape(-1) for b_ in Bb])
    tg_lm = torch.cat([v.unsqueeze(0).expand(BT, -1).reshape(-1) for v in tg])
    tb_lm = torch.cat([v.unsqueeze(0).expand(BT, -1).reshape(-1) for v in tb])
    return G_lm, Bb_lm, tg_lm, tb_lm, tuple(widths)


def _hyper_for_kernel(G_lm, Bb_lm, tg_lm, tb_lm, BT, widths):
    """The layer-major hyper tensors in the form the solve kernels read (ops.cnf_rk4): hyper (BT, [gate l0..l3 | bias l0..l3]) and
    tcol, one row of the time columns in the same order.  Detached: the kernels are not differentiated through."""
    hyper = torch.cat(_layer_views(G_lm.detach(), BT, widths) + _layer_views(Bb_lm.detach(), BT, widths), dim=1).contiguous()
    tcol = torch.cat([v[0] for v in _layer_views(tg_lm.detach(), BT, widths) + _layer_views(tb_lm.detach(), BT, widths)]).contiguous()
    return hyper, tcol


# the packs of one hidden layer for a sampling node under ops.CNF_TAPE_SPLIT = "f16x3": bf16x6 (ops.pack_cnf_x6) and f16x3 (ops.pack_cnf_h3)
_SolvePacks = collections.namedtuple("_SolvePacks", "x6 h3")


def _sample_tape_route(w1x, w2x, n):
    """Which forward launch a sampling node takes, by the rule ops.cnf_rk4 routes inference with (ops._cnf_route): the 128-point f16x3
    kernel when it takes n points and the switch is on (the packs then come as _SolvePacks), the 64-point bf16x6 kernel otherwise
    -> (f16x3?, w1, w2)."""
    if isinstance(w1x, _SolvePacks):
        if ops._cnf_route(n, True, True) == "h3" and ops.cnf_tape_split() == "f16x3":
            return True, w1x.h3, w2x.h3
        return False, w1x.x6, w2x.x6
    return False, w1x, w2x


def _block_node_inputs(block, context, device, tape_h3=False):
    """What a block node (CnfBlockSolve, CnfSampleSolve, CnfSampleSolveFrames) takes of its block:
    -> (G_lm, Bb_lm, tg_lm, tb_lm, widths) of _hyper_layer_major, t_end (0-dim, differentiable when the block trains it), the two packed
    512 x 512 weights of the solve kernel (w1x, w2x), and [w0, b0, ..., w3, b3].  tape_h3 (the two sampling nodes): with
    ops.CNF_TAPE_SPLIT = "f16x3" w1x / w2x each come as a _SolvePacks pair that also holds the block's f16x3 pack (block._weights_h3(),
    a cache that follows its parameters); the node's forward chooses by n (_sample_tape_route)."""
    hyper = _hyper_layer_major(block, context)
    t_end = block.sqrt_end_time * block.sqrt_end_time if block.train_T else torch.tensor(float(block.T), device=device)
    w1x, w2x = block._weights_x6()
    if tape_h3 and ops.cnf_tape_split() == "f16x3":
        w1h, w2h = block._weights_h3()
        w1x, w2x = _SolvePacks(w1x, w1h), _SolvePacks(w2x, w2h)
    return hyper, t_end, w1x, w2x, [p_ for l in block.odefunc.diffeq.layers for p_ in (l._layer.weight, l._layer.bias)]


def _rk4_reverse_sweep(ys, tapes, gy, g_rest, h_all, stage_time, start_time, evaluate, hyper, wb, widths, prefix=None):
    """The reverse sweep of a fixed-step RK4 solve of a CNF block, shared by CnfBlockSolve, CnfSampleSolve and CnfSampleSolveFrames.

    The forward kernels integrate, per step s = 0..S-1 with step size h and start time t0,
        y_i = y + c_i h k_{i-1},   k_i = f(t0 + (s + c_i) h, y_i)   (i = 1..4, c = TC),   y' = y + h sum_i w_i k_i   (w = CW)
    and tape every y_i (`ys`) and k_i (`tapes[0]`; a second output of f that is only summed, the log-density's integrand, has a tape
    and a constant cotangent of its own: `tapes[1]`, `g_rest[0]`).  Steps are walked S-1..0 and stages 4..1.
      Cotangent recursion: with gy = dL/dy', stage i receives  k_i_bar = w_i h gy + c_{i+1} h y_{i+1}_bar  (the second term absent for
        i = 4), a summed output w_i h times its cotangent.  ONE evaluation is rebuilt from its stored y_i under enable_grad
        (`evaluate`), the cotangents are pushed through it with torch.autograd.grad, the tape of that evaluation is dropped;
        y_i_bar comes back and dL/dy = gy + sum_i y_i_bar.
      h enters by three routes, all summed into dL/dh in f64: the state update (<gy, sum_i w_i k_i>, one dot per output tape), the
        stage inputs (c_i <y_i_bar, k_{i-1}>) and the stage times ((s + c_i) dL/dt_i).
      Start time: t_i = t0 + (s + c_i) h also gives dL/dt0 = sum dL/dt_i, kept when `start_time` (t0 = t_end on the reversed axis).
      Fixed order: stage-major within a step, steps descending, every hyper and weight gradient ADDED into a buffer allocated before
        the loop -- no atomics, two runs give the same bits.

    What differs between the nodes is handed in:
      h_all, stage_time(s, c, h) -> the stage time in that node's own rounding (h s + c h forward, t0 + (s + c) h reversed);
      evaluate(t, y_in, hyp, F) -> the tuple of outputs of one evaluation on F frames (through the module's _cnf_eval_* at call time);
      prefix None: uniform step count -- h_all 0-dim, a 0-dim time leaf, dots summed over everything, 0-dim f64 accumulators, `hyper`
        the node's four layer-major tensors made leaves once;
      prefix = [F_s for s in 0..S-1]: a count per frame, frames in launch order (longest first) -- only the first F_s = #{f: S_f > s}
        frames take part at step s: h_all (BT,), an (F_s,) time leaf expanded to layer-major, dots and accumulators per frame, the hyper
        leaves rebuilt from `hyper` (detached, launch order) and the prefix's gradients flushed into the full buffers when F_s changes.
    -> gy (dL/dy; written in place where a prefix is given), the four hyper gradients, the weight gradients (None where not required),
    dL/dh and dL/dt0 (None without start_time) in f64."""
    S, _, BT, _, _ = ys.shape
    dev = ys.device
    per_frame = prefix is not None
    wsel = [i for i, w in enumerate(wb) if w.requires_grad]
    d_hyp = [torch.zeros_like(v) for v in hyper]
    d_wb = [torch.zeros_like(w) if w.requires_grad else None for w in wb]
    dh = torch.zeros((BT,) if per_frame else (), device=dev, dtype=torch.float64)
    dt0 = torch.zeros((BT,) if per_frame else (), device=dev, dtype=torch.float64) if start_time else None
    CW = (1.0 / 6.0, 2.0 / 6.0, 2.0 / 6.0, 1.0 / 6.0)              # weights of k1..k4 in the RK4 combination
    TC = (0.0, 0.5, 0.5, 1.0)                                      # stage i: time + TC[i] h, input y + TC[i] h k_{i-1}
    if per_frame:
        dot = lambda u, v: (u.double() * v.double()).flatten(1).sum(1)
        head = lambda v: v[:F]                                     # the frames taking part, of a tensor whose first axis is the frame
        F, hyp, acc = 0, None, None
    else:
        dot = lambda u, v: (u.double() * v.double()).sum()
        head = lambda v: v
        F, hyp, acc = BT, [v.detach().requires_grad_(True) for v in hyper], d_hyp

    def flush():                                                   # the prefix's hyper gradients into the rows of that prefix
        if acc is not None:
            for buf, part in zip(d_hyp, acc):
                for full, pre in zip(_layer_views(buf, BT, widths), _layer_views(part, F, widths)):
                    full[:F].add_(pre)
    for s in range(S - 1, -1, -1):
        if per_frame and prefix[s] != F:                           # (grows as s falls: once per distinct count)
            flush()
            F = prefix[s]
            hyp = [torch.cat([u[:F].reshape(-1) for u in _layer_views(v, BT, widths)]).requires_grad_(True) for v in hyper]
            acc = [torch.zeros_like(v) for v in hyp]
        h_F, g_s, dh_s, dt0_s = head(h_all), head(gy), head(dh), head(dt0) if start_time else None
        h = h_F.view(F, 1, 1) if per_frame else h_F
        ks = [[head(tp[s, i]) for i in range(4)] for tp in tapes]
        dh_s += functools.reduce(torch.add, [dot(c, k[0] + 2.0 * k[1] + 2.0 * k[2] + k[3]) for c, k in zip((g_s,) + g_rest, ks)]) / 6.0
        gy_next, g_in = g_s.clone(), None                          # g_in: cotangent of the NEXT stage's input
        for st in (3, 2, 1, 0):
            ka_bar = (CW[st] * h) * g_s
            if g_in is not None:
                ka_bar = torch.addcmul(ka_bar, g_in, TC[st + 1] * h)
            bars = (ka_bar,) + tuple((CW[st] * h) * c for c in g_rest)
            with torch.enable_grad():
                tl = stage_time(s, TC[st], h_F).detach().requires_grad_(True)
                t = torch.cat([tl.unsqueeze(1).expand(F, w).reshape(-1) for w in widths]) if per_frame else tl   # layer-major, as G_lm + t * tg_lm wants it
                y_in = head(ys[s, st]).detach().requires_grad_(True)
                outs = evaluate(t, y_in, hyp, F)
                g = torch.autograd.grad(outs, [y_in, tl] + hyp + [wb[i] for i in wsel], bars)
            del outs
            g_in = g[0]
            for buf, gi in zip(acc, g[2:6]):
                buf.add_(gi)
            for i, gi in zip(wsel, g[6:]):
                d_wb[i].add_(gi)
            if start_time:
                dt0_s += g[1].double()                             # through the start time of t = t0 + (s + TC) h
            dh_s += g[1].double() * (s + TC[st])                   # through the stage time
            if st > 0:
                dh_s += TC[st] * dot(g_in, ks[0][st - 1])          # through the stage input y + TC h k_{st-1}
            gy_next.add_(g_in)
            del g
        if per_frame:
            gy[:F] = gy_next
        else:
            gy = gy_next
    if per_frame:
        flush()
    return gy, d_hyp, d_wb, dh, dt0


class CnfBlockSolve(torch.autograd.Function):
    """A CNF block's whole RK4 solve (forward direction, Hutchinson divergence for a given e) as ONE autograd node whose tape does not
    grow with the layer width: forward = one launch of caspr_cnf_train_fwd_f32, which keeps every layer product on chip and writes only
    the (BT,n,3) point state of each evaluation (stage input, stage outputs); backward = _rk4_reverse_sweep (see there) with
    h = t_end / S, stage times h s + c_i h, the evaluation on the training kernels (_cnf_eval_fused: SplitLayers -> CnfIn -> CnfHidden
    -> CnfOut) with the outputs (a, nd), the log-density's cotangent the same at every step, and dL/dt_end = (dL/dh) / S.
    Discretise-then-optimise, as the taped route: the gradient of the map the forward kernel integrates, up to the rounding between the
    inference-class forward and the training kernels of the recomputation.
    x (BT,n,3), logpx (BT,n,1), G_lm / Bb_lm / tg_lm / tb_lm layer-major as in cnf_block_train, t_end 0-dim tensor, e (BT,n,3),
    w1x / w2x (ops.pack_cnf_x6), steps, widths, then w0, b0, ..., w3, b3 -> (x_T, logp_T)."""

    @staticmethod
    def forward(ctx, x, logpx, G_lm, Bb_lm, tg_lm, tb_lm, t_end, e, w1x, w2x, steps, widths, *wb):
        BT, n, _ = x.shape
        hyper, tcol = _hyper_for_kernel(G_lm, Bb_lm, tg_lm, tb_lm, BT, widths)
        w0, b0, w1, b1, w2, b2, w3, b3 = [t_.detach().contiguous() for t_ in wb]
        ec = e.detach().contiguous()
        y, lp, ys, ka, knd = T.cnf_train_fwd(x.detach().contiguous(), logpx.detach().contiguous(), ec, hyper, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3,
                                             t_end.detach().reshape(1).contiguous(), steps)
        ctx.save_for_backward(ys, ka, knd, G_lm, Bb_lm, tg_lm, tb_lm, t_end, ec)
        ctx.steps, ctx.widths, ctx.wb = steps, widths, wb
        return y, lp

    @staticmethod
    def backward(ctx, gy, glp):
        ys, ka, knd, G_lm, Bb_lm, tg_lm, tb_lm, t_end, e = ctx.saved_tensors
        S, widths, wb = ctx.steps, ctx.widths, ctx.wb
        _, _, BT, n, _ = ys.shape
        gy = torch.zeros(BT, n, 3, device=ys.device, dtype=ys.dtype) if gy is None else gy.contiguous()
        glp = torch.zeros(BT, n, 1, device=ys.device, dtype=ys.dtype) if glp is None else glp.contiguous()   # logp_{s+1} = logp_s + ...: the same cotangent at every step
        h = (t_end.detach() / S).reshape(())
        e_rows = e.reshape(BT * n, 3)
        gy, d_hyp, d_wb, dh, _ = _rk4_reverse_sweep(
            ys, (ka, knd), gy, (glp,), h, lambda s, c, h_: h_ * s + c * h_, False,
            lambda t, y_in, hyp, F: _cnf_eval_fused(wb, t, y_in, hyp[0], hyp[1], hyp[2], hyp[3], e_rows, F, n, widths),
            (G_lm, Bb_lm, tg_lm, tb_lm), wb, widths)
        dt_end = (dh / S).to(t_end.dtype).reshape(t_end.shape)
        return (gy, glp, d_hyp[0], d_hyp[1], d_hyp[2], d_hyp[3], dt_end, None, None, None, None, None) + tuple(d_wb)


class CnfBlockSolveReg(torch.autograd.Function):
    """CnfBlockSolve with the kinetic and Jacobian regularisers (Finlay et al. 2020) as a third output: forward = one launch of
    caspr_cnf_block_reg_fwd_f32, the same kernel's REG instantiation, which also integrates r' = (|a|^2, |J e|^2) from r(0) = 0 and tapes
    every evaluation's integrands kq (S,4,BT,n,2); x_T, logp_T and the tape ys / ka / knd are CnfBlockSolve's bits.  Backward =
    _rk4_reverse_sweep with the third tape kq and r_T's cotangent beside logp_T's (r_{s+1} = r_s + ...: the same at every step, as
    logp's), the evaluation _cnf_eval_fused_reg (CnfOutReg at its end); dL/dt_end = (dL/dh) / S then holds <gr, sum_i w_i q_i> through
    the sweep's dot over the output tapes.  With r_T left out of the loss (autograd hands None for its cotangent: the node does not
    have it materialised) the backward is CnfBlockSolve's, call for call -- CnfOut, two tapes -- and so are the gradients' bits.
    Arguments as CnfBlockSolve's -> (x_T, logp_T, r_T (BT,n,2))."""

    @staticmethod
    def forward(ctx, x, logpx, G_lm, Bb_lm, tg_lm, tb_lm, t_end, e, w1x, w2x, steps, widths, *wb):
        BT, n, _ = x.shape
        hyper, tcol = _hyper_for_kernel(G_lm, Bb_lm, tg_lm, tb_lm, BT, widths)
        w0, b0, w1, b1, w2, b2, w3, b3 = [t_.detach().contiguous() for t_ in wb]
        ec = e.detach().contiguous()
        y, lp, r, ys, ka, knd, kq = T.cnf_block_reg_fwd(x.detach().contiguous(), logpx.detach().contiguous(), ec, hyper, tcol, w0, b0, w1x, b1, w2x, b2,
                                                        w3, b3, t_end.detach().reshape(1).contiguous(), steps)
        ctx.save_for_backward(ys, ka, knd, kq, G_lm, Bb_lm, tg_lm, tb_lm, t_end, ec)
        ctx.steps, ctx.widths, ctx.wb = steps, widths, wb
        ctx.set_materialize_grads(False)               # a None for r_T's cotangent says that r is not in the loss
        return y, lp, r

    @staticmethod
    def backward(ctx, gy, glp, gr):
        ys, ka, knd, kq, G_lm, Bb_lm, tg_lm, tb_lm, t_end, e = ctx.saved_tensors
        S, widths, wb = ctx.steps, ctx.widths, ctx.wb
        _, _, BT, n, _ = ys.shape
        gy = torch.zeros(BT, n, 3, device=ys.device, dtype=ys.dtype) if gy is None else gy.contiguous()
        glp = torch.zeros(BT, n, 1, device=ys.device, dtype=ys.dtype) if glp is None else glp.contiguous()
        h = (t_end.detach() / S).reshape(())
        e_rows = e.reshape(BT * n, 3)
        if gr is None:                                   # CnfBlockSolve.backward's computation
            tapes, g_rest = (ka, knd), (glp,)
            evaluate = lambda t, y_in, hyp, F: _cnf_eval_fused(wb, t, y_in, hyp[0], hyp[1], hyp[2], hyp[3], e_rows, F, n, widths)
        else:
            tapes, g_rest = (ka, knd, kq), (glp, gr.contiguous())
            evaluate = lambda t, y_in, hyp, F: _cnf_eval_fused_reg(wb, t, y_in, hyp[0], hyp[1], hyp[2], hyp[3], e_rows, F, n, widths)
        gy, d_hyp, d_wb, dh, _ = _rk4_reverse_sweep(ys, tapes, gy, g_rest, h, lambda s, c, h_: h_ * s + c * h_, False, evaluate,
                                                    (G_lm, Bb_lm, tg_lm, tb_lm), wb, widths)
        dt_end = (dh / S).to(t_end.dtype).reshape(t_end.shape)
        return (gy, glp, d_hyp[0], d_hyp[1], d_hyp[2], d_hyp[3], dt_end, None, None, None, None, None) + tuple(d_wb)


def cnf_block_train(block, x, context, logpx, e, reg=False):
    """x (BT,n,3), context (BT,zdim), logpx (BT,n,1), e (BT,n,3) fixed Hutchinson noise.  Forward direction
    t: 0 -> sqrt_end_time^2 with `block.rk4_steps` RK4 steps.  -> (x_T, logp_T), differentiable in every parameter.
    reg=True (opt-in; Finlay et al. 2020): the ODE state gains r (BT,n,2), r(0) = 0, r' = (|f|^2, |J e|^2) -- the kinetic energy and
    the Hutchinson estimate of |df/dy|_F^2 along every trajectory, integrated by the same RK4 weights as logp -> (x_T, logp_T, r_T);
    x_T and logp_T are the bits of reg=False.  J e is what the tangent rows carry (forward mode), so the Jacobian term is |J e|^2, not
    RNODE's |e^T J|^2; both have expectation |J|_F^2 for e ~ N(0, I).  On the taped and checkpointed routes, and on the block node with
    config.train_cnf_block_node_reg (opt-in; CnfBlockSolveReg, where CnfBlockSolve would take the shape; the taped reg=True route
    otherwise).  With config.train_cnf_block_node alone reg=True raises: the plain node's forward does not write J e -- whenever that
    switch is on, also for a shape the node would not take (n no multiple of 64, no bf16x6): the answer does not depend on the batch."""
    layers = block.odefunc.diffeq.layers
    BT, n, _ = x.shape
    if reg and BLOCK_NODE and not BLOCK_NODE_REG:
        raise ValueError("cnf_block_train(reg=True) does not run on the block node (config.train_cnf_block_node): its one-launch forward "
                         "does not write J e, which the Jacobian regulariser integrates; turn that switch off (it refuses for every shape, "
                         "also one the node would not take); config.train_cnf_checkpoint is the low-memory route that carries the regularisers.  "
                         "config.train_cnf_block_node_reg, turned on beside it, runs the node that does integrate them (CnfBlockSolveReg)")
    fused = all(_fused_layer_ok(l, n) for l in layers[1:3])
    # BLOCK_NODE (config.train_cnf_block_node; off by default): the whole solve as one node with a tape of (BT,n,3) tensors only
    # (CnfBlockSolve; reg=True under BLOCK_NODE_REG: CnfBlockSolveReg), where the fused-layer kernels and the bf16x6 CNF kernel apply;
    # `_block_node_used` tells tests / tools which route ran
    block._block_node_used = bool(BLOCK_NODE and fused and ops.CNF_BF16X6 and tuple(l._layer.weight.shape[0] for l in layers) == (512, 512, 512, 3))
    if block._block_node_used:
        (G_lm, Bb_lm, tg_lm, tb_lm, widths), t_end, w1x, w2x, wb = _block_node_inputs(block, context, x.device)
        out = (CnfBlockSolveReg if reg else CnfBlockSolve).apply(x, logpx, G_lm, Bb_lm, tg_lm, tb_lm, t_end, e, w1x, w2x, block.rk4_steps, widths, *wb)
        block.odefunc._num_evals.fill_(4 * block.rk4_steps)
        return out
    # hyper networks: the context columns once per solve, the time column per evaluation; layer-major 1-D tensors (_hyper_layer_major)
    G_lm, Bb_lm, tg_lm, tb_lm, widths = _hyper_layer_major(block, context)
    e_rows = e.reshape(BT * n, 3)
    # row layout of the (2R, C) tensors of this solve (include/caspr_hip_train.h): blocks of 32 value rows + the tangent rows of the
    # same points when the hidden layers run with the activation in the conv's epilogue (CnfLayer), [values | tangents] otherwise
    blk = 32 if fused else BT * n

    def func(t, y, _lp):
        R = BT * n
        h = None
        parts = SplitLayers.apply(torch.sigmoid(G_lm + t * tg_lm), Bb_lm + t * tb_lm, BT, widths)   # context part + time column
        for i, l in enumerate(layers):
            gate, bias = parts[i], parts[len(layers) + i]
            if i == 0:                                                    # 3 -> C: fused product + gate + softplus, value | tangent rows
                h = CnfIn.apply(y.reshape(R, 3), e_rows, l._layer.weight, l._layer.bias, gate, bias, n, blk)
                continue
            if i == 1 and fused and not HIDDEN_NODE:
                h = CnfLayer.apply(h, l._layer.weight, l._layer.bias, gate, bias, n)   # product + gate + softplus in one launch
                continue
            if i == 2 and fused and not HIDDEN_NODE:                      # ... and the output product behind the last hidden layer
                z = CnfLayerOut.apply(h, l._layer.weight, l._layer.bias, gate, bias, layers[3]._layer.weight, n)
                continue
            if i == 1 and fused:                                          # both hidden layers + the output product: one node
                l2 = layers[2]
                z = CnfHidden.apply(h, l._layer.weight, l._layer.bias, gate, bias, l2._layer.weight, l2._layer.bias,
                                    parts[2], parts[len(layers) + 2], layers[3]._layer.weight, n)
                continue
            if i == 2 and fused:
                continue
            if not (i == 3 and fused):
                z = linear_rows(h, l._layer.weight, None)
            if i < 3:
                h = CnfAct.apply(z, l._layer.bias, gate, bias, n, blk)    # fused gate + softplus on value / tangent rows
            else:                                                         # 512 -> 3 output layer: (BT,n,3) tensors
                if OUT_NODE and reg:                                      # ... and q = (|a|^2, |zt g|^2)
                    return CnfOutReg.apply(z, l._layer.bias, gate, bias, e_rows, n, blk)
                if OUT_NODE:
                    a, nd = CnfOut.apply(z, l._layer.bias, gate, bias, e_rows, n, blk)    # (zv + b) g + beta,  - sum_j zt_j g_j e_j
                else:                                                     # the same in torch element-wise ops (A/B timing, debugging)
                    cout = l._layer.weight.shape[0]
                    zz = z.view(R // blk, 2, blk, cout)
                    a = (zz[:, 0].reshape(BT, n, cout) + l._layer.bias) * gate.unsqueeze(1) + bias.unsqueeze(1)
                    nd = -((zz[:, 1].reshape(BT, n, cout) * gate.unsqueeze(1)) * e).sum(dim=-1, keepdim=True)
                    if reg:
                        jt = zz[:, 1].reshape(BT, n, cout) * gate.unsqueeze(1)
                        return a, nd, torch.stack([(a * a).sum(dim=-1), (jt * jt).sum(dim=-1)], dim=-1)
        return a, nd

    t_end = block.sqrt_end_time * block.sqrt_end_time if block.train_T else torch.tensor(float(block.T), device=x.device)
    steps = block.rk4_steps
    hstep = t_end / steps
    def rk4_step(t, y, lp, r=None):
        k1 = func(t, y, lp)
        k2 = func(t + 0.5 * hstep, y + 0.5 * hstep * k1[0], lp)
        k3 = func(t + 0.5 * hstep, y + 0.5 * hstep * k2[0], lp)
        k4 = func(t + hstep, y + hstep * k3[0], lp)
        out = (y + (hstep / 6.0) * (k1[0] + 2.0 * k2[0] + 2.0 * k3[0] + k4[0]),
               lp + (hstep / 6.0) * (k1[1] + 2.0 * k2[1] + 2.0 * k3[1] + k4[1]))
        if r is None:
            return out
        return out + (r + (hstep / 6.0) * (k1[2] + 2.0 * k2[2] + 2.0 * k3[2] + k4[2]),)

    # CHECKPOINT_STEPS (config.train_cnf_checkpoint; off by default): keep only the state (y, logp) at the RK4 step boundaries and
    # recompute a step's four evaluations when the backward pass reaches it -- what the reference's adjoint does too (cnf.py:100-110:
    # O(1) memory, the trajectory re-integrated backwards).  The tape of ALL 4 S evaluations is 63 GB at the cfg-3 shard; of one
    # step, 1 / S of that.  Costs one more forward of the block (same kernels, same bits: the step is a pure function of its inputs).
    ckpt = CHECKPOINT_STEPS and torch.is_grad_enabled()
    if ckpt:
        from torch.utils.checkpoint import checkpoint
    state = (x, logpx, torch.zeros(BT, n, 2, device=x.device, dtype=x.dtype)) if reg else (x, logpx)
    for s in range(steps):
        t = hstep * s
        state = checkpoint(rk4_step, t, *state, use_reentrant=False) if ckpt else rk4_step(t, *state)
    block.odefunc._num_evals.fill_(4 * steps)
    return state


def point_cnf_train(flow, x, context, logpx, e=None, reg=False):
    """SequentialFlow in the forward (training / NLL) direction (cnf.py:33-48): [MBN, CNF x k, MBN].
    reg=True -> (x, logpx, r): r (BT,n,2) = the kinetic and Jacobian integrals of cnf_block_train(reg=True) summed over the CNF blocks
    (the Jacobian term as |J e|^2, forward mode -- see there); the MovingBatchNorm layers contribute nothing."""
    from ..models.cnf import CNF
    if e is None:
        e = torch.randn_like(x)                                           # odefunc.py:127-128
    r = None
    for layer in flow.chain:
        if isinstance(layer, CNF):
            layer.odefunc._e = e
            if reg:
                x, logpx, r_b = cnf_block_train(layer, x, context, logpx, e, reg=True)
                r = r_b if r is None else r + r_b
            else:
                x, logpx = cnf_block_train(layer, x, context, logpx, e)
        else:
            x, logpx = layer(x, context, logpx, None, False)
    return (x, logpx, r) if reg else (x, logpx)


# ---------------------------------------------------------------------------------------------
# point CNF block in the SAMPLING direction (cnf.py:70-128 with reverse = True, logpx = None; caspr.py:262 calls it from decode() and
# the reference differentiates it through torchdiffeq): no Hutchinson tangent, no log-density -- value rows only
# ---------------------------------------------------------------------------------------------
class CnfEvalValue(torch.autograd.Function):
    """One evaluation of the ODE function on value rows as ONE node over the value-only kernels (csrc/backward_flow_value.hip) and the
    bf16x6 conv / weight-gradient kernels for the two 512 x 512 products.  y (R, 3), then per layer (w, b, gate, beta) with gate / beta
    (frames, C_l) -> a (R, 3) = dy/dt.  Tape: the two layer products and the three activations, (R, C) each, alive for one evaluation.
    The (R, C) tensors between the layers hold R rounded up to 128 rows, so that the products run on the bf16x6 conv kernels for every
    n (ops.conv1x1 takes the f32 kernel otherwise); the value-only kernels touch rows 0..R-1 only and hand the padding rows back as
    zeros, so they add nothing to a weight gradient (train_ops.py)."""

    @staticmethod
    def forward(ctx, y, w0, b0, g0, be0, w1, b1, g1, be1, w2, b2, g2, be2, w3, b3, g3, be3, n):
        if not y.is_cuda:
            raise ValueError("CnfEvalValue runs on the GPU only (HIP kernels)")
        R = y.shape[0]
        y = y.detach().contiguous()
        b0, g0, be0, b1, g1, be1, b2, g2, be2, b3, g3, be3 = [t_.detach().contiguous() for t_ in (b0, g0, be0, b1, g1, be1, b2, g2, be2, b3, g3, be3)]
        w0c = w0.detach().contiguous()
        Rp = (R + 127) // 128 * 128
        h0 = T.cnf_in_value(y, w0c, b0, g0, be0, n, rows=Rp)
        z1 = ops.conv1x1_train(_packed(w1, False), None, h0.view(1, Rp, -1)).view(Rp, -1)
        h1 = T.cnf_act_value(z1, b1, g1, be1, n)
        z2 = ops.conv1x1_train(_packed(w2, False), None, h1.view(1, Rp, -1)).view(Rp, -1)
        h2 = T.cnf_act_value(z2, b2, g2, be2, n)
        zo = ops.conv1x1_train(_packed(w3, False), None, h2.view(1, Rp, -1)).view(Rp, -1)
        a = T.cnf_out_value(zo, b3, g3, be3, n)
        ctx.save_for_backward(y, w0c, b0, g0, be0, w1, b1, g1, be1, w2, b2, g2, be2, w3, b3, g3, h0, z1, h1, z2, h2, zo)
        ctx.n = n
        return a

    @staticmethod
    def backward(ctx, da):
        y, w0, b0, g0, be0, w1, b1, g1, be1, w2, b2, g2, be2, w3, b3, g3, h0, z1, h1, z2, h2, zo = ctx.saved_tensors
        n, R = ctx.n, y.shape[0]
        c1, c2 = w1.shape[0], w2.shape[0]
        dev = y.device
        rows = lambda t_: t_.view(1, t_.shape[0], t_.shape[1])           # R rounded up to 128 rows; the padding rows of every d* are zero
        dzo, dg3, dbe3 = T.cnf_out_value_bwd(da.contiguous(), zo, b3, g3, n)
        dw3 = torch.empty(w3.shape[0], c2, device=dev, dtype=torch.float32)
        T.conv1x1_wgrad(rows(dzo), rows(h2), c2, w3.shape[0], dw3, None)
        # last hidden layer: dH = dzo W3 formed inside the activation backward
        dz2, dg2, dbe2 = T.cnf_act_value_bwd(z2, b2, g2, be2, n, dzo=dzo, wo=w3.detach().contiguous())
        dw2 = torch.empty(c2, c1, device=dev, dtype=torch.float32)
        T.conv1x1_wgrad(rows(dz2), rows(h1), c1, c2, dw2, None)
        dh1 = ops.conv1x1_train(_packed(w2, True), None, rows(dz2))[0]
        dz1, dg1, dbe1 = T.cnf_act_value_bwd(z1, b1, g1, be1, n, dh=dh1)
        dw1 = torch.empty(c1, w1.shape[1], device=dev, dtype=torch.float32)
        T.conv1x1_wgrad(rows(dz1), rows(h0), w1.shape[1], c1, dw1, None)
        dh0 = ops.conv1x1_train(_packed(w1, True), None, rows(dz1))[0]
        dy, dw0, dg0, dbe0 = T.cnf_in_value_bwd(y, w0, b0, g0, be0, dh0, n)
        db = lambda g, dbe: (g * dbe).sum(dim=0)                           # d/db = sum_r da*g = sum_f g[f]*dbeta[f]
        return (dy, dw0, db(g0, dbe0), dg0, dbe0, dw1, db(g1, dbe1), dg1, dbe1, dw2, db(g2, dbe2), dg2, dbe2, dw3, db(g3, dbe3), dg3, dbe3, None)


def _cnf_eval_value(wb, t, y, G_lm, Bb_lm, tg_lm, tb_lm, BT, n, widths):
    """One evaluation of the ODE function without the Hutchinson term on the value-only kernels: what CnfSampleSolve's reverse sweep
    rebuilds and differentiates.  wb = (w0, b0, ..., w3, b3); y (BT,n,3) -> a (BT,n,3)."""
    w0, b0, w1, b1, w2, b2, w3, b3 = wb
    parts = SplitLayers.apply(torch.sigmoid(G_lm + t * tg_lm), Bb_lm + t * tb_lm, BT, widths)
    a = CnfEvalValue.apply(y.reshape(BT * n, 3), w0, b0, parts[0], parts[4], w1, b1, parts[1], parts[5], w2, b2, parts[2], parts[6],
                           w3, b3, parts[3], parts[7], n)
    return a.view(BT, n, 3)


class CnfSampleSolve(torch.autograd.Function):
    """A CNF block's whole SAMPLING solve (RK4 from t_end down to 0, no divergence) as ONE autograd node with a tape of point-sized
    tensors: forward = one launch of caspr_cnf_sample_tape_f32, which writes the (BT,n,3) stage input and stage output of every
    evaluation (24 bytes per point and evaluation) and no layer product; backward = _rk4_reverse_sweep (see there) on the reversed
    time axis: h = -t_end / S, stage times t_end + (s + c_i) h, the evaluation on the value-only kernels (_cnf_eval_value) with the one
    output a, and dL/dt_end = dL/dt0 - (dL/dh) / S.  With ops.CNF_TAPE_SPLIT = "f16x3" and n >= 128 the forward launch is
    caspr_cnf_sample_tape_h3_f32 (_sample_tape_route; w1x / w2x then come as _SolvePacks): the same tape, the bits of the inference solve.
    y (BT,n,3), G_lm / Bb_lm / tg_lm / tb_lm layer-major (_hyper_layer_major), t_end 0-dim tensor, w1x / w2x (ops.pack_cnf_x6), steps,
    widths, then w0, b0, ..., w3, b3 -> x (BT,n,3)."""

    @staticmethod
    def forward(ctx, y, G_lm, Bb_lm, tg_lm, tb_lm, t_end, w1x, w2x, steps, widths, *wb):
        BT, n, _ = y.shape
        hyper, tcol = _hyper_for_kernel(G_lm, Bb_lm, tg_lm, tb_lm, BT, widths)
        w0, b0, w1, b1, w2, b2, w3, b3 = [t_.detach().contiguous() for t_ in wb]
        h3, w1p, w2p = _sample_tape_route(w1x, w2x, n)
        x, ys, ka = (T.cnf_sample_tape_h3 if h3 else T.cnf_sample_tape)(y.detach().contiguous(), hyper, tcol, w0, b0, w1p, b1, w2p, b2, w3, b3,
                                                                        t_end.detach().reshape(1).contiguous(), steps)
        ctx.save_for_backward(ys, ka, G_lm, Bb_lm, tg_lm, tb_lm, t_end)
        ctx.steps, ctx.widths, ctx.wb = steps, widths, wb
        return x

    @staticmethod
    def backward(ctx, gy):
        ys, ka, G_lm, Bb_lm, tg_lm, tb_lm, t_end = ctx.saved_tensors
        S, widths, wb = ctx.steps, ctx.widths, ctx.wb
        n = ys.shape[3]
        t0 = t_end.detach().reshape(())
        gy, d_hyp, d_wb, dh, dt0 = _rk4_reverse_sweep(
            ys, (ka,), gy.contiguous(), (), -t0 / S, lambda s, c, h: t0 + (s + c) * h, True,      # reversed time axis: t_end -> 0
            lambda t, y_in, hyp, F: (_cnf_eval_value(wb, t, y_in, hyp[0], hyp[1], hyp[2], hyp[3], F, n, widths),),
            (G_lm, Bb_lm, tg_lm, tb_lm), wb, widths)
        dt_end = (dt0 - dh / S).to(t_end.dtype).reshape(t_end.shape)   # h = -t_end / S
        return (gy, d_hyp[0], d_hyp[1], d_hyp[2], d_hyp[3], dt_end, None, None, None, None) + tuple(d_wb)


def _frames_plan(steps, max_steps):
    """What CnfSampleSolveFrames needs of its step table on the host: ONE read of (table, launch order) -> counts per frame, the
    launch order as a list, and the order tensor itself.  An entry outside 1..max_steps is refused with the frame's index: the
    kernel's clamp is for memory safety, not an interface."""
    if not torch.is_tensor(steps) or steps.dim() != 1 or steps.dtype != torch.int32:
        raise ValueError("frame_steps must be a (BT,) int32 tensor of RK4 step counts, got %s" %
                         ("%s %s" % (steps.dtype, tuple(steps.shape)) if torch.is_tensor(steps) else type(steps).__name__))
    order = ops.cnf_steps_order(steps)                                   # longest first, stable
    host = torch.stack([steps, order]).cpu()                             # the one synchronisation of the solve
    counts, perm = host[0].tolist(), host[1].tolist()
    for f, s in enumerate(counts):
        if not 1 <= s <= int(max_steps):
            raise ValueError("frame_steps: frame %d asks for %d RK4 steps, outside 1..%d" % (f, s, int(max_steps)))
    pos = [counts[f] for f in perm]
    if sorted(perm) != list(range(len(counts))) or any(a < b for a, b in zip(pos, pos[1:])):
        raise RuntimeError("frame_steps: the launch order is not the longest-first permutation of the frames")
    return counts, perm, order


class CnfSampleSolveFrames(torch.autograd.Function):
    """CnfSampleSolve with an RK4 step count PER FRAME, each held fixed: the gradient of the map frame f -> RK4 with S_f steps of
    h_f = -t_end / S_f (the count is piecewise constant in the parameters, so this is the gradient wherever it is defined; the EMD
    gradients hold their matching fixed in the same way).  Forward = one launch of caspr_cnf_sample_tape_frames_f32 in the order longest
    first (ops.cnf_steps_order), which writes frame order[p]'s tape at POSITION p, steps s < S_f only; the tape has max_f S_f step rows
    and the rows a frame did not write are never read.  The forward reads the table to the host ONCE (steps.cpu()): this route is a
    Python reverse sweep and was never capturable, so one synchronisation per solve is its price for knowing the loop bounds.
    Backward = _rk4_reverse_sweep (see there) as CnfSampleSolve calls it, in its per-frame form: the cotangent and the hyper rows are
    permuted to launch order once, h_f and t_f = t_end + (s + c_i) h_f are per frame, at step s only the first F_s = #{f : S_f > s}
    positions take part (the value kernels run on F_s n rows, finished frames cost nothing), and dL/dt_end = sum_f (dt0_f - dh_f / S_f).
    dL/dy and the hyper gradients go back to frame order by index assignment over unique indices: no atomics, two runs give the same bits.
    y (BT,n,3), G_lm / Bb_lm / tg_lm / tb_lm layer-major, t_end 0-dim tensor, w1x / w2x, steps (BT,) int32 on y's device, max_steps (the
    largest count a frame may ask for), widths, then w0, b0, ..., w3, b3 -> x (BT,n,3)."""

    @staticmethod
    def forward(ctx, y, G_lm, Bb_lm, tg_lm, tb_lm, t_end, w1x, w2x, steps, max_steps, widths, *wb):
        BT, n, _ = y.shape
        if steps.shape[0] != BT:
            raise ValueError("frame_steps holds %d counts for %d frames" % (steps.shape[0], BT))
        counts, perm, order = _frames_plan(steps, max_steps)
        hyper, tcol = _hyper_for_kernel(G_lm, Bb_lm, tg_lm, tb_lm, BT, widths)
        w0, b0, w1, b1, w2, b2, w3, b3 = [t_.detach().contiguous() for t_ in wb]
        h3, w1p, w2p = _sample_tape_route(w1x, w2x, n)
        x, ys, ka = (T.cnf_sample_tape_h3_frames if h3 else T.cnf_sample_tape_frames)(y.detach().contiguous(), hyper, tcol, w0, b0, w1p, b1, w2p, b2, w3, b3,
                                                                                      t_end.detach().reshape(1).contiguous(), steps, max(counts), order)
        ctx.save_for_backward(ys, ka, G_lm, Bb_lm, tg_lm, tb_lm, t_end, order)
        ctx.counts, ctx.perm, ctx.widths, ctx.wb = counts, perm, widths, wb
        return x

    @staticmethod
    def backward(ctx, gy):
        ys, ka, G_lm, Bb_lm, tg_lm, tb_lm, t_end, order = ctx.saved_tensors
        widths, wb = ctx.widths, ctx.wb
        S_alloc, _, BT, n, _ = ys.shape
        pidx = order.long()                                            # position p of the launch order holds frame pidx[p]
        S_pos = [ctx.counts[f] for f in ctx.perm]                      # non-increasing
        t0 = t_end.detach().reshape(())
        S_t = torch.tensor(S_pos, device=ys.device, dtype=t0.dtype)
        h_all = -t0 / S_t                                              # (BT,) launch order: h_f = -t_end / S_f
        gy = gy.contiguous()[pidx]                                     # launch order from here on
        in_launch_order = lambda v: torch.cat([u[pidx].reshape(-1) for u in _layer_views(v.detach(), BT, widths)])
        gy, d_hyp, d_wb, dh, dt0 = _rk4_reverse_sweep(
            ys, (ka,), gy, (), h_all, lambda s, c, h: t0 + (s + c) * h, True,
            lambda t, y_in, hyp, F: (_cnf_eval_value(wb, t, y_in, hyp[0], hyp[1], hyp[2], hyp[3], F, n, widths),),
            [in_launch_order(v) for v in (G_lm, Bb_lm, tg_lm, tb_lm)], wb, widths,
            prefix=[sum(1 for c in S_pos if c > s) for s in range(S_alloc)])      # the frames still integrating at step s
        dt_end = (dt0 - dh / S_t.double()).sum().to(t_end.dtype).reshape(t_end.shape)      # h_f = -t_end / S_f
        # back to frame order: an index assignment over the permutation (unique indices)
        dy = torch.empty_like(gy)
        dy[pidx] = gy
        outs = []
        for buf in d_hyp:
            o = torch.empty_like(buf)
            for dst, src in zip(_layer_views(o, BT, widths), _layer_views(buf, BT, widths)):
                dst[pidx] = src
            outs.append(o)
        return (dy, outs[0], outs[1], outs[2], outs[3], dt_end, None, None, None, None, None) + tuple(d_wb)


def cnf_block_sample_train(block, y, context, frame_steps=None, max_steps=None):
    """One CNF block in the sampling direction, differentiable in y, the context and every parameter of the block: y (BT,n,3),
    context (BT,zdim) -> x (BT,n,3) at t = 0 after `block.rk4_steps` RK4 steps from sqrt_end_time^2.
    frame_steps: a (BT,) int32 tensor on y's device gives every frame its own step count, 1..max_steps (default: the kernel's limit,
    ops.CNF_MAX_TABLE_STEPS), held fixed under differentiation (CnfSampleSolveFrames); `block.rk4_steps` is not used then."""
    table = frame_steps is not None
    if table:
        max_steps = ops.CNF_MAX_TABLE_STEPS if max_steps is None else int(max_steps)
    widths = tuple(l._layer.weight.shape[0] for l in block.odefunc.diffeq.layers)
    own_table = not table and block.frame_steps is not None          # the uniform route refuses a block that carries a table of its own
    if widths != (512, 512, 512, 3) or block.method != "rk4" or own_table:
        raise ValueError("the differentiable sampling solve is built for the 3-512-512-512-3 ODE function on %sRK4 steps (got widths %s, method %r%s)"
                         % ("" if table else "uniform ", widths, block.method, ", per-frame step counts" if own_table else ""))
    if table:
        ops._chk_frame_table("frame_steps", frame_steps, y.shape[0], y.device)
    (G_lm, Bb_lm, tg_lm, tb_lm, widths), t_end, w1x, w2x, wb = _block_node_inputs(block, context, y.device, tape_h3=True)
    if table:
        x = CnfSampleSolveFrames.apply(y, G_lm, Bb_lm, tg_lm, tb_lm, t_end, w1x, w2x, frame_steps, max_steps, widths, *wb)
        block.odefunc._num_evals.copy_(4 * frame_steps.max())      # 4 max_f S_f, on the device: no host read
    else:
        x = CnfSampleSolve.apply(y, G_lm, Bb_lm, tg_lm, tb_lm, t_end, w1x, w2x, block.rk4_steps, widths, *wb)
        block.odefunc._num_evals.fill_(4 * block.rk4_steps)
    return x


def point_cnf_sample_train(flow, y, context, frame_steps=None, max_steps=None):
    """SequentialFlow in the reverse (sampling) direction (cnf.py:33-48 with reverse = True, logpx = None), differentiable: the chain
    walked backwards, MovingBatchNorm1d(reverse=True) in torch, every CNF block through CnfSampleSolve.  y (BT,n,3), context (BT,zdim)
    -> x (BT,n,3).  No fallback: what the route needs is stated in the error.
    frame_steps (BT,) int32 on y's device: every CNF block of the chain takes this table of step counts (CnfSampleSolveFrames), as the
    inference route shares one table; max_steps: the largest count an entry may hold (see cnf_block_sample_train)."""
    from ..models.cnf import CNF
    if not (torch.is_tensor(y) and torch.is_tensor(context) and y.is_cuda and context.is_cuda):
        raise ValueError("point_cnf_sample_train runs on the GPU only (HIP kernels): y and context must be GPU tensors")
    if not ops.CNF_BF16X6:
        raise ValueError("point_cnf_sample_train needs the bf16x6 CNF kernels (ops.CNF_BF16X6 is off)")
    if not torch.is_grad_enabled():
        raise ValueError("point_cnf_sample_train records a gradient: it was called with grad mode off (torch.no_grad())")
    x = y.reshape(-1, y.shape[-2], y.shape[-1]).float()
    for layer in reversed(flow.chain):
        if isinstance(layer, CNF):
            x = cnf_block_sample_train(layer, x, context, frame_steps, max_steps)
        else:
            x = layer(x, context, None, None, True)
    return x
