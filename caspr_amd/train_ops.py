"""Host wrappers of the training-tier entries of libcaspr_hip.so (include/caspr_hip_train.h).

These are the gradient kernels torch.autograd supplies in the reference (train_utils.py:173).  Same rules as
ops.py: float32 GPU tensors, point-major rows, no CPU fallback.
"""
import torch

from . import lib as _lib
from . import ops
from .ops import _chk_f32, _chk_i32, _chk_rows, _p, _stream, _workspace


def gn_stats_train(y, C, gamma, beta, groups=16, eps=1e-5, want_max=False):
    """As ops.gn_stats, and also the moments: -> scale (B,C), shift (B,C), mean (B,G), rstd (B,G) [, pmax (B,C)]."""
    _chk_f32(gamma, beta)
    ldy = _chk_rows(y)
    B, P, _ = y.shape
    dev = y.device
    scale = torch.empty(B, C, device=dev, dtype=torch.float32)
    shift = torch.empty(B, C, device=dev, dtype=torch.float32)
    mean = torch.empty(B, groups, device=dev, dtype=torch.float32)
    rstd = torch.empty(B, groups, device=dev, dtype=torch.float32)
    pmax = torch.empty(B, C, device=dev, dtype=torch.float32) if want_max else None
    L = _lib.load()
    ws = _workspace(L.caspr_gn_ws_bytes(B, P, C, groups), dev)
    _lib.check(L.caspr_gn_stats_train_f32(_p(y), ldy, B, P, C, groups, _p(gamma), _p(beta), float(eps), _p(scale), _p(shift), _p(pmax),
                                          _p(mean), _p(rstd), _p(ws), ws.numel(), _stream()), "caspr_gn_stats_train_f32")
    return (scale, shift, mean, rstd, pmax) if want_max else (scale, shift, mean, rstd)


def conv1x1_wgrad(dy, x, cin, cout, dw, dbias=None, in_scale=None, in_shift=None, in_relu=False, in_relu_from=0, accumulate=False):
    """dw (cout,cin) (+)= dy^T . in(x), dbias (cout) (+)= column sums of dy.  dy (B,P,>=cout), x (B,P,>=cin)."""
    _chk_f32(dw, dbias, in_scale, in_shift)
    lddy, ldx = _chk_rows(dy), _chk_rows(x)
    B, P, _ = x.shape
    if dy.shape[0] != B or dy.shape[1] != P:
        raise ValueError("conv1x1_wgrad: dy and x disagree on (B,P)")
    if tuple(dw.shape) != (cout, cin) or (dbias is not None and dbias.numel() != cout):
        raise ValueError("conv1x1_wgrad: dw must be (%d,%d)" % (cout, cin))
    L = _lib.load()
    ws = _workspace(L.caspr_wgrad_ws_bytes(B * P, cin, cout), x.device)
    # matrix products as ops.set_matmul_mode says: the exact bf16 three-way split where the tile is reasonably filled, f32 MFMA otherwise
    x6 = ops.CONV_BF16X6 and cin >= 32 and cout >= 32
    fn, name = (L.caspr_conv1x1_wgrad_bf16x6_f32, "caspr_conv1x1_wgrad_bf16x6_f32") if x6 else (L.caspr_conv1x1_wgrad_f32, "caspr_conv1x1_wgrad_f32")
    with ops.timed("k:%s:%d:%d:%d" % ("wgrad_bf16x6" if x6 else "wgrad_f32", cin, cout, B * P), 2):
        _lib.check(fn(_p(dy), lddy, _p(x), ldx, _p(in_scale), _p(in_shift), int(in_relu), int(in_relu_from), B, P, cin, cout,
                      _p(dw), _p(dbias), int(accumulate), _p(ws), ws.numel(), _stream()), name)
    return dw


def gn_bwd(y, da, C, mean, rstd, gamma, beta, dgamma, dbeta, groups=16, relu=True, accumulate=False, dmax=None, amax=None, out=None):
    """GroupNorm(+ReLU) backward.  da (B,P,>=C) or None (zero); dmax/amax (B,C) = gradient / arg-max point of the max over
    points of the un-rectified normalised feature.  Result in `out` (default: in place over da)."""
    _chk_f32(mean, rstd, gamma, beta, dgamma, dbeta, dmax)
    ldy = _chk_rows(y)
    B, P, _ = y.shape
    if out is None:
        if da is None:
            raise ValueError("gn_bwd: give `out` when da is None")
        out = da
    ldd, ldo = _chk_rows(da), _chk_rows(out)
    if amax is not None:
        _chk_i32(amax)
    L = _lib.load()
    ws = _workspace(L.caspr_gn_bwd_ws_bytes(B, P, C, groups), y.device)
    _lib.check(L.caspr_gn_bwd_f32(_p(y), ldy, _p(da), ldd, _p(dmax), _p(amax), _p(out), ldo, B, P, C, groups, _p(mean), _p(rstd), _p(gamma),
                                  _p(beta), int(relu), _p(dgamma), _p(dbeta), int(accumulate), _p(ws), ws.numel(), _stream()), "caspr_gn_bwd_f32")
    return out


def argmax_points(y, C, scale, shift):
    """(B,C) int32: first point attaining max_p (y*scale+shift)."""
    _chk_f32(scale, shift)
    ldy = _chk_rows(y)
    B, P, _ = y.shape
    out = torch.empty(B, C, device=y.device, dtype=torch.int32)
    L = _lib.load()
    ws = _workspace(L.caspr_argmax_ws_bytes(B, P, C), y.device)
    _lib.check(L.caspr_argmax_points_f32(_p(y), ldy, B, P, C, _p(scale), _p(shift), _p(out), _p(ws), ws.numel(), _stream()), "caspr_argmax_points_f32")
    return out


def colsum_batched(a, C):
    """(B,P,>=C) -> (B,C) sums over points."""
    ld = _chk_rows(a)
    B, P, _ = a.shape
    out = torch.empty(B, C, device=a.device, dtype=torch.float32)
    L = _lib.load()
    ws = _workspace(L.caspr_colsum_ws_bytes(B, P, C), a.device)
    _lib.check(L.caspr_colsum_batched_f32(_p(a), ld, B, P, C, _p(out), _p(ws), ws.numel(), _stream()), "caspr_colsum_batched_f32")
    return out


def three_interp_bwd(dout, idx, weight, C, dfeat):
    """dfeat (B,m,>=C) += scatter of dout (B,n,>=C) through the three-NN indices / weights."""
    _chk_f32(weight)
    _chk_i32(idx)
    ldo, ldf = _chk_rows(dout), _chk_rows(dfeat)
    B, n, _ = dout.shape
    m = dfeat.shape[1]
    _lib.check(_lib.load().caspr_three_interp_bwd_f32(_p(dout), ldo, _p(idx), _p(weight), B, m, n, C, _p(dfeat), ldf, _stream()),
               "caspr_three_interp_bwd_f32")
    return dfeat


def group_rows(xyz, new_xyz, feat, C, idx, centred=False, feat_kind=0, align=4):
    """-> G (B, M*ns, roundup(3+C, align)) rows [dxyz | feat | 0]; centred: minus the neighbourhood's sample-0 row
    (include/caspr_hip_train.h), feat_kind as ops.sa_mlp_max."""
    _chk_f32(xyz, new_xyz)
    _chk_i32(idx)
    B, n, _ = xyz.shape
    M, ns = idx.shape[1], idx.shape[2]
    ldf = 0 if feat is None else _chk_rows(feat)
    ldg = (3 + C + align - 1) // align * align
    G = torch.empty(B, M * ns, ldg, device=xyz.device, dtype=torch.float32)
    _lib.check(_lib.load().caspr_group_rows_f32(_p(xyz), _p(new_xyz), _p(feat), ldf, _p(idx), B, n, M, C, ns, int(bool(centred)), int(feat_kind),
                                                _p(G), ldg, _stream()),
               "caspr_group_rows_f32")
    return G


def group_rows_bwd(dG, idx, C, dfeat):
    """dfeat (B,n,>=C) += scatter of the feature columns of dG (B, M*ns, >=3+C)."""
    _chk_i32(idx)
    ldg, ldf = _chk_rows(dG), _chk_rows(dfeat)
    B, n, _ = dfeat.shape
    M, ns = idx.shape[1], idx.shape[2]
    _lib.check(_lib.load().caspr_group_rows_bwd_f32(_p(dG), ldg, _p(idx), B, n, M, C, ns, _p(dfeat), ldf, _stream()), "caspr_group_rows_bwd_f32")
    return dfeat


def gn_rows(y, ns, C, gamma, beta, relu, eps=1e-5, maxout=None):
    """Per-neighbourhood GroupNorm(16): y (B, M*ns, >=C).  -> (A (same shape, C cols) | None, mean, rstd, arg | None).
    maxout: (B, M, >=C) column slice receiving max over the ns rows (last layer of the point MLP)."""
    _chk_f32(gamma, beta)
    ldy = _chk_rows(y)
    NB = y.shape[0] * y.shape[1] // ns
    dev = y.device
    mean = torch.empty(NB, 16, device=dev, dtype=torch.float32)
    rstd = torch.empty(NB, 16, device=dev, dtype=torch.float32)
    A, arg, lda, ldm = None, None, 0, 0
    if maxout is None:
        A = torch.empty(y.shape[0], y.shape[1], C, device=dev, dtype=torch.float32)
        lda = C
    else:
        ldm = _chk_rows(maxout)
        arg = torch.empty(NB, C, device=dev, dtype=torch.int32)
    _lib.check(_lib.load().caspr_gn_rows_f32(_p(y), ldy, NB, ns, C, _p(gamma), _p(beta), float(eps), int(relu), _p(A), lda, _p(mean), _p(rstd),
                                             _p(maxout), ldm, _p(arg), _stream()), "caspr_gn_rows_f32")
    return A, mean, rstd, arg


def gn_rows_bwd(y, ns, C, gamma, beta, relu, mean, rstd, dgamma, dbeta, da=None, dmax=None, arg=None, out=None, accumulate=False):
    """Backward of gn_rows: da (dense) or dmax (B,M,>=C slice) + arg.  -> dY (same shape as y rows, C cols)."""
    _chk_f32(gamma, beta, mean, rstd, dgamma, dbeta)
    ldy = _chk_rows(y)
    NB = y.shape[0] * y.shape[1] // ns
    if out is None:
        out = da if da is not None else torch.empty(y.shape[0], y.shape[1], C, device=y.device, dtype=torch.float32)
    lda, ldm, ldo = _chk_rows(da), _chk_rows(dmax), _chk_rows(out)
    L = _lib.load()
    ws = _workspace(L.caspr_gn_rows_bwd_ws_bytes(C), y.device)
    _lib.check(L.caspr_gn_rows_bwd_f32(_p(y), ldy, NB, ns, C, _p(gamma), _p(beta), int(relu), _p(mean), _p(rstd), _p(da), lda, _p(dmax), ldm,
                                       _p(arg), _p(out), ldo, _p(dgamma), _p(dbeta), int(accumulate), _p(ws), ws.numel(), _stream()),
               "caspr_gn_rows_bwd_f32")
    return out


def latent_dopri5_tape(z0, times, rtol, atol, wts, max_attempts=1000, max_steps=64):
    """ops.latent_dopri5 with the step tape its reverse sweep needs (caspr_latent_dopri5_tape_f32, csrc/ode_latent_dp5.hip: the same
    kernel text; latent_ode_model.py:45-70): same arguments, and out, trace and counters are that call's bits.
    -> out (B,Tu,D), info (the dict of ops.latent_dopri5(return_trace=True)), tape = {"counters" (B,4) int32, "z" (B,max_steps,D) the start
    state of every accepted step, "dt" (B,max_steps) its size, "times", "max_steps"}.  Never synchronises.  A sequence that would accept
    more than max_steps steps stops like one that used up max_attempts (finished = 0, NaN in the rows it did not reach); the deferred
    CasprHipError names both budgets."""
    B, D, H, rtol, atol, max_attempts = ops._latent_dp5_args("latent_dopri5_tape", z0, times, rtol, atol, wts, max_attempts)
    max_steps = int(max_steps)
    if max_steps < 1:
        raise ValueError("latent_dopri5_tape: max_steps must be positive, got %d" % max_steps)
    Tu, dev = times.shape[0], z0.device
    HEAD, ROW = ops.LATENT_DP5_TRACE_HEAD, ops.LATENT_DP5_TRACE_ROW
    out = torch.empty(B, Tu, D, device=dev, dtype=torch.float32)
    trace = torch.empty(B, HEAD + ROW * max_attempts, device=dev, dtype=torch.float32)
    counters = torch.empty(B, 4, device=dev, dtype=torch.int32)
    tz = torch.zeros(B, max_steps, D, device=dev, dtype=torch.float32)
    tdt = torch.zeros(B, max_steps, device=dev, dtype=torch.float32)
    ptrs = [_p(w.data) if isinstance(w, ops.PackedWeight) else _p(w) for w in wts]
    with ops._latent_dp5.on(dev) as status:
        with ops.timed("latent_dopri5_tape"):
            _lib.check(_lib.load().caspr_latent_dopri5_tape_f32(_p(z0), z0.stride(0), _p(times), B, Tu, D, H, rtol, atol, max_attempts, max_steps, *ptrs,
                                                                _p(out), _p(trace), _p(counters), _p(tz), _p(tdt), _stream()), "caspr_latent_dopri5_tape_f32")
        status.post(counters[:, 3], (max_attempts, max_steps))
    info = {"d0": trace[:, 0], "d1": trace[:, 1], "d2": trace[:, 2], "h0": trace[:, 3], "dt0": trace[:, 4],
            "attempts": trace[:, HEAD:].view(B, max_attempts, ROW), "accepted": counters[:, 0], "rejected": counters[:, 1], "nfe": counters[:, 2]}
    return out, info, {"counters": counters, "z": tz, "dt": tdt, "times": times, "max_steps": max_steps}


def latent_dopri5_adjoint(gout, tape, wts, wts_t):
    """The reverse sweep of latent_dopri5_tape in one launch (caspr_latent_dopri5_adjoint_f32, csrc/ode_latent_dp5_adjoint.inc): the
    gradient of the solve's own discrete map, accepted steps held fixed.  gout (B,Tu,D) = dL/d(out); tape: that call's; wts: the solve's
    [PackedWeight0, b0, .., PackedWeight3, b3]; wts_t: PackedWeights of the TRANSPOSED W3, W2, W1, W0 (in that order).
    -> gz (B,D) = dL/dz0 (NaN rows for unfinished sequences), inputs = [x (R,xw), h1, h2, h3 (R,H)], deltas = [d0, d1, d2 (R,H), d3 (R,xw)]:
    R = B (1 + 6 max_steps) rows, zero where a sequence made no evaluation; dW_l = deltas[l]^T inputs[l], db_l = colsum(deltas[l]).
    Memory: R x (3 H + 2 roundup4(D)) floats x 2 (inputs and deltas): about 39 MB at B = 8 and 315 MB at B = 64 with max_steps = 64,
    H = 512.  Never synchronises and reads no count on the host."""
    _chk_f32(gout, *[w for w in wts[1::2]])
    counters, tz, tdt, times, max_steps = tape["counters"], tape["z"], tape["dt"], tape["times"], tape["max_steps"]
    _chk_f32(tz, tdt, times)
    _chk_i32(counters)
    B, Tu, D = gout.shape
    H = wts[0].cout
    if wts[0].cin != D or tuple(tz.shape) != (B, max_steps, D) or tuple(tdt.shape) != (B, max_steps) or tuple(counters.shape) != (B, 4) or times.shape[0] != Tu:
        raise ValueError("latent_dopri5_adjoint: gout (B,Tu,D) = %s does not match the tape (z %s, dt %s, counters %s, %d stamps) or the dynamics net (%d inputs)"
                         % (tuple(gout.shape), tuple(tz.shape), tuple(tdt.shape), tuple(counters.shape), times.shape[0], wts[0].cin))
    shapes = [(w.cout, w.cin) for w in wts_t]
    if shapes != [(H, D), (H, H), (H, H), (D, H)]:
        raise ValueError("latent_dopri5_adjoint: wts_t must pack W3^T (H,D), W2^T, W1^T (H,H), W0^T (D,H), got %s" % (shapes,))
    if not gout.is_contiguous():
        raise ValueError("latent_dopri5_adjoint: gout must be contiguous")
    dev = gout.device
    R, xw = B * (1 + 6 * max_steps), (D + 3) // 4 * 4
    inputs = [torch.zeros(R, xw, device=dev, dtype=torch.float32)] + [torch.zeros(R, H, device=dev, dtype=torch.float32) for _ in range(3)]
    deltas = [torch.zeros(R, H, device=dev, dtype=torch.float32) for _ in range(3)] + [torch.zeros(R, xw, device=dev, dtype=torch.float32)]
    gz = torch.empty(B, D, device=dev, dtype=torch.float32)
    ptrs = [_p(w.data) if isinstance(w, ops.PackedWeight) else _p(w) for w in wts]
    # the launch reports nothing of its own: an unfinished sequence was posted by the taping launch (the _latent_dp5 channel) and is raised
    # by the next solve on the stream or by ops.check_deferred_errors(), not from inside a backward pass
    with ops.timed("latent_dopri5_adjoint"):
        _lib.check(_lib.load().caspr_latent_dopri5_adjoint_f32(_p(gout), _p(times), B, Tu, D, H, max_steps, _p(counters), _p(tz), _p(tdt), *ptrs,
                                                               *[_p(w.data) for w in wts_t], _p(inputs[0]), xw, _p(inputs[1]), _p(inputs[2]),
                                                               _p(inputs[3]), _p(deltas[0]), _p(deltas[1]), _p(deltas[2]), _p(deltas[3]), _p(gz),
                                                               _stream()), "caspr_latent_dopri5_adjoint_f32")
    return gz, inputs, deltas


def cnf_train_fwd(y, logp, e, hyper, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, t_end, steps):
    """Training forward of one CNF block in one launch (caspr_cnf_train_fwd_f32): y, e (BT,n,3), logp (BT,n,1), hyper (BT, >= 3078) and
    tcol as ops.cnf_rk4 takes them, w1x / w2x = ops.pack_cnf_x6, t_end a one-element DEVICE tensor.
    -> y_T (BT,n,3), logp_T (BT,n,1), stage inputs ys (steps,4,BT,n,3), stage outputs ka (steps,4,BT,n,3), knd (steps,4,BT,n,1)."""
    _chk_f32(y, logp, e, hyper, tcol, w0, b0, b1, b2, w3, b3, t_end)
    BT, n = ops._chk_cnf("cnf_train_fwd", y, hyper, e, logp, train=(tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, t_end), steps=steps)
    dev = y.device
    out = torch.empty(BT, n, 3, device=dev, dtype=torch.float32)
    lp_out = torch.empty(BT, n, 1, device=dev, dtype=torch.float32)
    ys = torch.empty(steps, 4, BT, n, 3, device=dev, dtype=torch.float32)
    ka = torch.empty(steps, 4, BT, n, 3, device=dev, dtype=torch.float32)
    knd = torch.empty(steps, 4, BT, n, 1, device=dev, dtype=torch.float32)
    ops._cnf_launch("x6", "train_fwd", "cnf_train_fwd", dev, ops._cnf_head(y, hyper, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3),
                    (_p(t_end), int(steps)), (_p(e), _p(logp), _p(lp_out), _p(out), _p(ys), _p(ka), _p(knd), BT, n))
    return out, lp_out, ys, ka, knd


def cnf_block_reg_fwd(y, logp, e, hyper, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, t_end, steps):
    """cnf_train_fwd with the kinetic / Jacobian regularisers integrated beside the log-density (caspr_cnf_block_reg_fwd_f32, the same
    kernel's REG instantiation): same arguments -> y_T (BT,n,3), logp_T (BT,n,1), r_T (BT,n,2) = the integrals of (|dy/dt|^2, |J e|^2),
    ys, ka, knd as there -- those five the bits of cnf_train_fwd -- and every evaluation's integrands kq (steps,4,BT,n,2)."""
    _chk_f32(y, logp, e, hyper, tcol, w0, b0, b1, b2, w3, b3, t_end)
    BT, n = ops._chk_cnf("cnf_block_reg_fwd", y, hyper, e, logp, train=(tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, t_end), steps=steps)
    dev = y.device
    out = torch.empty(BT, n, 3, device=dev, dtype=torch.float32)
    lp_out = torch.empty(BT, n, 1, device=dev, dtype=torch.float32)
    r_out = torch.empty(BT, n, 2, device=dev, dtype=torch.float32)
    ys = torch.empty(steps, 4, BT, n, 3, device=dev, dtype=torch.float32)
    ka = torch.empty(steps, 4, BT, n, 3, device=dev, dtype=torch.float32)
    knd = torch.empty(steps, 4, BT, n, 1, device=dev, dtype=torch.float32)
    kq = torch.empty(steps, 4, BT, n, 2, device=dev, dtype=torch.float32)
    ops._cnf_launch("x6", "train_fwd_reg", "cnf_block_reg_fwd", dev, ops._cnf_head(y, hyper, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3),
                    (_p(t_end), int(steps)), (_p(e), _p(logp), _p(lp_out), _p(out), _p(r_out), _p(ys), _p(ka), _p(knd), _p(kq), BT, n))
    return out, lp_out, r_out, ys, ka, knd, kq


def _cnf_sample_tape(who, route, y, hyper, tcol, w0, b0, w1, b1, w2, b2, w3, b3, t_end, steps, table=None):
    """The four sampling solves with a tape: `route` "x6" | "h3" with its packs w1 / w2; steps an int, or with table = (max_steps, order,
    ys, ka) a step count per frame -> x_0, ys, ka."""
    _chk_f32(y, hyper, tcol, w0, b0, b1, b2, w3, b3, t_end, *(table or ())[2:])
    BT, n = ops._chk_cnf(who, y, hyper, train=(tcol, w0, b0, w1, b1, w2, b2, w3, b3, t_end), route=route,
                         steps=steps if table is None and route == "x6" else None)
    dev = y.device
    if table is not None:
        max_steps, ys, ka = ops._cnf_step_table(who, y, steps, table[1], table[0], table[2:])
        step_args = (_p(steps), max_steps, _p(table[1]))
    else:
        if steps <= 0:                                   # (the bf16x6 wrapper has said so with t_end's message)
            raise ValueError("%s: steps must be positive" % who)
        ys = torch.empty(steps, 4, BT, n, 3, device=dev, dtype=torch.float32)
        ka = torch.empty(steps, 4, BT, n, 3, device=dev, dtype=torch.float32)
        step_args = (int(steps),)
    out = torch.empty(BT, n, 3, device=dev, dtype=torch.float32)
    ops._cnf_launch(route, "tape" if table is None else "tape_frames", "cnf_sample_tape", dev,
                    ops._cnf_head(y, hyper, tcol, w0, b0, w1, b1, w2, b2, w3, b3), (_p(t_end), *step_args), (_p(out), _p(ys), _p(ka), BT, n))
    return out, ys, ka


def cnf_sample_tape(y, hyper, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, t_end, steps):
    """Sampling solve of one CNF block with its tape in one launch (caspr_cnf_sample_tape_f32): RK4 from t_end down to 0, no divergence.
    y (BT,n,3), hyper (BT, >= 3078) and tcol as ops.cnf_rk4 takes them, w1x / w2x = ops.pack_cnf_x6, t_end a one-element DEVICE tensor.
    -> x_0 (BT,n,3), stage inputs ys (steps,4,BT,n,3), stage outputs ka (steps,4,BT,n,3)."""
    return _cnf_sample_tape("cnf_sample_tape", "x6", y, hyper, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, t_end, steps)


def cnf_sample_tape_frames(y, hyper, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, t_end, steps, max_steps, order=None, ys=None, ka=None):
    """cnf_sample_tape with an RK4 step count per frame (caspr_cnf_sample_tape_frames_f32; the same kernel).  steps (BT,) int32 GPU
    tensor: frame f takes S_f = min(max(steps[f], 0), max_steps) steps of h_f = -t_end / S_f (0 skips the frame: its rows of x_0 stay
    as allocated); order (BT,) int32 GPU tensor or None: the launch order (ops.cnf_steps_order).  The tape is written in LAUNCH order:
    position p of the frame axis holds frame order[p] (p itself without an order), rows s < S_f only -- the rest of ys / ka is left
    as it was.  ys / ka (max_steps,4,BT,n,3) may be handed in (a test poisons them); allocated with torch.empty otherwise.
    -> x_0 (BT,n,3), ys, ka."""
    return _cnf_sample_tape("cnf_sample_tape_frames", "x6", y, hyper, tcol, w0, b0, w1x, b1, w2x, b2, w3, b3, t_end, steps,
                            (max_steps, order, ys, ka))


def cnf_sample_tape_h3(y, hyper, tcol, w0, b0, w1h, b1, w2h, b2, w3, b3, t_end, steps):
    """cnf_sample_tape on the 128-point f16x3 evaluation of inference (caspr_cnf_sample_tape_h3_f32; ops.CNF_TAPE_SPLIT = "f16x3"): same
    arguments with w1h / w2h = ops.pack_cnf_h3 in place of the bf16x6 packs, n >= 128.  x_0 is bit for bit what
    ops.cnf_rk4(..., w1h=, w2h=, reverse=True) returns for the same inputs, the same float32 t_end and the same steps.  The range guard
    (a point with a hidden activation of 4095 or more gets NaN in x_0) reports through ops.check_deferred_errors, as ops.cnf_rk4's.
    -> x_0 (BT,n,3), stage inputs ys (steps,4,BT,n,3), stage outputs ka (steps,4,BT,n,3)."""
    return _cnf_sample_tape("cnf_sample_tape_h3", "h3", y, hyper, tcol, w0, b0, w1h, b1, w2h, b2, w3, b3, t_end, steps)


def cnf_sample_tape_h3_frames(y, hyper, tcol, w0, b0, w1h, b1, w2h, b2, w3, b3, t_end, steps, max_steps, order=None, ys=None, ka=None):
    """cnf_sample_tape_frames on the 128-point f16x3 evaluation (caspr_cnf_sample_tape_h3_frames_f32; the kernel of cnf_sample_tape_h3):
    same arguments with w1h / w2h = ops.pack_cnf_h3, n >= 128; the tape in LAUNCH order, rows s < S_f only, ys / ka may be handed in.
    Frame f's x_0 is bit for bit what cnf_sample_tape_h3 gives on that frame alone with S_f steps.  -> x_0 (BT,n,3), ys, ka."""
    return _cnf_sample_tape("cnf_sample_tape_h3_frames", "h3", y, hyper, tcol, w0, b0, w1h, b1, w2h, b2, w3, b3, t_end, steps,
                            (max_steps, order, ys, ka))


# ---- the gated softplus layers on value rows only (csrc/backward_flow_value.hip): R = frames * n rows, point p in row p.
# gate / beta (frames, C) contiguous; the backward wrappers return dgate / dbeta (frames, C) with the point splits already summed.
# The (rows, C) tensors may hold MORE than R rows: the caller rounds the row count up (to the 128 rows the bf16x6 conv kernels want of
# the products between these layers).  The kernels read and write rows 0..R-1 only; every wrapper that returns such a tensor hands its
# padding rows back as zeros, so that they add nothing to a weight gradient taken over all rows.
def _chk_value(name, gate, n, *rows):
    _chk_f32(gate)
    R = gate.shape[0] * n
    for t in rows:
        if t is None:
            continue
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) % 4 != 0 or t.data_ptr() % 16 != 0:
            raise ValueError("%s: (rows, C) float32 GPU tensors with unit column stride, a row stride that is a multiple of 4 and 16-byte alignment are required" % name)
        if t.shape[0] < R:
            raise ValueError("%s: %d rows for %d frames of n = %d points" % (name, t.shape[0], gate.shape[0], n))
    if n <= 0 or R <= 0:
        raise ValueError("%s: no points (frames %d, n %d)" % (name, gate.shape[0], n))
    return R


def _rows_out(rows, R, C, device):
    t = torch.empty(rows, C, device=device, dtype=torch.float32)
    if rows > R:
        t[R:].zero_()
    return t


def _sum_splits(part, ns):
    return part[:, 0] if ns == 1 else part.sum(dim=1)


def cnf_in_value(y, w0, b, gate, beta, n, rows=None):
    """H = softplus((W0 y + b) gate[f] + beta[f]); y (R, 3), w0 (C, 3), gate / beta (R / n, C) -> (rows >= R, C), rows past R zero."""
    _chk_f32(y, w0, b, gate, beta)
    R, C = y.shape[0], w0.shape[0]
    rows = R if rows is None else int(rows)
    if tuple(y.shape) != (R, 3) or tuple(w0.shape) != (C, 3) or C % 4 != 0 or R % n != 0 or tuple(gate.shape) != (R // n, C) or tuple(beta.shape) != (R // n, C) or rows < R:
        raise ValueError("cnf_in_value: y (R,3), w0 (C,3) with C % 4 == 0, gate / beta (R/n, C) and rows >= R are required")
    h = _rows_out(rows, R, C, y.device)
    with ops.timed("k:cnf_in_value", 2):
        _lib.check(_lib.load().caspr_cnf_in_value_f32(_p(y), _p(w0), _p(b), _p(gate), _p(beta), R, n, C, _p(h), C, _stream()), "caspr_cnf_in_value_f32")
    return h


def cnf_in_value_bwd(y, w0, b, gate, beta, dh, n):
    """dh (>= R, C) -> dy (R, 3), dW0 (C, 3), dgate (frames, C), dbeta (frames, C)."""
    R = _chk_value("cnf_in_value_bwd", gate, n, dh)
    _chk_f32(y, w0, b, beta)
    C = w0.shape[0]
    if tuple(y.shape) != (R, 3) or tuple(w0.shape) != (C, 3) or tuple(gate.shape) != (R // n, C) or dh.shape[1] < C:
        raise ValueError("cnf_in_value_bwd: y (R,3), w0 (C,3), gate / beta (R/n, C), dh (>= R, >= C) are required")
    L = _lib.load()
    ns, frames, chunks = L.caspr_cnf_value_splits(n), R // n, (C + 255) // 256
    dev = y.device
    dgate = torch.empty(frames, ns, C, device=dev, dtype=torch.float32)
    dbeta = torch.empty(frames, ns, C, device=dev, dtype=torch.float32)
    dw_part = torch.empty(frames * ns, C, 3, device=dev, dtype=torch.float32)
    dy_part = torch.empty(chunks, R, 3, device=dev, dtype=torch.float32)
    with ops.timed("k:cnf_in_value_bwd", 2):
        _lib.check(L.caspr_cnf_in_value_bwd_f32(_p(y), _p(w0), _p(b), _p(gate), _p(beta), _p(dh), dh.stride(0), R, n, C, _p(dgate), _p(dbeta), _p(dw_part),
                                                _p(dy_part), _stream()), "caspr_cnf_in_value_bwd_f32")
    return dy_part.sum(dim=0), dw_part.sum(dim=0), _sum_splits(dgate, ns), _sum_splits(dbeta, ns)


def cnf_act_value(z, b, gate, beta, n):
    """H = softplus((Z + b) gate[f] + beta[f]) on the columns 0..C-1 of z (rows >= R, >= C), C = b.numel() -> (rows, C), rows past R zero."""
    R = _chk_value("cnf_act_value", gate, n, z)
    _chk_f32(b, beta)
    C = b.numel()
    h = _rows_out(z.shape[0], R, C, z.device)
    with ops.timed("k:cnf_act_value", 2):
        _lib.check(_lib.load().caspr_cnf_act_value_f32(_p(z), z.stride(0), _p(b), _p(gate), _p(beta), R, n, C, _p(h), C, _stream()), "caspr_cnf_act_value_f32")
    return h


def cnf_act_value_bwd(z, b, gate, beta, n, dh=None, dzo=None, wo=None):
    """Backward of cnf_act_value from dh (>= R, C), or -- the layer in front of the 3-channel output layer -- from dzo (>= R, >= 3) and
    wo (3, C): dH = dzo wo formed inside the kernel.  -> dz (rows of z, C) with the rows past R zero, dgate (frames, C), dbeta (frames, C)."""
    R = _chk_value("cnf_act_value_bwd", gate, n, z, dh)
    _chk_f32(b, beta, wo)
    if (dh is None) == (dzo is None or wo is None):
        raise ValueError("cnf_act_value_bwd: give dh, or dzo and wo")
    C = b.numel()
    L = _lib.load()
    ns, frames = L.caspr_cnf_value_splits(n), R // n
    dev = z.device
    dz = _rows_out(z.shape[0], R, C, dev)
    dgate = torch.empty(frames, ns, C, device=dev, dtype=torch.float32)
    dbeta = torch.empty(frames, ns, C, device=dev, dtype=torch.float32)
    if dh is not None:
        with ops.timed("k:cnf_act_value_bwd", 2):
            _lib.check(L.caspr_cnf_act_value_bwd_f32(_p(z), z.stride(0), _p(b), _p(gate), _p(beta), _p(dh), dh.stride(0), R, n, C, _p(dz), C, _p(dgate),
                                                     _p(dbeta), _stream()), "caspr_cnf_act_value_bwd_f32")
    else:
        if not dzo.is_cuda or dzo.dtype != torch.float32 or dzo.dim() != 2 or dzo.shape[0] < R or dzo.stride(1) != 1 or dzo.shape[1] < 3 or tuple(wo.shape) != (3, C):
            raise ValueError("cnf_act_value_bwd: dzo must be (>= R, >= 3) float32 GPU rows and wo a contiguous (3, C)")
        with ops.timed("k:cnf_act_value_bwd_out", 2):
            _lib.check(L.caspr_cnf_act_value_bwd_out_f32(_p(z), z.stride(0), _p(b), _p(gate), _p(beta), _p(dzo), dzo.stride(0), _p(wo), C, R, n, C, _p(dz), C,
                                                         _p(dgate), _p(dbeta), _stream()), "caspr_cnf_act_value_bwd_out_f32")
    return dz, _sum_splits(dgate, ns), _sum_splits(dbeta, ns)


def cnf_out_value(zo, b, gate, beta, n):
    """a (R, 3) = (zo[:R, :3] + b) gate[f] + beta[f]; zo (>= R, >= 3), gate / beta (frames, 3) rows with a common row stride."""
    _chk_f32(zo, b)
    R = gate.shape[0] * n
    if zo.dim() != 2 or zo.shape[0] < R or zo.shape[1] < 3 or gate.stride(1) != 1 or beta.stride(1) != 1 or gate.stride(0) != beta.stride(0) or R <= 0 \
            or not gate.is_cuda or gate.dtype != torch.float32 or beta.dtype != torch.float32 or tuple(gate.shape) != tuple(beta.shape) or gate.shape[1] != 3:
        raise ValueError("cnf_out_value: zo (>= R, >= 3), float32 GPU gate / beta (frames, 3) with unit column stride and a common row stride are required")
    a = torch.empty(R, 3, device=zo.device, dtype=torch.float32)
    with ops.timed("k:cnf_out_value", 2):
        _lib.check(_lib.load().caspr_cnf_out_value_f32(_p(zo), zo.stride(0), _p(b), _p(gate), _p(beta), gate.stride(0), R, n, _p(a), _stream()),
                   "caspr_cnf_out_value_f32")
    return a


def cnf_out_value_bwd(da, zo, b, gate, n):
    """da (R, 3) -> dzo (rows of zo, 4) (column 3 and the rows past R zero), dgate (frames, 3), dbeta (frames, 3)."""
    _chk_f32(da, zo, b)
    R = gate.shape[0] * n
    if tuple(da.shape) != (R, 3) or zo.dim() != 2 or zo.shape[0] < R or zo.shape[1] < 3 or gate.stride(1) != 1 or gate.shape[1] != 3 or not gate.is_cuda \
            or gate.dtype != torch.float32:
        raise ValueError("cnf_out_value_bwd: da must be a contiguous (R, 3), zo (>= R, >= 3), gate float32 GPU (frames, 3) rows with unit column stride")
    dev = zo.device
    dzo = _rows_out(zo.shape[0], R, 4, dev)
    dgate = torch.empty(R // n, 3, device=dev, dtype=torch.float32)
    dbeta = torch.empty(R // n, 3, device=dev, dtype=torch.float32)
    with ops.timed("k:cnf_out_value_bwd", 2):
        _lib.check(_lib.load().caspr_cnf_out_value_bwd_f32(_p(da), _p(zo), zo.stride(0), _p(b), _p(gate), gate.stride(0), R, n, _p(dzo), _p(dgate), _p(dbeta),
                                                           _stream()), "caspr_cnf_out_value_bwd_f32")
    return dzo, dgate, dbeta


class Segments:
    """CSR of a scatter: for every target row the contributing source rows (ascending) and their weights.
    Built from flat int tensors `target` (nnz), optional `weight` (nnz) and optional `src_rows` (nnz; default: entry e
    reads source row e)."""

    def __init__(self, target, n_targets, weight=None, src_rows=None):
        tgt = target.reshape(-1).long()
        order = torch.sort(tgt, stable=True)[1]            # stable: equal targets keep ascending source order
        counts = torch.bincount(tgt, minlength=n_targets)
        self.start = torch.zeros(n_targets + 1, device=tgt.device, dtype=torch.int32)
        self.start[1:] = torch.cumsum(counts, 0).to(torch.int32)
        self.row = (order if src_rows is None else src_rows.reshape(-1)[order]).to(torch.int32).contiguous()
        self.w = None if weight is None else weight.reshape(-1)[order].contiguous().float()
        self.n_targets = n_targets


def segment_sum(src, seg, C, dst, col0=0, accumulate=True):
    """dst (targets, >=C) (+)= gather-sum of src rows (any leading shape, rows flattened) through `seg`, columns col0..col0+C."""
    src2 = src.reshape(-1, src.shape[-1])
    dst2 = dst.reshape(-1, dst.shape[-1])
    if src2.stride(1) != 1 or dst2.stride(1) != 1:
        raise ValueError("segment_sum: unit column stride required")
    _lib.check(_lib.load().caspr_segment_sum_f32(_p(src2), src2.stride(0), col0, _p(seg.start), _p(seg.row), _p(seg.w), seg.n_targets, C,
                                                 _p(dst2), dst2.stride(0), int(accumulate), _stream()), "caspr_segment_sum_f32")
    return dst


def chamfer_bwd(p, q, idx1, idx2, g1=None, g2=None, want_p=True, want_q=True):
    """Gradient of ops.chamfer_distance(p, q, return_indices=True)'s two distance vectors (caspr_chamfer_bwd_f32): p (B,n,3), q (B,m,3),
    idx1 (B,n) / idx2 (B,m) int32 as returned there, g1 (B,n) / g2 (B,m) = dL/d dist1 / dL/d dist2 (None = zero).
    -> (dp (B,n,3) | None, dq (B,m,3) | None): a gradient that is not wanted is not computed.  Fixed summation order, no atomics."""
    _chk_f32(p, q, g1, g2)
    _chk_i32(idx1, idx2)
    B, n, _ = p.shape
    m = q.shape[1]
    if q.shape[0] != B or tuple(idx1.shape) != (B, n) or tuple(idx2.shape) != (B, m):
        raise ValueError("chamfer_bwd: p %s, q %s, idx1 %s, idx2 %s disagree" % (tuple(p.shape), tuple(q.shape), tuple(idx1.shape), tuple(idx2.shape)))
    if (g1 is not None and tuple(g1.shape) != (B, n)) or (g2 is not None and tuple(g2.shape) != (B, m)):
        raise ValueError("chamfer_bwd: g1 must be (%d,%d) and g2 (%d,%d)" % (B, n, B, m))
    if not (want_p or want_q):
        return None, None
    dp = torch.empty_like(p) if want_p else None
    dq = torch.empty_like(q) if want_q else None
    _lib.check(_lib.load().caspr_chamfer_bwd_f32(_p(p), _p(q), B, n, m, _p(idx1), _p(idx2), _p(g1), _p(g2), _p(dp), _p(dq), _stream()),
               "caspr_chamfer_bwd_f32")
    return dp, dq


def emd_bwd(p, q, tape, g, want_p=True, want_q=True):
    """Gradient of ops.earth_mover_distance(p, q, transpose=False, return_tape=True)'s cost with the match held fixed (caspr_emd_bwd_f32;
    utils/emd.py:17-21): p (B,n,3), q (B,m,3), tape (B,10,n+m) as returned there, g (B,) = dL/d cost.
    -> (dp (B,n,3) | None, dq (B,m,3) | None): a gradient that is not wanted is not computed.  Fixed summation order, no atomics."""
    _chk_f32(p, q, tape, g)
    B, n, _ = p.shape
    m = q.shape[1]
    if q.shape[0] != B or p.shape[2] != 3 or q.dim() != 3 or q.shape[2] != 3 or tuple(tape.shape) != (B, 10, n + m):
        raise ValueError("emd_bwd: p %s, q %s, tape %s disagree (tape must be (B,10,n+m))" % (tuple(p.shape), tuple(q.shape), tuple(tape.shape)))
    if tuple(g.shape) != (B,):
        raise ValueError("emd_bwd: g must be (%d,), got %s" % (B, tuple(g.shape)))
    if not (want_p or want_q):
        return None, None
    dp = torch.empty_like(p) if want_p else None
    dq = torch.empty_like(q) if want_q else None
    _lib.check(_lib.load().caspr_emd_bwd_f32(_p(p), _p(q), B, n, m, _p(tape), _p(g), _p(dp), _p(dq), _stream()), "caspr_emd_bwd_f32")
    return dp, dq


def emd_exact_bwd(p, q, assign, g, want_p=True, want_q=True):
    """Gradient of ops.earth_mover_distance_exact(p, q, transpose=False, return_match=True)'s cost with the matching held fixed
    (caspr_emd_exact_bwd_f32; the place of utils/emd.py:17-21): p, q (B,n,3), assign (B,n) int32 as returned there, g (B,) = dL/d cost.
    -> (dp (B,n,3) | None, dq (B,n,3) | None): a gradient that is not wanted is not computed.  dp_i = g (p_i - q_assign[i]) / |.|, dq_j the
    negative of the term of the i matched to j; a coincident pair contributes zero, a frame with assign = -1 gets NaN.  No atomics."""
    _chk_f32(p, q, g)
    if p.dim() != 3 or q.dim() != 3 or p.shape[2] != 3 or tuple(q.shape) != tuple(p.shape):
        raise ValueError("emd_exact_bwd: p %s and q %s must both be (B,n,3)" % (tuple(p.shape), tuple(q.shape)))
    B, n, _ = p.shape
    if not torch.is_tensor(assign) or assign.dtype != torch.int32 or tuple(assign.shape) != (B, n) or not assign.is_contiguous() or assign.device != p.device:
        raise ValueError("emd_exact_bwd: assign must be a contiguous int32 (%d,%d) tensor on %s, got %s %s"
                         % (B, n, p.device, getattr(assign, "dtype", type(assign).__name__), tuple(getattr(assign, "shape", ()))))
    if tuple(g.shape) != (B,):
        raise ValueError("emd_exact_bwd: g must be (%d,), got %s" % (B, tuple(g.shape)))
    if not (want_p or want_q):
        return None, None
    dp = torch.empty_like(p) if want_p else None
    dq = torch.empty_like(q) if want_q else None
    _lib.check(_lib.load().caspr_emd_exact_bwd_f32(_p(p), _p(q), _p(assign), _p(g), B, n, _p(dp), _p(dq), _stream()), "caspr_emd_exact_bwd_f32")
    return dp, dq
