"""Python front-end of the C-ABI kernels (include/caspr_hip.h) on torch tensors.

Mirrors the operator surface the reference imports from Kaolin at models/pointnet2.py:7
(`furthest_point_sampling`, `fps_gather_by_index`, `ball_query`, `three_nn`, `three_interpolate`)
plus the fused / MFMA kernels of this build.  PyTorch only owns memory and streams here; every
tensor must live on a HIP device -- there is no CPU fallback (calls raise instead).

Layouts: activations are point-major (B, P, C) float32 with row stride = last-dim size unless a
leading-dimension is given; index tensors are int32.
"""
import contextlib
import ctypes
import functools

import torch

from . import lib as _lib
from .config import config as _cfg


# Optional stage timing with HIP events recorded on the launch stream (bench.py's roofline numbers).
TIMING = False
TIMERS = {}
TIMING_ONLY = None      # a set of names: at TIMING == True only these level-1 timers record (bench.py keeps the dominant kernel's
                        # pair inside the timed region and takes the stage breakdown from its separate detail pass)


class timed:
    """with ops.timed("name"): ...  -> appends a (start, end) event pair to TIMERS[name] when TIMING is on.
    level 2 = per-kernel timers (one pair per launch, keyed by kernel and shape): recorded only when TIMING >= 2, i.e. in
    bench.py's separate detail pass, never inside the timed region of the headline number."""

    def __init__(self, name, level=1):
        self.name = name
        self.level = level

    def __enter__(self):
        self.on = TIMING >= self.level and (TIMING_ONLY is None or TIMING != True or self.name in TIMING_ONLY)
        if self.on:
            self.t0 = torch.cuda.Event(enable_timing=True)
            self.t0.record(torch.cuda.current_stream())
        return self

    def __exit__(self, *exc):
        if self.on:
            t1 = torch.cuda.Event(enable_timing=True)
            t1.record(torch.cuda.current_stream())
            TIMERS.setdefault(self.name, []).append((self.t0, t1))
        return False


class untimed:
    """with ops.untimed(): ...  -> no timer records inside (the accuracy guard's check solves must not enter bench.py's per-kernel means)."""

    def __enter__(self):
        global TIMING
        self.prev, TIMING = TIMING, False
        return self

    def __exit__(self, *exc):
        global TIMING
        TIMING = self.prev
        return False


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _on_current_device(t):
    """The C entries launch on the CURRENT device's stream and never call hipSetDevice (include/caspr_hip.h): a tensor of
    another GPU would be dereferenced by the wrong device.  One process per GPU sets its device once (bench.py)."""
    if t.is_cuda and t.device.index != torch.cuda.current_device():
        raise ValueError("tensor lives on %s but the current device is cuda:%d: wrap the call in torch.cuda.device(t.device)"
                         % (t.device, torch.cuda.current_device()))


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _chk_f32(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError("caspr_amd kernels need tensors on the GPU (got %s): there is no CPU fallback" % t.device)
        _on_current_device(t)
        if t.dtype != torch.float32:
            raise TypeError("expected float32, got %s" % t.dtype)
        if not t.is_contiguous():
            raise ValueError("expected a contiguous tensor")


def _chk_rows(t):
    """(B,P,C) float32 GPU tensor whose rows may be a column slice of a wider buffer: returns the row stride."""
    if t is None:
        return 0
    if not t.is_cuda:
        raise ValueError("caspr_amd kernels need tensors on the GPU (got %s): there is no CPU fallback" % t.device)
    _on_current_device(t)
    if t.dtype != torch.float32 or t.dim() != 3 or t.stride(2) != 1 or t.stride(0) != t.shape[1] * t.stride(1):
        raise ValueError("expected a float32 (B,P,C) tensor with unit channel stride and packed rows")
    if t.stride(1) % 4 != 0 or t.data_ptr() % 16 != 0:
        raise ValueError("row stride must be a multiple of 4 floats and the base 16-byte aligned")
    return t.stride(1)


def _chk_i32(*ts):
    for t in ts:
        if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError("expected a contiguous int32 GPU tensor")


# ---------------------------------------------------------------------------------------------
def prep_input(x, quad=True, pairs=True):
    """x (B,T,N,4) -> xyz (B*T,N,3), feat (B*T,N,8) [x2,y2,z2,xz,xy,yz,0,0]  (tpointnet2.py:79-90)."""
    _chk_f32(x)
    B, T, N, _ = x.shape
    xyz = torch.empty(B * T, N, 3, device=x.device, dtype=torch.float32)
    feat = torch.empty(B * T, N, 8, device=x.device, dtype=torch.float32)
    _lib.check(_lib.load().caspr_prep_input_f32(_p(x), B * T, N, int(quad), int(pairs), _p(xyz), _p(feat), _stream()),
               "caspr_prep_input_f32")
    return xyz, feat


def furthest_point_sampling(xyz, M, guard=True, return_xyz=False):
    """Kaolin `furthest_point_sampling(xyz, M)` (pointnet2.py:384): (B,n,3) -> (B,M) int32."""
    _chk_f32(xyz)
    B, n, _ = xyz.shape
    idx = torch.empty(B, M, device=xyz.device, dtype=torch.int32)
    new_xyz = torch.empty(B, M, 3, device=xyz.device, dtype=torch.float32) if return_xyz else None
    _lib.check(_lib.load().caspr_fps_f32(_p(xyz), B, n, M, int(bool(guard)), _p(idx), _p(new_xyz), _stream()), "caspr_fps_f32")
    return (idx, new_xyz) if return_xyz else idx


def ball_query_pair(radius_a, ns_a, radius_b, ns_b, xyz, new_xyz):
    """The two ball queries of a set-abstraction level (one grouper per radius over the same xyz / new_xyz, pointnet2.py:338-342,391) in ONE
    pass over the cloud -> (idx_a (B,M,ns_a), idx_b (B,M,ns_b)), each what ball_query returns for its radius, bit for bit."""
    _chk_f32(xyz, new_xyz)
    B, n, _ = xyz.shape
    M = new_xyz.shape[1]
    ia = torch.empty(B, M, ns_a, device=xyz.device, dtype=torch.int32)
    ib = torch.empty(B, M, ns_b, device=xyz.device, dtype=torch.int32)
    _lib.check(_lib.load().caspr_ball_query2_f32(_p(xyz), _p(new_xyz), B, n, M, float(radius_a), ns_a, _p(ia), float(radius_b), ns_b, _p(ib), _stream()),
               "caspr_ball_query2_f32")
    return ia, ib


def gather_points(feat, idx):
    """Point-major `fps_gather_by_index`: feat (B,n,C), idx (B,M) -> (B,M,C)  (pointnet2.py:385)."""
    _chk_f32(feat)
    _chk_i32(idx)
    B, n, C = feat.shape
    M = idx.shape[1]
    out = torch.empty(B, M, C, device=feat.device, dtype=torch.float32)
    _lib.check(_lib.load().caspr_gather_points_f32(_p(feat), C, _p(idx), B, n, M, C, _p(out), C, _stream()), "caspr_gather_points_f32")
    return out


def fps_gather_by_index(feat_cf, idx):
    """Reference-shaped `fps_gather_by_index`: feat (B,C,n) channels-first -> (B,C,M)."""
    return gather_points(feat_cf.transpose(1, 2).contiguous(), idx).transpose(1, 2)


def ball_query(radius, ns, xyz, new_xyz):
    """Kaolin `ball_query(radius, ns, xyz, new_xyz)` (pointnet2.py:340-342,391) -> (B,M,ns) int32."""
    _chk_f32(xyz, new_xyz)
    B, n, _ = xyz.shape
    M = new_xyz.shape[1]
    idx = torch.empty(B, M, ns, device=xyz.device, dtype=torch.int32)
    _lib.check(_lib.load().caspr_ball_query_f32(_p(xyz), _p(new_xyz), B, n, M, float(radius), ns, _p(idx), _stream()), "caspr_ball_query_f32")
    return idx


def group_points(xyz, new_xyz, feat, idx):
    """Reference-shaped grouper output (B,M,3+C,ns) (pointnet2.py:391-398); feat point-major (B,n,C) or None."""
    _chk_f32(xyz, new_xyz, feat)
    _chk_i32(idx)
    B, n, _ = xyz.shape
    M, ns = idx.shape[1], idx.shape[2]
    C = 0 if feat is None else feat.shape[2]
    out = torch.empty(B, M, 3 + C, ns, device=xyz.device, dtype=torch.float32)
    _lib.check(_lib.load().caspr_group_points_f32(_p(xyz), _p(new_xyz), _p(feat), C, _p(idx), B, n, M, C, ns, _p(out), _stream()),
               "caspr_group_points_f32")
    return out


def three_nn(unknown, known, with_weights=False):
    """Kaolin `three_nn` (pointnet2.py:514): -> dist (B,n,3) [sqrt], idx (B,n,3) [, normalised inverse-distance weights :516-518].
    At most 8192 known points (the cloud is kept in LDS; more raise).  With m < 3 known points the slots m..2 are never filled, as
    upstream: distance +inf, index 0, and weight exactly 0 (1 / (inf + 1e-8)), so the weights of the m real neighbours still sum to 1."""
    _chk_f32(unknown, known)
    B, n, _ = unknown.shape
    m = known.shape[1]
    dist = torch.empty(B, n, 3, device=unknown.device, dtype=torch.float32)
    idx = torch.empty(B, n, 3, device=unknown.device, dtype=torch.int32)
    w = torch.empty(B, n, 3, device=unknown.device, dtype=torch.float32) if with_weights else None
    _lib.check(_lib.load().caspr_three_nn_f32(_p(unknown), _p(known), B, n, m, _p(dist), _p(idx), _p(w), _stream()), "caspr_three_nn_f32")
    return (dist, idx, w) if with_weights else (dist, idx)


def three_interpolate(feat, idx, weight, skip=None, skip_channels=None, in_scale=None, in_shift=None, in_relu=False, C=None, align=4):
    """Point-major `three_interpolate` (+ concat of skip features): feat (B,m,>=C) -> (B,n,roundup(C+C2, align))
    (pointnet2.py:519-523), columns past C+C2 zero.  in_scale/in_shift (B,C): feat is read as relu(feat*scale+shift)."""
    _chk_f32(weight, in_scale, in_shift)
    _chk_i32(idx)
    ldf = _chk_rows(feat)
    lds = _chk_rows(skip)
    B, m, _ = feat.shape
    C = feat.shape[2] if C is None else C
    n = idx.shape[1]
    C2 = 0 if skip is None else (skip.shape[2] if skip_channels is None else skip_channels)
    if align % 4:
        raise ValueError("three_interpolate: align must be a multiple of 4")
    ldo = (C + C2 + align - 1) // align * align
    out = torch.empty(B, n, ldo, device=feat.device, dtype=torch.float32)
    _lib.check(_lib.load().caspr_three_interp_f32(_p(feat), ldf, _p(idx), _p(weight), _p(in_scale), _p(in_shift), int(in_relu),
                                                  _p(skip), lds, B, m, n, C, C2, _p(out), ldo, _stream()),
               "caspr_three_interp_f32")
    return out


def three_interp_add_gn(u, idx, weight, skip, skip_channels, wskip, bias, gamma, beta, groups=16, eps=1e-5):
    """Feature propagation's first layer AFTER its conv ran on the coarse level (include/caspr_hip.h: caspr_three_interp_add_gn_f32):
    u (B,m,>=C) = W_p h, idx / weight (B,n,3) from three_nn, skip (B,n,>=C2) | None, wskip (C,C2) -> (y (B,n,C) raw, scale (B,C), shift (B,C))."""
    _chk_f32(u, weight, skip, wskip, bias, gamma, beta)
    _chk_i32(idx)
    ldu, lds = _chk_rows(u), _chk_rows(skip)
    B, m, _ = u.shape
    n = idx.shape[1]
    C = gamma.numel()
    C2 = 0 if skip is None else int(skip_channels)
    y = torch.empty(B, n, C, device=u.device, dtype=torch.float32)
    scale = torch.empty(B, C, device=u.device, dtype=torch.float32)
    shift = torch.empty(B, C, device=u.device, dtype=torch.float32)
    L = _lib.load()
    nb = L.caspr_three_interp_add_gn_ws_bytes(B, n, groups)
    ws = _workspace(nb, u.device)
    with timed("k:three_interp_add_gn:%d:%d:%d" % (C2, C, B * n), 2):
        _lib.check(L.caspr_three_interp_add_gn_f32(_p(u), ldu, _p(idx), _p(weight), _p(skip), lds, C2, _p(wskip), _p(bias), B, m, n, C, _p(y), C,
                                                   groups, _p(gamma), _p(beta), float(eps), _p(scale), _p(shift), _p(ws), ws.numel(), _stream()),
                   "caspr_three_interp_add_gn_f32")
    return y, scale, shift


# ---------------------------------------------------------------------------------------------
# Matrix products.  Every contraction of this model is f32 arithmetic; there are two ways to run it on gfx950:
#   "bf16x6" (default): each f32 operand is split EXACTLY into three bf16 numbers (x = x1 + x2 + x3) and a product is
#       evaluated as the six partial products a3b1 + a2b2 + a1b3 + a2b1 + a1b2 + a1b1 on the bf16 matrix pipe with f32
#       accumulation (csrc/gemm_bf16x6.hip, csrc/ode_bf16x6.hip): every partial product is exact, the dropped terms are
#       below 2^-23 |a||b| -- measured at or below the f32 MFMA kernels' own error against f64 on every test -- at 16x the
#       per-instruction FLOP rate, i.e. a 2.67x higher ceiling (2500 / 6 = 416.7 f32-equivalent TFLOP/s vs 157.3);
#   "f32": v_mfma_f32_16x16x4_f32 only (csrc/gemm.hip, csrc/ode.hip), bit-for-bit an ordered fmaf chain.
# Shapes the bf16x6 kernels do not cover (Cin < 192 or not a multiple of 32, fewer than 128 rows per batch entry, the
# set-abstraction MLPs, the latent ODE) run on the f32 MFMA kernels in either mode.  config.matmul = "f32" (or, under
# CASPR_DEBUG=1 only, CASPR_MATMUL=f32) selects the f32 kernels at import; set_matmul_mode() switches at run time (bench.py times both in one process).
_mode = _cfg.matmul            # caspr_amd/config.py (the environment only under CASPR_DEBUG=1)
CONV_BF16X6 = _mode == "bf16x6"      # pointwise convs (conv1x1) on the bf16x6 kernel where the shape allows
CONV_X6W = _cfg.conv_x6w             # ... and the layers with >= 512 output channels on the 512-channel kernel
CNF_BF16X6 = _mode == "bf16x6"       # point-CNF solves on the bf16x6 kernel
CNF_SPLIT = _cfg.cnf_split           # "f16x3": the sampling solve (no divergence, n >= 128) on three f16 products per f32 product (csrc/ode_f16x3w.hip);
                                     # matmul_mode()["cnf"] says "bf16x6" for both (the family; bench.py keys its roofline block on that string)
CNF_DP5_SPLIT = _cfg.cnf_dp5_split   # "f16x3": the ADAPTIVE solve's sampling direction (cnf_method="dopri5", no divergence, n >= 128) on csrc/ode_dp5_f16x3w.hip;
                                     # "bf16x6" (the default): csrc/ode_dp5.hip on every call.  Independent of CNF_SPLIT, whose default is "f16x3"
CNF_TAPE_SPLIT = _cfg.cnf_tape_split   # "f16x3": the sampling solve WITH THE TAPE (train/flow_grad.py: CnfSampleSolve / CnfSampleSolveFrames, n >= 128) on
                                     # csrc/ode_sample_tape_h3w.hip: the bits of cnf_rk4's f16x3 route; "bf16x6" (the default): csrc/ode_sample_tape.hip on every call

CONV_SPLIT = _cfg.conv_split         # "f16x3": the layers of the persistent 512-channel conv on three f16 products per f32 product (csrc/gemm_f16x3w.hip),
                                     # inference only; matmul_mode()["conv"] says "bf16x6" for both (the family), the timer keys stay what they are


def _split_switch(name):
    """The switch `name` of this module, validated where it is read (a run-time switch: a misspelt value must not select bf16x6 silently)."""
    value = globals()[name]
    if value not in ("bf16x6", "f16x3"):
        raise ValueError("caspr_amd.ops.%s must be 'bf16x6' or 'f16x3', got %r" % (name, value))
    return value


def conv_split():
    """CONV_SPLIT, validated where it is read."""
    return _split_switch("CONV_SPLIT")


def cnf_dp5_split():
    """CNF_DP5_SPLIT, validated where it is read."""
    return _split_switch("CNF_DP5_SPLIT")


def cnf_tape_split():
    """CNF_TAPE_SPLIT, validated where it is read."""
    return _split_switch("CNF_TAPE_SPLIT")


def cnf_split():
    """CNF_SPLIT, validated where it is read."""
    return _split_switch("CNF_SPLIT")


_X6_MIN_CIN = 192     # below this the f32 LDS kernel is used anyway (set-abstraction / input layers)
# the 512-channel kernel (gemm_bf16x6w.hip) from this many input channels.  Round 3: 1024 (one workgroup per tile, prologue / epilogue
# exposed: only the 1600-wide head layer's 50-chunk K loop amortised them).  Round 4: the kernel is persistent and its statistics
# epilogue shorter (6.8 vs 7.07 ms on the head layer), so the layers with >= 512 output channels, >= 512 input channels and >= 1024 rows
# per batch entry (_X6W_MIN_ROWS: the coarse levels -- 640 tiles at cfg-2 -- quantise badly onto a persistent grid of 256 workgroups) take it:
# in-step at cfg-2 576 -> 1600: 3.40 -> 3.24 ms, 512 -> 512: 0.92 -> 0.87, 544 -> 512: 0.89 -> 0.84; the 128 -> 1024 layer (4 k-chunks per
# tile) and the 81,920-row levels are faster on the 256-channel kernel.  (config.x6w_min_cin)
_X6W_MIN_CIN = _cfg.x6w_min_cin
_X6W_MIN_ROWS = 1024
_X6_GN_MIN_CIN = 64   # conv + GroupNorm statistics in one pass (conv1x1_gn): pays from a smaller width (no second pass over the output)


def _x6w_fills(pw, B, P):
    """Rows per batch entry from which the persistent 512-channel kernel is chosen.  By the entry's shape only, NEVER by the number of
    entries: a sequence's result must not depend on the batch around it (bitwise sharding invariance), and the two kernels round
    differently."""
    return P >= _X6W_MIN_ROWS


def set_matmul_mode(mode=None, conv=None, cnf=None):
    """Select the kernels of the matrix products: mode "bf16x6" | "f32", or conv= / cnf= booleans individually.
    Returns the previous (conv, cnf) pair.  Packed weights of both kinds are built on first use and cached."""
    global CONV_BF16X6, CNF_BF16X6
    prev = (CONV_BF16X6, CNF_BF16X6)
    if mode is not None:
        if mode not in ("bf16x6", "f32"):
            raise ValueError("mode must be 'bf16x6' or 'f32'")
        CONV_BF16X6 = CNF_BF16X6 = mode == "bf16x6"
    if conv is not None:
        CONV_BF16X6 = bool(conv)
    if cnf is not None:
        CNF_BF16X6 = bool(cnf)
    return prev


def matmul_mode():
    return {"conv": "bf16x6" if CONV_BF16X6 else "f32", "cnf": "bf16x6" if CNF_BF16X6 else "f32"}


class PackedWeight:
    """A (Cout, Cin) weight matrix in MFMA A-fragment order (see csrc/common.h), plus -- built on first use -- the
    three-way bf16 split of csrc/gemm_bf16x6.hip when the shape is supported (`x3()`)."""

    def __init__(self, w2d, col0=0, ncols=None):
        _chk_f32(w2d)
        self.cout, ldw = w2d.shape
        self.cin = ldw - col0 if ncols is None else ncols
        size = _lib.load().caspr_packed_size(self.cout, self.cin)
        self.data = torch.empty(size, device=w2d.device, dtype=torch.float32)
        _lib.check(_lib.load().caspr_pack_weight_f32(_p(w2d), ldw, self.cout, col0, self.cin, _p(self.data), _stream()),
                   "caspr_pack_weight_f32")
        self.x6_ok = self.cin % 32 == 0 and self.cin >= _X6_MIN_CIN and self.cout % 4 == 0 and self.cout >= 128
        self.x6_gn_ok = self.cin % 32 == 0 and self.cin >= _X6_GN_MIN_CIN and self.cout % 4 == 0 and self.cout >= 128
        self._x3 = None
        self._xw = None
        self._xh = None
        # the 128-point x 512-channel kernel (csrc/gemm_bf16x6w.hip) takes the layers with >= 512 output channels and >= 8 k chunks
        self.x6w_ok = self.cin % 32 == 0 and self.cin >= _X6W_MIN_CIN and self.cout % 4 == 0 and self.cout >= 512
        # kept for the lazy bf16x3 pack only, with the version the f32 pack was taken at: w2d may be a VIEW of a parameter
        # (detach()[:, :, 0]), and a pack made after an in-place update would silently disagree with self.data
        self._src = (w2d, ldw, col0, w2d._version) if (self.x6_gn_ok or self.x6w_ok) else None

    def x3(self):
        if self._x3 is None:
            w2d, ldw, col0, version = self._src
            if w2d._version != version:
                raise RuntimeError("PackedWeight.x3(): the weight tensor was modified in place after this pack was built; re-create the "
                                   "PackedWeight (WeightCache does: it is keyed by (data_ptr, _version))")
            nbytes = _lib.load().caspr_bf16x3_packed_bytes(self.cout, self.cin)
            self._x3 = torch.empty(nbytes, device=w2d.device, dtype=torch.uint8)
            _lib.check(_lib.load().caspr_pack_weight_bf16x3(_p(w2d), ldw, self.cout, col0, self.cin, _p(self._x3), _stream()),
                       "caspr_pack_weight_bf16x3")
            if not self.x6w_ok or (self._xw is not None and self._xh is not None):
                self._src = None        # every pack exists: release the (possibly padded) copy of the weight
        return self._x3

    def xw(self):
        """(main, tail) packs of caspr_conv1x1_x6w_f32: the first cout - cout % 512 rows for the 512-channel kernel, the rest (or
        None) as a bf16x3 pack for the 256-channel kernel."""
        if self._xw is None:
            w2d, ldw, col0, version = self._src
            if w2d._version != version:
                raise RuntimeError("PackedWeight.xw(): the weight tensor was modified in place after this pack was built")
            L = _lib.load()
            cmain = self.cout - self.cout % 512
            main = torch.empty(L.caspr_x6w_packed_bytes(cmain, self.cin), device=w2d.device, dtype=torch.uint8)
            _lib.check(L.caspr_pack_weight_x6w(_p(w2d), ldw, cmain, col0, self.cin, _p(main), _stream()), "caspr_pack_weight_x6w")
            tail = None
            if cmain != self.cout:
                wt = w2d[cmain:]
                tail = torch.empty(L.caspr_bf16x3_packed_bytes(self.cout - cmain, self.cin), device=w2d.device, dtype=torch.uint8)
                _lib.check(L.caspr_pack_weight_bf16x3(_p(wt), ldw, self.cout - cmain, col0, self.cin, _p(tail), _stream()), "caspr_pack_weight_bf16x3")
            self._xw = (main, tail)
            if self._x3 is not None and self._xh is not None:
                self._src = None
        return self._xw

    def xh(self):
        """(main, tail) packs of caspr_conv1x1_h3w_f32 (conv_split = "f16x3"): the first cout - cout % 512 rows as two f16 planes with
        the layer's power-of-two scale behind them (found on the device: no host synchronisation), the rest (or None) as the bf16x3
        pack of xw() -- the remainder stays on bf16x6.  Built on first use from the same source, under the same version check."""
        if self._xh is None:
            w2d, ldw, col0, version = self._src
            if w2d._version != version:
                raise RuntimeError("PackedWeight.xh(): the weight tensor was modified in place after this pack was built")
            L = _lib.load()
            cmain = self.cout - self.cout % 512
            main = torch.empty(L.caspr_h3w_packed_bytes(cmain, self.cin), device=w2d.device, dtype=torch.uint8)
            _lib.check(L.caspr_pack_weight_h3w(_p(w2d), ldw, cmain, col0, self.cin, _p(main), _stream()), "caspr_pack_weight_h3w")
            tail = None
            if cmain != self.cout:
                if self._xw is not None:
                    tail = self._xw[1]
                else:
                    wt = w2d[cmain:]
                    tail = torch.empty(L.caspr_bf16x3_packed_bytes(self.cout - cmain, self.cin), device=w2d.device, dtype=torch.uint8)
                    _lib.check(L.caspr_pack_weight_bf16x3(_p(wt), ldw, self.cout - cmain, col0, self.cin, _p(tail), _stream()), "caspr_pack_weight_bf16x3")
            self._xh = (main, tail)
            if self._x3 is not None and self._xw is not None:
                self._src = None
        return self._xh


CONV_ROW_INVARIANT = 0x100     # include/caspr_hip.h: act flag


# ---------------------------------------------------------------------------------------------
# The deferred status channel.  A kernel-side failure (a team barrier that gave up, a used-up attempt budget, a range guard, a capped
# frame, an accuracy check above its tolerance) is a status on the device.  Reading it right away would put a host synchronisation
# back into the path, so it is copied to pinned host memory behind the launch and examined once that copy has arrived: at the next
# call of the same kind on the stream, or when the caller asks (check_deferred_errors, e.g. after a synchronize).  One record per
# launch, never overwritten before it has been read: a failed launch followed by a clean one still raises.
# The two functions below (and _zero_word) are all that touches the device; the CPU test of the channel replaces them.
# ---------------------------------------------------------------------------------------------
def _pinned(n, dtype):
    return torch.empty(n, dtype=dtype).pin_memory()


def _copy_behind(host, src, stream=None):
    """host <- src behind the work queued on `stream` (None: the current one) -> the event that tells when it has arrived."""
    ev = torch.cuda.Event()
    if stream is None:
        host.copy_(src, non_blocking=True)
        ev.record(torch.cuda.current_stream())
    else:
        with torch.cuda.stream(stream):
            host.copy_(src, non_blocking=True)
            ev.record(stream)
    return ev


class _Deferred:
    """One channel: report(records) raises or warns from the arrived records [(values, meta)], oldest first, values = the copied
    words as a Python list."""
    BACKLOG = 64         # records outstanding on one key before a post blocks on the oldest

    def __init__(self, report):
        self.report = report
        self.rings = {}      # key -> [(pinned host tensor, event, meta)], oldest first
        self.pool = {}       # (dtype, numel) -> pinned tensors that have been read and may be reused

    @staticmethod
    def key(device):
        return (device.index, torch.cuda.current_stream().cuda_stream)

    def post(self, key, src, meta=None, stream=None):
        ring = self.rings.setdefault(key, [])
        if len(ring) >= self.BACKLOG:                # nobody drained: bound the backlog (blocks on the oldest; a failure raises from here)
            ring[0][1].synchronize()
            self.poll(key)
        free = self.pool.get((src.dtype, src.numel()))
        host = free.pop() if free else _pinned(src.numel(), src.dtype)     # no fill value: the copy overwrites all of it
        ring.append((host, _copy_behind(host, src, stream), meta))

    def poll(self, key, wait=False):
        """Drain the records of `key` whose copy has arrived (all of them with wait=True), up to the first that has not, and report."""
        ring = self.rings.get(key)
        if not ring:
            return
        records = []
        while ring:
            host, ev, meta = ring[0]
            if wait:
                ev.synchronize()
            if not ev.query():
                break
            ring.pop(0)
            records.append((host.tolist(), meta))
            self.pool.setdefault((host.dtype, host.numel()), []).append(host)
        if records:
            self.report(records)

    def poll_all(self, wait=False):
        for key in list(self.rings):
            self.poll(key, wait)

    def on(self, device):
        """with channel.on(device) as status: <launch>; status.post(src, meta)  -- reports what has arrived of the stream's earlier
        launches first, without waiting.  Under stream capture it does neither: no event queries, no host copies there."""
        return _DeferredScope(self, device)


class _DeferredScope:
    __slots__ = ("chan", "device", "key", "live")

    def __init__(self, chan, device):
        self.chan, self.device = chan, device

    def __enter__(self):
        self.key = self.chan.key(self.device)
        self.live = not torch.cuda.is_current_stream_capturing()
        if self.live:
            self.chan.poll(self.key)
        return self

    def __exit__(self, *exc):
        return False

    def post(self, src=None, meta=None):
        if self.live:
            self.chan.post(self.key, src, meta)

    @property
    def word(self):
        return self.chan.word(self.key, self.device)


class _DeferredWord(_Deferred):
    """A channel whose kernels report into one persistent int32 device word per (device, stream)."""

    def __init__(self, report):
        super().__init__(report)
        self.words = {}      # key -> (device word, the torch stream it belongs to)

    def word(self, key, device):
        ent = self.words.get(key)
        if ent is None:
            ent = self.words[key] = (torch.zeros(1, device=device, dtype=torch.int32), torch.cuda.current_stream())
        return ent[0]


def _zero_word(word, stream):
    with torch.cuda.stream(stream):
        word.zero_()


class _DeferredSticky(_DeferredWord):
    """The word is never cleared by a launch, so one copy shows every trip before it: a post behind an outstanding copy only marks the
    stream stale (eight wide layers per encoder pass would otherwise queue eight copies), a waiting poll first fetches what the
    skipped copies would have shown, and the word is cleared, on its own stream, once a trip has been reported."""

    def __init__(self, report):
        super().__init__(report)
        self.stale = set()   # keys with launches behind the last copy

    def post(self, key, src=None, meta=None):
        if self.rings.get(key):
            self.stale.add(key)
        else:
            self._fetch(key)

    def _fetch(self, key):
        word, stream = self.words[key]
        super().post(key, word, None, stream)
        self.stale.discard(key)

    def poll(self, key, wait=False):
        try:
            if wait and key in self.stale and not self.rings.get(key):
                self._fetch(key)
            super().poll(key, wait)
            if wait and key in self.stale:             # launches behind the copy that was outstanding
                self._fetch(key)
                super().poll(key, True)
        except _lib.CasprHipError:
            _zero_word(*self.words[key])               # reported: the next call starts clean
            raise


# The f16x3 conv's range guard (csrc/gemm_f16x3w.hip): an input value that is not finite in f16 after the 2^4 scale makes its row NaN and
# ORs into the stream's sticky status word.
def _conv_h3_report(records):
    if any(words[0] for words, _ in records):
        raise _lib.CasprHipError("caspr_conv1x1_h3w_f32: the range guard of the f16x3 pointwise conv tripped: an input activation (after the "
                                 "producer's GroupNorm / ReLU) reached 4095 in magnitude or was not finite, which f16 cannot hold after the kernel's "
                                 "2^4 prescale; the outputs of the affected rows were set to NaN.  Remedy: conv_split=\"bf16x6\" "
                                 "(caspr_amd.config.config.conv_split / caspr_amd.ops.CONV_SPLIT), the six-product bf16 kernel, which has f32's "
                                 "exponent range")


_conv_h3 = _DeferredSticky(_conv_h3_report)
CONV_ROUTE_COUNT = {"h3w": 0}      # launches of the f16x3 entries so far (tests assert the route from it)


@contextlib.contextmanager
def _conv_h3_launch(x):
    """with _conv_h3_launch(x) as word: <launch an f16x3 conv that ORs into word>  -- reports an earlier launch's trip first."""
    CONV_ROUTE_COUNT["h3w"] += 1
    with _conv_h3.on(x.device) as status:
        yield _p(status.word)
        status.post()


def conv1x1_train(*args, **kwargs):
    """conv1x1 for the training tier (train/encoder_grad.py, train/flow_grad.py): always the bf16x6 / f32 kernels, whatever CONV_SPLIT says."""
    return conv1x1(*args, split="bf16x6", **kwargs)


# The route table of the pointwise conv ("The pointwise conv's route table"): which kernel takes a layer, and the entry of
# each route per kind of call.  A new form of a kernel is one row here and one branch of _conv_route.
_CONV_ENTRY = {
    "f32": {"conv": "caspr_conv1x1_f32"},
    "x6": {"conv": "caspr_conv1x1_bf16x6_f32", "gn": "caspr_conv1x1_gn_bf16x6_f32", "pooled": "caspr_conv1x1_gn_pooled_bf16x6_f32"},
    "x6w": {"conv": "caspr_conv1x1_x6w_f32", "gn": "caspr_conv1x1_x6w_f32", "pooled": "caspr_conv1x1_x6w_pooled_f32", "part": "caspr_conv1x1_x6w_part_f32"},
    "h3w": {"conv": "caspr_conv1x1_h3w_f32", "gn": "caspr_conv1x1_h3w_f32", "pooled": "caspr_conv1x1_h3w_pooled_f32", "part": "caspr_conv1x1_h3w_part_f32"},
}
_CONV_WIDE = ("x6w", "h3w")                # the persistent 512-channel kernel's two forms
_CONV_NO_GN = (0, None, None, 0.0, None, None, None, None, None, None, 0)      # a wide entry as a plain conv: G = 0, no statistics, no workspace


def _conv_route(pw, B, P, in_relu_from=0, act=0, row_invariant=False, groups=None, split=None):
    """The kernel that takes this call: "f32" | "x6" (256-channel bf16x6) | "x6w" | "h3w" (the 512-channel kernel on bf16x6 / f16x3), from
    the weight's flags, the call's shape and flags and this module's switches, read now.  groups: None for a plain conv; conv1x1_gn's
    group count otherwise, and then None comes back when no kernel takes conv and statistics in one pass.  split: None = CONV_SPLIT;
    the training tier passes "bf16x6" (conv1x1_train, conv1x1_gn(split=)): its forward, backward and tapes keep the bits they had.
    Four rules that read like accidents and are not:
      1. an epilogue (act != 0) or row_invariant keeps a plain conv off the wide kernel, which has neither;
      2. a GroupNorm call asks x6_gn_ok and C % groups before anything else: without them it is conv1x1 + gn_stats, whatever else holds;
      3. ... and that conv1x1 asks again without groups, so a layer with x6w_ok but not x6_gn_ok (Cin = 32 under a lowered
         _X6W_MIN_CIN) still lands on the wide kernel, as a plain conv (G = 0);
      4. CONV_SPLIT is read here as it stands.  It is validated (conv_split()) only on calls with split=None that go on: by conv1x1 when
         the wide kernel takes the call, by the GroupNorm paths -- all three, the 256-channel route included -- once their workspace is
         sized.  conv1x1_gn_early_ok never validates."""
    mfma = CONV_BF16X6 and P % 128 == 0 and in_relu_from % 8 == 0 and not row_invariant
    if groups is not None and not (mfma and pw.x6_gn_ok and pw.cout % groups == 0):
        return None
    if mfma and CONV_X6W and pw.x6w_ok and act == 0 and _x6w_fills(pw, B, P):
        return "h3w" if (CONV_SPLIT if split is None else split) == "f16x3" else "x6w"
    if groups is not None or (mfma and pw.x6_ok):
        return "x6"
    return "f32"


def _conv_ldx(who, pw, x):
    ldx = _chk_rows(x)
    if x.shape[2] < pw.cin and ldx < (pw.cin + 3) // 4 * 4:
        raise ValueError("%s: input rows hold %d channels, weight needs %d" % (who, x.shape[2], pw.cin))
    return ldx


def _conv_head(pw, bias, bbias, x, ldx, in_scale, in_shift, in_relu, in_relu_from, y, ldy):
    """The arguments every conv entry takes behind its packed weight(s)."""
    B, P, _ = x.shape
    return (_p(bias), _p(bbias), _p(x), ldx, _p(in_scale), _p(in_shift), int(in_relu), int(in_relu_from), _p(y), ldy, B, P, pw.cin, pw.cout)


def _conv_wide_packs(route, pw):
    """The (main, tail) pack of a wide route, None for the others.  A pack is BUILT on first use, by launches on the current stream: a
    caller resolves it once, on its own stream, in front of its timer and of any stream switch -- a part queued on a side stream must
    find it finished, and the first call of a layer must not time the pack kernels."""
    return pw.xh() if route == "h3w" else pw.xw() if route == "x6w" else None


def _conv_launch(route, kind, pw, packs, x, head, rest):
    """The one launch site: entry _CONV_ENTRY[route][kind] on (the route's pack(s), head, rest[, the f16x3 status word], stream).
    packs: what _conv_wide_packs gave the caller."""
    name = _CONV_ENTRY[route][kind]
    entry = getattr(_lib.load(), name)
    if packs is None:
        packs = (pw.x3(),) if route == "x6" else (pw.data,)
    args = (*map(_p, packs), *head, *rest)
    if route == "h3w":
        with _conv_h3_launch(x) as word:
            _lib.check(entry(*args, word, _stream()), name)
    else:
        _lib.check(entry(*args, _stream()), name)


def _conv_timer(route, pw, x):
    B, P, _ = x.shape
    return "k:conv1x1_%s:%d:%d:%d" % ("f32" if route == "f32" else "bf16x6", pw.cin, pw.cout, B * P)


def conv1x1(pw, bias, x, bbias=None, in_scale=None, in_shift=None, in_relu=False, in_relu_from=0, act=0, out=None, row_invariant=False, split=None):
    """Pointwise conv on MFMA: x (B,P,>=Cin) point-major (may be a column slice of a wider buffer) ->
    (B,P,roundup4(Cout)) or into `out` (same rules).  See caspr_conv1x1_f32.
    row_invariant: a row's result depends on that row only (not on P / its position): for convs over frames-as-rows."""
    if row_invariant:
        act = act | CONV_ROW_INVARIANT
    _chk_f32(bias, bbias, in_scale, in_shift)
    ldx = _conv_ldx("conv1x1", pw, x)
    B, P, _ = x.shape
    if out is None:
        out = torch.empty(B, P, (pw.cout + 3) // 4 * 4, device=x.device, dtype=torch.float32)
    ldy = _chk_rows(out)
    route = _conv_route(pw, B, P, in_relu_from, act, row_invariant, None, split)
    if route in _CONV_WIDE and split is None:
        conv_split()
    packs = _conv_wide_packs(route, pw)
    with timed(_conv_timer(route, pw, x), 2):
        _conv_launch(route, "conv", pw, packs, x, _conv_head(pw, bias, bbias, x, ldx, in_scale, in_shift, in_relu, in_relu_from, out, ldy),
                     _CONV_NO_GN if route in _CONV_WIDE else (act,))
    return out


_ws_cache = {}


def _workspace(nbytes, device):
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), device=device, dtype=torch.uint8)
        _ws_cache[key] = ws
    return ws


def gn_stats(y, C, gamma, beta, groups=16, eps=1e-5, want_max=False):
    """GroupNorm statistics of y (B,P,ldy) -> scale (B,C), shift (B,C) [, max over points of the normalised output (B,C)]."""
    _chk_f32(gamma, beta)
    ldy = _chk_rows(y)
    B, P, _ = y.shape
    scale = torch.empty(B, C, device=y.device, dtype=torch.float32)
    shift = torch.empty(B, C, device=y.device, dtype=torch.float32)
    pmax = torch.empty(B, C, device=y.device, dtype=torch.float32) if want_max else None
    nbytes = _lib.load().caspr_gn_ws_bytes(B, P, C, groups)
    ws = _workspace(nbytes, y.device)
    _lib.check(_lib.load().caspr_gn_stats_f32(_p(y), ldy, B, P, C, groups, _p(gamma), _p(beta), float(eps), _p(scale), _p(shift), _p(pmax),
                                              _p(ws), ws.numel(), _stream()), "caspr_gn_stats_f32")
    return (scale, shift, pmax) if want_max else (scale, shift)


def _conv_gn_buffers(pw, x, pool=1, moments=0, want_max=False, out=None, write=True):
    """What a conv with GroupNorm statistics writes -> (y | None, ldy, scale, shift, mean, rstd, pmax, workspace): statistics per `pool`
    batch entries, mean / rstd (`moments` = the group count) and pmax only when asked for."""
    B, P, _ = x.shape
    C, Bs, dev = pw.cout, B // pool, x.device
    y = out
    if y is None and write:
        y = torch.empty(B, P, (C + 3) // 4 * 4, device=dev, dtype=torch.float32)
    ldy = _chk_rows(y) if y is not None else 0
    scale = torch.empty(Bs, C, device=dev, dtype=torch.float32)
    shift = torch.empty(Bs, C, device=dev, dtype=torch.float32)
    mean = torch.empty(Bs, moments, device=dev, dtype=torch.float32) if moments else None
    rstd = torch.empty(Bs, moments, device=dev, dtype=torch.float32) if moments else None
    pmax = torch.empty(Bs, C, device=dev, dtype=torch.float32) if want_max else None
    return y, ldy, scale, shift, mean, rstd, pmax, _workspace(_lib.load().caspr_conv_gn_ws_bytes(B, P, C), dev)


def _conv_gn_result(y, scale, shift, mean=None, rstd=None, pmax=None):
    return (y, scale, shift) + (() if mean is None else (mean, rstd)) + (() if pmax is None else (pmax,))


def conv1x1_gn(pw, bias, x, gamma, beta, groups=16, eps=1e-5, want_max=False, want_moments=False, write=True, bbias=None,
               in_scale=None, in_shift=None, in_relu=False, in_relu_from=0, out=None, pool=1, split=None):
    """conv1x1 followed by the statistics of the GroupNorm on its output (the model's conv -> GroupNorm -> ReLU block):
    -> (y | None, scale (B,C), shift (B,C)[, mean (B,G), rstd (B,G)][, pmax (B,C)]).  On the bf16x6 path the statistics come
    out of the conv's epilogue (caspr_conv1x1_gn_bf16x6_f32) and `write=False` skips the output altogether; otherwise this is
    conv1x1 + gn_stats (`write` is then ignored: y is returned)."""
    _chk_f32(bias, bbias, in_scale, in_shift, gamma, beta)
    B, P, _ = x.shape
    C = pw.cout
    # pool: the statistics are taken over `pool` consecutive batch entries together (-> (B / pool, C) outputs) while in_scale /
    # in_shift / bbias stay per entry (caspr_conv1x1_gn_pooled_bf16x6_f32)
    if pool < 1 or B % pool:
        raise ValueError("conv1x1_gn: pool=%d must divide the %d batch entries" % (pool, B))
    route = _conv_route(pw, B, P, in_relu_from, groups=groups, split=split)
    if route is None:
        y = conv1x1(pw, bias, x, bbias=bbias, in_scale=in_scale, in_shift=in_shift, in_relu=in_relu, in_relu_from=in_relu_from, out=out, split=split)
        yg = y.view(B // pool, pool * P, y.shape[2]) if pool > 1 else y
        if want_moments:
            from . import train_ops
            return (y,) + tuple(train_ops.gn_stats_train(yg, C, gamma, beta, groups, eps, want_max))
        return (y,) + tuple(gn_stats(yg, C, gamma, beta, groups, eps, want_max))
    ldx = _conv_ldx("conv1x1_gn", pw, x)
    y, ldy, scale, shift, mean, rstd, pmax, ws = _conv_gn_buffers(pw, x, pool, groups if want_moments else 0, want_max, out, write)
    if split is None:
        conv_split()
    packs = _conv_wide_packs(route, pw)
    with timed(_conv_timer(route, pw, x), 2):           # conv + statistics epilogue + the finalize kernel
        _conv_launch(route, "pooled" if pool > 1 else "gn", pw, packs, x, _conv_head(pw, bias, bbias, x, ldx, in_scale, in_shift, in_relu, in_relu_from, y, ldy),
                     (groups,) + ((int(pool),) if pool > 1 else ()) + (_p(gamma), _p(beta), float(eps), _p(scale), _p(shift), _p(pmax), _p(mean), _p(rstd),
                                                                       _p(ws), ws.numel()))
    return _conv_gn_result(y, scale, shift, mean, rstd, pmax)


def _conv_part(route, pw, packs, x, head, ws, mt0, mt1, with_tail, reserve):
    """Channel tiles [mt0, mt1) of a layer on the 512-channel kernel, with or without the < 512-channel remainder, partial statistics into ws;
    all but `reserve` compute units."""
    _conv_launch(route, "part", pw, packs, x, head, (mt0, mt1, int(with_tail), int(reserve), _p(ws), ws.numel()))


def _conv_gn_finalize(ws, x, C, groups, pool, gamma, beta, eps, scale, shift, pmax, g0, g1):
    """The statistics of GroupNorm groups [g0, g1) from the partials the parts left in ws."""
    _lib.check(_lib.load().caspr_conv_gn_finalize_f32(_p(ws), ws.numel(), x.shape[0], x.shape[1], C, groups, g0, g1, int(pool), _p(gamma), _p(beta),
                                                      float(eps), _p(scale), _p(shift), _p(pmax), None, None, _stream()), "caspr_conv_gn_finalize_f32")


def conv1x1_gn_early_ok(pw, B, P, groups, early_channels):
    """Can conv1x1_gn_early run this layer in pieces?  The 512-channel kernel must take it, in at least two channel tiles, and the
    channels the caller wants early must lie inside GroupNorm group 0, inside the first tile."""
    C = pw.cout
    return bool(_conv_route(pw, B, P) in _CONV_WIDE and C % groups == 0 and C // 512 >= 2 and early_channels <= min(C // groups, 512))


def conv1x1_gn_early(pw, bias, x, gamma, beta, on_early, groups=16, eps=1e-5, in_scale=None, in_shift=None, in_relu=False, in_relu_from=0,
                     reserve_cus=1, tail_stream=None):
    """conv1x1_gn(..., want_max=True) in two pieces (caspr_conv1x1_x6w_part_f32 / caspr_conv_gn_finalize_f32): after the FIRST 512-channel
    tile the statistics of GroupNorm group 0 are final -- `on_early(pmax)` is called with the (B, C) max-over-points tensor whose
    group-0 columns are valid, on the current stream, and may queue work on another stream behind an event (the latent solve: it
    starts from pmax[:, :64], caspr.py:169) -- then the remaining tiles run on all but `reserve_cus` compute units, and the full
    finalize follows.  Returns (y, scale, shift, pmax) with the values of conv1x1_gn, bit for bit.
    tail_stream: the stream on_early queued its work on.  The < 512-channel remainder of the layer (a pass of its own kind over the whole
    input, bound by reading it once: 0.6 ms at cfg-2) is then queued THERE, behind that work, instead of behind the main tiles: the
    compute units reserved for the early kernel are free again long before the main tiles finish (the solve takes 2.6 of their 4.8 ms),
    and the remainder runs on them beside the tiles instead of after them."""
    _chk_f32(bias, in_scale, in_shift, gamma, beta)
    B, P, _ = x.shape
    C = pw.cout
    if not conv1x1_gn_early_ok(pw, B, P, groups, 1):
        raise ValueError("conv1x1_gn_early: this layer does not run on the 512-channel kernel in >= 2 channel tiles")
    ldx = _chk_rows(x)
    y, ldy, scale, shift, _, _, pmax, ws = _conv_gn_buffers(pw, x, want_max=True)
    conv_split()
    route = _conv_route(pw, B, P)
    part = functools.partial(_conv_part, route, pw, _conv_wide_packs(route, pw), x,
                             _conv_head(pw, bias, None, x, ldx, in_scale, in_shift, in_relu, in_relu_from, y, ldy), ws)
    finalize = functools.partial(_conv_gn_finalize, ws, x, C, groups, 1, gamma, beta, eps, scale, shift, pmax)
    mt_all = C // 512
    with timed(_conv_timer(route, pw, x), 2):
        part(0, 1, False, 0)
        finalize(0, 1)
        on_early(pmax)
        if tail_stream is not None and C % 512 and reserve_cus > 0:
            main_stream = torch.cuda.current_stream()
            issued = torch.cuda.Event()
            issued.record(main_stream)               # the remainder reads x and writes its own columns of y / of the partials: nothing of tile 0's
            with torch.cuda.stream(tail_stream):
                tail_stream.wait_event(issued)
                part(mt_all, mt_all, True, 0)        # the remainder only, behind whatever on_early queued on that stream
                tail_done = torch.cuda.Event()
                tail_done.record(tail_stream)
            part(1, mt_all, False, reserve_cus)
            main_stream.wait_event(tail_done)
            for t_ in (x, y, ws, in_scale, in_shift):
                if t_ is not None:
                    t_.record_stream(tail_stream)
        else:
            part(1, mt_all, True, reserve_cus)
        finalize(1, groups)         # group 0 is final already (and the side stream may be reading its pmax / scale / shift right now)
    return y, scale, shift, pmax


def conv1x1_gn_tail_beside(pw, bias, x, gamma, beta, tail_stream, groups=16, eps=1e-5, bbias=None, in_scale=None, in_shift=None, in_relu=False,
                           in_relu_from=0, pool=1):
    """conv1x1_gn(...) of a layer that runs on the persistent 512-channel kernel with a < 512-channel remainder (1600 = 3 x 512 + 64), the
    remainder's pass -- bound by reading the input once -- queued on `tail_stream` BESIDE the main tiles instead of behind them (its
    workgroups need 4 KB of LDS and 116 registers: they share the compute units with the persistent kernel's one wave per SIMD).  Same
    pieces (caspr_conv1x1_x6w_part_f32 / caspr_conv_gn_finalize_f32), same bits as conv1x1_gn; falls back to it when the layer does not
    take that kernel.  -> (y, scale, shift)."""
    B, P, _ = x.shape
    C = pw.cout
    if not (tail_stream is not None and (route := _conv_route(pw, B, P, in_relu_from, groups=groups)) in _CONV_WIDE and C % 512 != 0 and C > 512
            and B % pool == 0 and not torch.cuda.is_current_stream_capturing()):
        return conv1x1_gn(pw, bias, x, gamma, beta, groups, eps, bbias=bbias, in_scale=in_scale, in_shift=in_shift, in_relu=in_relu,
                          in_relu_from=in_relu_from, pool=pool)
    _chk_f32(bias, bbias, in_scale, in_shift, gamma, beta)
    ldx = _chk_rows(x)
    y, ldy, scale, shift, _, _, _, ws = _conv_gn_buffers(pw, x, pool)
    conv_split()
    part = functools.partial(_conv_part, route, pw, _conv_wide_packs(route, pw), x,
                             _conv_head(pw, bias, bbias, x, ldx, in_scale, in_shift, in_relu, in_relu_from, y, ldy), ws)
    mt_all = C // 512
    with timed(_conv_timer(route, pw, x), 2):
        main_stream = torch.cuda.current_stream()
        tail_stream.wait_stream(main_stream)
        with torch.cuda.stream(tail_stream):
            part(mt_all, mt_all, True, 0)            # the remainder only: its own columns of y and of the partials
            tail_done = torch.cuda.Event()
            tail_done.record(tail_stream)
        part(0, mt_all, False, 0)
        main_stream.wait_event(tail_done)
        for t_ in (x, y, ws, in_scale, in_shift, bbias, bias):
            if t_ is not None:
                t_.record_stream(tail_stream)
        _conv_gn_finalize(ws, x, C, groups, pool, gamma, beta, eps, scale, shift, None, 0, groups)
    return y, scale, shift


FEAT_QUAD, FEAT_PAIRS, FEAT_LO_IN, FEAT_LO_OUT = 1, 2, 4, 8     # include/caspr_hip.h
SA_ONLY_MFMA, SA_ONLY_F64 = 16, 32                              # the call in two halves (two streams): the MFMA kernel / the f64 re-evaluation


def sa_mlp_max(xyz, new_xyz, feat, idx, C, layers, out, out_off, feat_kind=0, part=None):
    """Fused grouper + 3-layer point MLP + GroupNorm + max (pointnet2.py:391-409,649-703).
    feat (B,n,ldf) point-major with C valid channels; layers = 3 x (PackedWeight, bias, gamma, beta).
    feat_kind: FEAT_QUAD | FEAT_PAIRS when feat is prep_input's quadratic augmentation of xyz (first level); FEAT_LO_OUT: `out` rows are
    [channels | their low parts] (the second half of the row receives what the f32 output lacks of the kernel's f64 result); FEAT_LO_IN:
    `feat` rows are [C channels .. | low parts from column ldf / 2] as a FEAT_LO_OUT call wrote them (include/caspr_hip.h).
    part: None = the whole call; "mfma" / "f64" = one of its two halves (SA_ONLY_MFMA / SA_ONLY_F64: the MFMA kernel over the neighbourhoods
    the f64 re-evaluation does not take / that re-evaluation alone), for a caller that runs them on two streams -- together they write what
    the whole call writes, bit for bit."""
    if part not in (None, "mfma", "f64"):
        raise ValueError("sa_mlp_max: part must be None, 'mfma' or 'f64'")
    feat_kind = int(feat_kind) | (SA_ONLY_MFMA if part == "mfma" else (SA_ONLY_F64 if part == "f64" else 0))
    _chk_f32(xyz, new_xyz, feat, out)
    _chk_i32(idx)
    B, n, _ = xyz.shape
    M, ns = idx.shape[1], idx.shape[2]
    ldf = 0 if feat is None else feat.shape[2]
    args = []
    for (pw, b, g, be) in layers:
        _chk_f32(b, g, be)
        args += [_p(pw.data), _p(b), _p(g), _p(be), pw.cout]
    # 2 FLOP per multiply-add of the three layers over every gathered sample (C + 3 input channels: xyz first)
    flop = 2.0 * B * M * ns * ((C + 3) * layers[0][0].cout + layers[0][0].cout * layers[1][0].cout + layers[1][0].cout * layers[2][0].cout)
    with timed("k:sa_mlp_max%s:%d:%d:%d:%d" % ("" if part is None else "_" + part, C + 3, layers[2][0].cout, B * M * ns, int(flop // 1000000) if part != "f64" else 0), 2):
        # scratch for the register kernel's list of the neighbourhoods the f64 re-evaluation leaves to it (include/caspr_hip.h); the
        # wider shapes take the LDS kernel and no scratch
        ws = None
        if max(l_[0].cout for l_ in layers) <= 64:
            ws = torch.empty(_lib.load().caspr_sa_mlp_max_workspace_ints(B, M), dtype=torch.int32, device=xyz.device)
        _lib.check(_lib.load().caspr_sa_mlp_max_ws_f32(_p(xyz), _p(new_xyz), _p(feat), ldf, _p(idx), B, n, M, C, ns, int(feat_kind), *args,
                                                       _p(out), out.shape[2], out_off, _p(ws), _stream()), "caspr_sa_mlp_max_ws_f32")
    return out


def group_rows_pre(xyz, new_xyz, pre, idx, wx, bias):
    """The pre-aggregated first layer as rows (include/caspr_hip.h: caspr_group_rows_pre_f32): -> Y (B, M*ns, C1) raw layer-1 output."""
    _chk_f32(xyz, new_xyz, pre, wx, bias)
    _chk_i32(idx)
    B, n, _ = xyz.shape
    M, ns = idx.shape[1], idx.shape[2]
    C1 = bias.numel()
    Y = torch.empty(B, M * ns, C1, device=xyz.device, dtype=torch.float32)
    _lib.check(_lib.load().caspr_group_rows_pre_f32(_p(xyz), _p(new_xyz), _p(pre), _chk_rows(pre), _p(idx), B, n, M, C1, ns, _p(wx), _p(bias), _p(Y), C1,
                                                    _stream()), "caspr_group_rows_pre_f32")
    return Y


def sa_mlp_max_pre(xyz, new_xyz, pre, idx, wx, layers, out, out_off):
    """sa_mlp_max with the first layer pre-aggregated (include/caspr_hip.h: caspr_sa_mlp_max_pre_f32): pre (B,n,>=C1) = W_f . feat over the
    level's source points, wx (C1,3) the layer's coordinate columns; layers = 3 x (PackedWeight | None, bias, gamma, beta) -- the first
    entry's weight is not used."""
    _chk_f32(xyz, new_xyz, pre, wx, out)
    _chk_i32(idx)
    B, n, _ = xyz.shape
    M, ns = idx.shape[1], idx.shape[2]
    ldp = _chk_rows(pre)
    (_, b1, g1, be1), (pw2, b2, g2, be2), (pw3, b3, g3, be3) = layers
    _chk_f32(b1, g1, be1, b2, g2, be2, b3, g3, be3)
    C1 = g1.numel()
    # FLOPs of the REFERENCE's formulation (every gathered sample through all three layers), so that the rate stays comparable
    flop = 2.0 * B * M * ns * (C1 * pw2.cout + pw2.cout * pw3.cout)
    with timed("k:sa_mlp_max_pre:%d:%d:%d:%d" % (C1, pw3.cout, B * M * ns, int(flop // 1000000)), 2):
        _lib.check(_lib.load().caspr_sa_mlp_max_pre_f32(_p(xyz), _p(new_xyz), _p(pre), ldp, _p(idx), B, n, M, ns, _p(wx), _p(b1), _p(g1), _p(be1), C1,
                                                        _p(pw2.data), _p(b2), _p(g2), _p(be2), pw2.cout, _p(pw3.data), _p(b3), _p(g3), _p(be3), pw3.cout,
                                                        _p(out), out.shape[2], out_off, _stream()), "caspr_sa_mlp_max_pre_f32")
    return out


LATENT_TEAM = _cfg.latent_team   # multi-workgroup latent ODE kernel (False: single-workgroup kernel)
_team_ws = {}


def _team_workspace(nbytes, device):
    """Dedicated (not shared with other ops) 256-byte aligned scratch of the team kernel: its barrier counters must not
    be recycled by another launch while a solve is in flight on a different stream."""
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    ws = _team_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, device=device, dtype=torch.uint8)
        _team_ws[key] = ws
    return ws


# A team barrier that gives up (its workgroups were not co-resident within the spin bound) poisons the solve's output with
# NaN and sets an error word per group of 16 sequences in the workspace.
_LM_WS_STRIDE_WORDS = (256 + (2 * 128 * 16 * 4 + 32 * 4 * 256) * 4) // 4      # LM_WS_STRIDE of csrc/ode.hip, in 32-bit words


def _team_words(ws, B):
    """The error word of each group of the team kernel's workspace, as a strided int32 view."""
    groups = (B + 15) // 16
    return ws[:groups * _LM_WS_STRIDE_WORDS * 4].view(torch.int32)[16::_LM_WS_STRIDE_WORDS]


def _team_report(records):
    if any(any(words) for words, _ in records):
        raise _lib.CasprHipError("caspr_latent_rk4_team_f32: a team barrier gave up (the 32 x ceil(B/16) workgroups were not co-resident "
                                 "within the spin bound); the solve's output was poisoned with NaN.  Set caspr_amd.ops.LATENT_TEAM = False "
                                 "(config.latent_team; it also takes the early solve of reconstruct() off the team kernel) to use the "
                                 "single-workgroup kernel when other streams / processes saturate the GPU")


_team = _Deferred(_team_report)


def check_deferred_errors(wait=True):
    """Raise CasprHipError if an earlier asynchronous kernel reported a failure (the latent team kernel's barrier, the adaptive
    latent solve's attempt budget, the range guard of the f16x3 CNF solve or of the f16x3 convs, a frame capped by the per-frame step controller), or
    CasprAccuracyError / warn if a run-time accuracy check of the fixed-step integrators came back above its tolerance
    (guard_track).  wait=True blocks until the status words of every outstanding solve / check have arrived."""
    for chan in (_team, _latent_dp5, _cnf_h3, _conv_h3, _steps, _guard):
        chan.poll_all(wait)


# ---------------------------------------------------------------------------------------------
# Run-time accuracy guard of the fixed-step integrators (models/caspr.py: CaSPR.check_tol).  The reference's dopri5 bounds its
# integration error at every call (flow.py:96-99, cnf.py:100-119, latent_ode_model.py:38,83); a fixed step count does not.  With the
# guard on, every solve is repeated on a subsample at half (or twice) the step count on a side stream, the two results are compared
# ON THE DEVICE, and the maximum difference travels through the deferred channel: the verdict is read at the next guarded call or by
# check_deferred_errors().
# ---------------------------------------------------------------------------------------------
class CasprAccuracyError(_lib.CasprHipError):
    """A guarded RK4 solve whose step-halving error estimate exceeds the tolerance asked for (CaSPR.check_tol)."""


GUARD_LAST = {}          # name -> the last drained record {"diff", "estimate", "tol", "steps", "other_steps", "ok"}
GUARD_HISTORY_MAX = 0.0  # largest estimate / tol ratio seen since reset_guard()


def reset_guard():
    global GUARD_HISTORY_MAX
    GUARD_LAST.clear()
    GUARD_HISTORY_MAX = 0.0


def guard_track(diff, scale, meta):
    """diff: 0-dim float32 device tensor = max |x_S - x_S'| of a check, scale: 0-dim = max |x_S| (both on the CURRENT stream); meta:
    {"name", "tol", "factor", "steps", "other_steps", "action", "what"} -- estimate = factor * diff is compared with
    tol * (1 + scale), i.e. torchdiffeq's  atol + rtol |x|  with atol = rtol = tol (what the reference sets: flow.py:96-99,
    latent_ode_model.py:83), when the copy has arrived."""
    _guard.poll_all()
    _guard.post(None, torch.stack([diff.reshape(()), scale.reshape(())]), meta)      # one ring for all streams: key None


def _guard_report(records):
    import math
    import warnings
    global GUARD_HISTORY_MAX
    failed = []
    for (d, xmax), meta in records:
        est = meta["factor"] * d
        bound = meta["tol"] * (1.0 + xmax) if math.isfinite(xmax) else meta["tol"]
        ok = math.isfinite(est) and est <= bound
        GUARD_LAST[meta["name"]] = {"diff": d, "estimate": est, "tol": meta["tol"], "solution_absmax": xmax, "bound": bound, "steps": meta["steps"],
                                    "other_steps": meta["other_steps"], "ok": ok}
        GUARD_HISTORY_MAX = max(GUARD_HISTORY_MAX, est / bound if math.isfinite(est) else float("inf"))
        if not ok:
            msg = ("%s: RK4 with %d steps is not converged to the tolerance asked for: max |x_%d - x_%d| = %.3e on the checked subsample -> "
                   "error estimate %.3e > %.3e = check_tol %.1e x (1 + max |x| %.2f).  Raise the step count (CaSPR.calibrate_rk4_steps picks "
                   "it by step doubling) or the tolerance." % (meta["what"], meta["steps"], meta["steps"], meta["other_steps"], d, est, bound,
                                                              meta["tol"], xmax))
            if meta["action"] == "warn":
                warnings.warn(msg, RuntimeWarning, stacklevel=5)      # the caller of guard_track / check_deferred_errors: above poll_all, poll and this
            else:
                failed.append(msg)
    if failed:
        raise CasprAccuracyError("; ".join(failed))


_guard = _Deferred(_guard_report)


def latent_rk4(z0, times, steps, wts, team=None):
    """Fixed-step RK4 of the latent dynamics (latent_ode_model.py:45-70): z0 (B,D) (rows may be a column
    slice of a wider tensor); wts = [PackedWeight0, b0, PackedWeight1, b1, PackedWeight2, b2, PackedWeight3, b3].  -> (B,Tu,D).
    team: True / False forces the 32-workgroup team kernel / the single-workgroup kernel (None: LATENT_TEAM where the shape allows).
    Same values up to the re-association of the layer sums (tests: <= 5e-6)."""
    _chk_f32(times, *[w for w in wts[1::2]])
    if not z0.is_cuda or z0.dtype != torch.float32 or z0.dim() != 2 or z0.stride(1) != 1:
        raise ValueError("latent_rk4: z0 must be a float32 GPU (B,D) tensor with unit column stride")
    B = z0.shape[0]
    D, H = wts[0].cin, wts[0].cout
    if z0.shape[1] != D:
        raise ValueError("latent_rk4: z0 has %d columns, the dynamics net expects %d" % (z0.shape[1], D))
    Tu = times.shape[0]
    out = torch.empty(B, Tu, D, device=z0.device, dtype=torch.float32)
    ptrs = [_p(w.data) if isinstance(w, PackedWeight) else _p(w) for w in wts]
    L = _lib.load()
    if (LATENT_TEAM if team is None else team) and H == 512 and D <= 64 and B <= 64:
        # 32 workgroups per 16 sequences with LDS-resident weights (csrc/ode.hip): the serial chain runs ~3x faster
        with _team.on(z0.device) as status:
            with timed("latent_rk4"):
                ws = _team_workspace(L.caspr_latent_team_ws_bytes(B), z0.device)
                _lib.check(L.caspr_latent_rk4_team_f32(_p(z0), z0.stride(0), _p(times), B, Tu, D, H, int(steps), *ptrs, _p(out), _p(ws), ws.numel(),
                                                       _stream()), "caspr_latent_rk4_team_f32")
            status.post(_team_words(ws, B))
        return out
    with timed("latent_rk4"):
        _lib.check(L.caspr_latent_rk4_f32(_p(z0), z0.stride(0), _p(times), B, Tu, D, H, int(steps), *ptrs, _p(out), _stream()), "caspr_latent_rk4_f32")
    return out


LATENT_DP5_TRACE_HEAD, LATENT_DP5_TRACE_ROW = 8, 4      # include/caspr_hip.h: the trace layout of caspr_latent_dopri5_f32
# The adaptive latent solve reports a used-up attempt budget through its `finished` words (B,), posted with max_attempts.
def _latent_dp5_report(records):
    for words, budget in records:
        if not all(words):
            if isinstance(budget, tuple):        # the taping launch (train_ops.latent_dopri5_tape): (max_attempts, max_steps)
                raise _lib.CasprHipError("caspr_latent_dopri5_tape_f32 (code %d, CASPR_ENOCONV): %d of %d sequences had not reached the last time stamp after "
                                         "max_attempts = %d attempts or max_steps = %d accepted (taped) steps; the rows of the stamps they did not reach "
                                         "hold NaN, and so will their dL/dz0 rows.  Raise LatentODE.train_max_steps (the tape's capacity), max_attempts "
                                         "or the tolerance" % ((-4, words.count(0), len(words)) + budget))
            raise _lib.CasprHipError("caspr_latent_dopri5_f32 (code %d, CASPR_ENOCONV): %d of %d sequences had not reached the last time stamp after "
                                     "max_attempts = %d attempts; the rows of the stamps they did not reach hold NaN.  Raise max_attempts or the "
                                     "tolerance" % (-4, words.count(0), len(words), budget))


_latent_dp5 = _Deferred(_latent_dp5_report)


def _latent_dp5_args(who, z0, times, rtol, atol, wts, max_attempts):
    """The argument checks of the adaptive latent solve, shared with its taping launch (train_ops.latent_dopri5_tape)
    -> (B, D, H, rtol, atol, max_attempts)."""
    _chk_f32(times, *[w for w in wts[1::2]])
    if not z0.is_cuda or z0.dtype != torch.float32 or z0.dim() != 2 or z0.stride(1) != 1:
        raise ValueError("%s: z0 must be a float32 GPU (B,D) tensor with unit column stride" % who)
    _on_current_device(z0)
    B = z0.shape[0]
    D, H = wts[0].cin, wts[0].cout
    if z0.shape[1] != D:
        raise ValueError("%s: z0 has %d columns, the dynamics net expects %d" % (who, z0.shape[1], D))
    if times.dim() != 1 or times.shape[0] < 1 or B < 1:
        raise ValueError("%s: times must be a non-empty (Tu,) tensor and z0 hold at least one sequence" % who)
    rtol, atol, max_attempts = float(rtol), float(atol), int(max_attempts)
    if not (0 < rtol < float("inf") and 0 < atol < float("inf")):
        raise ValueError("%s: rtol and atol must be positive and finite, got %r / %r" % (who, rtol, atol))
    if max_attempts < 1:
        raise ValueError("%s: max_attempts must be positive, got %d" % (who, max_attempts))
    return B, D, H, rtol, atol, max_attempts


def latent_dopri5(z0, times, rtol, atol, wts, max_attempts=1000, return_trace=False):
    """Adaptive Dormand-Prince 5(4) solve of the latent dynamics to a tolerance (latent_ode_model.py:45-70 as the reference runs it:
    torchdiffeq's dopri5), error control PER SEQUENCE, the whole solve in one launch with the step control on the device
    (csrc/ode_latent_dp5.hip).  z0, times, wts as latent_rk4; times ascending, repeats allowed.  -> (B,Tu,D); with return_trace a dict
    is appended: "d0", "d1", "d2", "h0", "dt0" (B,), "attempts" (B, max_attempts, 4) rows [t, dt, ratio, accepted], "accepted",
    "rejected", "nfe" (B,) int32 -- all on the device.
    Never synchronises and runs under stream capture.  A sequence that has not reached the last stamp after max_attempts attempts
    leaves NaN in the rows it did not reach; CasprHipError is raised by the next solve on the stream or by check_deferred_errors()
    (not tracked under capture, as latent_rk4)."""
    B, D, H, rtol, atol, max_attempts = _latent_dp5_args("latent_dopri5", z0, times, rtol, atol, wts, max_attempts)
    if torch.is_grad_enabled() and (z0.requires_grad or times.requires_grad):
        raise ValueError("latent_dopri5: no gradient through the adaptive solve (training keeps RK4; config.train_latent_dopri5 trains through it "
                         "on LatentODE(method='dopri5'))")
    Tu = times.shape[0]
    out = torch.empty(B, Tu, D, device=z0.device, dtype=torch.float32)
    trace = torch.empty(B, LATENT_DP5_TRACE_HEAD + LATENT_DP5_TRACE_ROW * max_attempts, device=z0.device, dtype=torch.float32) if return_trace else None
    counters = torch.empty(B, 4, device=z0.device, dtype=torch.int32)
    ptrs = [_p(w.data) if isinstance(w, PackedWeight) else _p(w) for w in wts]
    with _latent_dp5.on(z0.device) as status:
        with timed("latent_dopri5"):
            _lib.check(_lib.load().caspr_latent_dopri5_f32(_p(z0), z0.stride(0), _p(times), B, Tu, D, H, rtol, atol, max_attempts, *ptrs, _p(out),
                                                           _p(trace), _p(counters), _stream()), "caspr_latent_dopri5_f32")
        status.post(counters[:, 3], max_attempts)
    if return_trace:
        return out, {"d0": trace[:, 0], "d1": trace[:, 1], "d2": trace[:, 2], "h0": trace[:, 3], "dt0": trace[:, 4],
                     "attempts": trace[:, LATENT_DP5_TRACE_HEAD:].view(B, max_attempts, LATENT_DP5_TRACE_ROW),
                     "accepted": counters[:, 0], "rejected": counters[:, 1], "nfe": counters[:, 2]}
    return out


def pack_cnf_x6(w):
    """(512,512) hidden-layer weight of the ODE function -> the three-plane bf16 pack of caspr_cnf_rk4_x6_f32."""
    _chk_f32(w)
    if tuple(w.shape) != (512, 512):
        raise ValueError("pack_cnf_x6: expected a (512,512) weight, got %s" % (tuple(w.shape),))
    out = torch.empty(_lib.load().caspr_cnf_x6_packed_bytes(), device=w.device, dtype=torch.uint8)
    _lib.check(_lib.load().caspr_pack_weight_cnf_x6(_p(w), w.stride(0), _p(out), _stream()), "caspr_pack_weight_cnf_x6")
    return out


CNF_NARROW = 2        # include/caspr_hip.h: CASPR_CNF_NARROW
BEFORE_CNF_LAUNCH = None      # one-shot callable run between a CNF block's hyper-network conv and its launch (models/cnf.py: CNF.integrate);
                              # reconstruct() hands the encoder's deferred T-NOCS regression to it


def pack_cnf_h3(w):
    """(512,512) hidden-layer weight of the ODE function -> the two-plane f16 pack of caspr_cnf_rk4_h3_f32 (cnf_split = "f16x3"); the
    layer's power-of-two scale is found on the device and stored behind the planes: no host synchronisation, capturable."""
    _chk_f32(w)
    if tuple(w.shape) != (512, 512):
        raise ValueError("pack_cnf_h3: expected a (512,512) weight, got %s" % (tuple(w.shape),))
    out = torch.empty(_lib.load().caspr_cnf_h3_packed_bytes(), device=w.device, dtype=torch.uint8)
    _lib.check(_lib.load().caspr_pack_weight_cnf_h3(_p(w), w.stride(0), _p(out), _stream()), "caspr_pack_weight_cnf_h3")
    return out


# The f16x3 solve's range guard (csrc/ode_f16x3w.hip): a hidden activation that is not finite in f16 after the 2^4 scale poisons its
# point with NaN and sets the launch's status word (zeroed by the C entry in front of every launch, copied out behind it).
def _cnf_h3_report(records):
    bits = 0                                         # 1: cnf_rk4_h3w_kernel, 2: cnf_dp5_h3w_kernel, 4: cnf_sample_tape_h3w_kernel (include/caspr_hip.h)
    for words, _ in records:
        bits |= words[0]
    if bits:
        # one error for everything that has arrived: each kernel whose guard tripped is named with its own remedy
        what = []
        if bits & 1:
            what.append(_CNF_ENTRY["h3"]["rk4"] + " (the fixed-step sampling solve): the samples of the affected points were set to NaN.  Remedy: "
                        "cnf_split=\"bf16x6\" (caspr_amd.config.config.cnf_split / caspr_amd.ops.CNF_SPLIT)")
        if bits & 2:
            what.append(_CNF_ENTRY["h3"]["dopri5"] + " (the adaptive solve): the affected FRAMES were retired with NaN in all of their samples.  Remedy: "
                        "cnf_dp5_split=\"bf16x6\" (caspr_amd.config.config.cnf_dp5_split / caspr_amd.ops.CNF_DP5_SPLIT)")
        if bits & 4:
            what.append(_CNF_ENTRY["h3"]["tape"] + " (the sampling solve with the tape of the differentiable decode): the samples of the affected "
                        "points were set to NaN, their tape rows are not to be trusted.  Remedy: "
                        "cnf_tape_split=\"bf16x6\" (caspr_amd.config.config.cnf_tape_split / caspr_amd.ops.CNF_TAPE_SPLIT)")
        raise _lib.CasprHipError("the range guard of the f16x3 point-CNF solve tripped: a hidden activation of the ODE function reached 4095, which is "
                                 "not finite in f16 after the kernel's 2^4 prescale.  " + ";  ".join(what) + ": the six-product bf16 kernel, which has "
                                 "f32's exponent range")


_cnf_h3 = _DeferredWord(_cnf_h3_report)


CNF_MAX_TABLE_STEPS = 4096      # include/caspr_hip.h: the largest max_steps of the *_frames_* entries


def _chk_frame_table(name, t, BT, device):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError("cnf_rk4: %s must be an int32 tensor on the GPU, got %s" % (name, t.device if torch.is_tensor(t) else type(t).__name__))
    if t.device != device:
        raise ValueError("cnf_rk4: %s lives on %s, the samples on %s" % (name, t.device, device))
    if t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] != BT or not t.is_contiguous():
        raise ValueError("cnf_rk4: %s must be a contiguous int32 (BT,) tensor with BT = %d, got %s %s" % (name, BT, t.dtype, tuple(t.shape)))


CNF_HIDDEN = 512                          # the ODE function the solve kernels are built for: 3-512-512-512-3
CNF_HYPER = 2 * (3 * CNF_HIDDEN + 3)      # the floats of a hyper row, and of tcol, they read: [gate l0..l3 | bias l0..l3]
CNF_H3_POINTS = 128                       # the f16x3 workgroup's point count

# The route table of the point CNF ("The point CNF's route table"): the kernel family that takes a solve, and the entry of
# each route per kind of call.  An absent cell: the kernel does not exist.  A new form of a solve is one cell here.
_CNF_ENTRY = {
    "f32": {"rk4": "caspr_cnf_rk4_f32"},
    "x6": {"rk4": "caspr_cnf_rk4_x6_f32", "frames": "caspr_cnf_rk4_x6_frames_f32", "dopri5": "caspr_cnf_dopri5_f32",
           "train_fwd": "caspr_cnf_train_fwd_f32", "train_fwd_reg": "caspr_cnf_block_reg_fwd_f32", "tape": "caspr_cnf_sample_tape_f32",
           "tape_frames": "caspr_cnf_sample_tape_frames_f32"},
    "h3": {"rk4": "caspr_cnf_rk4_h3_f32", "frames": "caspr_cnf_rk4_h3_frames_f32", "dopri5": "caspr_cnf_dopri5_h3_f32",
           "tape": "caspr_cnf_sample_tape_h3_f32", "tape_frames": "caspr_cnf_sample_tape_h3_frames_f32"},
}
_CNF_DP5_WS_BYTES = {"x6": "caspr_cnf_dopri5_ws_bytes", "h3": "caspr_cnf_dopri5_h3_ws_bytes"}


def _cnf_route(n, x6, h3, e=None, narrow=False):
    """The kernel family that takes a solve of n points a frame: "f32" | "x6" (bf16x6, 64 points a workgroup) | "h3" (f16x3, 128 points),
    from the packs that were handed over (x6: both of w1x / w2x; h3: both of w1h / w2h), the direction (e: the Hutchinson noise of a
    solve with the divergence) and the narrow flag.  cnf_rk4, cnf_dopri5, the f16x3 tape wrappers (as their acceptance rule) and
    train/flow_grad.py: _sample_tape_route (which adds its switch) all ask here.  Seven rules that read like accidents and are not:
      1. the f16x3 route needs BOTH h3 packs, no e, not narrow (cnf_rk4 alone has the flag) and n >= 128; any other call goes where
         it would go without them, silently, and the h3 packs' size and dtype are looked at only when the route is taken;
      2. a step table requires the x6 packs even when the f16x3 kernel then takes the call (cnf_rk4 checks that, not this function);
      3. CNF_NARROW is or-ed into the plain x6 entry's flags only when e is None, into the frames entry's whenever narrow;
      4. only one of w1x / w2x is no x6: the call falls through to the f32 route, which reads w1p.data / w2p.data;
      5. cnf_rk4 and cnf_dopri5 leave the hidden width to C, the training wrappers check the 3-512-512-512-3 shape in Python; both pass
         w0's rows as H (_cnf_head), which is 512 behind that check;
      6. the x6 tape wrappers do not look at their packs' dtype, the h3 ones do (_cnf_packs_ok);
      7. cnf_dopri5 sizes its workspace inside the status scope and in front of the timer (_cnf_launch: a callable `after`), and on every
         h3 launch the timer closes before the status word is posted."""
    if h3 and e is None and not narrow and n >= CNF_H3_POINTS:
        return "h3"
    return "x6" if x6 else "f32"


def cnf_dp5_kernel(route, divergence):
    """The name of the Dormand-Prince kernel a route runs (the "kernel" item of cnf_dopri5's trace dict)."""
    return "cnf_dp5_h3w_kernel" if route == "h3" else "cnf_dp5_kernel<%s>" % ("true" if divergence else "false")


def _cnf_packs_ok(route, w1, w2):
    """Whether w1 / w2 are the route's two hidden-layer packs (pack_cnf_h3 by size and dtype, pack_cnf_x6 by size)."""
    if route == "h3":
        nbytes = _lib.load().caspr_cnf_h3_packed_bytes()
        return all(w is not None and w.numel() == nbytes and w.dtype == torch.uint8 for w in (w1, w2))
    return w1 is not None and w2 is not None and w1.numel() == _lib.load().caspr_cnf_x6_packed_bytes() and w2.numel() == w1.numel()


def _chk_cnf(who, y, hyper, e=None, logp=None, mbn_in=None, mbn_out=None, train=None, route="x6", steps=None):
    """The argument checks of the CNF front-end (the dtype, device and contiguity of the f32 tensors are _chk_f32's) -> (BT, n).
    train: None for cnf_rk4 / cnf_dopri5; (tcol, w0, b0, w1, b1, w2, b2, w3, b3, t_end) for a wrapper of the training tier, which checks
    what those two leave to C, its packs w1 / w2 of `route`, and the device scalar t_end (with steps > 0 when `steps` is given)."""
    if y.dim() != 3 or y.shape[2] != 3:
        raise ValueError("%s: y must be (BT,n,3), got %s" % (who, tuple(y.shape)))
    BT, n, _ = y.shape
    if train is None:
        if hyper.dim() != 2 or hyper.shape[0] != BT:
            raise ValueError("%s: hyper has %s rows for %d frames" % (who, tuple(hyper.shape), BT))
        if (e is None) != (logp is None):
            raise ValueError("%s: the Hutchinson noise e and the initial log-density come together" % who)
    if e is not None and (tuple(e.shape) != tuple(y.shape) or tuple(logp.shape) != (BT, n, 1)):
        raise ValueError("%s: e %s / logp %s do not match y %s" % (who, tuple(e.shape), tuple(logp.shape), tuple(y.shape)))
    for name, m_ in (("mbn_in", mbn_in), ("mbn_out", mbn_out)):
        if m_ is not None and m_.numel() != 12:
            raise ValueError("%s: %s must hold 12 floats [weight | bias | running_mean | running_var]" % (who, name))
    if train is not None:
        tcol, w0, b0, w1, b1, w2, b2, w3, b3, t_end = train
        if _cnf_route(n, True, route == "h3") != route:
            raise ValueError("%s: n = %d is below the %d-point workgroup of the f16x3 kernel: %s is the wrapper for it"
                             % (who, n, CNF_H3_POINTS, who.replace("_h3", "")))
        if hyper.dim() != 2 or hyper.shape[0] != BT or hyper.stride(1) != 1 or hyper.shape[1] < CNF_HYPER or tcol.numel() < CNF_HYPER:
            raise ValueError("%s: hyper must be (BT, >= %d) rows and tcol hold %d floats, got %s / %s"
                             % (who, CNF_HYPER, CNF_HYPER, tuple(hyper.shape), tuple(tcol.shape)))
        if (tuple(w0.shape) != (CNF_HIDDEN, 3) or tuple(w3.shape) != (3, CNF_HIDDEN) or b0.numel() != CNF_HIDDEN or b1.numel() != CNF_HIDDEN
                or b2.numel() != CNF_HIDDEN or b3.numel() != 3):
            raise ValueError("%s: the kernel is built for the 3-%d-%d-%d-3 ODE function" % (who, CNF_HIDDEN, CNF_HIDDEN, CNF_HIDDEN))
        if not _cnf_packs_ok(route, w1, w2):
            raise ValueError("%s: the %s (ops.pack_cnf_%s) are required"
                             % (who, "f16x3 weight packs w1h / w2h" if route == "h3" else "bf16x6 weight packs w1x / w2x", route))
        if t_end.numel() != 1 or not t_end.is_cuda or (steps is not None and steps <= 0):
            raise ValueError("%s: t_end must be a one-element device tensor%s" % (who, "" if steps is None else " and steps positive"))
    return BT, n


def _cnf_step_table(who, y, steps, order, max_steps, tape=None):
    """The checks of a per-frame step table (steps, order: (BT,) int32 on y's device; max_steps in 1..4096, None = 4096) -> max_steps, and
    with tape = (ys, ka), what a *_frames tape wrapper was handed or None: -> max_steps, ys, ka, checked or allocated."""
    BT, n, _ = y.shape
    _chk_frame_table("steps", steps, BT, y.device)
    if order is not None:
        _chk_frame_table("order", order, BT, y.device)
    max_steps = CNF_MAX_TABLE_STEPS if max_steps is None else int(max_steps)
    if not 1 <= max_steps <= CNF_MAX_TABLE_STEPS:
        raise ValueError("%s: max_steps must lie in 1..%d, got %d" % (who, CNF_MAX_TABLE_STEPS, max_steps))
    if tape is None:
        return max_steps
    shape = (max_steps, 4, BT, n, 3)           # max_steps is the kernel's clamp AND the tape's step rows: they must be the same number
    for name, t in zip(("ys", "ka"), tape):
        if t is not None and (tuple(t.shape) != shape or t.device != y.device or not t.is_contiguous()):
            raise ValueError("%s: %s must be a contiguous %s tensor on %s, got %s on %s" % (who, name, shape, y.device, tuple(t.shape), t.device))
    return (max_steps, *(torch.empty(shape, device=y.device, dtype=torch.float32) if t is None else t for t in tape))


def _cnf_head(y, hyper, tcol, w0, b0, w1, b1, w2, b2, w3, b3):
    """The thirteen arguments every CNF entry begins with; w1 / w2: the hidden layers' weights in the route's form."""
    return (_p(y), _p(hyper), hyper.shape[1], _p(tcol), _p(w0), _p(b0), _p(w1), _p(b1), _p(w2), _p(b2), _p(w3), _p(b3), w0.shape[0])


@contextlib.contextmanager
def _cnf_h3_launch(device):
    """with _cnf_h3_launch(device) as word: <launch an f16x3 solve that reports into word>  -- reports an earlier launch's trip first and
    posts the word behind this one (not under stream capture)."""
    with _cnf_h3.on(device) as status:
        word = status.word
        yield _p(word)
        status.post(word)


def _cnf_launch(route, kind, timer, device, head, before, after):
    """The one launch site: entry _CNF_ENTRY[route][kind] on (head, before[, the f16x3 status word], after, stream) under timed(timer).
    The word's place is the C ABI's and differs by kind -- behind mbn_out (rk4, frames, dopri5), behind the step arguments (tape,
    tape_frames) -- always in front of the result: the caller cuts its arguments there.  A callable `after` is called inside the status
    scope and in front of the timer (cnf_dopri5 sizes its workspace there)."""
    name = _CNF_ENTRY[route][kind]
    entry = getattr(_lib.load(), name)
    with _cnf_h3_launch(device) if route == "h3" else contextlib.nullcontext() as word:
        after = after() if callable(after) else after
        with timed(timer):
            _lib.check(entry(*head, *before, *(() if word is None else (word,)), *after, _stream()), name)


def cnf_rk4(y, hyper, tcol, w0, b0, w1p, b1, w2p, b2, w3, b3, t_end, steps, reverse, mbn_in=None, mbn_out=None,
            e=None, logp=None, w1x=None, w2x=None, narrow=False, w1h=None, w2h=None, order=None, max_steps=None, out=None):
    """Fixed-step RK4 of one CNF block (cnf.py:70-128).  y (BT,n,3); hyper (BT,ldh).  Returns x or (x, logp).
    w1x / w2x (pack_cnf_x6): when given, the bf16x6 kernel runs the solve (with or without the divergence).
    narrow: the 64-point sampling kernel (a launch that does not fill the chip lasts as long as one workgroup: the accuracy guard).
    w1h / w2h (pack_cnf_h3): when both are given and the call is a plain sampling solve (e is None, not narrow, n >= 128), the f16x3
    kernel runs it (three f16 products per f32 product); every other call goes where it goes without them.  Its range guard reports
    through check_deferred_errors (not tracked under stream capture, as latent_rk4).
    steps may be a (BT,) int32 GPU tensor: a step count PER FRAME (plain sampling calls with the packs w1x / w2x only; routed as
    above).  Frame f takes min(max(steps[f], 0), max_steps) steps (max_steps in 1..4096, default 4096); 0 skips the frame: its rows of
    the result are left as allocated (uninitialised).  order: (BT,) int32 GPU tensor, the launch order of the frames (a permutation;
    the result does not depend on it).  Frame f's rows equal, bit for bit, a call on that frame alone with its count.  out (with a
    table only): a contiguous f32 tensor of y's shape to write into -- the rows of skipped frames keep what it holds."""
    _chk_f32(y, hyper, tcol, w0, b0, b1, b2, w3, b3, mbn_in, mbn_out, e, logp)
    BT, n = _chk_cnf("cnf_rk4", y, hyper, e, logp, mbn_in, mbn_out)
    x6 = w1x is not None and w2x is not None
    table = torch.is_tensor(steps)
    if table:
        if e is not None or logp is not None:
            raise ValueError("cnf_rk4: a step table is for the sampling direction only (no e / logp)")
        if not x6:
            raise ValueError("cnf_rk4: a step table needs the bf16x6 weight packs w1x / w2x (pack_cnf_x6)")
        max_steps = _cnf_step_table("cnf_rk4", y, steps, order, max_steps)
        if out is not None:
            _chk_f32(out)
            if tuple(out.shape) != tuple(y.shape) or out.device != y.device:
                raise ValueError("cnf_rk4: out %s on %s does not match y %s on %s" % (tuple(out.shape), out.device, tuple(y.shape), y.device))
    elif order is not None or max_steps is not None or out is not None:
        raise ValueError("cnf_rk4: order / max_steps / out come with a step table (steps as a (BT,) int32 tensor)")
    route = _cnf_route(n, x6, w1h is not None and w2h is not None, e, narrow)
    if route == "h3" and not _cnf_packs_ok(route, w1h, w2h):
        raise ValueError("cnf_rk4: w1h / w2h must be the packs of pack_cnf_h3")
    w1, w2 = (w1h, w2h) if route == "h3" else (w1x, w2x) if route == "x6" else (w1p.data, w2p.data)
    out = torch.empty_like(y) if out is None else out
    lp_out = torch.empty(BT, n, 1, device=y.device, dtype=torch.float32) if e is not None else None
    flags = int(bool(reverse)) | (CNF_NARROW if narrow and route == "x6" and (table or e is None) else 0)
    _cnf_launch(route, "frames" if table else "rk4", "cnf_rk4", y.device, _cnf_head(y, hyper, tcol, w0, b0, w1, b1, w2, b2, w3, b3),
                (float(t_end), *(() if table else (int(steps),)), flags, _p(mbn_in), _p(mbn_out)),
                (*(() if table or route == "h3" else (_p(e), _p(logp), _p(lp_out))), _p(out), BT, n,
                 *((_p(steps), max_steps, _p(order)) if table else ())))
    return out if e is None else (out, lp_out)


# The per-frame step controller (csrc/cnf_frame_steps.hip): a frame that still fails the criterion at the largest rung is CAPPED there.
# The count of capped frames is posted behind the pilot, with (S_max, tol).
def _steps_report(records):
    msgs = ["%d frame(s) capped at %d steps (tol %.1e)" % (words[0], s_max, tol) for words, (s_max, tol) in records if words[0]]
    if msgs:
        raise CasprAccuracyError("point CNF, per-frame step counts (cnf_steps=\"frame\"): " + "; ".join(msgs) + ": the step-halving estimate of "
                                 "these frames still exceeds tol x (1 + max |x|) at the largest count the controller may choose, and they were "
                                 "solved with it.  Raise cnf_steps_max (a power of two <= 256) or the tolerance")


_steps = _Deferred(_steps_report)


def cnf_steps_update(x_prev, x_cur, P, tol, safety, max_steps, steps, next_tab, capped, stats):
    """One update of the per-frame step controller after rung P (include/caspr_hip.h: caspr_cnf_steps_update_f32).  x_prev / x_cur
    (BT,g,3) f32: the pilot solutions at P/2 and P steps; steps (in-out, 0 = undecided), next_tab, capped (BT,) int32; stats (BT,4) f64."""
    _chk_f32(x_prev, x_cur)
    if x_prev.dim() != 3 or x_prev.shape[2] != 3 or tuple(x_cur.shape) != tuple(x_prev.shape):
        raise ValueError("cnf_steps_update: x_prev / x_cur must be (BT,g,3) of one shape, got %s / %s" % (tuple(x_prev.shape), tuple(x_cur.shape)))
    BT, g, _ = x_prev.shape
    for name, t in (("steps", steps), ("next_tab", next_tab), ("capped", capped)):
        _chk_frame_table(name, t, BT, x_prev.device)
    if stats.dtype != torch.float64 or tuple(stats.shape) != (BT, 4) or not stats.is_contiguous() or stats.device != x_prev.device:
        raise ValueError("cnf_steps_update: stats must be a contiguous float64 (BT,4) tensor on the samples' device")
    P, max_steps = int(P), int(max_steps)
    if max_steps < 2 or max_steps > 256 or max_steps & (max_steps - 1):
        raise ValueError("cnf_steps_update: max_steps must be a power of two in 2..256, got %d" % max_steps)
    if P < 2 or P > max_steps or P & (P - 1):
        raise ValueError("cnf_steps_update: the rung must be a power of two in 2..max_steps, got %d" % P)
    if not (0.0 <= float(tol) < float("inf") and 1.0 <= float(safety) < float("inf")):
        raise ValueError("cnf_steps_update: tol must be finite and >= 0, safety finite and >= 1, got %r / %r" % (tol, safety))
    _lib.check(_lib.load().caspr_cnf_steps_update_f32(_p(x_prev), _p(x_cur), BT, g, P, float(tol), float(safety), max_steps, _p(steps), _p(next_tab),
                                                      _p(capped), _p(stats), _stream()), "caspr_cnf_steps_update_f32")


def cnf_steps_order(steps):
    """(BT,) int32 step counts -> (BT,) int32: the stable permutation that sorts the frames by descending count (longest first)."""
    if not torch.is_tensor(steps) or steps.dim() != 1:
        raise ValueError("cnf_steps_order: steps must be a (BT,) int32 tensor on the GPU")
    _chk_frame_table("steps", steps, steps.shape[0], steps.device)
    if not 1 <= steps.shape[0] <= 65535:
        raise ValueError("cnf_steps_order: 1..65535 frames, got %d" % steps.shape[0])
    _on_current_device(steps)
    order = torch.empty_like(steps)
    _lib.check(_lib.load().caspr_cnf_steps_order(_p(steps), steps.shape[0], _p(order), _stream()), "caspr_cnf_steps_order")
    return order


def cnf_frame_steps(run_rung, BT, g, tol, safety=1.2, max_steps=64, device=None):
    """Choose an RK4 step count per frame on the device (csrc/cnf_frame_steps.hip): the pilot ladder 1, 2, 4, .., max_steps.
    run_rung(table) launches ONE rung -- the sampling solve of the g pilot points of every frame with the (BT,) int32 step table
    `table` (0 = skip the frame) -- and returns its (BT,g,3) result.  After every rung from 2 on the update kernel decides the frames
    whose Richardson estimate passes tol x (1 + max |x|) and doubles the others' table entry.  Every launch is enqueued
    unconditionally (a rung whose table is all zero is an empty launch); nothing is read by the host, so the ladder is capturable.
    -> (steps, order, info): steps (BT,) int32 in 2..max_steps, order (BT,) int32 = longest first, info = {"stats" (BT,4) f64
    [d, bound, prediction, deciding rung], "capped" (BT,) int32, "pilot_steps" (BT,) int32 = the RK4 steps the pilot spent on the frame,
    1 + 2 + .. + its deciding rung}.  A capped frame is reported through check_deferred_errors (not tracked under stream capture)."""
    BT, g, max_steps = int(BT), int(g), int(max_steps)
    if max_steps < 2 or max_steps > 256 or max_steps & (max_steps - 1):
        raise ValueError("cnf_frame_steps: max_steps must be a power of two in 2..256, got %d" % max_steps)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    steps = torch.zeros(BT, device=dev, dtype=torch.int32)
    capped = torch.zeros(BT, device=dev, dtype=torch.int32)
    stats = torch.zeros(BT, 4, device=dev, dtype=torch.float64)
    x_prev = run_rung(torch.ones(BT, device=dev, dtype=torch.int32))
    tab, P = torch.full((BT,), 2, device=dev, dtype=torch.int32), 2
    while P <= max_steps:
        x_cur = run_rung(tab)
        nxt = torch.empty_like(tab)
        cnf_steps_update(x_prev, x_cur, P, tol, safety, max_steps, steps, nxt, capped, stats)
        x_prev, tab, P = x_cur, nxt, 2 * P
    order = cnf_steps_order(steps)
    with _steps.on(dev) as status:
        if status.live:                              # (no reduction in a captured graph either)
            status.post(capped.sum(dtype=torch.int32).reshape(1), (max_steps, float(tol)))
    pilot = (2 * stats[:, 3] - 1).to(torch.int32)
    return steps, order, {"stats": stats, "capped": capped, "pilot_steps": pilot}


DP5_TRACE_HEAD, DP5_TRACE_ROW = 8, 5      # include/caspr_hip.h: the trace layout of caspr_cnf_dopri5_f32


def cnf_dopri5(y, hyper, tcol, w0, b0, b1, b2, w3, b3, w1x, w2x, t_end, rtol, atol, reverse, mbn_in=None, mbn_out=None,
               e=None, logp=None, max_attempts=1000, return_trace=False, w1h=None, w2h=None):
    """Adaptive Dormand-Prince 5(4) solve of one CNF block to a tolerance (cnf.py:96-118: what the reference runs on every call), error
    control PER FRAME (csrc/ode_dp5.hip).  Arguments as cnf_rk4 with the bf16x6 packs w1x / w2x (pack_cnf_x6) required.  Returns x or
    (x, logp); with return_trace a dict is appended: "d0", "d1", "d2", "h0", "dt0" (BT,), "attempts" (BT, max_attempts, 5) rows
    [t, dt, ratio x, ratio logp, accepted], "accepted", "rejected", "nfe" (BT,) int32 -- all on the device.
    w1h / w2h (pack_cnf_h3): when both are given and the call is a plain sampling solve (e is None, n >= 128), the f16x3 kernel runs it
    (csrc/ode_dp5_f16x3w.hip, three f16 products per f32 product); every other call goes where it goes without them.  Its range guard
    retires a frame with NaN in all of its rows and reports through check_deferred_errors.  A call that hands the packs over gets two
    more items in its trace dict, whichever kernel ran: "kernel", the kernel's name (a str, the only item that is not a tensor), and
    "finished" (BT,) int32 (1: reached t_end; 3: retired by the range guard).  Without the packs the dict is what it always was.
    The host reads one device word per attempt: not usable under stream capture or with autograd (training keeps RK4).
    Raises CasprHipError when a frame has not reached t_end after max_attempts attempts."""
    _chk_f32(y, hyper, tcol, w0, b0, b1, b2, w3, b3, mbn_in, mbn_out, e, logp)
    BT, n = _chk_cnf("cnf_dopri5", y, hyper, e, logp, mbn_in, mbn_out)
    if w1x is None or w2x is None:
        raise ValueError("cnf_dopri5: the bf16x6 weight packs w1x / w2x (pack_cnf_x6) are required")
    rtol, atol, max_attempts = float(rtol), float(atol), int(max_attempts)
    if not (0 < rtol < float("inf") and 0 < atol < float("inf")):
        raise ValueError("cnf_dopri5: rtol and atol must be positive and finite, got %r / %r" % (rtol, atol))
    if not (0 < float(t_end) < float("inf")):
        raise ValueError("cnf_dopri5: t_end must be positive and finite, got %r" % (t_end,))
    if max_attempts < 1:
        raise ValueError("cnf_dopri5: max_attempts must be positive, got %d" % max_attempts)
    if torch.is_grad_enabled() and any(t_ is not None and t_.requires_grad for t_ in (y, hyper, e, logp)):
        raise ValueError("cnf_dopri5: no gradient through the adaptive solve (training keeps RK4)")
    if torch.cuda.is_current_stream_capturing():
        raise ValueError("cnf_dopri5: the host loop reads the device after every attempt and cannot run under stream capture")
    out = torch.empty_like(y)
    lp_out = torch.empty(BT, n, 1, device=y.device, dtype=torch.float32) if e is not None else None
    trace = torch.empty(BT, DP5_TRACE_HEAD + DP5_TRACE_ROW * max_attempts, device=y.device, dtype=torch.float32)
    counters = torch.empty(BT, 4, device=y.device, dtype=torch.int32)
    route = _cnf_route(n, True, w1h is not None and w2h is not None, e)
    if route == "h3" and not _cnf_packs_ok(route, w1h, w2h):
        raise ValueError("cnf_dopri5: w1h / w2h must be the packs of pack_cnf_h3")
    w1, w2 = (w1h, w2h) if route == "h3" else (w1x, w2x)

    def after():
        ws = _workspace(getattr(_lib.load(), _CNF_DP5_WS_BYTES[route])(BT, n, max_attempts), y.device)
        return (*(() if route == "h3" else (_p(e), _p(logp), _p(lp_out))), _p(out), BT, n, _p(ws), ws.numel(), _p(trace), _p(counters))

    _cnf_launch(route, "dopri5", "cnf_dopri5", y.device, _cnf_head(y, hyper, tcol, w0, b0, w1, b1, w2, b2, w3, b3),
                (float(t_end), rtol, atol, max_attempts, int(bool(reverse)), _p(mbn_in), _p(mbn_out)), after)
    res = (out,) if e is None else (out, lp_out)
    if return_trace:
        info = {"d0": trace[:, 0], "d1": trace[:, 1], "d2": trace[:, 2], "h0": trace[:, 3], "dt0": trace[:, 4],
                "attempts": trace[:, DP5_TRACE_HEAD:].view(BT, max_attempts, DP5_TRACE_ROW),
                "accepted": counters[:, 0], "rejected": counters[:, 1], "nfe": counters[:, 2]}
        if w1h is not None and w2h is not None:
            info["finished"] = counters[:, 3]
            info["kernel"] = cnf_dp5_kernel(route, e is not None)
        res = res + (info,)
    return res[0] if len(res) == 1 else res


def chamfer_distance(p, q, return_indices=False):
    """tk3dv `ChamferDistance()(pred, gt)` (evaluations.py:40): -> dist1 (B,n), dist2 (B,m) squared NN distances.
    return_indices: -> (dist1, dist2, idx1 (B,n), idx2 (B,m)) from caspr_chamfer_idx_f32: the same distances bit for bit and the
    smallest index attaining each (int32; -1 with dist = +inf where no candidate is at a finite distance).  No gradient is
    recorded here: caspr_amd.losses.chamfer_distance is the differentiable form."""
    _chk_f32(p, q)
    B, n, _ = p.shape
    m = q.shape[1]
    d1 = torch.empty(B, n, device=p.device, dtype=torch.float32)
    d2 = torch.empty(B, m, device=p.device, dtype=torch.float32)
    if return_indices:
        if p.dim() != 3 or q.dim() != 3 or p.shape[2] != 3 or q.shape[2] != 3 or q.shape[0] != B:
            raise ValueError("chamfer_distance: p (F,n,3) and q (F,m,3) must agree on F, got %s and %s" % (tuple(p.shape), tuple(q.shape)))
        i1 = torch.empty(B, n, device=p.device, dtype=torch.int32)
        i2 = torch.empty(B, m, device=p.device, dtype=torch.int32)
        _lib.check(_lib.load().caspr_chamfer_idx_f32(_p(p), _p(q), B, n, m, _p(d1), _p(d2), _p(i1), _p(i2), _stream()), "caspr_chamfer_idx_f32")
        return d1, d2, i1, i2
    _lib.check(_lib.load().caspr_chamfer_f32(_p(p), _p(q), B, n, m, _p(d1), _p(d2), _stream()), "caspr_chamfer_f32")
    return d1, d2


EMD_ROUTE = _cfg.emd_route           # "frame": one workgroup per frame (caspr_emd_f32 / caspr_emd_tape_f32); "rows": the rows of every frame over the grid
                                     # (caspr_emd_rows_f32: the same ratios bit for bit, the cost summed in another order); opt-in, csrc/emd.hip
EMD_ROUTES = ("frame", "rows")


def earth_mover_distance(xyz1, xyz2, transpose=True, return_tape=False, route=None):
    """`utils.emd.earth_mover_distance` (emd.py:24-45): approximate EMD cost per cloud pair, (b,3,n) inputs when
    `transpose` (as the reference), else (b,n,3).  -> (b,) ; evaluations.py:46 divides by the point count.
    return_tape: -> (cost, tape (b,10,n+m)) from caspr_emd_tape_f32: the same cost bit for bit and the ten levels' ratioL (n) | ratioR (m),
    from which train_ops.emd_bwd rebuilds the match matrix.  No gradient is recorded here: caspr_amd.losses.earth_mover_distance is the
    differentiable form.
    route: None (ops.EMD_ROUTE), "frame" (one workgroup per frame: caspr_emd_f32 / caspr_emd_tape_f32) or "rows" (caspr_emd_rows_f32, with
    or without the tape: every frame's rows over the grid -- the same tape bit for bit, the cost within rounding of the other route's)."""
    if route is None:
        route = EMD_ROUTE
    if route not in EMD_ROUTES:
        raise ValueError("earth_mover_distance: route must be 'frame' or 'rows' (None: ops.EMD_ROUTE), got %r" % (route,))
    if xyz1.dim() == 2:
        xyz1 = xyz1.unsqueeze(0)
    if xyz2.dim() == 2:
        xyz2 = xyz2.unsqueeze(0)
    if transpose:
        xyz1, xyz2 = xyz1.transpose(1, 2), xyz2.transpose(1, 2)
    xyz1, xyz2 = xyz1.contiguous().float(), xyz2.contiguous().float()
    _chk_f32(xyz1, xyz2)
    B, n, _ = xyz1.shape
    m = xyz2.shape[1]
    cost = torch.empty(B, device=xyz1.device, dtype=torch.float32)
    L = _lib.load()
    rows = route == "rows"
    ws = _workspace(L.caspr_emd_rows_ws_bytes(B, n, m) if rows else L.caspr_emd_ws_bytes(B, n, m), xyz1.device)
    if return_tape:
        if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.shape[2] != 3 or xyz2.shape[2] != 3 or xyz2.shape[0] != B:
            raise ValueError("earth_mover_distance: xyz1 (b,n,3) and xyz2 (b,m,3) must agree on b, got %s and %s" % (tuple(xyz1.shape), tuple(xyz2.shape)))
        tape = torch.empty(B, 10, n + m, device=xyz1.device, dtype=torch.float32)
        assert tape.numel() * 4 == L.caspr_emd_tape_bytes(B, n, m)
        if rows:
            _lib.check(L.caspr_emd_rows_f32(_p(xyz1), _p(xyz2), B, n, m, _p(cost), _p(tape), _p(ws), ws.numel(), _stream()), "caspr_emd_rows_f32")
        else:
            _lib.check(L.caspr_emd_tape_f32(_p(xyz1), _p(xyz2), B, n, m, _p(cost), _p(tape), _p(ws), ws.numel(), _stream()), "caspr_emd_tape_f32")
        return cost, tape
    if rows:
        _lib.check(L.caspr_emd_rows_f32(_p(xyz1), _p(xyz2), B, n, m, _p(cost), None, _p(ws), ws.numel(), _stream()), "caspr_emd_rows_f32")
        return cost
    _lib.check(L.caspr_emd_f32(_p(xyz1), _p(xyz2), B, n, m, _p(cost), _p(ws), ws.numel(), _stream()), "caspr_emd_f32")
    return cost


EMD_EXACT_MAX_POINTS = 2048          # what the LDS of one workgroup holds (csrc/emd_exact.hip)
EMD_EXACT_BIDS_PER_POINT = 4096      # max_bids=None: 4096 n bids per frame


def earth_mover_distance_exact(xyz1, xyz2, transpose=True, eps=1e-6, max_bids=None, return_match=False):
    """The EXACT earth mover's distance between clouds of equal size: the cost of the optimal one-to-one assignment, by a forward auction
    with epsilon scaling in f64 (caspr_emd_exact_f32, csrc/emd_exact.hip; the reference has only the approximation of emd.py:11-12).
    Layouts of earth_mover_distance: (b,3,n) inputs when `transpose`, else (b,n,3); a 2-D cloud is one frame.  1 <= n <= 2048.
    -> cost (b,) f32 = sum_i |p_i - q_assign[i]|, within n * eps of the optimum (the caller divides by n for evaluations.py:46's scale);
    return_match: -> (cost, assign (b,n) int32 -- a permutation, prices (b,n) f64 -- the dual certificate:
    cost - (sum_i min_j (c[i,j] + prices[j]) - sum_j prices[j]) <= n * eps, info (b,4) int32 = {converged, phases, rounds, bids}).
    eps: the final bidding increment, finite and > 0, in the units of the coordinates.
    max_bids: the bid budget of a frame, 1 .. 2^31 - 1; None: 4096 * n.  That covers ordinary clouds (3-8 n rounds of 5-20 bids), clouds
    of a few distinct points repeated many times (about 1050 n bids at n = 1024) -- every input measured except a target of (nearly)
    all-identical points at n >= 1024 (about 4650 n bids at n = 1024).  A frame that exhausts the budget comes back with converged = 0,
    cost = NaN and assign = -1; nothing is raised here and the other frames are unaffected: look at info[:, 0].
    Bit-reproducible; a frame's result does not depend on the batch it is in.  No gradient is recorded here:
    caspr_amd.losses.exact_earth_mover_distance is the differentiable form."""
    if not (torch.is_tensor(xyz1) and torch.is_tensor(xyz2)):
        raise ValueError("earth_mover_distance_exact: xyz1 and xyz2 must be tensors, got %s and %s" % (type(xyz1).__name__, type(xyz2).__name__))
    if xyz1.dim() == 2:
        xyz1 = xyz1.unsqueeze(0)
    if xyz2.dim() == 2:
        xyz2 = xyz2.unsqueeze(0)
    if transpose and xyz1.dim() == 3 and xyz2.dim() == 3:
        xyz1, xyz2 = xyz1.transpose(1, 2), xyz2.transpose(1, 2)
    if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.shape[2] != 3 or xyz2.shape[2] != 3 or xyz1.shape[0] != xyz2.shape[0] or xyz1.shape[0] < 1:
        raise ValueError("earth_mover_distance_exact: xyz1 and xyz2 must be %s with the same b >= 1, got %s and %s"
                         % ("(b,3,n)" if transpose else "(b,n,3)", tuple(xyz1.shape), tuple(xyz2.shape)))
    B, n, _ = xyz1.shape
    m = xyz2.shape[1]
    if n != m:
        raise ValueError("earth_mover_distance_exact: a one-to-one assignment needs equal point counts, got n = %d and m = %d: "
                         "use earth_mover_distance (the approximate EMD) for clouds of different sizes" % (n, m))
    if not 1 <= n <= EMD_EXACT_MAX_POINTS:
        raise ValueError("earth_mover_distance_exact: n = %d: a frame lives in the LDS of one workgroup, 1 <= n <= %d" % (n, EMD_EXACT_MAX_POINTS))
    if B > 65535:
        raise ValueError("earth_mover_distance_exact: b = %d: b <= 65535" % B)
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (0.0 < float(eps) < float("inf")):
        raise ValueError("earth_mover_distance_exact: eps must be positive and finite, got %r" % (eps,))
    if max_bids is None:
        max_bids = EMD_EXACT_BIDS_PER_POINT * n
    if isinstance(max_bids, bool) or not isinstance(max_bids, int) or not 1 <= max_bids <= 2 ** 31 - 1:
        raise ValueError("earth_mover_distance_exact: max_bids must be an integer in 1 .. 2^31 - 1 (None: %d * n), got %r"
                         % (EMD_EXACT_BIDS_PER_POINT, max_bids))
    for name, t in (("xyz1", xyz1), ("xyz2", xyz2)):   # the type first, the device last: what is wrong with a tensor is said wherever it lives
        if t.dtype != torch.float32:
            raise TypeError("earth_mover_distance_exact: %s must be float32, got %s" % (name, t.dtype))
    for name, t in (("xyz1", xyz1), ("xyz2", xyz2)):
        if not t.is_cuda:
            raise ValueError("earth_mover_distance_exact: %s is on %s: caspr_amd kernels need tensors on the GPU, there is no CPU fallback" % (name, t.device))
        _on_current_device(t)
    xyz1, xyz2 = xyz1.contiguous(), xyz2.contiguous()   # the (b,n,3) view of a (b,3,n) input is copied, as earth_mover_distance does
    dev = xyz1.device
    cost = torch.empty(B, device=dev, dtype=torch.float32)
    assign = torch.empty(B, n, device=dev, dtype=torch.int32)
    prices = torch.empty(B, n, device=dev, dtype=torch.float64)
    info = torch.empty(B, 4, device=dev, dtype=torch.int32)
    L = _lib.load()
    need = L.caspr_emd_exact_ws_bytes(B, n)
    ws = _workspace(need, dev) if need else None
    _lib.check(L.caspr_emd_exact_f32(_p(xyz1), _p(xyz2), B, n, float(eps), int(max_bids), _p(cost), _p(assign), _p(prices), _p(info),
                                     _p(ws), ws.numel() if ws is not None else 0, _stream()), "caspr_emd_exact_f32")
    return (cost, assign, prices, info) if return_match else cost


def ransac_rigid_from_correspondences(src, dst, threshold=0.015, num_hypotheses=5000, sample_size=4, seed=0, refine=False):
    """Open3D `registration_ransac_based_on_correspondence` with point-to-point estimation without scaling, as the camera-pose
    evaluation calls it (evaluations.py:370-375: ransac_n = 4, threshold 0.015, RANSACConvergenceCriteria(50000, 5000) ->
    5000 hypotheses), for correspondences src_i <-> dst_i given index for index (csrc/pose.hip; parity UNPINNED).

    src, dst: (F,N,3|4) or (N,3|4) float GPU tensors of the same shape (only x, y, z are read).  The hypotheses come from a counter
    hash of `seed`: one seed gives bitwise-equal results.  refine: refit on the winner's inliers and report the refit's score.
    -> T (F,4,4) f64 with dst ~ T[:3,:3] src + T[:3,3], fitness (F,) f64, inlier_rmse (F,) f64, inliers (F,) int32, best (F,) int32."""
    if src.dim() == 2:
        src = src.unsqueeze(0)
    if dst.dim() == 2:
        dst = dst.unsqueeze(0)
    if src.dim() != 3 or src.shape[2] not in (3, 4):
        raise ValueError("src must be (F,N,3|4) or (N,3|4), got %s" % (tuple(src.shape),))
    if dst.shape[:2] != src.shape[:2] or dst.shape[2] not in (3, 4):
        raise ValueError("dst %s does not match src %s" % (tuple(dst.shape), tuple(src.shape)))
    if src.shape[2] != dst.shape[2]:   # one row stride for both clouds
        src, dst = src[..., :3], dst[..., :3]
    F, N, rs = src.shape
    n, K = int(sample_size), int(num_hypotheses)
    if not 3 <= n <= 8:
        raise ValueError("sample_size must lie in 3..8, got %d" % n)
    if N < n:
        raise ValueError("%d correspondences, fewer than the sample size %d" % (N, n))
    if K < 1:
        raise ValueError("num_hypotheses must be positive, got %d" % K)
    if not (threshold > 0 and threshold < float("inf")):
        raise ValueError("threshold must be positive and finite, got %r" % (threshold,))
    src, dst = src.contiguous().float(), dst.contiguous().float()
    _chk_f32(src, dst)
    dev = src.device
    T = torch.empty(F, 4, 4, device=dev, dtype=torch.float64)
    rmse = torch.empty(F, device=dev, dtype=torch.float64)
    inliers = torch.empty(F, device=dev, dtype=torch.int32)
    best = torch.empty(F, device=dev, dtype=torch.int32)
    L = _lib.load()
    ws = _workspace(L.caspr_pose_ransac_ws_bytes(F, N, K), dev)
    _lib.check(L.caspr_pose_ransac_f32(_p(src), _p(dst), F, N, rs, K, n, float(threshold), int(seed) & 0xFFFFFFFFFFFFFFFF, int(bool(refine)),
                                       _p(T), _p(inliers), _p(rmse), _p(best), _p(ws), ws.numel(), _stream()), "caspr_pose_ransac_f32")
    return T, inliers.double() / N, rmse, inliers, best


def base_samples(F, n, seed, draw, frame_ids, trunc_std=None, radii=None, raw=False):
    """The decoder's base-distribution draw on the device (csrc/base_sample.hip; caspr.py:228-258): F frames of n points from a
    counter-based generator (Philox4x32-10), each sample a function of (seed, draw, frame_ids[f], point, component) alone -- not of
    the host generators, of F, or of which frames share a call.

    frame_ids: (F,) int64 GPU tensor of global frame ids.  seed: any integer (taken mod 2^64); draw: 0 <= draw < 2^28.
    trunc_std (> 0): models/utils.py:truncated_normal's rule; radii (R >= 1 values): the reference's sample_contours -- a float32
    tensor on the device is used as it is, a sequence or host tensor costs a synchronous host-to-device copy per call; neither:
    three normals per point.  raw=True also returns the (F,n,4) int32 Philox words of block 0.
    -> y (F,n,3) f32, logp_y (F,n) f32 == standard_normal_logprob(y).sum(2) [, raw]."""
    F, n, draw = int(F), int(n), int(draw)
    if F < 1 or n < 1:
        raise ValueError("F and n must be positive, got %d, %d" % (F, n))
    if not 0 <= draw < (1 << 28):
        raise ValueError("draw must lie in 0 .. 2^28 - 1, got %d" % draw)
    if not torch.is_tensor(frame_ids) or not frame_ids.is_cuda:
        raise ValueError("caspr_amd kernels need tensors on the GPU (frame_ids: %s): there is no CPU fallback"
                         % (frame_ids.device if torch.is_tensor(frame_ids) else type(frame_ids).__name__))
    _on_current_device(frame_ids)
    if frame_ids.dtype != torch.int64 or frame_ids.dim() != 1 or frame_ids.shape[0] != F or not frame_ids.is_contiguous():
        raise ValueError("frame_ids must be a contiguous int64 (F,) tensor with F = %d, got %s %s" % (F, frame_ids.dtype, tuple(frame_ids.shape)))
    if trunc_std is not None and radii is not None:
        raise ValueError("trunc_std and radii exclude each other")
    ts = 0.0
    if trunc_std is not None:
        ts = float(trunc_std)
        if not (ts > 0.0 and ts < float("inf")):
            raise ValueError("trunc_std must be positive and finite, got %r" % (trunc_std,))
    dev = frame_ids.device
    rad, R = None, 0
    if radii is not None:
        if torch.is_tensor(radii) and radii.device == dev and radii.dtype == torch.float32:
            rad = radii.reshape(-1).contiguous()
        else:
            rad = torch.as_tensor(radii, dtype=torch.float32).reshape(-1).to(dev).contiguous()
        R = rad.numel()
        if R < 1:
            raise ValueError("radii must hold at least one radius")
        _chk_f32(rad)
    y = torch.empty(F, n, 3, device=dev, dtype=torch.float32)
    logp = torch.empty(F, n, device=dev, dtype=torch.float32)
    words = torch.empty(F, n, 4, device=dev, dtype=torch.int32) if raw else None
    _lib.check(_lib.load().caspr_base_sample_f32(F, n, int(seed) & 0xFFFFFFFFFFFFFFFF, draw, _p(frame_ids), ts, _p(rad), R, _p(y), _p(logp),
                                                 _p(words), _stream()), "caspr_base_sample_f32")
    return (y, logp, words) if raw else (y, logp)
