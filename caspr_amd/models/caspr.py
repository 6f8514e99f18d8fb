"""CaSPR model surface (reference: caspr/models/caspr.py) on the MI355X HIP kernels.

Drop-in for `caspr.models.caspr.CaSPR`: same constructor arguments, methods, return tuples and
state_dict keys, so train.py / test.py / viz.py-style callers and reference
checkpoints work unchanged.  Extra keyword-only knobs of this build: `cnf_rk4_steps`,
`latent_rk4_steps` (fixed-step RK4 replaces torchdiffeq's adaptive dopri5); `base_sampler` / `base_seed`
(where decode's base samples are drawn: the host generators as the reference, or the counter-based device sampler).

Inference: `encode`, `reconstruct`, `decode`, and `forward` for NLL / T-NOCS loss values.
Training: in train() mode with grad enabled `forward` is differentiable end to end -- the encoder as one autograd node
with a HIP backward (caspr_amd/train/encoder_grad.py), the latent ODE and the CNF through the discrete RK4 map with
every matrix product on the HIP kernels (caspr_amd/train/flow_grad.py).
"""
import weakref

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..config import config as _cfg
from .tpointnet2 import TPointNet2
from .latent_ode_model import LatentODE
from .flow import get_point_cnf, count_nfe, PointCNFArgs
from .utils import standard_normal_logprob, sample_gaussian, sphere_surface_points, truncated_normal


class _EarlyLatent:
    """The latent solve started from inside the encoder's last layer (TPointNet2.forward(early=...)): the ODE's initial state is the
    first `channels` columns of z0 (caspr.py:169), final after that layer's first channel tile; the solve then runs on a side stream
    BESIDE the layer's remaining two thirds -- on the team kernel with 32 RESERVED compute units per 16 sequences (its LDS-resident
    weights make it immune to the layer's L2 traffic: 2.65 ms), or, when the team kernel is switched off (ops.LATENT_TEAM = False or
    config.early_latent_team = False), on the single-workgroup kernel with one reserved unit -- instead of 2.3 ms in front of the flow
    with the rest of the chip idle.  The kernel is the one every other solve of the process uses (ops.LATENT_TEAM decides both), so a
    sequence's latent codes do not depend on which path solved them."""

    def __init__(self, latent_ode, plan, stream):
        self.latent_ode, self.plan, self.stream = latent_ode, plan, stream
        self.channels = latent_ode.input_size
        self.out, self.event = None, None

    @staticmethod
    def team():
        return bool(ops.LATENT_TEAM and EARLY_LATENT_TEAM)

    def reserve_cus(self, B):
        if self.latent_ode.method == "dopri5":
            return (B + 15) // 16          # the adaptive solve is single-workgroup: one unit per 16 sequences
        return (32 if self.team() else 1) * ((B + 15) // 16)

    def __call__(self, z0_partial):
        main = torch.cuda.current_stream()
        self.stream.wait_stream(main)
        with torch.cuda.stream(self.stream):
            z_init = z0_partial[:, :self.channels]
            if self.latent_ode.method == "dopri5":
                # one launch, the step control on the device: nothing here waits on the host (the measured count is installed by solve_dopri5)
                out = self.latent_ode.solve_dopri5(z_init, self.plan["sorted_t"])
            else:
                out = ops.latent_rk4(z_init, self.plan["sorted_t"], self.latent_ode.rk4_steps, self.latent_ode._weights(), team=self.team())
            # what aggregate_and_solve_latent does with the solution, here too: off the path between the encoder's last kernel and the flow
            self.out = out[self.plan["rows"], self.plan["pos"], :]                      # (B, T, H): the requested stamps
            if self.latent_ode.method != "dopri5":
                self.latent_ode.ode_func._num_evals.mul_(0).add_(self.plan["evals"])    # evaluations actually run (an element-wise op, not a blit)
            self.event = torch.cuda.Event()
            self.event.record()
        z0_partial.record_stream(self.stream)
        self.out.record_stream(main)
        if self.latent_ode.method == "dopri5":
            self.latent_ode.last_nfe_per_sequence.record_stream(main)


# the latent solve beside the encoder's last layer (config.early_latent = False: in front of the flow, as in rounds 1-3)
JOIN_TNOCS_LATE = True        # reconstruct(): join the deferred T-NOCS regression behind the flow's launch (False: in front of it, rounds 2-4)
EARLY_LATENT = _cfg.early_latent
EARLY_LATENT_TEAM = _cfg.early_latent_team
_EARLY_STREAM = {}
_EARLY_DRAW = {}      # (id(model), device, sample size) -> pinned buffer, copy stream, last copy's event (CaSPR._draw_early)


def _drop_early_draw(owner):
    for k in [k for k in _EARLY_DRAW if k[0] == owner]:
        _EARLY_DRAW.pop(k, None)


_GUARD_STREAM = {}
_UNSET = object()
_CONTOUR_RADII = {}   # (radii, device) -> float32 device tensor: the device sampler's sample_contours argument, copied to the device once


def _contour_radii(radii, device):
    if torch.is_tensor(radii):
        return radii
    key = (tuple(float(r) for r in radii), str(device))
    if key not in _CONTOUR_RADII:
        if len(_CONTOUR_RADII) >= 16:
            _CONTOUR_RADII.clear()
        _CONTOUR_RADII[key] = torch.tensor(key[0], dtype=torch.float32, device=device)
    return _CONTOUR_RADII[key]


def _guard_stream(device):
    key = str(device)
    if key not in _GUARD_STREAM:
        _GUARD_STREAM[key] = torch.cuda.Stream(device=device)
    return _GUARD_STREAM[key]


def _other_steps(S):
    """The step count a guarded solve is compared with, and the factor that turns max |x_S - x_other| into the error estimate of the
    S-step result (RK4, global error ~ C h^4): S' = S // 2 steps when S >= 2 -- x_S' - x_S = ((S / S')^4 - 1) e_S, so estimate =
    diff / ((S / S')^4 - 1): 1 / 15 for an even S, and the same cheap half-cost check for an odd one (S = 11 -> S' = 5, 1 / 22.4) --
    else twice the steps: x_1 - x_2 = (15 / 16) e_1, estimate = diff * 16 / 15."""
    if S >= 2:
        S2 = S // 2
        return S2, 1.0 / ((float(S) / S2) ** 4 - 1.0)
    return 2 * S, 16.0 / 15.0


def _first_passing(diff_of, candidates, tol, refine=True, max_tries=3):
    """Step-count search of calibrate_rk4_steps.  diff_of(S) = max |x_S - x_2S| (15/16 of the S-step error of a 4th-order method).
    Walk `candidates` in ascending order to the first count that passes (diff <= tol); then, with `refine`, look BETWEEN the last
    failing candidate and it: predict the smallest passing count from the two measured differences (observed order p = log2 of their
    ratio per doubling, clipped to [2, 4]; diff(S) ~ diff(fail) (fail / S)^p), and VERIFY the prediction by an actual S-vs-2S solve,
    moving up one count at a time (at most `max_tries` solves) -- a trained flow that fails at 8 and passes at 16 usually passes at
    11 or 12, which is a quarter fewer function evaluations than 16.  -> (chosen, {S: diff} of every count tried)."""
    import math
    diffs, chosen, fail = {}, None, None
    for S in sorted(candidates):
        diffs[S] = diff_of(S)
        if diffs[S] <= tol:
            chosen = S
            break
        fail = S
    if chosen is None:
        return max(candidates), diffs
    if refine and fail is not None and chosen - fail > 1:
        d_fail, d_pass = diffs[fail], diffs[chosen]
        order = 4.0
        if math.isfinite(d_fail) and d_pass > 0 and d_fail > d_pass:
            order = min(4.0, max(2.0, math.log(d_fail / d_pass) / math.log(float(chosen) / fail)))
        guess = chosen
        if math.isfinite(d_fail) and d_fail > 0:
            guess = max(fail + 1, int(math.ceil(fail * (d_fail / tol) ** (1.0 / order) - 1e-9)))
        S, tries = guess, 0
        while S < chosen and tries < max_tries:
            diffs[S] = diff_of(S)
            tries += 1
            if diffs[S] <= tol:
                chosen = S
                break
            S += 1
    return chosen, diffs


def _check_pilot_options(cnf_steps_max, cnf_steps_safety, cnf_steps_points, cnf_steps_tol):
    """What the per-frame step pilot (ops.cnf_frame_steps) needs of its four options: checked by the constructor for cnf_steps="frame" and
    at the call by decode(differentiable=True, frame_steps="pilot"), which a model built with cnf_steps="uniform" may make too."""
    if not (isinstance(cnf_steps_max, int) and 2 <= cnf_steps_max <= 256 and cnf_steps_max & (cnf_steps_max - 1) == 0):
        raise ValueError("cnf_steps_max must be a power of two in 2..256, got %r" % (cnf_steps_max,))
    if not (1.0 <= float(cnf_steps_safety) < float("inf")):
        raise ValueError("cnf_steps_safety must be finite and >= 1, got %r" % (cnf_steps_safety,))
    if int(cnf_steps_points) < 1:
        raise ValueError("cnf_steps_points must be positive, got %r" % (cnf_steps_points,))
    if cnf_steps_tol is not None and not (0.0 < float(cnf_steps_tol) < float("inf")):
        raise ValueError("cnf_steps_tol must be positive and finite, got %r" % (cnf_steps_tol,))


class CaSPR(nn.Module):
    # class-level defaults: a model pickled before these attributes existed keeps drawing on the host
    base_sampler, base_seed, _base_draw = "host", 0, 0
    cnf_steps, cnf_steps_tol, cnf_steps_safety, cnf_steps_max, cnf_steps_points = "uniform", None, 1.2, 64, 64
    cnf_reg = False

    def __init__(self, radii_list=[0.02, 0.05, 0.1, 0.2, 0.4, 0.8], local_feat_size=512, latent_feat_size=1600,
                 ode_hidden_size=512, motion_feat_size=64, pretrain_tnocs=False, augment_quad=True, augment_pairs=True,
                 cnf_blocks=1, regress_tnocs=True, *, cnf_rk4_steps=8, latent_rk4_steps=2, check_tol=1e-5, latent_check_tol=None,
                 check_action="warn", check_points=64, cnf_method="rk4", cnf_atol=1e-5, cnf_rtol=1e-5,
                 latent_method="rk4", latent_rtol=1e-3, latent_atol=1e-3, base_sampler="host", base_seed=0,
                 cnf_steps="uniform", cnf_steps_tol=None, cnf_steps_safety=1.2, cnf_steps_max=64, cnf_steps_points=64, cnf_reg=False):
        super(CaSPR, self).__init__()
        # cnf_reg=True (opt-in, training): the differentiable forward() also returns the point CNF's kinetic and Jacobian integrals per point,
        # (B,T,N,2) = int |f|^2 dt and int |J e|^2 dt along every trajectory (train/flow_grad.py: cnf_block_train(reg=True); Finlay et al.
        # 2020), for train/loop.py: training_loss(kinetic_weight=, jacobian_weight=).  Under no_grad that element is None.
        if cnf_reg and pretrain_tnocs:
            raise ValueError("cnf_reg=True regularises the point CNF: pretrain_tnocs=True builds none")
        self.cnf_reg = bool(cnf_reg)
        # How many RK4 steps the point CNF's SAMPLING solve (decode / reconstruct) takes.  "uniform" (default): cnf_rk4_steps for every
        # frame.  "frame": a count per frame, chosen on the device at every call by a pilot on the first cnf_steps_points samples of
        # each frame (ops.cnf_frame_steps: the ladder 1, 2, 4, .., cnf_steps_max, the guard's Richardson estimate against
        # cnf_steps_tol x (1 + max |x|), refined below the passing rung by the fourth-order law x cnf_steps_safety).  cnf_steps_tol =
        # None: check_tol, or 1e-5 without a guard.  Inference only; forward() (density, training) keeps cnf_rk4_steps.
        if cnf_steps not in ("uniform", "frame"):
            raise ValueError("cnf_steps must be \"uniform\" or \"frame\", got %r" % (cnf_steps,))
        if cnf_steps == "frame":
            if cnf_method != "rk4":
                raise ValueError("cnf_steps=\"frame\" chooses RK4 step counts: it does not combine with cnf_method=%r" % (cnf_method,))
            _check_pilot_options(cnf_steps_max, cnf_steps_safety, cnf_steps_points, cnf_steps_tol)
        self.cnf_steps = cnf_steps
        self.cnf_steps_tol = cnf_steps_tol
        self.cnf_steps_safety = float(cnf_steps_safety)
        self.cnf_steps_max = cnf_steps_max
        self.cnf_steps_points = int(cnf_steps_points)
        self.last_frame_steps = None        # frame mode: (steps, order, info) of the last decode(), device tensors (ops.cnf_frame_steps)
        # Where decode() draws its base samples.  "host" (default): torch's CPU generator / numpy's global one, as the reference, so
        # torch.manual_seed reproduces the reference's samples.  "device": the counter-based sampler (ops.base_samples): a sample is a
        # function of (base_seed, draw number, global frame id, point, component), identical however a batch is sharded, and no host
        # generator is touched.  The draw number is a plain int (deepcopy / torch.save keep it): one per drawing decode(), see seed_base().
        if base_sampler not in ("host", "device"):
            raise ValueError("base_sampler must be \"host\" or \"device\", got %r" % (base_sampler,))
        self.base_sampler = base_sampler
        self.base_seed = int(base_seed)
        self._base_draw = 0
        # Run-time accuracy guard of the fixed-step integrators: ON by default at the reference's own tolerances, reporting as a
        # RuntimeWarning (check_action="raise": CasprAccuracyError; check_tol=None: off).  The reference's dopri5 controls its error at every
        # call (CNF atol = rtol = 1e-5, flow.py:96-99; latent ODE 1e-3, latent_ode_model.py:38,83); a fixed step count does not -- a trained
        # checkpoint loaded at the default 8 / 2 steps must not be silently under-resolved (calibrate_rk4_steps installs counts that pass).
        # With check_tol set, every inference solve (reconstruct / decode / forward / aggregate_and_solve_latent under no_grad) is repeated at half
        # the step count on `check_points` samples per frame (the latent solve: all of it, on one compute unit) on a side stream, the
        # results are compared on the device, and the Richardson estimate of the delivered solution's error is examined through
        # ops.check_deferred_errors() / at the next guarded call: CasprAccuracyError (check_action "raise") or a RuntimeWarning
        # ("warn") when it exceeds check_tol x (1 + max |x|) -- torchdiffeq's atol + rtol |x| with atol = rtol = check_tol, as the
        # reference sets them (latent: latent_check_tol, default 100 x check_tol = the reference's ratio).
        self.check_tol = check_tol
        self.latent_check_tol = latent_check_tol
        self.check_action = check_action
        self.check_points = check_points
        self.pretrain_tnocs = pretrain_tnocs
        self.augment_quad = augment_quad
        self.augment_pairs = augment_pairs
        self.motion_feat_size = motion_feat_size
        self.regress_tnocs = regress_tnocs
        self.tnocs_point_size = 4
        self.encoder = TPointNet2(radii_list, local_feat_size=local_feat_size, out_feat_size=latent_feat_size,
                                  augment_quad=self.augment_quad, augment_pairs=self.augment_pairs,
                                  tnocs_point_size=self.tnocs_point_size, regress_tnocs=self.regress_tnocs)
        if self.pretrain_tnocs:
            return
        # latent_method="dopri5": the latent ODE integrates to latent_rtol / latent_atol (the reference's 1e-3) with the adaptive kernel
        # (per-sequence error control; under autograd only with config.train_latent_dopri5); the guard and calibrate_rk4_steps skip it, as they skip a dopri5 block
        self.latent_ode = LatentODE(input_size=self.motion_feat_size, hidden_size=ode_hidden_size, num_layers=2,
                                    nonlinearity=nn.Tanh, rk4_steps=latent_rk4_steps, method=latent_method, rtol=latent_rtol, atol=latent_atol)
        self.cnf_args = PointCNFArgs()
        self.cnf_args.zdim = latent_feat_size
        self.cnf_args.num_blocks = cnf_blocks
        self.cnf_args.rk4_steps = cnf_rk4_steps
        # cnf_method="dopri5": the point CNF integrates to cnf_atol / cnf_rtol with the adaptive kernel (inference only; per-frame error
        # control); the accuracy guard and calibrate_rk4_steps then have nothing to halve and skip the block
        self.cnf_args.method = cnf_method
        self.cnf_args.atol = cnf_atol
        self.cnf_args.rtol = cnf_rtol
        self.point_cnf = get_point_cnf(self.cnf_args)

    # ------------------------------------------------------------------------------------------
    def forward(self, x, sample_points, aggregate_points=None, e=None):
        """caspr.py:76-122.  x, sample_points (B,T,N,4) -> (recon_loss (B,T,N), tnocs_loss (B,T,N,4)).
        `e` (B*T,N,3) optionally fixes the Hutchinson noise (odefunc.py:115-117).
        A model built with cnf_reg=True returns a third element: the CNF's regulariser integrals (B,T,N,2) with a grad_fn on the
        differentiable path, None under no_grad (the inference kernels do not form them)."""
        if self._differentiable(x, sample_points):
            return self._forward_train(x, sample_points, e)
        with torch.no_grad():
            z0, tnocs_pred = self.encode(x)
            B, H = z0.size()
            _, T, N, _ = sample_points.size()
            tnocs_loss = None
            if self.regress_tnocs:
                tnocs_loss = self.encoder.loss(tnocs_pred[:, :, :, :self.tnocs_point_size],
                                               sample_points[:, :, :, :self.tnocs_point_size])
            if self.pretrain_tnocs:
                return tuple([tnocs_loss])
            ode_feat_dim = self.cnf_args.zdim
            all_times = sample_points[:, :, 0, 3]                                               # :106
            sample_feats = self.aggregate_and_solve_latent(z0, all_times)
            z = sample_feats.reshape(B * T, ode_feat_dim)
            pts = sample_points.reshape(B * T, N, 4)[:, :, :3].contiguous()                     # :112
            init_logprob = torch.zeros(B * T, N, 1, device=pts.device, dtype=pts.dtype)
            guard = None
            if self.check_tol is not None and pts.is_cuda and not self.training:
                if e is None:
                    e = torch.randn_like(pts)                                                   # what the solve would draw (odefunc.py:127-128)
                guard = self._guard_cnf_begin(pts, z, init_logprob, e.reshape(B * T, N, -1))
            cnf_result = self.point_cnf(pts, z, init_logprob, e=e)
            if guard is not None:
                self._guard_cnf_end(guard, cnf_result)
            recon_loss = self.get_nll_loss(cnf_result, B, T)
            if self.cnf_reg:
                return tuple([recon_loss, tnocs_loss, None])
            return tuple([recon_loss, tnocs_loss])

    def _differentiable(self, *inputs):
        """The reference's forward is differentiable whenever autograd records (train() or eval() alike; its callers wrap
        evaluation in torch.no_grad(), train.py:152, test.py:124,141).  Same rule here: the taped path runs iff grad mode
        is on and a parameter or an input asks for a gradient; under no_grad the inference kernels run."""
        if not torch.is_grad_enabled():
            return False
        return any(t.requires_grad for t in inputs if torch.is_tensor(t)) or any(p.requires_grad for p in self.parameters())

    def _forward_train(self, x, sample_points, e=None):
        """Differentiable forward (train_utils.py:125 calls it under model.train()): the encoder is one autograd node with
        a HIP backward (train/encoder_grad.py); the latent ODE and the CNF differentiate the RK4 map (train/flow_grad.py)."""
        from ..train.flow_grad import point_cnf_train
        z0, tnocs_pred = self.encode(x)
        B, _ = z0.size()
        _, T, N, _ = sample_points.size()
        tnocs_loss = None
        if self.regress_tnocs:
            tnocs_loss = self.encoder.loss(tnocs_pred[:, :, :, :self.tnocs_point_size], sample_points[:, :, :, :self.tnocs_point_size])
        if self.pretrain_tnocs:
            return tuple([tnocs_loss])
        all_times = sample_points[:, :, 0, 3]
        sample_feats = self.aggregate_and_solve_latent(z0, all_times)
        z = sample_feats.reshape(B * T, self.cnf_args.zdim)
        pts = sample_points.reshape(B * T, N, 4)[:, :, :3].contiguous()
        init_logprob = torch.zeros(B * T, N, 1, device=pts.device, dtype=pts.dtype)
        if self.cnf_reg:
            y, delta_log_py, r = point_cnf_train(self.point_cnf, pts, z, init_logprob, e=e, reg=True)
            return tuple([self.get_nll_loss((y, delta_log_py), B, T), tnocs_loss, r.view(B, T, N, 2)])
        cnf_result = point_cnf_train(self.point_cnf, pts, z, init_logprob, e=e)
        return tuple([self.get_nll_loss(cnf_result, B, T), tnocs_loss])

    def get_nll_loss(self, cnf_result_list, B, T):
        """caspr.py:124-146."""
        batch_size = B * T
        y, delta_log_py = cnf_result_list
        cloud_dim = y.size()[1]
        log_py = standard_normal_logprob(y).sum(2)
        delta_log_py = delta_log_py.view(batch_size, cloud_dim)
        log_px = log_py - delta_log_py
        return (-log_px).view((B, T, -1))

    def encode(self, x):
        """caspr.py:148-155."""
        return self.encoder(x)

    def aggregate_and_solve_latent(self, z0, time_tensor, _plan=None, _presolved=None):
        """caspr.py:157-183: unique sorted times -> latent ODE -> map back -> concat the static feature.
        Inference on the GPU takes the synchronisation-free route of LatentODE.solve_at (same values); _plan: what
        reconstruct() prepared ahead of the encoder (LatentODE.plan_times)."""
        B, T = time_tensor.size()
        z_init = z0[:, :self.latent_ode.input_size]
        z_global = z0[:, self.latent_ode.input_size:]
        if _presolved is not None and _presolved.event is not None:
            # the solve already ran beside the encoder's last layer (_EarlyLatent): join it, gather the requested stamps
            torch.cuda.current_stream().wait_event(_presolved.event)
            sample_feats = _presolved.out
        elif z0.is_cuda and not self._differentiable(z0, time_tensor):
            if _plan is not None and _plan.get("event") is not None:
                torch.cuda.current_stream().wait_event(_plan["event"])                   # the plan was made on another stream
                for v in _plan.values():
                    if torch.is_tensor(v):
                        v.record_stream(torch.cuda.current_stream())
            sample_feats = self.latent_ode.solve_at(z_init, time_tensor, _plan)
        else:
            solve_t, time_map = torch.unique(time_tensor, sorted=True, return_inverse=True)
            pred_z = self.gen_latent(z_init, solve_t)
            batch_inds = torch.arange(B, device=z0.device).view((-1, 1)).repeat((1, T))
            sample_feats = pred_z[batch_inds, time_map, :]
        if self.check_tol is not None and z0.is_cuda and not self._differentiable(z0, time_tensor):
            self._guard_latent(z_init, time_tensor, sample_feats, _plan)
        B_global, H_global = z_global.size()
        z_global = z_global.unsqueeze(1).expand(B_global, sample_feats.size()[1], H_global)
        return torch.cat([sample_feats, z_global], dim=2)

    # ------------------------------------------------------------------------------------------ run-time accuracy guard
    def _guard_latent(self, z_init, time_tensor, sample_feats, plan):
        """The latent solve once more at half (or twice) the steps per interval, on the single-workgroup kernel (one compute unit,
        no co-residency requirement: it may run beside anything) on the guard stream; max |z_L - z_L'| over the requested stamps
        goes to the deferred channel (ops.guard_track).  Nothing on the current stream waits for it."""
        if self.latent_ode.method == "dopri5":
            return                # the adaptive solve controls its own error: no step count to halve, no check solve
        L = self.latent_ode.rk4_steps
        L2, factor = _other_steps(L)
        tol = self.latent_check_tol if self.latent_check_tol is not None else 100.0 * self.check_tol
        main = torch.cuda.current_stream()
        gs = _guard_stream(z_init.device)
        gs.wait_stream(main)
        with torch.cuda.stream(gs), ops.untimed():
            if plan is None or plan["shape"] != tuple(time_tensor.shape):
                plan = self.latent_ode.plan_times(time_tensor)
            zc = ops.latent_rk4(z_init, plan["sorted_t"], L2, self.latent_ode._weights(), team=False)[plan["rows"], plan["pos"], :]
            diff = (sample_feats - zc).abs().amax()
            ops.guard_track(diff, sample_feats.abs().amax(), {"name": "latent", "tol": float(tol), "factor": factor, "steps": L, "other_steps": L2, "action": self.check_action,
                                   "what": "latent ODE (latent_ode_model.py:45-70; reference: dopri5 at rtol = atol = 1e-3)"})
        # everything the guard stream reads was allocated on another stream (the plan: on the plan / copy stream): keep it alive until
        # the check has run, also when reconstruct() drops the plan right after this call
        for t_ in (z_init, sample_feats, time_tensor) + tuple(v for v in plan.values() if torch.is_tensor(v)):
            t_.record_stream(gs)

    def _guard_cnf_begin(self, y, z, logpx=None, e=None):
        """What the check of this solve needs, captured BEFORE the main launch (the weight packs / end time are built on first use: on the
        MAIN stream, before the guard stream reads them).  -> what _guard_cnf_end needs.
        logpx / e given: the density direction of forward() (cnf.py:70-128 with the Hutchinson divergence, same noise on the same
        samples); otherwise the sampling direction of decode()."""
        from .cnf import CNF
        blocks = [l for l in self.point_cnf.chain if isinstance(l, CNF) and l.method == "rk4"]
        if not blocks or len(blocks) != sum(isinstance(l, CNF) for l in self.point_cnf.chain):
            return None           # dopri5 blocks control their own error: no step count to halve, no check solve
        for b in blocks:
            b._weights()
            if ops.CNF_BF16X6:
                b._weights_x6()
            b.end_time()
        S = blocks[0].rk4_steps
        S2, factor = _other_steps(S)
        return {"y": y, "z": z, "logpx": logpx, "e": e, "blocks": blocks, "g": min(int(self.check_points), y.shape[1]), "S": S, "S2": S2, "factor": factor,
                "stream": _guard_stream(y.device)}

    def _guard_cnf_end(self, ctx, x):
        """The point CNF once more on the first `check_points` samples of every frame at half (S = 1: twice) the step count on the guard
        stream, queued BEHIND the main launch (round 6; rounds 5 queued it beside the launch, where each of its 160 workgroups held up one
        of the 256 compute units' ten main workgroups: +3 % of a step): the check then runs under whatever the caller does next -- in a loop
        over batches the first, latency-bound milliseconds of the next call's encoder (farthest-point sampling on 160 of 256 units) -- and
        its verdict, which travels through the deferred channel anyway (ops.guard_track), arrives a millisecond later.
        max |x_S - x_S'| on the checked samples -> the deferred channel; nothing on the current stream waits."""
        gs, g, blocks = ctx["stream"], ctx["g"], ctx["blocks"]
        y, z, logpx, e = ctx["y"], ctx["z"], ctx["logpx"], ctx["e"]
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream())
        saved = [(b, b.rk4_steps) for b in blocks]
        with torch.cuda.stream(gs), ops.untimed():
            gs.wait_event(done)
            try:
                for b in blocks:
                    b.rk4_steps, b._count_evals, b.odefunc._count_evals, b._narrow = _other_steps(b.rk4_steps)[0], False, False, g <= 64
                if logpx is None:
                    xh = self.point_cnf(y[:, :g].contiguous(), z, reverse=True)
                else:
                    xh = self.point_cnf(y[:, :g].contiguous(), z, logpx[:, :g].contiguous(), e=e[:, :g].contiguous())
            finally:
                for b, st in saved:
                    b.rk4_steps, b._count_evals, b.odefunc._count_evals, b._narrow = st, True, True, False
            meta = {"tol": float(self.check_tol), "factor": ctx["factor"], "steps": ctx["S"], "other_steps": ctx["S2"], "action": self.check_action}
            if torch.is_tensor(x):
                diff = (x[:, :g] - xh).abs().amax()
                ops.guard_track(diff, x[:, :g].abs().amax(), dict(meta, name="cnf", what="point CNF (cnf.py:70-128; reference: dopri5 at atol = rtol = 1e-5)"))
            else:               # density direction: the state is (y, logp), both integrated (cnf.py:112-126)
                for i, (nm, what) in enumerate((("cnf_fwd_y", "point CNF, density direction, y"), ("cnf_fwd_logp", "point CNF, density direction, log-density"))):
                    diff = (x[i][:, :g] - xh[i]).abs().amax()
                    ops.guard_track(diff, x[i][:, :g].abs().amax(), dict(meta, name=nm, what=what + " (cnf.py:70-128; reference: dopri5 at atol = rtol = 1e-5)"))
        for t_ in (y, z, logpx, e) + ((x,) if torch.is_tensor(x) else tuple(x)):
            if t_ is not None:
                t_.record_stream(gs)

    # ------------------------------------------------------------------------------------------ per-frame step counts
    def _decode_frame_steps(self, y, z):
        """decode()'s solve with cnf_steps="frame": the hyper conv of every block once, the pilot ladder on the first cnf_steps_points
        samples of every frame through the whole flow (one table shared by all blocks, narrow kernel), then the solve with the chosen
        (steps, order).  No host read anywhere: capturable.  y (BT,n,3), z (BT,H) -> x (BT,n,3)."""
        from .cnf import CNF
        if self._differentiable(y, z):
            raise ValueError("cnf_steps=\"frame\" is an inference option: call decode() / reconstruct() under torch.no_grad() "
                             "(no gradient through a solve with per-frame step counts)")
        blocks = [l for l in self.point_cnf.chain if isinstance(l, CNF)]
        if any(b.method != "rk4" for b in blocks):
            raise ValueError("cnf_steps=\"frame\" chooses RK4 step counts: a dopri5 block has none")
        g, s_max = min(self.cnf_steps_points, y.shape[1]), int(self.cnf_steps_max)
        tol = self.cnf_steps_tol if self.cnf_steps_tol is not None else (self.check_tol if self.check_tol is not None else 1e-5)
        yp = y[:, :g].contiguous()
        try:
            for b in blocks:
                b._hyper = b.hyper_of(z)
            if ops.BEFORE_CNF_LAUNCH is not None:          # reconstruct()'s deferred T-NOCS regression: in front of the pilot, not of the solve
                hook, ops.BEFORE_CNF_LAUNCH = ops.BEFORE_CNF_LAUNCH, None
                hook()
            steps, order, info = self._pilot_frame_steps(blocks, yp, z, tol, s_max)
            for b in blocks:
                b.frame_steps, b.frame_order, b.frame_max_steps = steps, order, s_max
            with ops.timed("cnf_main"):
                x = self.point_cnf(y, z, reverse=True)
        finally:
            for b in blocks:
                b.frame_steps, b.frame_order, b.frame_max_steps, b._hyper = None, None, None, None
        pilot_evals = 4 * info["pilot_steps"].max()
        for b in blocks:
            b.last_pilot_steps_per_frame = info["pilot_steps"]
            b.odefunc._num_evals += pilot_evals.to(b.odefunc._num_evals.dtype)       # on the device, as the dopri5 route counts
        self.last_frame_steps = (steps, order, info)
        if self.check_tol is not None and not torch.cuda.is_current_stream_capturing():
            self._guard_cnf_frames(blocks, y, z, x, steps, s_max)
        return x

    def _pilot_frame_steps(self, blocks, yp, z, tol, s_max):
        """The pilot ladder of ops.cnf_frame_steps on the pilot points yp (BT,g,3) through the whole flow: narrow kernel, one table for all
        blocks, not counted by get_nfe() (the callers add info["pilot_steps"]).  Expects every block's `_hyper` in place and leaves the
        last rung's table on the blocks: the caller sets or clears `frame_steps`.  -> (steps, order, info)."""
        def run_rung(tab):
            for b in blocks:
                b.frame_steps, b.frame_order, b.frame_max_steps = tab, None, s_max
            return self.point_cnf(yp, z, reverse=True)
        for b in blocks:
            b._count_evals, b.odefunc._count_evals, b._narrow = False, False, True
        try:
            with ops.timed("cnf_pilot"):
                return ops.cnf_frame_steps(run_rung, yp.shape[0], yp.shape[1], tol, self.cnf_steps_safety, s_max, device=yp.device)
        finally:
            for b in blocks:
                b._count_evals, b.odefunc._count_evals, b._narrow = True, True, False

    def _pilot_for_gradient(self, y, z):
        """decode(differentiable=True, frame_steps="pilot"): the step counts the inference route would choose for (y, z) -- the same pilot
        on the same first cnf_steps_points samples with the model's cnf_steps_tol / _safety / _max, under no_grad on detached tensors
        (the counts are held fixed by the gradient).  A capped frame reports through the deferred channel.  -> (steps, order, info)."""
        from .cnf import CNF
        _check_pilot_options(self.cnf_steps_max, self.cnf_steps_safety, self.cnf_steps_points, self.cnf_steps_tol)
        blocks = [l for l in self.point_cnf.chain if isinstance(l, CNF)]
        g, s_max = min(self.cnf_steps_points, y.shape[1]), int(self.cnf_steps_max)
        tol = self.cnf_steps_tol if self.cnf_steps_tol is not None else (self.check_tol if self.check_tol is not None else 1e-5)
        with torch.no_grad():
            yd, zd = y.detach(), z.detach()
            try:
                for b in blocks:
                    b._hyper = b.hyper_of(zd)
                return self._pilot_frame_steps(blocks, yd[:, :g].contiguous(), zd, tol, s_max)
            finally:
                for b in blocks:
                    b.frame_steps, b.frame_order, b.frame_max_steps, b._hyper = None, None, None, None

    def _guard_cnf_frames(self, blocks, y, z, x, steps, s_max):
        """The accuracy guard of a frame-mode solve: the first check_points samples of every frame once more with the table S_f // 2 on
        the guard stream, behind the main launch; the criterion frame by frame -- diff_f / ((S_f / S'_f)^4 - 1) against check_tol x
        (1 + max |x_f|) -- reduced on the device to the worst frame, which travels through the deferred channel (ops.guard_track)."""
        g = min(int(self.check_points), y.shape[1])
        gs = _guard_stream(y.device)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream())
        with torch.cuda.stream(gs), ops.untimed():
            gs.wait_event(done)
            half = torch.div(steps, 2, rounding_mode="floor").to(torch.int32)         # S_f >= 2: at least one step
            try:
                for b in blocks:
                    b.frame_steps, b.frame_order, b.frame_max_steps = half, None, s_max
                    b._count_evals, b.odefunc._count_evals, b._narrow = False, False, g <= 64
                xh = self.point_cnf(y[:, :g].contiguous(), z, reverse=True)
            finally:
                for b in blocks:
                    b.frame_steps, b.frame_order, b.frame_max_steps = None, None, None
                    b._count_evals, b.odefunc._count_evals, b._narrow = True, True, False
            xs = x[:, :g]
            diff = (xs - xh).abs().flatten(1).amax(1).double()
            scale = xs.abs().flatten(1).amax(1)
            est = diff / ((steps.double() / half.double()) ** 4 - 1.0)
            ratio = torch.nan_to_num(est / (float(self.check_tol) * (1.0 + scale.double())), nan=float("inf"))
            worst = ratio.argmax()
            ops.guard_track(est[worst].float(), scale[worst], {"name": "cnf", "tol": float(self.check_tol), "factor": 1.0, "steps": s_max, "other_steps": s_max // 2,
                                                               "action": self.check_action,
                                                               "what": "point CNF, per-frame step counts (at most the count named; the estimate is the worst "
                                                                       "frame's, each against half its own count) (cnf.py:70-128; reference: dopri5 at atol = rtol = 1e-5)"})
        for t_ in (y, z, x, steps):
            t_.record_stream(gs)

    def gen_latent(self, z0, timestamps):
        """caspr.py:185-196."""
        return self.latent_ode(z0, timestamps)

    def get_nfe(self):
        """caspr.py:198-202."""
        return np.array([count_nfe(self.latent_ode), count_nfe(self.point_cnf)])

    def _draw_early(self, B, T, num_points, constant_in_time, device):
        """The Gaussian base samples of decode, drawn as the reference draws them -- torch.randn on the CPU generator, then moved
        (models/utils.py:25-26; caspr.py:252) -- but EARLY in reconstruct(): the encoder's kernels are already queued, so the
        ~7 ms draw of a cfg-2 batch (983,040 values, serial MT19937) runs on the host while the GPU encodes; the copy goes from a
        pinned buffer on a side stream.  Same values, same position in the CPU generator's stream (nothing else draws from it
        in between).  -> (device tensor, event the consuming stream must wait for)."""
        samp_batch = B if constant_in_time else B * T
        size = (samp_batch, num_points, self.cnf_args.input_dim)
        # pinned buffer + copy stream per (device, size), at most two entries (evicting the oldest releases its pinned memory); kept in a
        # module-level table, not on the module: streams / events must not end up in copy.deepcopy(model) or torch.save(model)
        key = (id(self), str(device), size)
        ent = _EARLY_DRAW.get(key)
        if ent is None:
            mine = [k for k in _EARLY_DRAW if k[0] == id(self)]
            for k in mine[:max(0, len(mine) - 1)]:
                old = _EARLY_DRAW.pop(k)
                if old["ev"] is not None:
                    old["ev"].synchronize()
            ent = _EARLY_DRAW[key] = {"buf": torch.empty(size, dtype=torch.float32, pin_memory=True), "ev": None, "stream": torch.cuda.Stream(device=device)}
            weakref.finalize(self, _drop_early_draw, id(self))
        if ent["ev"] is not None:
            ent["ev"].synchronize()          # the previous call's copy out of the pinned buffer (a whole step ago)
        torch.randn(*size, out=ent["buf"])   # == torch.randn(*size): same generator, same stream position
        with torch.cuda.stream(ent["stream"]):
            yd = ent["buf"].to(device, non_blocking=True)
            # log N(y; 0, I) of the draw (caspr.py:258) right behind the copy, under the encoder (decode uses it unless it alters y)
            lp = standard_normal_logprob(yd).view(samp_batch, num_points, -1).sum(2)
            ent["ev"] = torch.cuda.Event()
            ent["ev"].record(ent["stream"])
        return yd, ent["ev"], lp

    def seed_base(self, seed, draw=0):
        """Re-seed the device base sampler: the next drawing decode() / reconstruct() uses (seed, draw), the one after (seed, draw + 1), ...
        (the host sampler follows torch.manual_seed / np.random.seed and ignores this).  A draw number lies in 0 .. 2^28 - 1 (the
        counter's field for it); a decode() past the last one raises instead of reusing earlier samples: re-seed then."""
        if not 0 <= int(draw) < (1 << 28):
            raise ValueError("draw must lie in 0 .. 2^28 - 1, got %r" % (draw,))
        self.base_seed, self._base_draw = int(seed), int(draw)

    def _base_frame_ids(self, B, T, constant_in_time, frame_ids, device):
        """Global frame ids of the device draw's rows, int64 on `device`: (B*T,) = sequence * T + t, or with constant_in_time (B,) =
        sequence | 2^62 (one row per sequence; the high bit keeps it apart from every per-frame id).  Default: sequences 0 .. B-1."""
        rows = B if constant_in_time else B * T
        if frame_ids is None:
            ids = torch.arange(rows, device=device, dtype=torch.int64)
            return ids | (1 << 62) if constant_in_time else ids
        ids = torch.as_tensor(frame_ids).to(device=device, dtype=torch.int64).reshape(-1).contiguous()
        if ids.numel() != rows:
            raise ValueError("frame_ids must hold %d ids (%s), got %d" % (rows, "one per sequence with constant_in_time" if constant_in_time else "B * T", ids.numel()))
        return ids

    def _base_samples(self, B, T, num_points, constant_in_time, truncate_std, sample_contours, y, like, early=None, frame_ids=None):
        """The base-distribution draw of decode (caspr.py:228-256) -> (B*T, num_points, 3) on `like`'s device, and its log-density
        (B*T, num_points) where the draw came with one (the device sampler), else None."""
        samp_batch = B if constant_in_time else B * T
        input_dim = self.cnf_args.input_dim
        samp_size = (samp_batch, num_points, input_dim)
        logp_y = None
        if y is not None:
            y = y.to(like).reshape(B * T, num_points, input_dim)
            constant_in_time = False
        elif self.base_sampler == "device":
            # one launch on the current stream; contours take precedence over truncation, as in the reference's branch order
            ids = self._base_frame_ids(B, T, constant_in_time, frame_ids, like.device)
            if self._base_draw >= (1 << 28):
                raise RuntimeError("the device base sampler has used all 2^28 draw numbers of this seed: call seed_base() with another seed")
            radii = None if sample_contours is None else _contour_radii(sample_contours, like.device)
            y, logp_y = ops.base_samples(samp_batch, num_points, self.base_seed, self._base_draw, ids,
                                         trunc_std=truncate_std if sample_contours is None else None, radii=radii)
            self._base_draw += 1
            if constant_in_time:
                logp_y = logp_y.view(B, 1, num_points).expand(B, T, num_points).reshape(B * T, num_points)
        elif sample_contours is not None:
            radii = sample_contours
            contours = []
            nsamp_pts = 0
            for radius in radii:
                last = radius == radii[-1]
                cnt = (num_points - nsamp_pts) if last else (num_points // len(radii))
                pts = sphere_surface_points(samp_batch * cnt, radius=radius).reshape((samp_batch, cnt, 3))
                contours.append(pts)
                nsamp_pts += num_points // len(radii)
            y = torch.from_numpy(np.concatenate(contours, axis=1)).to(like).view(samp_size)
        elif early is not None:
            y, ev = early[0], early[1]
            torch.cuda.current_stream().wait_event(ev)
            y.record_stream(torch.cuda.current_stream())
            if truncate_std is not None:
                truncated_normal(y, mean=0, std=1, trunc_std=truncate_std)
        else:
            y = sample_gaussian(samp_size, truncate_std, device=like.device)
        if constant_in_time:
            y = y.view((B, 1, num_points, input_dim)).expand((B, T, num_points, input_dim)).reshape((B * T, num_points, input_dim))
        return y.contiguous(), logp_y

    def _check_differentiable(self, what, frame_steps=None):
        """decode(differentiable=True) / reconstruct(differentiable=True): the options the gradient route does not cover, refused with
        the reason (train/flow_grad.py: point_cnf_sample_train states the rest -- GPU tensors, the 512-wide ODE function, ops.CNF_BF16X6).
        With frame_steps (a table or "pilot") the per-frame counts are the caller's choice and cnf_steps="frame" is no obstacle."""
        from .cnf import CNF
        if not torch.is_grad_enabled():
            raise ValueError("%s(differentiable=True) records a gradient, but grad mode is off (torch.no_grad()): drop the keyword for inference" % what)
        if frame_steps is None and self.cnf_steps == "frame":
            raise ValueError("%s(differentiable=True) differentiates the uniform RK4 solve: no gradient through per-frame step counts "
                             "chosen inside the call (cnf_steps=\"frame\" is an inference option); pass frame_steps=\"pilot\" or a table "
                             "of counts to differentiate the solve with every frame's count held fixed" % what)
        if frame_steps is not None and not torch.is_tensor(frame_steps) and frame_steps != "pilot":
            raise ValueError("%s: frame_steps must be None, \"pilot\" or a (B*T,) int32 tensor of RK4 step counts, got %r" % (what, frame_steps))
        if any(isinstance(l, CNF) and l.method != "rk4" for l in self.point_cnf.chain):
            raise ValueError("%s(differentiable=True) differentiates the RK4 solve: no gradient through the adaptive solve "
                             "(cnf_method=\"dopri5\" is an inference option)" % what)

    def decode(self, z, num_points=1024, constant_in_time=False, truncate_std=None, sample_contours=None, y=None, _early=None, frame_ids=None,
               frame_steps=None, differentiable=False):
        """caspr.py:204-267.  `y` (B,T,num_points,3) optionally supplies the base samples.
        frame_ids (device sampler only; ignored with the host sampler or a given `y`): the global ids the draw is keyed by, int64,
        B*T of them (sequence * T + t) or, with constant_in_time, B (see _base_frame_ids); default: this batch is sequences 0 .. B-1.
        differentiable: False (default) runs the inference kernels whatever the grad mode -- under grad mode the returned `x` is DETACHED
        from the graph (no grad_fn; the accuracy guard is skipped there).  True: `x` is differentiable in z, in a given `y` and in every
        parameter of the point CNF, as the reference's decode is (caspr.py:262 through torchdiffeq): the sampling solve runs as one
        autograd node per block with a tape of (BT,n,3) tensors (train/flow_grad.py: point_cnf_sample_train; discretise-then-optimise:
        the gradient of the RK4 map itself).  Needs grad mode, GPU tensors, uniform RK4 steps (not cnf_method="dopri5", not
        cnf_steps="frame"): otherwise a ValueError says which; no guard on this route.  With config.cnf_tape_split = "f16x3" (opt-in) and
        num_points >= 128 its forward launch is the f16x3 evaluation of the inference solve: per block the bits decode() itself returns.
        frame_steps (with differentiable=True only; inference has cnf_steps="frame"): None (default) = cnf_rk4_steps for every frame.  A
        (B*T,) int32 tensor on z's device = the RK4 step count of every frame, 1..cnf_steps_max; "pilot" = chosen here as the inference
        route chooses them (the pilot of cnf_steps="frame" with the model's cnf_steps_tol / _safety / _max / _points, run under no_grad;
        get_nfe() counts pilot + solve; last_frame_steps = (steps, order, info) afterwards).  The gradient is that of the RK4 map with
        every frame's count held fixed (train/flow_grad.py: CnfSampleSolveFrames); every CNF block takes the same table.  Works on a
        model built with either cnf_steps."""
        if frame_steps is not None and not differentiable:
            raise ValueError("decode: frame_steps comes with differentiable=True (inference chooses per-frame counts with cnf_steps=\"frame\")")
        if differentiable:
            self._check_differentiable("decode", frame_steps)
        B, T, H = z.size()
        input_dim = self.cnf_args.input_dim
        given = y is not None
        y, logp_y = self._base_samples(B, T, num_points, constant_in_time, truncate_std, sample_contours, y, z, early=_early, frame_ids=frame_ids)
        if logp_y is not None:                       # the device draw's own launch wrote it (the same bits: csrc/base_sample.hip)
            logp_y = logp_y.contiguous()
        elif _early is not None and not given and sample_contours is None and truncate_std is None and not constant_in_time:
            logp_y = _early[2]                       # computed behind the draw's copy (same values: same op on the same tensor)
            logp_y.record_stream(torch.cuda.current_stream())
        else:
            logp_y = standard_normal_logprob(y).view(B * T, num_points, -1).sum(2)
        z = z.reshape((B * T, H))
        if differentiable:
            from ..train.flow_grad import point_cnf_sample_train
            if frame_steps is None:
                x = point_cnf_sample_train(self.point_cnf, y, z)
            else:
                x = self._decode_differentiable_frames(y, z, frame_steps)
        elif self.cnf_steps == "frame" and y.is_cuda:
            x = self._decode_frame_steps(y, z)
        else:
            guard = self._guard_cnf_begin(y, z) if (self.check_tol is not None and y.is_cuda and not torch.is_grad_enabled()) else None
            x = self.point_cnf(y, z, reverse=True)
            if guard is not None:
                self._guard_cnf_end(guard, x)
        return y.view((B, T, num_points, input_dim)), logp_y.view((B, T, num_points)), x.view((B, T, num_points, input_dim))

    def _decode_differentiable_frames(self, y, z, frame_steps):
        """decode(differentiable=True)'s solve with a step count per frame: the table as given, or the pilot's.  y (BT,n,3), z (BT,H)."""
        from .cnf import CNF
        from ..train.flow_grad import point_cnf_sample_train
        if not (y.is_cuda and z.is_cuda):
            raise ValueError("decode(differentiable=True) runs on the GPU only (HIP kernels): z and y must be GPU tensors")
        order = info = None
        if torch.is_tensor(frame_steps):
            steps = frame_steps
        else:
            steps, order, info = self._pilot_for_gradient(y, z)
        x = point_cnf_sample_train(self.point_cnf, y, z, steps, int(self.cnf_steps_max))
        if info is not None:
            pilot_evals = 4 * info["pilot_steps"].max()
            for b in self.point_cnf.chain:
                if isinstance(b, CNF):
                    b.last_pilot_steps_per_frame = info["pilot_steps"]
                    b.odefunc._num_evals += pilot_evals.to(b.odefunc._num_evals.dtype)   # on the device, as the inference route counts
        self.last_frame_steps = (steps, order, info)
        return x

    @staticmethod
    def _sequence_frame_ids(sequence_ids, B, T, constant_in_time, device):
        """reconstruct()'s sequence_ids (B,) -> the frame ids decode() keys the device draw by (_base_frame_ids)."""
        seq = torch.as_tensor(sequence_ids).to(device=device, dtype=torch.int64).reshape(-1)
        if seq.numel() != B:
            raise ValueError("sequence_ids must hold B = %d ids, got %d" % (B, seq.numel()))
        if constant_in_time:
            return seq | (1 << 62)
        return (seq.view(B, 1) * T + torch.arange(T, device=device, dtype=torch.int64).view(1, T)).reshape(-1)

    def reconstruct(self, x, num_points=1024, constant_in_time=False, timestamps=None, max_timestamp=5.0,
                    truncate_std=None, sample_contours=None, y=None, check_tol=_UNSET, sequence_ids=None, frame_steps=None,
                    differentiable=False):
        """caspr.py:269-308 -> (y, logp_y, x, tnocs_pred).  `y` (B,T,num_points,3) optionally supplies the base samples.
        differentiable=True: the plain serial composition the reference has -- encode -> aggregate_and_solve_latent ->
        decode(differentiable=True) -- on the current stream, recorded by autograd (encoder, latent ODE and point CNF each through their
        training route); no side streams, no early latent solve, no accuracy guard.  Same return tuple; see decode() for what it needs.
        config.cnf_tape_split = "f16x3" (opt-in) selects the forward launch of the point CNF's solve here as it does in decode().
        frame_steps (with differentiable=True only): None, a (B*T,) int32 table of RK4 step counts or "pilot", handed to decode().
        check_tol: the accuracy guard's tolerance for THIS call (default: the model's `check_tol` attribute; None = off).
        sequence_ids (device sampler only; ignored with the host sampler or a given `y`): int64 (B,), the global index of each
        sequence (default arange(B)); a shard that passes its sequences' global indices draws what the unsharded batch draws.
        A tensor on x's device costs nothing; a list or host tensor is copied to the device synchronously at every call."""
        if check_tol is not _UNSET:
            prev, self.check_tol = self.check_tol, check_tol
            try:
                return self.reconstruct(x, num_points, constant_in_time, timestamps, max_timestamp, truncate_std, sample_contours, y,
                                        sequence_ids=sequence_ids, frame_steps=frame_steps, differentiable=differentiable)
            finally:
                self.check_tol = prev
        if frame_steps is not None and not differentiable:
            raise ValueError("reconstruct: frame_steps comes with differentiable=True (inference chooses per-frame counts with cnf_steps=\"frame\")")
        if differentiable:
            self._check_differentiable("reconstruct", frame_steps)
            B, T, N, _ = x.size()
            all_times = x[:, :, 0, 3] / max_timestamp if timestamps is None else timestamps.view((1, -1)).repeat((B, 1)).to(x)
            z0, tnocs_pred = self.encode(x)
            frame_ids = None
            if self.base_sampler == "device" and y is None and sequence_ids is not None:
                frame_ids = self._sequence_frame_ids(sequence_ids, B, T, constant_in_time, x.device)
            z = self.aggregate_and_solve_latent(z0, all_times)
            y, logp_y, x = self.decode(z, num_points, constant_in_time, truncate_std, sample_contours, y=y, frame_ids=frame_ids, frame_steps=frame_steps,
                                       differentiable=True)
            return y, logp_y, x, tnocs_pred
        with torch.no_grad():
            B, T, N, _ = x.size()
            if timestamps is None:
                all_times = x[:, :, 0, 3] / max_timestamp
            else:
                all_times = timestamps.view((1, -1)).repeat((B, 1)).to(x)
            # the T-NOCS regression of the encoder's last layer runs on a side stream underneath the latent solve (32 workgroups,
            # latency-bound); joined before the flow starts
            defer = x.is_cuda and not self._differentiable(x)
            # what the latent solve needs from the time stamps alone is queued before the encoder (a dozen tiny kernels that
            # otherwise sit between the encoder's last layer and the solve, behind the T-NOCS layer's workgroups)
            plan, early_lat, st = None, None, None
            if defer:
                # (the time-stamp bookkeeping -- sort, inverse permutation, evaluation count: a dozen tiny kernels -- on the stream the
                # solve will run on, not in front of the encoder)
                st = _EARLY_STREAM.get(str(x.device))
                if st is None:
                    st = _EARLY_STREAM[str(x.device)] = torch.cuda.Stream(device=x.device)
                st.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(st):
                    plan = self.latent_ode.plan_times(all_times)
                    plan["event"] = torch.cuda.Event()
                    plan["event"].record()
                all_times.record_stream(st)
            # worth it while the reserved units cost the layer less than the solve takes: one team (<= 16 sequences = 32 units for the
            # two thirds of a layer that lasts ~5 ms per 327,680 rows) against ~2.3 ms of solve; larger batches / longer layers keep the
            # serial order (cfg-5: 4 teams would halve the chip under a 75 ms layer).  Either order gives the same bits.
            if defer and EARLY_LATENT and self.latent_ode.input_size <= 64 and B <= 16 and B * T * N <= 800000:
                early_lat = _EarlyLatent(self.latent_ode, plan, st)
            z0, tnocs_pred = self.encoder(x, defer_tnocs=True, early=early_lat) if defer else self.encode(x)
            # the encoder is queued: draw the base samples on the host now (as the reference does inside decode), under it
            early = None
            if defer and y is None and sample_contours is None and self.base_sampler == "host":
                early = self._draw_early(B, T, num_points, constant_in_time, x.device)
            frame_ids = None
            if self.base_sampler == "device" and y is None and sequence_ids is not None:
                frame_ids = self._sequence_frame_ids(sequence_ids, B, T, constant_in_time, x.device)
            with ops.timed("latent"):
                z = self.aggregate_and_solve_latent(z0, all_times, plan, early_lat)
            self._early_latent_used = bool(early_lat is not None and early_lat.event is not None)     # for tests / tools
            if defer and not JOIN_TNOCS_LATE:
                self.encoder.join()
            if defer and JOIN_TNOCS_LATE:
                ops.BEFORE_CNF_LAUNCH = self.encoder.launch_tnocs        # queued between the flow's hyper conv and the flow (tpointnet2.py)
            try:
                with ops.timed("decode"):
                    y, logp_y, x = self.decode(z, num_points, constant_in_time, truncate_std, sample_contours, y=y, _early=early, frame_ids=frame_ids)
            finally:
                ops.BEFORE_CNF_LAUNCH = None
                if defer and JOIN_TNOCS_LATE:
                    # the T-NOCS regression (a 0.5 ms HBM-bound conv on the side stream) is joined BEHIND the flow's launch, not in front of
                    # it: nothing of the flow reads it, and its workgroups drain while the flow's first ones start.  In the `finally`: a
                    # CasprAccuracyError of an EARLIER call surfacing inside decode() must not leave the side stream unjoined
                    self.encoder.join()
            return y, logp_y, x, tnocs_pred

    def calibrate_rk4_steps(self, x, tol=1e-6, candidates=(1, 2, 4, 8, 16, 32, 64, 128), num_points=512, timestamps=None, max_timestamp=5.0,
                            latent_tol=None, latent_candidates=(1, 2, 4, 8, 16, 32), refine=True, rtol=0.0):
        """Pick the CNF's fixed RK4 step count the way an adaptive solver picks its step: by an error estimate on the
        actual weights and input.  Decodes every sequence of `x` with S and 2S steps (same base samples) for each
        candidate S in ascending order and keeps the first S whose error estimate (16/15) max|x_S - x_2S| (Richardson: the
        step-doubling difference is 15/16 of the S-step error of a 4th-order method) is <= tol; with `refine` (default) the counts BETWEEN the last failing candidate and
        that one are then tried where the S^-4 law predicts they pass (_first_passing: prediction verified by an actual S-vs-2S
        solve), so the result need not be a power of two.  Sets `rk4_steps` on every CNF block; returns (S, {S: difference}) with the
        differences of the counts that were tried.  `rtol` > 0 relaxes the bound to tol + rtol max|x| (torchdiffeq's atol + rtol |x|,
        the form the run-time guard uses with atol = rtol = check_tol); the default is the absolute bound.  With `latent_tol` the latent ODE's steps per interval are chosen FIRST, the
        same way (max|z_L - z_2L| <= latent_tol over the requested stamps), and installed on `latent_ode.rk4_steps`; the return
        value then is (S, diffs, L, latent_diffs).
        The reference's dopri5 runs at atol = rtol = 1e-5 (flow.py:96-99; 1e-3 for the latent ODE, latent_ode_model.py:38,83);
        the defaults of this build (8 steps, 2 per interval) are kept unless this is called."""
        from .cnf import CNF
        blocks = [l for l in self.point_cnf.chain if isinstance(l, CNF) and l.method == "rk4"]       # a dopri5 block has no step count
        guard, self.check_tol = self.check_tol, None          # the candidates below are MEANT to be under-resolved: no guard while choosing
        try:
            return self._calibrate(blocks, x, tol, candidates, num_points, timestamps, max_timestamp, latent_tol, latent_candidates, refine, rtol)
        finally:
            self.check_tol = guard

    def _calibrate(self, blocks, x, tol, candidates, num_points, timestamps, max_timestamp, latent_tol, latent_candidates, refine=True, rtol=0.0):
        with torch.no_grad():
            xs = x                   # every sequence of x (round 4 looked at the first only: the worst one decides)
            z0, _ = self.encode(xs)
            times = xs[:, :, 0, 3] / max_timestamp if timestamps is None else timestamps.view(1, -1).repeat(xs.shape[0], 1).to(xs)
            lat = None
            if latent_tol is not None and self.latent_ode.method == "rk4":        # a dopri5 latent ODE has no step count: left alone
                zs = {}

                def zsol(L):
                    if L not in zs:
                        self.latent_ode.rk4_steps = L
                        zs[L] = self.aggregate_and_solve_latent(z0, times)
                    return zs[L]
                lchosen, ldiffs = _first_passing(lambda L: float((zsol(L) - zsol(2 * L)).abs().max()), latent_candidates, latent_tol * 15.0 / 16.0, refine)
                self.latent_ode.rk4_steps = lchosen
                lat = (lchosen, ldiffs)
            z = self.aggregate_and_solve_latent(z0, times)
            y = torch.randn(z.shape[0], z.shape[1], num_points, self.cnf_args.input_dim, device=x.device)
            sols = {}

            def sol(S):
                if S not in sols:
                    for b in blocks:
                        b.rk4_steps = S
                    sols[S] = self.decode(z, num_points, y=y)[2]
                return sols[S]
            bound = tol + rtol * float(sol(max(candidates)).abs().max()) if rtol > 0 else tol
            bound *= 15.0 / 16.0       # the criterion is on the ERROR of the S-step solution, (16 / 15) max |x_S - x_2S|, not on the difference
            chosen, diffs = _first_passing(lambda S: float((sol(S) - sol(2 * S)).abs().max()), candidates, bound, refine)
        for b in blocks:
            b.rk4_steps = chosen
        self.cnf_args.rk4_steps = chosen
        return (chosen, diffs) if lat is None else (chosen, diffs, lat[0], lat[1])
