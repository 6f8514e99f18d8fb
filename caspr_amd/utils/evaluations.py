"""Reconstruction / T-NOCS evaluation protocols (reference: caspr/utils/evaluations.py:26-295) on the HIP path.

Metric side of BASELINE.json's headline ("sequences/sec + Chamfer-L2"): the paper's protocol evaluates 10 steps x 2048
points, either all steps observed or steps [0,5,9] observed / [1,2,3,4,6,7,8] unobserved (evaluations.py:26-34), with
Chamfer = mean_i min_j |p_i-g_j|^2 + mean_j min_i |.|^2 per frame (evaluations.py:36-44; printed x1000) and the
approximate EMD / N (evaluations.py:45-46, caspr_emd_f32).  The camera-pose evaluation (evaluations.py:297-513) fits the
rigid transform from predicted T-NOCS to the observed points with the correspondence RANSAC of csrc/pose.hip
(ops.ransac_rigid_from_correspondences) in place of Open3D's; its parity with the Open3D release the reference calls is
UNPINNED: the hypotheses come from a seeded counter hash, not from the clock-seeded std::rand.
Differences from the reference, on purpose: bad protocol sizes raise ValueError instead of exit(); the inference
timer synchronises the device (evaluations.py:108-115 does not)."""
import time

import numpy as np
import torch

from .. import ops

PROTOCOL_NUM_STEPS = 10
PROTOCOL_NUM_PTS = 2048
ALL_OBSERVED_STEPS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
ALL_UNOBSERVED_STEPS = []
SPLIT_OBSERVED_STEPS = [0, 5, 9]
SPLIT_UNOBSERVED_STEPS = [1, 2, 3, 4, 6, 7, 8]


def eval_reconstr_frames(pred, gt, with_emd=True):
    """evaluations.py:36-49: pred, gt (F,N,3) on the GPU -> [per-frame Chamfer-L2 (F,), per-frame EMD / N (F,)] numpy."""
    dist1, dist2 = ops.chamfer_distance(pred.contiguous(), gt.contiguous())
    mean_dist = (torch.mean(dist1, dim=1) + torch.mean(dist2, dim=1)).cpu().numpy()
    cur_emd = None
    if with_emd:
        cur_emd = (ops.earth_mover_distance(pred, gt, transpose=False) / pred.size(1)).cpu().numpy()
    return [mean_dist, cur_emd]


def eval_exact_emd_frames(pred, gt, eps=1e-6):
    """pred, gt (F,N,3) on the GPU with the same N <= 2048 -> per-frame EXACT EMD / N (F,) numpy: the optimal one-to-one assignment cost
    (ops.earth_mover_distance_exact, within N * eps of the optimum) on the scale of eval_reconstr_frames' approximate EMD
    (evaluations.py:46), which it is the yardstick for.  A frame that exhausts the bid budget (a target of nearly identical points at
    N >= 1024) has no value: RuntimeError naming those frames."""
    cost, _, _, info = ops.earth_mover_distance_exact(pred, gt, transpose=False, eps=eps, return_match=True)
    bad = (info[:, 0] == 0).nonzero().flatten().cpu().tolist()
    if bad:
        raise RuntimeError("eval_exact_emd_frames: the auction did not converge within its bid budget on frame(s) %s of %d "
                           "(ops.earth_mover_distance_exact: max_bids)" % (bad, cost.shape[0]))
    return (cost / pred.size(1)).cpu().numpy()


def _stats(values, scale=1.0):
    v = np.asarray(values, dtype=np.float64) * scale
    return {"mean": float(np.mean(v)), "median": float(np.median(v)), "std": float(np.std(v))} if v.size else None


def test_shape_recon(model, batches, device, observed_steps=ALL_OBSERVED_STEPS, unobserved_steps=ALL_UNOBSERVED_STEPS,
                     protocol=True, base_samples=None):
    """evaluations.py:51-201.  `batches` yields (pcl_in (B,T,N,4), nocs_out (B,T,N,4)); only the observed steps are
    encoded, all steps are reconstructed at nocs_out's timestamps.  Returns chamfer x1000 statistics for observed /
    unobserved frames, mean NFE and mean inference time.  base_samples: optional list of (B,T,N,3) tensors (parity tests)."""
    model.eval()
    obs, unobs, nfe, times, obs_emd, unobs_emd = [], [], [], [], [], []
    for bi, (pcl_in, nocs_out) in enumerate(batches):
        pcl_in, nocs_out = pcl_in.to(device), nocs_out.to(device)
        B, T, N, _ = pcl_in.size()
        if protocol and T != PROTOCOL_NUM_STEPS:
            raise ValueError('Test protocol requires %d steps, but %d given!' % (PROTOCOL_NUM_STEPS, T))
        if protocol and N != PROTOCOL_NUM_PTS:
            raise ValueError('Test protocol requires %d points, but %d given!' % (PROTOCOL_NUM_PTS, N))
        observed_pcl_in = pcl_in[:, observed_steps, :, :].contiguous()
        y = None if base_samples is None else base_samples[bi].to(device)
        torch.cuda.synchronize(device)
        t0 = time.time()
        _, _, pred_pcl, _ = model.reconstruct(observed_pcl_in, num_points=N, timestamps=nocs_out[0, :, 0, 3],
                                              constant_in_time=False, y=y)
        torch.cuda.synchronize(device)
        times.append(time.time() - t0)
        nfe.append(model.get_nfe())
        gt = nocs_out[:, observed_steps, :, :3].reshape(B * len(observed_steps), N, 3)
        cd, em = eval_reconstr_frames(pred_pcl[:, observed_steps].reshape(B * len(observed_steps), N, 3), gt)
        obs.extend(cd.tolist())
        obs_emd.extend(em.tolist())
        if len(unobserved_steps) > 0:
            gt = nocs_out[:, unobserved_steps, :, :3].reshape(B * len(unobserved_steps), N, 3)
            cd, em = eval_reconstr_frames(pred_pcl[:, unobserved_steps].reshape(B * len(unobserved_steps), N, 3), gt)
            unobs.extend(cd.tolist())
            unobs_emd.extend(em.tolist())
    return {"observed_chamfer_x1000": _stats(obs, 1000.0), "unobserved_chamfer_x1000": _stats(unobs, 1000.0),
            "observed_chamfer": obs, "unobserved_chamfer": unobs,
            "observed_emd_x1000": _stats(obs_emd, 1000.0), "unobserved_emd_x1000": _stats(unobs_emd, 1000.0),
            "observed_emd": obs_emd, "unobserved_emd": unobs_emd,
            "nfe_mean": np.mean(nfe, axis=0).tolist() if nfe else None, "infer_time_mean": float(np.mean(times)) if times else None}


def test_tnocs_regression(model, batches, device, protocol=True):
    """evaluations.py:203-295: mean L2 distance in space and mean |dt| per (sequence, step)."""
    model.eval()
    space, tdiff = [], []
    for pcl_in, nocs_out in batches:
        pcl_in, nocs_out = pcl_in.to(device), nocs_out.to(device)
        B, T, N, _ = pcl_in.size()
        if protocol and (T != PROTOCOL_NUM_STEPS or N != PROTOCOL_NUM_PTS):
            raise ValueError('Test protocol requires %d steps x %d points, but %d x %d given!' % (PROTOCOL_NUM_STEPS, PROTOCOL_NUM_PTS, T, N))
        with torch.no_grad():
            _, pred_tnocs = model.encode(pcl_in)
        diff = pred_tnocs[:, :, :, :3] - nocs_out[:, :, :, :3]
        space.extend(torch.mean(torch.norm(diff, dim=3), dim=2).cpu().numpy().reshape(-1).tolist())
        if pred_tnocs.size(3) > 3:
            tdiff.extend(torch.mean(torch.abs(pred_tnocs[:, :, :, 3] - nocs_out[:, :, :, 3]), dim=2).cpu().numpy().reshape(-1).tolist())
    return {"space": _stats(space), "time": _stats(tdiff)}


def test_observed_camera_pose_ransac(model, batches, device, protocol=True, threshold=0.015, num_hypotheses=5000, seed=0, refine=False):
    """evaluations.py:297-513.  `batches` yields (pcl_in (B,T,N,4), nocs_out (B,T,N,4), pose (B,T,4,4)), the pose as
    DynamicPCLDataset.set_return_pose_data(True) provides it.  Per observed frame the rigid transform from the predicted T-NOCS
    (minus 0.5) to the input points, index for index, by RANSAC (evaluations.py:370-375: ransac_n = 4, threshold 0.015, 5000
    hypotheses; one op call for all B*T frames of a batch), then in f64 on the device (evaluations.py:380-430):
      trans = |t_pred - t_gt|,  rot = degrees(arccos(clip((tr(R_pred^T R_gt) - 1) / 2, -1, 1))),
      point / point_mean = median / mean over points of |R_pred (gt_nocs - 0.5) + t_pred - input|.
    Returns _stats of each ("trans", "rot", "point", "point_mean"), the per-frame lists ("per_frame") and the per-sequence means
    the reference writes to its CSV ("per_sequence"); nothing is written to disk."""
    model.eval()
    per = {"trans": [], "rot": [], "point": [], "point_mean": []}
    steps = None
    for pcl_in, nocs_out, pose in batches:
        pcl_in, nocs_out = pcl_in.to(device), nocs_out.to(device)
        B, T, N, _ = pcl_in.size()
        if protocol and T != PROTOCOL_NUM_STEPS:
            raise ValueError('Test protocol requires %d steps, but %d given!' % (PROTOCOL_NUM_STEPS, T))
        if protocol and N != PROTOCOL_NUM_PTS:
            raise ValueError('Test protocol requires %d points, but %d given!' % (PROTOCOL_NUM_PTS, N))
        if steps is not None and T != steps:
            raise ValueError('every batch needs the same number of steps (%d, then %d)' % (steps, T))
        steps = T
        with torch.no_grad():
            _, pred_tnocs = model.encode(pcl_in)
        # src = predicted T-NOCS - 0.5, dst = the input points; both (B*T,N,4) rows, of which the kernel reads x, y, z
        Tp, _, _, _, _ = ops.ransac_rigid_from_correspondences((pred_tnocs - 0.5).reshape(B * T, N, -1), pcl_in.reshape(B * T, N, -1),
                                                               threshold=threshold, num_hypotheses=num_hypotheses, seed=seed, refine=refine)
        R_pred, t_pred = Tp[:, :3, :3], Tp[:, :3, 3]
        pose = pose.to(device=device, dtype=torch.float64).reshape(B * T, 4, 4)
        R_gt, t_gt = pose[:, :3, :3], pose[:, :3, 3]
        trans = torch.linalg.norm(t_pred - t_gt, dim=1)
        cos = torch.clamp(((R_pred * R_gt).sum(dim=(1, 2)) - 1.0) / 2.0, -1.0, 1.0)    # tr(R_pred^T R_gt) = sum_ij R_pred,ij R_gt,ij
        rot = torch.rad2deg(torch.arccos(cos))
        gt_nocs = (nocs_out[:, :, :, :3] - 0.5).reshape(B * T, N, 3).double()          # f32 subtraction, as the reference's tensors
        inp = pcl_in[:, :, :, :3].reshape(B * T, N, 3).double()
        dist = torch.linalg.norm(torch.matmul(gt_nocs, R_pred.transpose(1, 2)) + t_pred[:, None, :] - inp, dim=2)
        srt = torch.sort(dist, dim=1).values                                             # np.median: the mean of the middle two
        median = srt[:, N // 2] if N % 2 else (srt[:, N // 2 - 1] + srt[:, N // 2]) / 2.0
        for k, v in (("trans", trans), ("rot", rot), ("point", median), ("point_mean", dist.mean(dim=1))):
            per[k].extend(v.cpu().numpy().tolist())
    out = {k: _stats(v) for k, v in per.items()}
    out["per_frame"] = per
    out["per_sequence"] = {k: (np.asarray(v).reshape(-1, steps).mean(axis=1).tolist() if v else []) for k, v in per.items()}
    return out


# keep pytest from collecting the reference-named entry points of this module
test_shape_recon.__test__ = False
test_tnocs_regression.__test__ = False
test_observed_camera_pose_ransac.__test__ = False
