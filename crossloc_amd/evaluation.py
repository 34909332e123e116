"""Evaluation harness either side of `dsacstar.forward_rgb` — our counterpart of the reference's
utils/evaluation.py (scene_coords_eval :135-190, get_pose_err :121-132, scene_coords_printout :193-244) and of
the per-image loop of test_single_task.py:328-366, plus what the reference does not have: batched
localisation (CNN forward + HIP DSAC* per batch) and image-level sharding over the GPUs of a node with ONE
all-gather of the per-image errors (the median is not decomposable, hence gather not reduce).
"""
import numpy as np

import torch

from . import switches


def get_pose_err(gt_pose, est_pose):
    """utils/evaluation.py:121-132.  Translation error (m) and rotation error (deg) between two 4x4
    cam->world matrices.  The reference takes ||cv2.Rodrigues(R_est^T R_gt)||, i.e. the rotation angle;
    computed here from the skew part and the trace (no OpenCV)."""
    gt_pose = np.asarray(gt_pose, np.float64)
    est_pose = np.asarray(est_pose, np.float64)
    transl_err = float(np.linalg.norm(gt_pose[0:3, 3] - est_pose[0:3, 3]))
    r = est_pose[0:3, 0:3].T.dot(gt_pose[0:3, 0:3])
    s = 0.5 * np.linalg.norm([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
    c = 0.5 * (np.trace(r) - 1.0)
    return transl_err, float(np.degrees(np.arctan2(s, c)))


def pose_errors(gt_poses, est_poses):
    """Batched get_pose_err on tensors [K,4,4] (any device) -> (t_err[K] m, r_err[K] deg), float64."""
    g = gt_poses.to(torch.float64)
    e = est_poses.to(torch.float64)
    t_err = torch.linalg.norm(g[:, :3, 3] - e[:, :3, 3], dim=1)
    r = e[:, :3, :3].transpose(1, 2) @ g[:, :3, :3]
    sk = torch.stack([r[:, 2, 1] - r[:, 1, 2], r[:, 0, 2] - r[:, 2, 0], r[:, 1, 0] - r[:, 0, 1]], dim=1)
    s = 0.5 * torch.linalg.norm(sk, dim=1)
    c = 0.5 * (r[:, 0, 0] + r[:, 1, 1] + r[:, 2, 2] - 1.0)
    return t_err, torch.rad2deg(torch.atan2(s, c))


def pick_valid_points(coord_input, nodata_value):
    """utils/learning.py:49-71 with boolean=True: [B,C,N] -> bool [B,N], true where no channel is nodata."""
    return torch.sum(coord_input == nodata_value, dim=1) == 0


def scene_coords_eval(scene_coords, gt_coords, gt_pose, nodata_value, focal_length, image_h, image_w,
                      hypotheses, threshold, inlier_alpha, max_pixel_error, output_subsample, verbose=False):
    """utils/evaluation.py:135-190 — batch size one, same arguments and return tuple
    (t_err, r_err, est_xyz, coords_error over has-data cells, out_pose 4x4).  The reference moves the
    prediction to the CPU before the solver (:161); here it may stay on the GPU."""
    import dsacstar
    gt_pose_np = gt_pose[0].detach().cpu().numpy()
    out_pose = torch.zeros((4, 4))
    dsacstar.forward_rgb(scene_coords, out_pose, hypotheses, threshold, focal_length,
                         float(image_w / 2), float(image_h / 2), inlier_alpha, max_pixel_error, output_subsample)
    t_err, r_err = get_pose_err(gt_pose_np, out_pose.numpy())
    est_xyz = out_pose[0:3, 3].tolist()
    sc = scene_coords.detach().cpu().view(scene_coords.size(0), 3, -1)
    gt = gt_coords.detach().cpu().view(gt_coords.size(0), 3, -1)
    mask = pick_valid_points(gt, nodata_value)
    coords_error = torch.norm(gt - sc, dim=1, p=2)
    coords_error_valdata = coords_error[mask].tolist()
    if verbose:
        print("\nRotation Error: %.2f deg, Translation Error: %.1f m, Mean coord prediction error: %.1f m" % (
            r_err, t_err, float(np.mean(coords_error_valdata)) if coords_error_valdata else float("nan")))
    return t_err, r_err, est_xyz, coords_error_valdata, out_pose.clone()


def accuracy_report(t_err_ls, r_err_ls, coords_error_ls=None):
    """The statistics and the text of utils/evaluation.py:207-230 (errors in metres / degrees; strict `<`)."""
    t = np.asarray(t_err_ls, np.float64)
    r = np.asarray(r_err_ls, np.float64)
    n = max(len(t), 1)
    buckets = [("30m10deg", 30.0, 10.0), ("20m10deg", 20.0, 10.0), ("10m7deg", 10.0, 7.0),
               ("10m10deg", 10.0, 10.0), ("5m5deg", 5.0, 5.0), ("3m3deg", 3.0, 3.0)]
    stats = {name: float(np.sum(np.logical_and(t < tm, r < rd))) / n * 100 for name, tm, rd in buckets}
    stats.update(median_r=float(np.median(r)), median_t=float(np.median(t)), mean_r=float(np.mean(r)),
                 std_r=float(np.std(r)), mean_t=float(np.mean(t)), std_t=float(np.std(t)))
    s = '\nAccuracy:'
    s += '\n30m10deg: %.1f%%\n20m10deg: %.1f%%' % (stats["30m10deg"], stats["20m10deg"])
    s += '\n10m7deg: %.1f%%' % stats["10m7deg"]
    s += '\n10m10deg: %.1f%%' % stats["10m10deg"] + '\n5m5deg: %.1f%%' % stats["5m5deg"]
    s += '\n3m3deg: %.1f%%' % stats["3m3deg"]
    s += "\nMedian Error: %.1f deg, %.2f m" % (stats["median_r"], stats["median_t"])
    s += "\nMean Errors: %.1f plus-minus %.1f deg, %.2f plus-minus %.2f m" % (
        stats["mean_r"], stats["std_r"], stats["mean_t"], stats["std_t"])
    if coords_error_ls is not None and len(coords_error_ls):
        ce = np.asarray(coords_error_ls, np.float64)
        s += "\nCoordinate regression error: mean {:.1f}, std {:.1f}, median {:.1f}".format(
            np.mean(ce), np.std(ce), np.median(ce))
    return stats, s


def selective_accuracy(t_err, r_err, sigma_pos, keep=(1.0, 0.9, 0.75, 0.5)):
    """Accuracy of the frames the solver itself trusts most: frames sorted by ascending predicted position uncertainty
    `sigma_pos` (column `sigma_pos_m` of dsacstar.pose_quality_batch; NaN - no covariance - last, ties by index), and for
    each fraction in `keep` the statistics of accuracy_report over the first ceil(keep * K) frames.  Pure numpy.
    Returns a list of (fraction, frames kept, stats dict), one per fraction."""
    t = np.asarray(t_err, np.float64)
    r = np.asarray(r_err, np.float64)
    s = np.asarray(sigma_pos, np.float64)
    K = len(t)
    order = np.lexsort((np.arange(K), np.where(np.isnan(s), np.inf, s), np.isnan(s)))
    out = []
    for frac in keep:
        n = min(K, int(np.ceil(frac * K)))
        idx = order[:n]
        if n == 0:
            out.append((float(frac), 0, None))
            continue
        out.append((float(frac), n, accuracy_report(t[idx], r[idx])[0]))
    return out


def selective_accuracy_table(t_err, r_err, sigma_pos, keep=(1.0, 0.9, 0.75, 0.5)):
    """The text crossloc_amd.pose_quality_single_task prints under the usual report."""
    s = "\nSelective accuracy (frames kept by ascending sigma_pos_m):"
    s += "\n  keep  frames  median_t[m]  median_r[deg]  5m5deg  3m3deg"
    for frac, n, st in selective_accuracy(t_err, r_err, sigma_pos, keep):
        if st is None:
            s += "\n  %4.0f%%  %6d  (no frames)" % (frac * 100, n)
        else:
            s += "\n  %4.0f%%  %6d  %11.3f  %13.3f  %5.1f%%  %5.1f%%" % (
                frac * 100, n, st["median_t"], st["median_r"], st["5m5deg"], st["3m3deg"])
    return s


def scene_coords_printout(t_err_ls, r_err_ls, est_xyz_ls, coords_error_ls, testing_log=None, section="test"):
    """utils/evaluation.py:193-244 without the numpy pose dumps: prints (and appends to testing_log)."""
    coords = np.concatenate([np.asarray(c, np.float64).ravel() for c in coords_error_ls]) if len(coords_error_ls) else None
    stats, s = accuracy_report(t_err_ls, r_err_ls, coords)
    print(s)
    if testing_log:
        with open(testing_log, 'a') as f:
            f.write("{:s} Evaluation on section {:s} {:s}".format('=' * 20, section, '=' * 20) + '\n')
            f.write(s)
            f.write('\n')
    return stats


# ------------------------------------------------------------------------------------------ semantics metrics

def confusion_matrix(gt_label, pred_label, num_class):
    """Rows = ground truth, columns = prediction; labels outside [0, num_class) are ignored
    (utils/evaluation.py:373-378).  Tensors [..] of equal shape, any device; returns int64 [num_class, num_class]."""
    g = gt_label.reshape(-1).to(torch.int64)
    p = pred_label.reshape(-1).to(device=g.device, dtype=torch.int64)
    m = (g >= 0) & (g < num_class)
    idx = num_class * g[m] + p[m]
    return torch.bincount(idx, minlength=num_class * num_class).reshape(num_class, num_class)


def segmentation_metrics(cm):
    """Pixel accuracy, mean IoU and frequency-weighted IoU of one confusion matrix (utils/evaluation.py:346-371;
    classes absent from both ground truth and prediction are left out of the mean like np.nanmean does)."""
    cm = np.asarray(cm.cpu() if isinstance(cm, torch.Tensor) else cm, np.float64)
    diag = np.diag(cm)
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = diag.sum() / cm.sum()
        iu = diag / (cm.sum(axis=1) + cm.sum(axis=0) - diag)
        freq = cm.sum(axis=1) / cm.sum()
    miou = float(np.nanmean(iu))
    fwiou = float((freq[freq > 0] * iu[freq > 0]).sum())
    return float(acc), miou, fwiou


def semantic_eval(semantic_logits, gt_label, mute=False):
    """utils/evaluation.py:388-415: per-image accuracy / mIoU / fwIoU of full-size class logits [B,6,H,W] against
    gt_label [B,1,H,W].  Returns (class_prediction [B,H,W] on the CPU, miou[B], fwiou[B], acc[B]) like the reference;
    arg-max and the confusion matrices are computed on the logits' device."""
    num_class = semantic_logits.shape[1]
    gt = gt_label.squeeze(1)
    pred = torch.argmax(semantic_logits, dim=1)               # arg-max of log-softmax = arg-max of the logits
    assert gt.shape == pred.shape
    miou_ls, fwiou_ls, acc_ls = [], [], []
    for g, p in zip(gt, pred):
        acc, miou, fwiou = segmentation_metrics(confusion_matrix(g.to(p.device), p, num_class))
        acc_ls.append(acc); miou_ls.append(miou); fwiou_ls.append(fwiou)
    miou_ls, fwiou_ls, acc_ls = np.array(miou_ls), np.array(fwiou_ls), np.array(acc_ls)
    if not mute:
        print("Metrics within the batch: mean accuracy: {:.2f}%, mean IoU: {:.2f}%, frequency weighted IoU: {:.2f}%".
              format(acc_ls.mean() * 100, miou_ls.mean() * 100, fwiou_ls.mean() * 100))
    return pred.cpu(), miou_ls, fwiou_ls, acc_ls


# ------------------------------------------------------------------------------------------ sharded evaluation

def shard_indices(num_images, rank, world_size):
    """Image i belongs to rank i % world_size."""
    return list(range(rank, num_images, world_size))


def gather_errors(local_vals, num_images, rank, world_size, group=None):
    """All-gather per-image values of the i%R sharding into the global order.

    local_vals: tensor [ceil-ish(K/R), D] on this rank's device (rows for images rank, rank+R, ...).
    Ragged shards are padded with NaN to ceil(K/R) rows and the padding dropped after
    the gather, so every rank ends up with the identical [K, D] tensor whatever R is."""
    per = (num_images + world_size - 1) // world_size
    D = local_vals.shape[1]
    pad = torch.full((per, D), float("nan"), dtype=local_vals.dtype, device=local_vals.device)
    pad[:local_vals.shape[0]] = local_vals
    if world_size == 1 and group is None:
        gathered = [pad]
    else:                                                    # (a one-rank group passed explicitly still runs the collective)
        import torch.distributed as dist
        gathered = [torch.empty_like(pad) for _ in range(world_size)]
        dist.all_gather(gathered, pad, group=group)
    out = torch.empty((per * world_size, D), dtype=local_vals.dtype, device=local_vals.device)
    for r in range(world_size):
        out[r::world_size] = gathered[r]
    return out[:num_images]


def _focal_args(focal, n):
    """focal: one number for the whole batch, or one per frame (sequence / tensor: the dataset computes it per frame from
    calibration/*.txt scaled by the stored image height, dataloader/dataloader.py:263-266).  -> (scalar, focals kwarg)."""
    import numbers
    if isinstance(focal, (numbers.Real, np.generic)):              # Python and numpy scalars alike
        return float(focal), None
    f = torch.as_tensor(focal, dtype=torch.float32).reshape(-1)
    if f.numel() == 1:                                             # 0-dim / one-element tensor or sequence: one focal for all
        return float(f[0]), None
    if f.numel() != n:
        raise RuntimeError("expected %d focal lengths, got %d" % (n, f.numel()))
    return float(f[0]), f


def cell_mask(sigma=None, max_sigma=None, class_map=None, exclude_classes=(), labels=None, nodata_value=-1, sub=8):
    """The per-cell validity mask of dsacstar.forward_rgb_masked_batch: uint8 [B,Ho,Wo] on the device of its inputs, 1 = usable,
    the AND of the criteria given (at least one):
      sigma, max_sigma   sigma [B,Ho,Wo] (e.g. the uncertainty channel pred[:, 3] of an MLE network): usable iff sigma <= max_sigma
                         (a NaN sigma is not usable)
      class_map, exclude_classes   integer classes (e.g. the arg-max of the semantics network), [B,Ho,Wo] per cell or full size
                         [B,Ho*sub,Wo*sub], which is read at the cell centres (sub*x + sub//2, sub*y + sub//2); usable iff the
                         class is not in exclude_classes.  A map that comes alone is taken per cell.
      labels, nodata_value   a label map [B,C,Ho,Wo] or [B,Ho,Wo]: usable iff no channel of the cell is nodata_value
                         (pick_valid_points)
    Plain torch ops on small tensors: plumbing, not a hot path."""
    if (sigma is None) != (max_sigma is None):
        raise RuntimeError("cell_mask: sigma and max_sigma go together")
    parts, shape = [], None
    if sigma is not None:
        if not isinstance(sigma, torch.Tensor) or sigma.dim() != 3:
            raise RuntimeError("cell_mask: sigma must be a [B,Ho,Wo] tensor")
        parts.append(sigma <= float(max_sigma))
        shape = tuple(sigma.shape)
    if labels is not None:
        if not isinstance(labels, torch.Tensor) or labels.dim() not in (3, 4):
            raise RuntimeError("cell_mask: labels must be a [B,C,Ho,Wo] or [B,Ho,Wo] tensor")
        lab = labels if labels.dim() == 4 else labels[:, None]
        has_data = pick_valid_points(lab, nodata_value)
        if shape is not None and tuple(has_data.shape) != shape:
            raise RuntimeError("cell_mask: labels %s do not match the %s cells of sigma" % (tuple(labels.shape), shape))
        parts.append(has_data)
        shape = tuple(has_data.shape)
    if class_map is not None:
        if not isinstance(class_map, torch.Tensor) or class_map.dim() != 3 or class_map.dtype.is_floating_point:
            raise RuntimeError("cell_mask: class_map must be an integer [B,H,W] tensor")
        cm = class_map
        if shape is not None and tuple(cm.shape) != shape:
            full = (shape[0], shape[1] * int(sub), shape[2] * int(sub))
            if tuple(cm.shape) != full:
                raise RuntimeError("cell_mask: class_map %s is neither per cell %s nor full size %s" % (tuple(cm.shape), shape, full))
            cm = cm[:, int(sub) // 2::int(sub), int(sub) // 2::int(sub)]
        keep = torch.ones(cm.shape, dtype=torch.bool, device=cm.device)
        for c in exclude_classes:
            keep &= cm != int(c)
        parts.append(keep)
    if not parts:
        raise RuntimeError("cell_mask needs at least one criterion: sigma and max_sigma, class_map or labels")
    out = parts[0]
    for p in parts[1:]:
        out = out & p.to(out.device)
    return out.to(torch.uint8).contiguous()


# the passes behind the masked RGB solver, over the mask it read (dsacstar.refine_pose_masked_batch: the plain re-fit over the
# inliers and the sigma-weighted one; dsacstar.pose_quality_masked_batch)
MASKED_REFINE_MODES = ("masked_inliers", "masked_sigma")


def _is_masked_quality(quality):
    return isinstance(quality, str) and quality == "masked"


def _check_mask_mode(mask, mask_max_sigma, quality, depth, cam_coords, refine, mask_sampler="reject"):
    """The mask reaches the RGB solver and, through the masked modes, the two passes behind it; `mask_sampler` is the masked
    solver's (dsacstar.MASK_SAMPLERS), so any but the default needs a mask.  -> whether the masked solver runs"""
    import dsacstar
    if mask_sampler not in dsacstar.MASK_SAMPLERS:
        raise RuntimeError("unknown mask_sampler %r (one of %s)" % (mask_sampler, ", ".join(dsacstar.MASK_SAMPLERS)))
    asked = [("quality", quality)] if _is_masked_quality(quality) else []
    if isinstance(refine, str) and refine in MASKED_REFINE_MODES:
        asked.append(("refine", refine))
    if mask_sampler != "reject":
        asked.append(("mask_sampler", mask_sampler))
    if mask is None and mask_max_sigma is None:
        for name, mode in asked:
            raise RuntimeError("%s=%r runs behind the masked RGB solver: it needs mask= or mask_max_sigma=" % (name, mode))
        return False
    if mask is not None and mask_max_sigma is not None:
        raise RuntimeError("mask and mask_max_sigma: pass one of them (AND a mask of your own with cell_mask(sigma=...))")
    for name, on in (("depth", depth is not None), ("cam_coords", cam_coords is not None)):
        if on:
            raise RuntimeError("mask together with %s is not supported: the mask reaches the RGB solver and its passes only" % name)
    if quality and not _is_masked_quality(quality):
        raise RuntimeError("mask together with quality=%r: that pass reads every cell; the pass over the mask is "
                           "quality=\"masked\"" % (quality,))
    if refine and not (isinstance(refine, str) and refine in MASKED_REFINE_MODES):
        raise RuntimeError("mask together with refine=%r: that pass reads every cell; the passes over the mask are "
                           "refine=\"masked_inliers\" and refine=\"masked_sigma\"" % (refine,))
    return True


def _solver_mask(mask, mask_max_sigma, pred, nt):
    """The mask the solver reads: the caller's, or sigma <= mask_max_sigma on the prediction's uncertainty channel"""
    if mask is not None:
        return mask
    if pred.shape[1] <= nt:
        raise RuntimeError("mask_max_sigma needs the network's uncertainty channel, and this network has none; pass mask=")
    return cell_mask(sigma=pred[:, nt], max_sigma=mask_max_sigma)


def _is_rgbd_quality(quality):
    return isinstance(quality, str) and quality == "rgbd"


def _check_quality_mode(quality, depth, cam_coords):
    """`quality`: False, True (the reprojection pass), "rgbd" (the 3-D pass, which needs the RGB-D solver's inputs) or "masked"
    (the reprojection pass over the solver's mask; _check_mask_mode has seen to the mask)"""
    if isinstance(quality, str) and quality not in ("rgbd", "masked"):
        raise RuntimeError("quality must be False, True or one of \"rgbd\" and \"masked\", got %r" % (quality,))
    if _is_rgbd_quality(quality) and depth is None and cam_coords is None:
        raise RuntimeError("quality=\"rgbd\" rates the RGB-D solver's pose: it needs depth or cam_coords")


def _check_refine_mode(refine, depth, cam_coords):
    """`refine`: False, "inliers" (unweighted re-fit over the inliers) or "sigma" (weighted by the predicted uncertainty);
    the pass re-fits the RGB solver's pose by its reprojection residuals, so it does not go with the RGB-D solver.
    "masked_inliers" / "masked_sigma": the same two over the masked solver's mask (_check_mask_mode has seen to the mask)"""
    if refine is False or refine is None:
        return False
    if refine in RGBD_REFINE_MODES:
        if depth is None and cam_coords is None:
            raise RuntimeError("refine=%r re-fits the RGB-D solver's pose: it needs depth or cam_coords" % (refine,))
        return True
    if refine in MASKED_REFINE_MODES:
        return True
    if refine not in ("inliers", "sigma"):
        raise RuntimeError("refine must be False, \"inliers\", \"sigma\", \"rgbd_inliers\", \"rgbd_sigma\", \"masked_inliers\" or "
                           "\"masked_sigma\", got %r" % (refine,))
    if depth is not None or cam_coords is not None:
        raise RuntimeError("refine=%r re-fits the RGB solver's pose: it does not take depth or cam_coords" % (refine,))
    return True


# the refinement behind the RGB-D solver (dsacstar.refine_pose_rgbd_batch): the plain re-fit over the inliers, and the re-fit
# under the per-cell information matrix of sigma, depth_sigma and depth_rel
RGBD_REFINE_MODES = ("rgbd_inliers", "rgbd_sigma")


def _refine_sigma(refine, sigma, pred, nt):
    """The sigma map the refinement reads: None for the "..inliers" modes; for "sigma" / "rgbd_sigma" / "masked_sigma" the side
    input if given, otherwise the uncertainty channel of the prediction (a strided channel view, read in place)"""
    if refine not in ("sigma", "rgbd_sigma", "masked_sigma"):
        return None
    if sigma is not None:
        return sigma
    if pred.shape[1] <= nt:
        raise RuntimeError("refine=\"%s\" needs the network's uncertainty channel, and this network has none; pass sigma= "
                           "or use refine=\"%s\"" % (refine, refine.replace("sigma", "inliers")))
    return pred[:, nt]


def _refine_rgbd(refine, coords, cam_coords, depth, sg, poses, rgbd_threshold, max_dist_error, depth_sigma, depth_rel,
                 sigma_floor_m, intr):
    """The RGB-D refinement behind the RGB-D solver on the current stream -> (refined poses, rows).  "rgbd_inliers" is the plain
    form: neither map nor depth_rel is passed on."""
    import dsacstar
    weighted = refine == "rgbd_sigma"
    return dsacstar.refine_pose_rgbd_batch(coords, cam_coords, sg, poses, rgbd_threshold, max_dist_error,
                                           depthSigma=depth_sigma if weighted else None,
                                           depthRel=depth_rel if weighted else 0.0, sigmaFloorM=sigma_floor_m, depth=depth, **intr)


def _masked_passes(refine, quality, coords, m, sg, poses, thr, f0, ppx, ppy, alpha, max_err, sub, sigma_floor_px, focals):
    """The passes behind the masked RGB solver on the current stream, all over the mask `m` it read: the refinement, then the
    quality pass, which rates the refined pose.  -> (poses, tail) with tail = ([quality rows][, refine rows])"""
    import dsacstar
    tail = ()
    if refine:
        poses, refine_rows = dsacstar.refine_pose_masked_batch(coords, m, sg, poses, thr, f0, ppx, ppy, max_err, sub,
                                                               sigmaFloorPx=sigma_floor_px, focals=focals)
        tail = (refine_rows,)
    if quality:
        tail = (dsacstar.pose_quality_masked_batch(coords, m, poses, thr, f0, ppx, ppy, alpha, max_err, sub, focals=focals),) + tail
    return poses, tail


def localize_batch(network, images, n_hyp, focal, image_h, image_w, image0=0, image_stride=1,
                   threshold=10.0, inlier_alpha=100.0, max_pixel_error=100.0, scene_coords=None, plant=None,
                   quality=False, depth=None, cam_coords=None, rgbd_threshold=10.0, max_dist_error=100.0,
                   refine=False, sigma=None, sigma_floor_px=1.0, depth_sigma=None, depth_rel=0.0, sigma_floor_m=0.01,
                   mask=None, mask_max_sigma=None, mask_sampler="reject"):
    """One batch of the test_single_task.py:347-366 loop on the GPU: eval-mode CNN forward, sigma dropped
    (:354) unless `refine="sigma"` asks for it, HIP DSAC* on all images of the batch.  Returns (poses [B,4,4] cuda,
    predictions [B,4,Ho,Wo]).
    `refine`: "inliers" or "sigma" enqueues the pose refinement (dsacstar.refine_pose_batch) behind the RGB solver on the
    solver's stream: an iteratively re-weighted re-fit over the inliers, unweighted or weighted by the per-cell standard
    deviation `sigma` [B,Ho,Wo] (a side input like `scene_coords`; default: the prediction's uncertainty channel, RuntimeError
    if the network has none) with the pixel floor `sigma_floor_px`.  The first returned value is then the REFINED poses and the
    refinement's rows [B,64] float64 are appended as the LAST value; a `quality=True` pass runs behind the refinement and
    rates the refined pose.  Not with `depth` / `cam_coords`.
    `refine`: "rgbd_inliers" or "rgbd_sigma" (only with `depth` or `cam_coords`, RuntimeError without) enqueues the RGB-D
    refinement (dsacstar.refine_pose_rgbd_batch) behind the RGB-D solver on its stream: the plain re-fit over the inliers of the
    metric 3-D residuals, or the re-fit under a 3x3 information matrix per cell from `sigma` (as above), `depth_sigma`
    [B,Ho,Wo] (the standard deviation of the depth in metres, e.g. a depth network's uncertainty channel; optional), the relative
    depth noise `depth_rel` and the floor `sigma_floor_m` in metres.  The refined poses come first and the rows [B,64] last; a
    `quality="rgbd"` pass behind it rates the refined pose.
    `quality=True`: the pose-quality pass (dsacstar.pose_quality_batch) is enqueued directly behind the solver on the
    solver's stream and its rows [B,64] float64 are returned as a third value.
    `focal`: a number, or one focal length per frame.
    `scene_coords` overrides the solver input (synthetic scenes: untrained weights do not predict a scene).
    `plant` [B,3,Ho,Wo]: written into the coordinate channels of the network output after the head; the solver then
    consumes the network's own output tensor (the strided `pred[:, :3]` view) exactly as with trained weights.
    `depth` [B,Ho,Wo] or `cam_coords` [B,3,Ho,Wo] (at most one; off by default): the RGB-D solver
    (dsacstar.forward_rgbd_batch: Kabsch hypotheses from the cells' camera coordinates) runs in place of the RGB one, with
    `rgbd_threshold` and `max_dist_error` in centimetres; `quality=True` still rates the pose by its reprojection residuals.
    `quality="rgbd"` (only with `depth` or `cam_coords`): the RGB-D pose-quality pass (dsacstar.pose_quality_rgbd_batch) runs
    behind the RGB-D solver instead and rates the pose by its metric 3-D residuals; its rows [B,64] are the third value
    (status and sigma_pos_m in the columns of the RGB row, so selective_accuracy takes either).
    `mask` (uint8 / bool [B,Ho,Wo], nonzero = usable; see cell_mask) or `mask_max_sigma` (the mask sigma <= mask_max_sigma from
    the prediction's uncertainty channel; RuntimeError if the network has none): the masked RGB solver
    (dsacstar.forward_rgb_masked_batch) runs in place of the plain one and its status [B] int32 (1: fewer than four usable
    cells, identity pose) is appended as the LAST value.  The passes behind it take the same mask tensor through modes of their
    own: `refine="masked_inliers"` / `"masked_sigma"` (dsacstar.refine_pose_masked_batch, on the solver's stream) and
    `quality="masked"` (dsacstar.pose_quality_masked_batch, behind the refinement: it rates the refined pose); the return is
    then (poses, pred[, quality rows][, refine rows], status) with the refined poses first.  These modes need a mask
    (RuntimeError without); a mask with `depth` / `cam_coords`, with `quality=True` / `"rgbd"` or with an unmasked `refine` mode
    raises RuntimeError (those passes read every cell).  `mask_sampler` (dsacstar.MASK_SAMPLERS; default "reject"): how the masked
    solver draws the cells of a try; "compact" draws from the usable cells only, which keeps the number of tries at the unmasked
    solver's level under a mask that keeps a minority of cells.  The masked passes work behind either sampler (they take a pose).
    A sampler other than "reject" without a mask raises RuntimeError.  Without a mask nothing changes."""
    import dsacstar
    if depth is not None and cam_coords is not None:
        raise RuntimeError("localize_batch takes at most one of depth and cam_coords")
    masked = _check_mask_mode(mask, mask_max_sigma, quality, depth, cam_coords, refine, mask_sampler)
    _check_quality_mode(quality, depth, cam_coords)
    refine = _check_refine_mode(refine, depth, cam_coords) and refine
    with torch.no_grad():
        pred = network(images)
    nt = network.num_task_channel
    if plant is not None:
        pred[:, :nt].copy_(plant)
    coords = pred[:, :nt] if scene_coords is None else scene_coords
    poses = torch.zeros((coords.shape[0], 4, 4), dtype=torch.float32, device=coords.device)
    f0, focals = _focal_args(focal, coords.shape[0])
    if depth is not None or cam_coords is not None:
        dsacstar.forward_rgbd_batch(coords, cam_coords, poses, n_hyp, rgbd_threshold, inlier_alpha, max_dist_error,
                                    image0=image0, image_stride=image_stride, depth=depth, focalLength=f0,
                                    ppointX=float(image_w / 2), ppointY=float(image_h / 2),
                                    subSampling=network.OUTPUT_SUBSAMPLE, focals=focals)
    elif masked:
        m = _solver_mask(mask, mask_max_sigma, pred, nt)                      # built once, read by the solver and its passes
        status = dsacstar.forward_rgb_masked_batch(coords, m, poses, n_hyp, threshold,
                                                   f0, float(image_w / 2), float(image_h / 2), inlier_alpha, max_pixel_error,
                                                   network.OUTPUT_SUBSAMPLE, image0=image0, image_stride=image_stride,
                                                   focals=focals, sampler=mask_sampler)
        poses, tail = _masked_passes(refine, quality, coords, m, _refine_sigma(refine, sigma, pred, nt), poses, threshold, f0,
                                     float(image_w / 2), float(image_h / 2), inlier_alpha, max_pixel_error,
                                     network.OUTPUT_SUBSAMPLE, sigma_floor_px, focals)
        return (poses, pred) + tail + (status,)
    else:
        dsacstar.forward_rgb_batch(coords, poses, n_hyp, threshold, f0, float(image_w / 2), float(image_h / 2),
                                   inlier_alpha, max_pixel_error, network.OUTPUT_SUBSAMPLE,
                                   image0=image0, image_stride=image_stride, focals=focals)
    tail = ()
    if refine in RGBD_REFINE_MODES:
        intr = dict(focalLength=f0, ppointX=float(image_w / 2), ppointY=float(image_h / 2), subSampling=network.OUTPUT_SUBSAMPLE,
                    focals=focals)
        poses, refine_rows = _refine_rgbd(refine, coords, cam_coords, depth, _refine_sigma(refine, sigma, pred, nt), poses,
                                          rgbd_threshold, max_dist_error, depth_sigma, depth_rel, sigma_floor_m, intr)
        tail = (refine_rows,)
    elif refine:
        poses, refine_rows = dsacstar.refine_pose_batch(coords, _refine_sigma(refine, sigma, pred, nt), poses, threshold, f0,
                                                        float(image_w / 2), float(image_h / 2), max_pixel_error,
                                                        network.OUTPUT_SUBSAMPLE, sigmaFloorPx=sigma_floor_px, focals=focals)
        tail = (refine_rows,)
    if _is_rgbd_quality(quality):
        rows = dsacstar.pose_quality_rgbd_batch(coords, cam_coords, poses, rgbd_threshold, inlier_alpha, max_dist_error,
                                                depth=depth, focalLength=f0, ppointX=float(image_w / 2),
                                                ppointY=float(image_h / 2), subSampling=network.OUTPUT_SUBSAMPLE, focals=focals)
        return (poses, pred, rows) + tail
    if quality:
        rows = dsacstar.pose_quality_batch(coords, poses, threshold, f0, float(image_w / 2), float(image_h / 2),
                                           inlier_alpha, max_pixel_error, network.OUTPUT_SUBSAMPLE, focals=focals)
        return (poses, pred, rows) + tail
    return (poses, pred) + tail


class PipelinedLocalizer:
    """Software pipeline over batches on HIP streams.  The CNN of a batch runs as `cnn_streams` sub-batches on their own
    streams (with 2, the MFMA-bound GEMMs of one overlap the HBM-bound Winograd transforms / GroupNorm passes of the
    other: +9 % images/s at 24 frames; 1 by default), and the DSAC* solver of batch s (24 workgroups, latency-bound: it cannot fill 256 CUs on its
    own) runs on a side stream under the CNN of batch s+1; events order solver(s) after CNN(s).  The reference
    serialises the two stages per image (GPU forward, .cpu(), CPU solver: test_single_task.py:347-363)."""

    def __init__(self, network, n_hyp, focal, image_h, image_w, threshold=10.0, inlier_alpha=100.0,
                 max_pixel_error=100.0, cnn_streams=1):
        self.net, self.n_hyp, self.focal = network, n_hyp, focal
        self.h, self.w = image_h, image_w
        self.thr, self.alpha, self.maxerr = threshold, inlier_alpha, max_pixel_error
        # (round 5) the solver's stream has the HIGHER priority: its 95 workgroups (64.8 KB of LDS each) otherwise queue behind the
        # persistent workgroups of the next batch's stem and GEMM kernels, and both stages run slow for 5 ms instead of the 2 ms
        # the solver needs when it gets its CUs at once (XL_SOLVER_PRIORITY=0: equal priorities, the round-4 behaviour)
        prio = -1 if switches.live("XL_SOLVER_PRIORITY") else 0
        self.side = torch.cuda.Stream(priority=prio)
        self.cnn = [torch.cuda.Stream() for _ in range(max(1, cnn_streams))]

    def forward_cnn(self, images, plant=None):
        """The network on `images`, split over the CNN streams.  Returns (predictions, events): the prediction tensor is
        complete once every event has fired (the caller's stream is NOT made to wait).  `plant`: see localize_batch."""
        main = torch.cuda.current_stream()
        n = min(len(self.cnn), images.shape[0])
        bounds = [round(i * images.shape[0] / n) for i in range(n + 1)]
        nt = self.net.num_task_channel
        outs, events = [], []
        for i in range(n):
            st = self.cnn[i]
            st.wait_stream(main)                           # the images (and `plant`) are ready on the caller's stream
            with torch.cuda.stream(st), torch.no_grad():
                outs.append(self.net(images[bounds[i]:bounds[i + 1]], plan_slot=i + 1))
                if plant is not None:
                    outs[-1][:, :nt].copy_(plant[bounds[i]:bounds[i + 1]])
                ev = torch.cuda.Event()
                ev.record(st)
                events.append(ev)
        if n == 1:
            return outs[0], events
        with torch.cuda.stream(self.cnn[0]):
            for ev in events[1:]:
                self.cnn[0].wait_event(ev)
            pred = torch.cat(outs, 0)
            ev = torch.cuda.Event()
            ev.record(self.cnn[0])
        for o, st in zip(outs, self.cnn):
            o.record_stream(self.cnn[0])
        return pred, [ev]

    def submit(self, images, image0=0, image_stride=1, scene_coords=None, plant=None, quality=False, depth=None,
               cam_coords=None, rgbd_threshold=10.0, max_dist_error=100.0, refine=False, sigma=None, sigma_floor_px=1.0,
               depth_sigma=None, depth_rel=0.0, sigma_floor_m=0.01, mask=None, mask_max_sigma=None, mask_sampler="reject"):
        """Enqueue one batch; returns (poses [B,4,4], predictions).  Both are valid after finish() (or after
        synchronising the side stream).  `quality=True`: the pose-quality pass runs directly behind the solver on the
        side stream and its rows [B,64] float64 are returned as a third value.  `depth` / `cam_coords` (at most one): the
        RGB-D solver runs in place of the RGB one, as in localize_batch; `quality="rgbd"` (only with them): the RGB-D
        pose-quality pass runs behind it instead of the reprojection pass.  `refine` ("inliers" / "sigma"), `sigma` and
        `sigma_floor_px` as in localize_batch: the refinement runs behind the RGB solver on the side stream, the first value
        is the refined poses, its rows [B,64] are the last value, and a `quality=True` pass rates the refined pose.
        `refine` "rgbd_inliers" / "rgbd_sigma" with `depth_sigma`, `depth_rel` and `sigma_floor_m` (only with `depth` or
        `cam_coords`): the RGB-D refinement runs behind the RGB-D solver on the side stream, as in localize_batch.
        `mask` / `mask_max_sigma` as in localize_batch: the masked RGB solver runs on the side stream and its status [B] int32 is
        appended as the last value; `refine="masked_inliers"` / `"masked_sigma"` and `quality="masked"` run the passes over the
        same mask behind it on the side stream, returned as (poses, pred[, quality rows][, refine rows], status).  Not with
        `depth` / `cam_coords` or the unmasked `quality` / `refine` modes.  `mask_sampler` as in localize_batch (only with a mask)."""
        import dsacstar
        if depth is not None and cam_coords is not None:
            raise RuntimeError("submit takes at most one of depth and cam_coords")
        masked = _check_mask_mode(mask, mask_max_sigma, quality, depth, cam_coords, refine, mask_sampler)
        _check_quality_mode(quality, depth, cam_coords)
        refine = _check_refine_mode(refine, depth, cam_coords) and refine
        pred, events = self.forward_cnn(images, plant)
        coords = pred[:, :self.net.num_task_channel] if scene_coords is None else scene_coords
        poses = torch.empty((coords.shape[0], 4, 4), dtype=torch.float32, device=coords.device)   # (the solver writes all 16)
        for ev in events:
            self.side.wait_event(ev)
        self.side.wait_stream(torch.cuda.current_stream())      # `poses` / `scene_coords` come from the caller's stream
        with torch.cuda.stream(self.side):
            if depth is not None or cam_coords is not None:
                f0, focals = _focal_args(self.focal, coords.shape[0])
                dsacstar.forward_rgbd_batch(coords, cam_coords, poses, self.n_hyp, rgbd_threshold, self.alpha, max_dist_error,
                                            image0=image0, image_stride=image_stride, depth=depth, focalLength=f0,
                                            ppointX=float(self.w / 2), ppointY=float(self.h / 2),
                                            subSampling=self.net.OUTPUT_SUBSAMPLE, focals=focals)
                (depth if depth is not None else cam_coords).record_stream(self.side)
            elif masked:
                f0, focals = _focal_args(self.focal, coords.shape[0])
                m = _solver_mask(mask, mask_max_sigma, pred, self.net.num_task_channel)     # built once, on the side stream
                solved = poses
                status = dsacstar.forward_rgb_masked_batch(coords, m, solved, self.n_hyp, self.thr, f0, float(self.w / 2),
                                                           float(self.h / 2), self.alpha, self.maxerr, self.net.OUTPUT_SUBSAMPLE,
                                                           image0=image0, image_stride=image_stride, focals=focals,
                                                           sampler=mask_sampler)
                poses, masked_tail = _masked_passes(refine, quality, coords, m,
                                                    _refine_sigma(refine, sigma, pred, self.net.num_task_channel), solved, self.thr,
                                                    f0, float(self.w / 2), float(self.h / 2), self.alpha, self.maxerr,
                                                    self.net.OUTPUT_SUBSAMPLE, sigma_floor_px, focals)
                solved.record_stream(self.side)
                for side_input in (mask, sigma if refine else None):
                    if side_input is not None:
                        side_input.record_stream(self.side)
            else:
                dsacstar.forward_rgb_batch(coords, poses, self.n_hyp, self.thr, self.focal, float(self.w / 2),
                                           float(self.h / 2), self.alpha, self.maxerr, self.net.OUTPUT_SUBSAMPLE,
                                           image0=image0, image_stride=image_stride)
            if masked:
                pass                                        # its passes ran above, over the solver's mask
            elif refine in RGBD_REFINE_MODES:
                sg = _refine_sigma(refine, sigma, pred, self.net.num_task_channel)
                solved = poses
                intr = dict(focalLength=f0, ppointX=float(self.w / 2), ppointY=float(self.h / 2),
                            subSampling=self.net.OUTPUT_SUBSAMPLE, focals=focals)
                poses, refine_rows = _refine_rgbd(refine, coords, cam_coords, depth, sg, solved, rgbd_threshold, max_dist_error,
                                                  depth_sigma, depth_rel, sigma_floor_m, intr)
                solved.record_stream(self.side)
                for side_input in (sigma, depth_sigma):
                    if side_input is not None:
                        side_input.record_stream(self.side)
            elif refine:
                f0, focals = _focal_args(self.focal, coords.shape[0])
                sg = _refine_sigma(refine, sigma, pred, self.net.num_task_channel)
                solved = poses
                poses, refine_rows = dsacstar.refine_pose_batch(coords, sg, solved, self.thr, f0, float(self.w / 2),
                                                                float(self.h / 2), self.maxerr, self.net.OUTPUT_SUBSAMPLE,
                                                                sigmaFloorPx=sigma_floor_px, focals=focals)
                solved.record_stream(self.side)
                if sigma is not None:
                    sigma.record_stream(self.side)
            if masked:
                pass
            elif _is_rgbd_quality(quality):
                rows = dsacstar.pose_quality_rgbd_batch(coords, cam_coords, poses, rgbd_threshold, self.alpha, max_dist_error,
                                                        depth=depth, focalLength=f0, ppointX=float(self.w / 2),
                                                        ppointY=float(self.h / 2), subSampling=self.net.OUTPUT_SUBSAMPLE,
                                                        focals=focals)
            elif quality:
                rows = dsacstar.pose_quality_batch(coords, poses, self.thr, self.focal, float(self.w / 2), float(self.h / 2),
                                                   self.alpha, self.maxerr, self.net.OUTPUT_SUBSAMPLE)
        pred.record_stream(self.side)
        poses.record_stream(self.side)
        tail = ()
        if masked:
            # allocated on the side stream, read by the caller's after finish()
            for t in (poses, status) + masked_tail:
                t.record_stream(torch.cuda.current_stream())
            return (poses, pred) + masked_tail + (status,)
        if refine:
            # allocated on the side stream, read by the caller's after finish()
            poses.record_stream(torch.cuda.current_stream())
            refine_rows.record_stream(torch.cuda.current_stream())
            tail = (refine_rows,)
        if quality:
            rows.record_stream(torch.cuda.current_stream())  # allocated on the side stream, read by the caller's after finish()
            return (poses, pred, rows) + tail
        return (poses, pred) + tail

    def finish(self):
        """Make the caller's stream wait for every enqueued CNN and solver launch."""
        for st in self.cnn:
            torch.cuda.current_stream().wait_stream(st)
        torch.cuda.current_stream().wait_stream(self.side)


# ------------------------------------------------------------------- depth / normal / semantics: fused per-image metric rows

TASK_CHANNELS = {'coord': 3, 'depth': 1, 'normal': 2, 'semantics': 6}    # utils/evaluation.py:86-95
ROW_WIDTH = {'depth': 3, 'normal': 2, 'semantics': 36}
_LABEL_CHANNELS = {'depth': 1, 'normal': 3, 'semantics': 1}


def task_metric_rows(task, predictions, gt_label, nodata_value=-1, class_map=None, as_float=False):
    """One row per image of the metric sums of `task`, on the device, from the HIP kernels of csrc/xl_metrics.hip
    (include/crossloc_metrics.h): depth float64 [B,3] = {sum |d-g|/g, sum (d-g)^2, n_valid}; normal float64 [B,2] = {sum of
    angles in degrees, n_valid}; semantics int64 [B,36] confusion counts (rows = ground truth), float64 with `as_float` (what
    gather_errors pads with NaN; counts are exact below 2^53).

    predictions [B,nt,H,W] float32 on the GPU: the task channels, sigma already split off - the strided `pred[:, :nt]` view
    of the network output is read in place.  gt_label [B,1|3,H,W] (any float dtype / device; moved and made contiguous).
    class_map: optional uint8 [B,H,W] on the device that receives the arg-max class (semantics).  No host synchronisation;
    a frame's row does not depend on the batch or the slot it is in."""
    import ctypes
    from . import _lib
    if task not in ROW_WIDTH:
        raise NotImplementedError(task)
    if not predictions.is_cuda:
        raise RuntimeError("crossloc_amd.evaluation.task_metric_rows runs on the GPU only (no CPU fallback)")
    nt = TASK_CHANNELS[task]
    if predictions.dim() != 4 or predictions.shape[1] != nt:
        raise RuntimeError("%s predictions must be [B,%d,H,W], got %s" % (task, nt, tuple(predictions.shape)))
    B, _, H, W = predictions.shape
    n = H * W
    pred = predictions.detach()
    if pred.dtype != torch.float32:
        pred = pred.float()
    if B > 0 and not pred[0, 0].is_contiguous():
        pred = pred.contiguous()                                   # e.g. channels_last: cells of a channel must be contiguous
    gt = gt_label.detach().to(device=pred.device, dtype=torch.float32).contiguous()
    if tuple(gt.shape) != (B, _LABEL_CHANNELS[task], H, W):
        raise RuntimeError("%s labels must be [%d,%d,%d,%d], got %s" % (task, B, _LABEL_CHANNELS[task], H, W, tuple(gt.shape)))
    sem = task == 'semantics'
    rows = torch.empty((B, ROW_WIDTH[task]), dtype=torch.int64 if sem else torch.float64, device=pred.device)
    if B == 0:
        return rows.double() if (sem and as_float) else rows
    L = _lib.lib()
    ws = torch.empty((int(L.xl_metrics_workspace_bytes(B, n)) + 7) // 8, dtype=torch.float64, device=pred.device)
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream(pred.device).cuda_stream)
    sb, sc = pred.stride(0), pred.stride(1)
    with torch.cuda.device(pred.device):
        if sem:
            cm_ptr = None
            if class_map is not None:
                if (class_map.dtype != torch.uint8 or tuple(class_map.shape) != (B, H, W) or not class_map.is_contiguous()
                        or class_map.device != pred.device):
                    raise RuntimeError("class_map must be a contiguous uint8 [B,H,W] tensor on the predictions' device")
                cm_ptr = vp(class_map.data_ptr())
            st = L.xl_metrics_semantics(vp(pred.data_ptr()), sb, sc, nt, vp(gt.data_ptr()), B, n, vp(ws.data_ptr()),
                                        vp(rows.data_ptr()), cm_ptr, stream)
        else:
            fn = L.xl_metrics_depth if task == 'depth' else L.xl_metrics_normal
            st = fn(vp(pred.data_ptr()), sb, sc, vp(gt.data_ptr()), B, n, float(nodata_value), vp(ws.data_ptr()),
                    vp(rows.data_ptr()), stream)
    _lib.check(st)
    return rows.double() if (sem and as_float) else rows


def depth_eval(depth, gt_depth, nodata_value):
    """utils/evaluation.py:247-267: (depth_abs_rel, depth_rms) over the has-data cells of the batch [B,1,H,W].  0-dim float64
    tensors on the device (the reference returns fp32 CPU tensors; nothing synchronises here until the caller reads them)."""
    s = task_metric_rows('depth', depth, gt_depth, nodata_value).sum(0)
    return s[0] / s[2], torch.sqrt(s[1] / s[2])


def normal_eval(normal_logits, gt_normals, nodata_value):
    """utils/evaluation.py:294-316: mean angular error in degrees over the has-data cells of the batch (0-dim float64
    tensor on the device)."""
    s = task_metric_rows('normal', normal_logits, gt_normals, nodata_value).sum(0)
    return s[0] / s[1]


def semantic_eval_rows(semantic_logits, gt_label, mute=False):
    """utils/evaluation.py:388-415 on the fused kernel: (class_prediction [B,H,W] int64 on the CPU, miou[B], fwiou[B], acc[B]),
    the return values of `semantic_eval` - one launch and one read-back for the batch instead of a pass per image."""
    B, _, H, W = semantic_logits.shape
    cmap = torch.empty((B, H, W), dtype=torch.uint8, device=semantic_logits.device)
    rows = task_metric_rows('semantics', semantic_logits, gt_label, class_map=cmap)
    acc_ls, miou_ls, fwiou_ls = group_metrics('semantics', rows.cpu().numpy())
    if not mute:
        print("Metrics within the batch: mean accuracy: {:.2f}%, mean IoU: {:.2f}%, frequency weighted IoU: {:.2f}%".
              format(acc_ls.mean() * 100, miou_ls.mean() * 100, fwiou_ls.mean() * 100))
    # widened on the device, so the host does no pass of its own over B*H*W elements; the int64 copy dominates
    return cmap.to(torch.int64).cpu(), miou_ls, fwiou_ls, acc_ls


def group_metrics(task, rows, group=4):
    """Host: per-image rows [K,D] in dataset order -> the lists the reference's evaluation loop collects
    (test_single_task.py:381-413).  The reference loader uses batch 4 for these tasks (utils/evaluation.py:69), so depth and
    normal figures are per GROUP of `group` consecutive frames (a shorter last group): the rows of a group are summed, then
    the formulas applied; a group without a valid cell gives NaN like the reference's 0/0.  Semantics is per image.
      depth -> (abs_rel[G], rms[G]);  normal -> angular_err[G];  semantics -> (accuracy[K], mean_iou[K], fw_iou[K])."""
    import warnings
    rows = np.asarray(rows.cpu() if isinstance(rows, torch.Tensor) else rows, np.float64)
    if rows.ndim != 2 or rows.shape[1] != ROW_WIDTH[task]:
        raise ValueError("%s rows must be [K,%d], got %s" % (task, ROW_WIDTH[task], rows.shape))
    if task == 'semantics':
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)        # an image without a labelled pixel: nanmean of all-NaN
            m = [segmentation_metrics(r.reshape(6, 6)) for r in rows]
        m = np.asarray(m, np.float64).reshape(-1, 3)
        return m[:, 0], m[:, 1], m[:, 2]
    sums = np.stack([rows[s:s + group].sum(0) for s in range(0, len(rows), group)]) if len(rows) else rows
    with np.errstate(divide="ignore", invalid="ignore"):
        if task == 'depth':
            return sums[:, 0] / sums[:, 2], np.sqrt(sums[:, 1] / sums[:, 2])
        return sums[:, 0] / sums[:, 1]


def _log_report(eval_str, testing_log, section, tail='\n'):
    if testing_log:
        with open(testing_log, 'a') as f:
            f.write("{:s} Evaluation on section {:s} {:s}".format('=' * 20, section, '=' * 20) + '\n')
            f.write(eval_str)
            f.write(tail)


def depth_printout(depth_abs_rel_ls, depth_rms_ls, testing_log=None, section="test"):
    """utils/evaluation.py:270-291"""
    depth_abs_rel_ls, depth_rms_ls = np.array(depth_abs_rel_ls), np.array(depth_rms_ls)
    eval_str = "Depth accuracy:"
    eval_str += "\nabsolute relative error, mean: {:.2f}%, median: {:.2f}%".format(
        np.mean(depth_abs_rel_ls) * 100.0, np.median(depth_abs_rel_ls) * 100.0)
    eval_str += "\nRMS error, mean: {:.2f}m, median: {:.2f}m".format(np.mean(depth_rms_ls), np.median(depth_rms_ls))
    print(eval_str)
    _log_report(eval_str, testing_log, section)
    return eval_str


def normal_printout(normal_angular_err_ls, testing_log=None, section="test"):
    """utils/evaluation.py:319-336"""
    normal_angular_err_ls = np.array(normal_angular_err_ls)
    eval_str = "Surface normal accuracy:"
    eval_str += "\nangular prediction error, mean: {:.1f} deg, median: {:.1f} deg".format(
        np.mean(normal_angular_err_ls), np.median(normal_angular_err_ls))
    print(eval_str)
    _log_report(eval_str, testing_log, section)
    return eval_str


def semantic_printout(accuracy_ls, mean_iou_ls, fw_iou_ls, testing_log=None, section="test"):
    """utils/evaluation.py:447-484; each argument is a list of per-batch arrays like the reference's, or one flat array."""
    def flat(ls):
        return np.concatenate([np.atleast_1d(np.asarray(a, np.float64)) for a in ls]) if len(ls) else np.zeros(0)
    accuracy_ls, mean_iou_ls, fw_iou_ls = flat(accuracy_ls), flat(mean_iou_ls), flat(fw_iou_ls)
    accuracy_str = "Pixel accuracy, mean: {:.2f}, median: {:.2f}".format(
        np.mean(accuracy_ls) * 100, np.median(accuracy_ls) * 100)
    print(accuracy_str)
    mean_iou_str = "Mean IoU, mean: {:.2f}, median: {:.2f}".format(np.mean(mean_iou_ls) * 100, np.median(mean_iou_ls) * 100)
    print(mean_iou_str)
    fw_iou_str = "Frequency weighted IoU, mean: {:.2f}, median: {:.2f}".format(
        np.mean(fw_iou_ls) * 100, np.median(fw_iou_ls) * 100)
    print(fw_iou_str)
    eval_str = accuracy_str + '\n' + mean_iou_str + '\n' + fw_iou_str
    _log_report(eval_str, testing_log, section, tail='\n\n')                  # :479-484 ends the block with a blank line
    return eval_str


def config_network(task, tiny, grayscale, uncertainty, fullsize, network_in=None, num_enc=0):
    """utils/evaluation.py:81-118 (TransPoseNet branch): the evaluation network of `task` on the GPU, in eval mode, with
    per-image statistics passes (a frame's output must not depend on the batch it lands in).  `network_in`: a reference
    state_dict loaded strictly; None -> the seeded generator's weights (tests and demos)."""
    from . import networks
    from .weights import seeded_state_dict
    if task not in TASK_CHANNELS:
        raise NotImplementedError(task)
    if uncertainty not in (None, 'MLE'):
        raise NotImplementedError(uncertainty)
    if task == 'semantics' and uncertainty is not None:
        raise NotImplementedError("semantics has no uncertainty channel")
    if task == 'semantics' and not fullsize:
        raise NotImplementedError("semantics needs fullsize")
    nt = TASK_CHANNELS[task]
    network = networks.TransPoseNet(torch.zeros(nt), tiny, grayscale, 2, 2, nt, 0 if uncertainty is None else 1, 32,
                                    num_enc, 0, fullsize)
    network.batch_invariant = True
    if network_in:
        network.load_state_dict(torch.load(network_in, map_location="cpu"), strict=True)
    else:
        network.load_state_dict(seeded_state_dict(network, seed=2021))
    return network.cuda().eval()


def evaluate_section(network, dataset, task, nodata_value=-1, batch=4, rank=0, world=1, process_group=None):
    """The depth / normal / semantics loop of test_single_task.py:328-413 over one dataset section (a CamLocDataset built
    with raw_image=True and the label of `task`): frame i goes to rank i % world; per batch the forward pass, the sigma
    split and task_metric_rows - nothing is read back inside the loop; ONE gather_errors of the rows at the end.
    Returns (rows [K,D] float64 numpy in dataset order, group_metrics(task, rows) on rank 0 / None elsewhere)."""
    if task not in ROW_WIDTH:
        raise NotImplementedError(task)
    dev = next(network.parameters()).device
    nt = network.num_task_channel
    K = len(dataset)
    mine = shard_indices(K, rank, world)
    out = []
    for s in range(0, len(mine), batch):
        items = [dataset[i] for i in mine[s:s + batch]]
        images = torch.stack([it[0] for it in items]).to(dev)
        labels = torch.stack([it[2] for it in items]).to(dev)
        with torch.no_grad():
            pred = network(images)
        out.append(task_metric_rows(task, pred[:, :nt], labels, nodata_value, as_float=True))   # sigma split: :351-356
    local = torch.cat(out, 0) if out else torch.empty((0, ROW_WIDTH[task]), dtype=torch.float64, device=dev)
    rows = gather_errors(local, K, rank, world, process_group).cpu().numpy()
    return rows, (group_metrics(task, rows) if rank == 0 else None)
