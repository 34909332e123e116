"""Per-pixel regression losses with the reference's call signatures, running the fused HIP kernels of
csrc/xl_loss.hip (forward + analytic backward in one pass, no host sync).

    loss/coord.py:87-188   scene_coords_regression_loss(min_depth, soft_clamp, hard_clamp, init_tolerance,
                           uncertainty, pixel_grid, nodata_value, cam_mat, scene_coords, uncertainty_map,
                           gt_poses, gt_coords, reduction='mean')
    loss/depth.py:7-76     depth_regression_loss(min_depth, hard_clamp, uncertainty, nodata_value, depth_map,
                           uncertainty_map, gt_depths, reduction='mean')
    loss/normal.py:8-127   normal_regression_loss(hard_clamp, uncertainty, nodata_value, normal_logits,
                           uncertainty_map, gt_normals, reduction='mean')

Each returns (loss, valid_pred_rate) like the reference; `loss` participates in autograd (backward hands out
the gradients the kernel already produced), `valid_pred_rate` is a 0-dim device tensor instead of a Python
float so nothing synchronises (the reference pays `.cpu()` + 4x `.item()` per call, coord.py:132, 170-175).
GPU only: there is no CPU fallback.
"""
import ctypes
import math

import torch

from . import _lib


def _bind():
    L = _lib.lib()
    if not hasattr(L, "_loss_bound"):
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.xl_loss_workspace_doubles.restype = ci
        L.xl_loss_workspace_doubles.argtypes = [ci, ci, ci]
        L.xl_loss_coord.restype = ci
        L.xl_loss_coord.argtypes = [vp, vp, vp, vp, ci, ci, ci, cf, cf, cf, cf, cf, cf, cf, cf, cf, ci, ci,
                                    vp, vp, vp, vp, vp]
        L.xl_loss_depth.restype = ci
        L.xl_loss_depth.argtypes = [vp, vp, vp, ci, ci, ci, cf, cf, cf, ci, ci, vp, vp, vp, vp, vp]
        L.xl_loss_normal.restype = ci
        L.xl_loss_normal.argtypes = [vp, vp, vp, ci, ci, ci, cf, cf, ci, ci, vp, vp, vp, vp, vp]
        L.xl_loss_semantics.restype = ci
        L.xl_loss_semantics.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp]
        L._loss_bound = True
    return L


def get_cam_mat(width, height, focal_length):
    """loss/coord.py:7-17 (kept on the host: only f, cx, cy are consumed by the kernel)."""
    cam_mat = torch.eye(3)
    cam_mat[0, 0] = focal_length
    cam_mat[1, 1] = focal_length
    cam_mat[0, 2] = width / 2
    cam_mat[1, 2] = height / 2
    return cam_mat


def get_pixel_grid(SUBSAMPLE):
    """utils/learning.py:20-35: centre-of-cell pixel positions [2,135,135]; vectorised, host tensor."""
    n = math.ceil(1080 / SUBSAMPLE)
    r = torch.arange(n, dtype=torch.float32) * SUBSAMPLE + SUBSAMPLE / 2
    return torch.stack([r[None, :].expand(n, n), r[:, None].expand(n, n)], 0).contiguous()


def _mode(uncertainty):
    if uncertainty is None:
        return 0
    if uncertainty == 'MLE':
        return 1
    raise NotImplementedError


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _prep(t):
    if not t.is_cuda:
        raise RuntimeError("crossloc_amd.loss runs on the GPU only (no CPU fallback)")
    return t.detach().to(torch.float32).contiguous()


class _FusedLoss(torch.autograd.Function):
    """forward = kernel call (loss + gradients); backward = scale the stored gradients."""

    @staticmethod
    def forward(ctx, launch, per_image, pred, unc):
        # the kernels write dense NCHW gradients: never inherit the memory format of `pred` (channels_last inputs)
        dpred = torch.empty(pred.shape, dtype=torch.float32, device=pred.device)
        dunc = torch.empty(unc.shape, dtype=torch.float32, device=unc.device) if unc is not None else None
        out = launch(dpred, dunc)
        ctx.per_image = per_image
        ctx.has_unc = unc is not None
        ctx.save_for_backward(dpred, dunc if dunc is not None else dpred.new_empty(0))
        ctx.mark_non_differentiable(out)
        B = pred.shape[0]
        loss = out[2:2 + B].clone() if per_image else out[0].clone()
        return loss, out

    @staticmethod
    def backward(ctx, gloss, _gout):
        dpred, dunc = ctx.saved_tensors
        if ctx.per_image:
            scale = gloss.reshape(-1, *([1] * (dpred.dim() - 1)))
            gp = dpred * scale
            gu = dunc * gloss.reshape(-1, *([1] * (dunc.dim() - 1))) if ctx.has_unc else None
        else:
            gp = dpred * gloss
            gu = dunc * gloss if ctx.has_unc else None
        return None, None, gp, gu


def _run(kind, launch_args_fn, pred, unc, reduction):
    if reduction not in ('mean', None):
        raise NotImplementedError
    per_image = reduction is None
    B, _, Ho, Wo = pred.shape
    dev = pred.device
    L = _bind()
    p32 = _prep(pred)
    u32 = _prep(unc) if unc is not None else None

    def launch(dpred, dunc):
        ws = torch.empty(L.xl_loss_workspace_doubles(B, Ho, Wo), dtype=torch.float64, device=dev)
        out = torch.empty(2 + B, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc = launch_args_fn(L, p32, u32, int(per_image), dpred, dunc, ws, out, stream)
        _lib.check(rc)
        return out

    loss, out = _FusedLoss.apply(launch, per_image, pred, unc)
    return loss, out[1]


def _frame_focals(focals, B, device):
    """One focal length per image as the float32 device array [B] xl_loss_coord_frames_ld reads."""
    f = torch.as_tensor(focals).detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    if f.numel() != B:
        raise RuntimeError("expected %d focal lengths, got %d" % (B, f.numel()))
    return f


def scene_coords_regression_loss(min_depth, soft_clamp, hard_clamp, init_tolerance, uncertainty,
                                 pixel_grid, nodata_value, cam_mat,
                                 scene_coords, uncertainty_map, gt_poses, gt_coords, reduction='mean', focals=None):
    """loss/coord.py:87-188.  pixel_grid / cam_mat as returned by get_pixel_grid / get_cam_mat above (host
    tensors; device tensors are accepted at the price of one D2H read).  focals: one focal length per image (sequence or
    tensor of B) in place of cam_mat's, which still supplies cx and cy; None: cam_mat's for every image, as the reference."""
    mode = _mode(uncertainty)
    cm = cam_mat.detach().cpu()
    pg = pixel_grid[:, 0, :2].detach().cpu()
    sub = float(pg[0, 1] - pg[0, 0])
    f, cx, cy = float(cm[0, 0]), float(cm[0, 2]), float(cm[1, 2])
    poses = _prep(gt_poses).reshape(-1, 16)
    gt = _prep(gt_coords)
    B, _, Ho, Wo = scene_coords.shape
    unc = uncertainty_map if mode == 1 else None
    fb = _frame_focals(focals, B, scene_coords.device) if focals is not None else None

    def args(L, p32, u32, per_image, dpred, dunc, ws, out, stream):
        if fb is not None:
            return _bind_ld().xl_loss_coord_frames_ld(
                _ptr(p32), _ptr(u32), _ptr(poses), _ptr(gt), B, Ho, Wo, 3, 1, _ptr(fb), cx, cy, sub, float(min_depth),
                float(soft_clamp), float(hard_clamp), float(init_tolerance), float(nodata_value), mode, per_image, _ptr(dpred),
                _ptr(dunc), _ptr(ws), _ptr(out), stream)
        return L.xl_loss_coord(_ptr(p32), _ptr(u32), _ptr(poses), _ptr(gt), B, Ho, Wo, f, cx, cy, sub,
                               float(min_depth), float(soft_clamp), float(hard_clamp), float(init_tolerance),
                               float(nodata_value), mode, per_image, _ptr(dpred), _ptr(dunc), _ptr(ws), _ptr(out), stream)

    return _run("coord", args, scene_coords, unc, reduction)


def depth_regression_loss(min_depth, hard_clamp, uncertainty, nodata_value, depth_map,
                          uncertainty_map, gt_depths, reduction='mean'):
    """loss/depth.py:7-76"""
    mode = _mode(uncertainty)
    gt = _prep(gt_depths)
    B, _, Ho, Wo = depth_map.shape
    unc = uncertainty_map if mode == 1 else None

    def args(L, p32, u32, per_image, dpred, dunc, ws, out, stream):
        return L.xl_loss_depth(_ptr(p32), _ptr(u32), _ptr(gt), B, Ho, Wo, float(min_depth), float(hard_clamp),
                               float(nodata_value), mode, per_image, _ptr(dpred), _ptr(dunc), _ptr(ws), _ptr(out), stream)

    return _run("depth", args, depth_map, unc, reduction)


def normal_regression_loss(hard_clamp, uncertainty, nodata_value, normal_logits,
                           uncertainty_map, gt_normals, reduction='mean'):
    """loss/normal.py:8-127"""
    mode = _mode(uncertainty)
    gt = _prep(gt_normals)
    B, _, Ho, Wo = normal_logits.shape
    unc = uncertainty_map if mode == 1 else None

    def args(L, p32, u32, per_image, dpred, dunc, ws, out, stream):
        return L.xl_loss_normal(_ptr(p32), _ptr(u32), _ptr(gt), B, Ho, Wo, float(hard_clamp), float(nodata_value),
                                mode, per_image, _ptr(dpred), _ptr(dunc), _ptr(ws), _ptr(out), stream)

    return _run("normal", args, normal_logits, unc, reduction)


class CrossEntropyLoss2d(torch.nn.Module):
    """loss/semantics.py:10-18 — the criterion object train_single_task.py:215 constructs.  Only the configuration the
    reference uses (no class weights, reduction='none', default ignore_index) is supported; the fused kernel of
    `semantics_classification_loss` implements it, this class just carries the settings."""

    def __init__(self, weight=None, reduction='none', ignore_index=-100):
        super().__init__()
        if weight is not None or reduction != 'none' or ignore_index != -100:
            raise NotImplementedError("only CrossEntropyLoss2d() as constructed by train_single_task.py:215")


def trim_semantic_label(raw_labels):
    """loss/semantics.py:21-41: raw class ids of the urbanscape / naturescape label maps -> the 6 training classes
    (0 sky, 1 unclassified + ground, 2 low vegetation, 3 buildings, 4 water, 5 bridge deck).  numpy in, numpy out."""
    import numpy as np
    raw_labels = np.asarray(raw_labels)
    out = raw_labels.copy()
    for old, new in zip((0, 1, 2, 3, 6, 9, 17), (0, 1, 1, 2, 3, 4, 5)):
        out[raw_labels == old] = new
    assert out.min() >= 0 and out.max() <= 5, "semantic label outside the 7 known raw classes"
    return out


def semantics_classification_loss(uncertainty, semantic_logits, uncertainty_map, gt_labels, criterion, reduction):
    """loss/semantics.py:44-91: cross entropy over the C class logits [B,C,H,W] against gt_labels [B,1,H,W];
    returns (loss, share of correctly classified pixels).  One fused kernel computes the loss, the arg-max accuracy
    and d loss / d logits; the reference's host synchronisation (.cpu().numpy(), :66) is gone, so the second return
    value is a device scalar tensor."""
    if uncertainty is not None:
        raise NotImplementedError                              # semantics.py:78-81
    if not isinstance(criterion, CrossEntropyLoss2d):
        raise NotImplementedError("criterion must be crossloc_amd.loss.CrossEntropyLoss2d()")
    if reduction not in ('mean', None):
        raise NotImplementedError
    per_image = reduction is None
    B, C, H, W = semantic_logits.shape
    dev = semantic_logits.device
    L = _bind()
    p32 = _prep(semantic_logits)
    lab = gt_labels.detach().to(device=dev, dtype=torch.float32).reshape(B, H, W).contiguous()

    def launch(dpred, dunc):
        ws = torch.empty(L.xl_loss_workspace_doubles(B, H, W), dtype=torch.float64, device=dev)
        out = torch.empty(2 + B, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc = L.xl_loss_semantics(_ptr(p32), _ptr(lab), B, C, H, W, int(per_image), _ptr(dpred), _ptr(ws), _ptr(out), stream)
        _lib.check(rc)
        return out

    loss, out = _FusedLoss.apply(launch, per_image, semantic_logits, None)
    return loss, out[1]


def _bind_ld():
    L = _bind()
    if not hasattr(L, "_loss_ld_bound"):
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.xl_loss_coord_ld.restype = ci
        L.xl_loss_coord_ld.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, cf, cf, cf, cf, cf, cf, cf, cf, cf, ci, ci,
                                       vp, vp, vp, vp, vp]
        L.xl_loss_coord_frames_ld.restype = ci
        L.xl_loss_coord_frames_ld.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, cf, cf, cf, cf, cf, cf, cf, cf, ci, ci,
                                              vp, vp, vp, vp, vp]
        L.xl_loss_depth_ld.restype = ci
        L.xl_loss_depth_ld.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, cf, cf, cf, ci, ci, vp, vp, vp, vp, vp]
        L.xl_loss_normal_ld.restype = ci
        L.xl_loss_normal_ld.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, cf, cf, ci, ci, vp, vp, vp, vp, vp]
        L._loss_ld_bound = True
    return L


def task_loss_and_output_gradient(task, uncertainty, prediction, num_task_channel, gt_labels, gt_poses=None,
                                  pixel_grid=None, cam_mat=None, nodata_value=-1, min_depth=0.1, soft_clamp=100.0,
                                  hard_clamp=1000.0, init_tolerance=50.0, focals=None):
    """The four losses of train_single_task.py:274-296 (reduction 'mean') in the form the training step uses: the kernels
    read the network output `prediction` [B, num_task_channel (+1 uncertainty channel), H, W] in place - no torch.split
    copies - and write d loss / d prediction into ONE tensor of its shape, ready for prediction.backward(grad) - no
    autograd node of the loss, hence no gradient scaling or concatenation kernels.  Returns (loss, valid_rate, grad);
    loss and valid_rate are 0-dim device tensors.  Same values and gradients as the functions above.  focals (coord task): one
    focal length per image in place of cam_mat's (scene_coords_regression_loss)."""
    mode = _mode(uncertainty)
    p = prediction.detach()
    if not p.is_cuda:
        raise RuntimeError("crossloc_amd.loss runs on the GPU only (no CPU fallback)")
    if p.dtype != torch.float32 or not p.is_contiguous():
        raise RuntimeError("task_loss_and_output_gradient reads the network output in place: contiguous float32 expected")
    B, C, Ho, Wo = p.shape
    if C != num_task_channel + mode:
        raise RuntimeError("expected %d channels (%d task + %d uncertainty), got %d" % (num_task_channel + mode,
                                                                                        num_task_channel, mode, C))
    if task == 'semantics' and mode:
        raise NotImplementedError                              # semantics.py:78-81
    dev, N = p.device, Ho * Wo
    grad = torch.empty_like(p)                                 # every element is written by the kernel
    L = _bind_ld()
    ws = torch.empty(L.xl_loss_workspace_doubles(B, Ho, Wo), dtype=torch.float64, device=dev)
    out = torch.empty(2 + B, dtype=torch.float32, device=dev)
    if focals is not None and task != 'coord':
        raise RuntimeError("focals belong to the coord task, not %s" % task)
    fb = _frame_focals(focals, B, dev) if focals is not None else None
    unc = ctypes.c_void_p(p.data_ptr() + 4 * num_task_channel * N) if mode else None
    dunc = ctypes.c_void_p(grad.data_ptr() + 4 * num_task_channel * N) if mode else None
    pp, gp, wp, op = _ptr(p), _ptr(grad), _ptr(ws), _ptr(out)
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if task == 'coord':
            cm = cam_mat.detach().cpu()
            pg = pixel_grid[:, 0, :2].detach().cpu()
            poses = _prep(gt_poses).reshape(-1, 16)
            gt = _prep(gt_labels)
            rest = (float(cm[0, 2]), float(cm[1, 2]), float(pg[0, 1] - pg[0, 0]), float(min_depth), float(soft_clamp),
                    float(hard_clamp), float(init_tolerance), float(nodata_value), mode, 0, gp, dunc, wp, op, stream)
            if fb is not None:
                rc = L.xl_loss_coord_frames_ld(pp, unc, _ptr(poses), _ptr(gt), B, Ho, Wo, C, C, _ptr(fb), *rest)
            else:
                rc = L.xl_loss_coord_ld(pp, unc, _ptr(poses), _ptr(gt), B, Ho, Wo, C, C, float(cm[0, 0]), *rest)
        elif task == 'depth':
            gt = _prep(gt_labels)
            rc = L.xl_loss_depth_ld(pp, unc, _ptr(gt), B, Ho, Wo, C, C, float(min_depth), float(hard_clamp),
                                    float(nodata_value), mode, 0, gp, dunc, wp, op, stream)
        elif task == 'normal':
            gt = _prep(gt_labels)
            rc = L.xl_loss_normal_ld(pp, unc, _ptr(gt), B, Ho, Wo, C, C, float(hard_clamp), float(nodata_value), mode, 0,
                                     gp, dunc, wp, op, stream)
        elif task == 'semantics':
            lab = gt_labels.detach().to(device=dev, dtype=torch.float32).reshape(B, Ho, Wo).contiguous()
            rc = L.xl_loss_semantics(pp, _ptr(lab), B, C, Ho, Wo, 0, gp, wp, op, stream)
        else:
            raise NotImplementedError(task)
    _lib.check(rc)
    return out[0], out[1], grad


# ------------------------------------------------------------------------------------------ end-to-end DSAC* training
E2E_MAX_TRIES = 4096            # sampler tries per hypothesis in a training step: 64 trips of a wave (the solver's own default,
#                                 1 000 000, lets a frame of unusable coordinates hold a workgroup for 15 000 trips per hypothesis)
E2E_STATS = 4                   # XL_E2E_STATS: doubles per row of the finishing op's statistics
# column of a per-frame row / of the summary row (the last one); meaning: include/crossloc_e2e.h
E2E_FRAME_FIELDS = {"loss": 0, "norm": 1, "scale": 2, "accepted": 3}
E2E_SUMMARY_FIELDS = {"mean_loss": 0, "accepted": 1, "max_norm": 2, "clipped": 3}


def finish_pose_gradient(g, losses, channels, weight=1.0, clip_norm=0.0, grad=None, beta=0.0):
    """The finishing op of the end-to-end step (csrc/xl_e2e.hip, rules: include/crossloc_e2e.h), one launch: the solver's
    gradient g [B,3,Ho,Wo] (float32 CUDA, any strides) and its expected losses [B] (float64 CUDA) become the gradient w.r.t.
    the network's `channels`-channel output.  Per frame: the norm of g; a frame whose loss or gradient is not finite is
    rejected and contributes exact zeros; the others are scaled by weight / B, and by clip_norm / norm where clip_norm > 0 and
    the norm exceeds it.  `grad` [B,channels,Ho,Wo] (contiguous float32) with `beta` != 0: the result is added onto
    beta * grad in place; with beta == 0 `grad` is overwritten without being read (allocated when None).  Returns
    (grad, stats): stats float64 [B+1,4], rows E2E_FRAME_FIELDS and, last, E2E_SUMMARY_FIELDS.  Nothing synchronises."""
    if not isinstance(g, torch.Tensor) or not g.is_cuda or not isinstance(losses, torch.Tensor) or not losses.is_cuda:
        raise RuntimeError("crossloc_amd.loss runs on the GPU only (no CPU fallback)")
    if g.dim() != 4 or g.size(1) != 3 or g.dtype != torch.float32:
        raise RuntimeError("the solver gradient must be float32 [B,3,Ho,Wo], got %s %s" % (g.dtype, tuple(g.shape)))
    B, _, Ho, Wo = g.shape
    if losses.dtype != torch.float64 or tuple(losses.shape) != (B,) or not losses.is_contiguous() or losses.device != g.device:
        raise RuntimeError("losses must be a contiguous float64 [B] tensor on the device of the gradient")
    if int(channels) < 3:
        raise RuntimeError("the network output has at least the 3 coordinate channels, got %d" % channels)
    shape = (B, int(channels), Ho, Wo)
    if grad is None:
        if beta != 0.0:
            raise RuntimeError("beta != 0 adds onto `grad`: pass it")
        grad = torch.empty(shape, dtype=torch.float32, device=g.device)
    elif (not isinstance(grad, torch.Tensor) or grad.dtype != torch.float32 or tuple(grad.shape) != shape
          or not grad.is_contiguous() or grad.device != g.device):
        raise RuntimeError("grad must be a contiguous float32 %s tensor on the device of the gradient" % (shape,))
    stats = torch.empty((B + 1, E2E_STATS), dtype=torch.float64, device=g.device)
    L = _lib.lib()
    with torch.cuda.device(g.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = L.xl_e2e_pose_gradient(_ptr(g), *g.stride(), _ptr(losses), B, Ho, Wo, int(channels), float(weight),
                                    float(clip_norm), float(beta), _ptr(grad), _ptr(stats), stream)
    _lib.check(rc)
    return grad, stats


def e2e_image_keys(image_keys, B):
    """(image0, image_stride) of frame keys that form an arithmetic sequence - the only form the solver's ABI keys a batch
    by.  Any other list is refused: a training step passes its sampler batch as image0 (training.e2e_keys) instead."""
    keys = [int(k) for k in image_keys]
    if len(keys) != B:
        raise ValueError("expected %d image keys, got %d" % (B, len(keys)))
    stride = keys[1] - keys[0] if B > 1 else 1
    if stride < 0 or any(keys[i] != keys[0] + i * stride for i in range(B)):
        raise ValueError("image_keys must be an arithmetic sequence with a non-negative step (image0 + b * image_stride), "
                         "got %s" % (keys,))
    return keys[0], stride


def expected_pose_loss_and_output_gradient(prediction, gt_poses, focals, image_h, image_w, hypotheses, threshold,
                                           inlier_alpha, max_pixel_error, weight_rot, weight_trans, soft_clamp, seed,
                                           image0=0, image_stride=1, image_keys=None, clip_norm=0.0, weight=1.0,
                                           grad=None, beta=0.0, depth=None, cam_coords=None, rgbd_threshold=10.0,
                                           max_dist_error=100.0, max_tries=E2E_MAX_TRIES, subsample=8, mask=None,
                                           mask_sampler="reject"):
    """The DSAC* expected pose loss of a batch and its gradient w.r.t. the network output, in the form the end-to-end step
    uses (the sibling of task_loss_and_output_gradient): `prediction` [B, C >= 3, Ho, Wo] (float32 CUDA) is read in place -
    its [:, :3] view goes to the solver as it is - dsacstar.backward_rgb_batch accumulates into a zeroed [B,3,Ho,Wo] buffer
    (with `depth` [B,Ho,Wo] or `cam_coords` [B,3,Ho,Wo]: dsacstar.backward_rgbd_batch, thresholds rgbd_threshold and
    max_dist_error in centimetres, Ho*Wo <= dsacstar.RGBD_MAX_CELLS), and finish_pose_gradient turns that into `grad`
    [B,C,Ho,Wo] for prediction.backward(grad).  Returns (mean_loss, stats, grad), device tensors only: mean_loss is the mean
    of the solver's losses over the accepted frames (a 0-dim float64 view of stats), stats as finish_pose_gradient.

    focals: one focal length per frame (sequence or tensor); the principal point is (image_w / 2, image_h / 2); `subsample`
    is the network's OUTPUT_SUBSAMPLE.  seed / image0 / image_stride key the sampler: frame b draws as image
    image0 + b * image_stride.  image_keys, when given, replaces image0 and image_stride and must be such an arithmetic
    sequence (e2e_image_keys); a batch of scattered dataset indices is keyed by its first index and the step's seed instead
    (training.e2e_keys), which is as deterministic and needs one solver call.  max_tries bounds the sampler per hypothesis.
    grad / beta / weight / clip_norm: finish_pose_gradient.

    mask (uint8 / bool [B,Ho,Wo], nonzero = usable; evaluation.cell_mask builds one): dsacstar.backward_rgb_masked_batch instead -
    masked-out cells are no evidence for the solver and their `grad[:, :3]` is exact zeros.  A frame with fewer than four usable
    cells is rejected like a frame whose loss is not finite: zeros contributed, not counted in `accepted`, not in the mean
    (its loss is turned into NaN on the device before the finishing op; nothing is read back).  The RGB-D path drops depth holes
    by itself and takes no mask: with `depth` or `cam_coords` a mask raises RuntimeError.  mask_sampler (dsacstar.MASK_SAMPLERS):
    the masked solver's sampler; "compact" draws from the usable cells only, so a mask that keeps a minority of the cells does
    not run the hypotheses out of their max_tries.  A sampler other than "reject" without a mask raises RuntimeError."""
    from . import dsacstar
    if mask_sampler not in dsacstar.MASK_SAMPLERS:
        raise RuntimeError("unknown mask_sampler %r (one of %s)" % (mask_sampler, ", ".join(dsacstar.MASK_SAMPLERS)))
    if mask is None and mask_sampler != "reject":
        raise RuntimeError("mask_sampler=%r is the masked solver's: it needs mask=" % (mask_sampler,))
    if mask is not None and (depth is not None or cam_coords is not None):
        raise RuntimeError("the RGB-D backward pass takes no mask (it drops depth holes itself): pass mask or depth / cam_coords")
    p = prediction.detach()
    if not p.is_cuda:
        raise RuntimeError("crossloc_amd.loss runs on the GPU only (no CPU fallback)")
    if p.dim() != 4 or p.dtype != torch.float32 or p.size(1) < 3:
        raise RuntimeError("prediction must be float32 [B, C >= 3, Ho, Wo], got %s %s" % (p.dtype, tuple(p.shape)))
    B, C, Ho, Wo = p.shape
    if image_keys is not None:
        image0, image_stride = e2e_image_keys(image_keys, B)
    coords = p[:, :3]
    focals = torch.as_tensor(focals, dtype=torch.float32).reshape(-1)
    if focals.numel() != B:
        raise RuntimeError("expected %d focal lengths, got %d" % (B, focals.numel()))
    g = torch.zeros((B, 3, Ho, Wo), dtype=torch.float32, device=p.device)
    ppx, ppy = image_w / 2, image_h / 2
    if mask is not None:
        losses, status = dsacstar.backward_rgb_masked_batch(
            coords, mask, g, gt_poses, hypotheses, threshold, 0.0, ppx, ppy, weight_rot, weight_trans, soft_clamp, inlier_alpha,
            max_pixel_error, subsample, seed, image0=image0, image_stride=image_stride, focals=focals, max_tries=max_tries,
            sampler=mask_sampler)
        losses = torch.where(status == 1, float("nan"), losses)                  # a dead frame: rejected below
    elif depth is None and cam_coords is None:
        losses = dsacstar.backward_rgb_batch(coords, g, gt_poses, hypotheses, threshold, 0.0, ppx, ppy, weight_rot,
                                             weight_trans, soft_clamp, inlier_alpha, max_pixel_error, subsample, seed,
                                             image0=image0, image_stride=image_stride, focals=focals, max_tries=max_tries)
    else:
        losses = dsacstar.backward_rgbd_batch(coords, cam_coords, g, gt_poses, hypotheses, rgbd_threshold, weight_rot,
                                              weight_trans, soft_clamp, inlier_alpha, max_dist_error, seed, image0=image0,
                                              image_stride=image_stride, max_tries=max_tries, depth=depth, ppointX=ppx,
                                              ppointY=ppy, subSampling=subsample, focals=focals)
    grad, stats = finish_pose_gradient(g, losses, C, weight, clip_norm, grad, beta)
    return stats[B, 0], stats, grad
