"""`dsacstar` module replacement: same names and positional signatures as the reference's pybind11
extension (/root/reference/dsacstar/dsacstar.cpp:887-892), backed by the HIP kernels in
libcrossloc_hip.so through the C ABI of include/crossloc_dsac.h.

    import torch, dsacstar                      # README.md:51 of the reference: torch first
    dsacstar.forward_rgb(scene_coords, out_pose, 64, 10.0, f, 360.0, 240.0, 100.0, 100.0, 8)

is the exact call utils/evaluation.py:162-172 makes.  Differences, all additive:
  * `sceneCoordinates` / `outPose` may live on the GPU (the reference dereferences them as host
    memory, dsacstar.cpp:78-79); CPU tensors take the host entry point (H2D, kernel, D2H, sync).
  * no stdout chatter (the reference prints ANSI-coloured timings, dsacstar.cpp:97-169).
  * the sampler is counter-based.  The reference's std::mt19937 state carries across calls
    (thread_rand.cpp:17); here every call consumes one "image index" from a module counter
    (reset with `set_image_index`), and results do not depend on thread or rank count.
  * `forward_rgb_batch` localises B images per launch (the reference is batch-1 only).
  * `forward_rgb_masked_batch` is forward_rgb_batch over a per-cell validity mask (uint8 / bool [B,Ho,Wo], nonzero = usable; build
    one with crossloc_amd.evaluation.cell_mask): masked-out cells are never sampled, scored or counted as inliers, and what is
    stored there cannot influence the result.  It returns a status per image (1: fewer than four usable cells, identity pose).
    `backward_rgb_masked_batch` is backward_rgb_batch over the same mask: masked-out cells are no evidence and get no gradient.
    `pose_quality_masked_batch` and `refine_pose_masked_batch` carry the mask through the two passes behind the solver: a
    masked-out cell is never read, is never an inlier and is counted in `n_masked` only.  `sampler="compact"` (MASK_SAMPLERS) makes
    the masked solver and its backward pass draw from the usable cells only.  The mask does not reach the RGB-D solver
    and its passes, forward_rgb or backward_rgb.
  * `backward_rgb` (dsacstar.cpp:200-483, exported by the reference but never called by CrossLoc) and its batched
    form `backward_rgb_batch` run on the GPU as well.
  * `forward_rgbd_batch` is the RGB-D solver (dsacstar.cpp:495-612) for B images per launch, from a camera-coordinate
    tensor or a depth map, and `backward_rgbd_batch` its backward pass (dsacstar.cpp:631-885): the expected pose loss and its
    gradient w.r.t. the scene coordinates; the reference-shaped `forward_rgbd` / `backward_rgbd` still raise NotImplementedError.
  * `pose_quality_batch` / `pose_quality_rgbd_batch` rate one given pose per image (inlier statistics, JtJ, covariance) by its
    reprojection residuals and by its metric 3-D residuals.
  * `refine_pose_batch` re-fits one given pose per image over its inliers, every cell weighted by the standard deviation the
    network predicts for it (or unweighted), and returns the refined poses with a row of diagnostics per image;
    `refine_pose_rgbd_batch` is its RGB-D twin: metric 3-D residuals under a 3x3 information matrix per cell (isotropic
    coordinate noise plus depth noise along the viewing ray).
There is no CPU fallback: without the HIP library the call raises.
"""
import ctypes

import torch

from . import _lib

RANSAC_SEED = 1305                      # thread_rand.h:101 default seed of the reference
MAX_HYPOTHESES_TRIES = 1000000          # dsacstar.cpp:48
MAX_REF_STEPS = 100                     # dsacstar.cpp:47 (compiled into the kernel)
MASK_SAMPLERS = ("reject", "compact")    # samplers of the masked RGB solver: XL_DSAC_SAMPLER_* of include/crossloc_dsac.h, by position
_image_index = 0


def set_image_index(index):
    """Next forward_rgb call is keyed as image `index` (then index+1, ...)."""
    global _image_index
    _image_index = int(index)


def _take_image_index():
    """The image index of the next single-image call, consumed (shared by the ctypes shim and the compiled binding)."""
    global _image_index
    image = _image_index
    _image_index += 1
    return image


def _check_coords(t, batched):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError("sceneCoordinates must be a torch.Tensor")
    if t.dim() != 4:
        # at::Tensor::accessor<float,4>() throws c10::Error -> RuntimeError (dsacstar.cpp:78)
        raise RuntimeError("expected 4 dims but tensor has %d" % t.dim())
    if t.dtype != torch.float32:
        raise RuntimeError("expected scalar type Float but found %s" % str(t.dtype).replace("torch.", ""))
    if t.size(1) != 3:
        raise RuntimeError("sceneCoordinates must be [B,3,H,W], got %s" % (tuple(t.shape),))
    if not batched and t.size(0) != 1:
        raise RuntimeError("forward_rgb supports batch size 1 only (dsacstar_util.h:161); use forward_rgb_batch")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _sampler_code(fn, sampler):
    """The sampler of a masked call as the C interface's code; an unknown name raises before any device work."""
    if sampler not in MASK_SAMPLERS:
        raise RuntimeError("%s: unknown sampler %r (one of %s)" % (fn, sampler, ", ".join(MASK_SAMPLERS)))
    return MASK_SAMPLERS.index(sampler)


def _check_mask(fn, sceneCoordinates, mask, out, out_name):
    """The mask checks of the masked entry points (`out`: the tensor the call writes next to it), before any device work: uint8 or
    bool, [B,Ho,Wo] contiguous CUDA on the device of sceneCoordinates.  Returns the mask as uint8 (a bool mask is viewed)."""
    if not isinstance(mask, torch.Tensor) or not isinstance(out, torch.Tensor):
        raise RuntimeError("mask and %s must be torch.Tensors" % out_name)
    if not sceneCoordinates.is_cuda or not out.is_cuda or not mask.is_cuda:
        raise RuntimeError("%s needs CUDA(HIP) tensors; there is no CPU fallback" % fn)
    B, _, Ho, Wo = sceneCoordinates.shape
    dev = sceneCoordinates.device
    if mask.dtype not in (torch.uint8, torch.bool):
        raise RuntimeError("mask must be uint8 or bool, got %s" % str(mask.dtype).replace("torch.", ""))
    if tuple(mask.shape) != (B, Ho, Wo) or not mask.is_contiguous():
        raise RuntimeError("mask must be a contiguous [B,Ho,Wo] tensor like sceneCoordinates, got %s" % (tuple(mask.shape),))
    if mask.device != dev or out.device != dev:
        raise RuntimeError("mask and %s must be on the device of sceneCoordinates" % out_name)
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def forward_rgb_batch(sceneCoordinates, outPoses, ransacHypotheses, inlierThreshold, focalLength, ppointX,
                      ppointY, inlierAlpha, maxReproj, subSampling, image0=0, image_stride=1, focals=None,
                      seed=None, max_tries=None, debug=False):
    """Localise B images in one launch. sceneCoordinates [B,3,Ho,Wo] float32 CUDA (any strides),
    outPoses [B,4,4] float32 CUDA contiguous, written in place (asynchronous on the current stream).
    Image b is keyed as image0 + b*image_stride.  With debug=True returns a dict of device tensors:
    cells [B,nHyp,4] int32, tries [B,nHyp] int32, scores [B,nHyp] float64, dbg [B,28] float64."""
    _check_coords(sceneCoordinates, True)
    if not sceneCoordinates.is_cuda or not outPoses.is_cuda:
        raise RuntimeError("forward_rgb_batch needs CUDA(HIP) tensors; there is no CPU fallback")
    B, _, Ho, Wo = sceneCoordinates.shape
    if outPoses.dtype != torch.float32 or tuple(outPoses.shape) != (B, 4, 4) or not outPoses.is_contiguous():
        raise RuntimeError("outPoses must be a contiguous float32 [B,4,4] tensor")
    dev = sceneCoordinates.device
    if focals is not None:
        focals = focals.to(device=dev, dtype=torch.float32).contiguous()
        assert focals.numel() == B
    out = None
    cells = tries = scores = dbg = None
    if debug:
        cells = torch.zeros((B, ransacHypotheses, 4), dtype=torch.int32, device=dev)
        tries = torch.zeros((B, ransacHypotheses), dtype=torch.int32, device=dev)
        scores = torch.zeros((B, ransacHypotheses), dtype=torch.float64, device=dev)
        dbg = torch.zeros((B, 28), dtype=torch.float64, device=dev)
        out = dict(cells=cells, tries=tries, scores=scores, dbg=dbg)
    sb, sc, sy, sx = sceneCoordinates.stride()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        rc = _lib.lib().xl_dsac_forward_rgb_batch(
            _ptr(sceneCoordinates), sb, sc, sy, sx, B, Ho, Wo, _ptr(outPoses),
            int(ransacHypotheses), float(inlierThreshold), float(focalLength), float(ppointX), float(ppointY),
            float(inlierAlpha), float(maxReproj), int(subSampling), _ptr(focals),
            int(RANSAC_SEED if seed is None else seed), int(image0), int(image_stride),
            int(MAX_HYPOTHESES_TRIES if max_tries is None else max_tries), ctypes.c_void_p(stream),
            _ptr(cells), _ptr(tries), _ptr(scores), _ptr(dbg))
    _lib.check(rc)
    return out


def forward_rgb_masked_batch(sceneCoordinates, mask, outPoses, ransacHypotheses, inlierThreshold, focalLength, ppointX,
                             ppointY, inlierAlpha, maxReproj, subSampling, image0=0, image_stride=1, focals=None,
                             seed=None, max_tries=None, debug=False, sampler="reject"):
    """forward_rgb_batch over the cells `mask` admits.  mask: uint8 or bool [B,Ho,Wo] CUDA contiguous on the device of
    sceneCoordinates, nonzero = usable; the other arguments as in forward_rgb_batch.  `sampler` (one of MASK_SAMPLERS) says how the
    four cells of a try are drawn.  "reject", the default: a try that drew a masked-out cell is rejected before P3P (the draws
    themselves are the unmasked solver's, so the expected number of tries grows as (usable fraction)^-4), and with an all-ones
    mask every output is forward_rgb_batch's bit for bit.  "compact": every draw is a rank among the usable cells of the image in
    row-major order, so no try is rejected by the mask and the number of tries stays at the unmasked solver's level whatever the
    usable fraction; the hypotheses come from the same distribution as under "reject" (uniform over usable quadruples) but are
    not the same ones, and an all-ones mask does not reproduce forward_rgb_batch.  Under both, the score sums the usable cells
    only, an inlier of the refinement is a usable cell below the threshold, and the values stored at masked-out cells (NaN and
    Inf included) influence no output bit.  No draw is weighted.  An image with fewer than four usable cells gets the 4x4 identity and status 1 (with
    debug: tries 0, scores 0, cells -1, winner -1).  Returns status, int32 [B] on the device (asynchronous on the current stream);
    with debug=True the debug dict of forward_rgb_batch with `status` in it.  Shape, dtype and device mismatches raise
    RuntimeError before any device work, an unknown sampler name too.  The backward pass over the same mask is
    backward_rgb_masked_batch (give it the same sampler), the passes behind the solver are pose_quality_masked_batch and
    refine_pose_masked_batch (they take a pose, not a sampler); the RGB-D solver and its backward pass, the single-image
    forward_rgb and the compiled binding take neither mask nor sampler."""
    sampler = _sampler_code("forward_rgb_masked_batch", sampler)
    _check_coords(sceneCoordinates, True)
    mask = _check_mask("forward_rgb_masked_batch", sceneCoordinates, mask, outPoses, "outPoses")
    B, _, Ho, Wo = sceneCoordinates.shape
    dev = sceneCoordinates.device
    if outPoses.dtype != torch.float32 or tuple(outPoses.shape) != (B, 4, 4) or not outPoses.is_contiguous():
        raise RuntimeError("outPoses must be a contiguous float32 [B,4,4] tensor")
    if int(ransacHypotheses) <= 0:
        raise RuntimeError("ransacHypotheses must be positive")
    if focals is not None:
        focals = focals.to(device=dev, dtype=torch.float32).contiguous()
        if focals.numel() != B:
            raise RuntimeError("expected %d focal lengths, got %d" % (B, focals.numel()))
    status = torch.empty((B,), dtype=torch.int32, device=dev)                     # (the kernel writes every entry)
    out = None
    cells = tries = scores = dbg = None
    if debug:
        cells = torch.zeros((B, ransacHypotheses, 4), dtype=torch.int32, device=dev)
        tries = torch.zeros((B, ransacHypotheses), dtype=torch.int32, device=dev)
        scores = torch.zeros((B, ransacHypotheses), dtype=torch.float64, device=dev)
        dbg = torch.zeros((B, 28), dtype=torch.float64, device=dev)
        out = dict(cells=cells, tries=tries, scores=scores, dbg=dbg, status=status)
    sb, sc, sy, sx = sceneCoordinates.stride()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        rc = _lib.lib().xl_dsac_forward_rgb_masked_sampled_batch(
            _ptr(sceneCoordinates), sb, sc, sy, sx, B, Ho, Wo, _ptr(mask), sampler, _ptr(outPoses), _ptr(status),
            int(ransacHypotheses), float(inlierThreshold), float(focalLength), float(ppointX), float(ppointY),
            float(inlierAlpha), float(maxReproj), int(subSampling), _ptr(focals),
            int(RANSAC_SEED if seed is None else seed), int(image0), int(image_stride),
            int(MAX_HYPOTHESES_TRIES if max_tries is None else max_tries), ctypes.c_void_p(stream),
            _ptr(cells), _ptr(tries), _ptr(scores), _ptr(dbg))
    _lib.check(rc)
    return out if debug else status


def forward_rgb(sceneCoordinates, outPose, ransacHypotheses, inlierThreshold, focalLength, ppointX, ppointY,
                inlierAlpha, maxReproj, subSampling):
    """dsacstar_rgb_forward (dsacstar.cpp:63-73): estimate the camera pose of ONE image from its scene
    coordinate prediction [1,3,H,W]; writes the 4x4 cam->world matrix into outPose in place."""
    _check_coords(sceneCoordinates, False)
    if not isinstance(outPose, torch.Tensor) or outPose.dim() != 2 or outPose.dtype != torch.float32 \
            or tuple(outPose.shape) != (4, 4):
        raise RuntimeError("outPose must be a float32 [4,4] tensor")
    image = _take_image_index()
    _, _, Ho, Wo = sceneCoordinates.shape
    if sceneCoordinates.is_cuda:
        dst = outPose if (outPose.is_cuda and outPose.is_contiguous()) else \
            torch.empty((4, 4), dtype=torch.float32, device=sceneCoordinates.device)
        forward_rgb_batch(sceneCoordinates, dst.view(1, 4, 4), ransacHypotheses, inlierThreshold, focalLength,
                          ppointX, ppointY, inlierAlpha, maxReproj, subSampling, image0=image)
        if dst is not outPose:
            outPose.copy_(dst)          # synchronising D2H copy, like the reference's blocking call
        return None
    if outPose.is_cuda:
        raise RuntimeError("outPose on the GPU needs sceneCoordinates on the GPU too")
    host_pose = outPose if outPose.is_contiguous() else torch.empty((4, 4), dtype=torch.float32)
    _, sc, sy, sx = sceneCoordinates.stride()
    rc = _lib.lib().xl_dsac_forward_rgb_host(
        _ptr(sceneCoordinates), sc, sy, sx, Ho, Wo, _ptr(host_pose), int(ransacHypotheses),
        float(inlierThreshold), float(focalLength), float(ppointX), float(ppointY), float(inlierAlpha),
        float(maxReproj), int(subSampling), int(RANSAC_SEED), int(image), int(MAX_HYPOTHESES_TRIES),
        None, None, None, None)
    _lib.check(rc)
    if host_pose is not outPose:
        outPose.copy_(host_pose)
    return None


QUALITY_DOUBLES = 64                     # XL_DSAC_QUALITY_DOUBLES: doubles per row of pose_quality_batch
# field name -> column (or columns) of a pose_quality_batch row; layout and meaning: include/crossloc_dsac.h
QUALITY_FIELDS = {
    "n_cells": 0, "n_inliers": 1, "soft_score": 2, "sum_err": 3, "sum_err2": 4, "sse": 5, "status": 6,
    "sigma_px": 7, "sigma_pos_m": 8, "sigma_rot_deg": 9,
    "JtJ": slice(10, 31), "cov": slice(31, 52), "cov_center": slice(52, 58), "n_masked": 58, "reserved": slice(59, 64),
}


def _pose_quality(fn, sceneCoordinates, mask, poses, inlierThreshold, focalLength, ppointX, ppointY, inlierAlpha, maxReproj,
                  subSampling, focals):
    """pose_quality_batch (mask None) and pose_quality_masked_batch: the checks, the row tensor and the call"""
    _check_coords(sceneCoordinates, True)
    if fn == "pose_quality_masked_batch":                                          # (a mask of None is refused there)
        mask = _check_mask(fn, sceneCoordinates, mask, poses, "poses")
    if not sceneCoordinates.is_cuda or not isinstance(poses, torch.Tensor) or not poses.is_cuda:
        raise RuntimeError("%s needs CUDA(HIP) tensors; there is no CPU fallback" % fn)
    B, _, Ho, Wo = sceneCoordinates.shape
    if poses.dtype != torch.float32 or tuple(poses.shape) != (B, 4, 4) or not poses.is_contiguous():
        raise RuntimeError("poses must be a contiguous float32 [B,4,4] tensor")
    dev = sceneCoordinates.device
    if poses.device != dev:
        raise RuntimeError("poses must be on the device of sceneCoordinates")
    if focals is not None:
        focals = focals.to(device=dev, dtype=torch.float32).contiguous()
        assert focals.numel() == B
    rows = torch.empty((B, QUALITY_DOUBLES), dtype=torch.float64, device=dev)      # (the kernel writes all 64 of every row)
    sb, sc, sy, sx = sceneCoordinates.stride()
    tail = (_ptr(poses), float(inlierThreshold), float(focalLength), float(ppointX), float(ppointY), float(inlierAlpha),
            float(maxReproj), int(subSampling), _ptr(focals), _ptr(rows))
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if mask is None:
            rc = _lib.lib().xl_dsac_pose_quality_batch(_ptr(sceneCoordinates), sb, sc, sy, sx, B, Ho, Wo, *tail, stream)
        else:
            rc = _lib.lib().xl_dsac_pose_quality_masked_batch(_ptr(sceneCoordinates), sb, sc, sy, sx, B, Ho, Wo, _ptr(mask), *tail,
                                                              stream)
    _lib.check(rc)
    return rows


def pose_quality_batch(sceneCoordinates, poses, inlierThreshold, focalLength, ppointX, ppointY, inlierAlpha, maxReproj,
                       subSampling, focals=None):
    """How far the poses of B images can be trusted: inlier statistics, JtJ of the reprojection residuals over the inliers
    and the pose covariance, at the given pose of each image (usually what forward_rgb_batch wrote; enqueue this behind it
    on the same stream).  sceneCoordinates [B,3,Ho,Wo] float32 CUDA (any strides, any grid size), poses [B,4,4] float32 CUDA
    contiguous cam->world; the other arguments as in forward_rgb_batch.  Returns a float64 CUDA tensor [B,64]
    (QUALITY_FIELDS names the columns), asynchronous on the current stream.  There is no CPU fallback."""
    return _pose_quality("pose_quality_batch", sceneCoordinates, None, poses, inlierThreshold, focalLength, ppointX, ppointY,
                         inlierAlpha, maxReproj, subSampling, focals)


def pose_quality_masked_batch(sceneCoordinates, mask, poses, inlierThreshold, focalLength, ppointX, ppointY, inlierAlpha,
                              maxReproj, subSampling, focals=None):
    """pose_quality_batch over the cells `mask` admits - usually behind forward_rgb_masked_batch, on the same mask.  mask: uint8
    or bool [B,Ho,Wo] CUDA contiguous on the device of sceneCoordinates, nonzero = usable; the other arguments and the returned
    rows as in pose_quality_batch.  A masked-out cell is not read: it is no inlier, adds nothing to `soft_score` (which sums the
    usable cells with the same factor, like the masked solver's score) or to any other sum, and is counted in `n_masked` only;
    `n_cells` stays Ho*Wo.  The values stored at masked-out cells (NaN and Inf included) influence no output bit, and with an
    all-ones mask every output is pose_quality_batch's bit for bit.  Mask mismatches raise RuntimeError before any device work."""
    return _pose_quality("pose_quality_masked_batch", sceneCoordinates, mask, poses, inlierThreshold, focalLength, ppointX,
                         ppointY, inlierAlpha, maxReproj, subSampling, focals)


REFINE_DOUBLES = 64                      # XL_DSAC_REFINE_DOUBLES: doubles per row of refine_pose_batch
REFINE_MAX_CELLS = 10128                 # XL_DSAC_REFINE_MAX_CELLS: largest Ho*Wo refine_pose_batch accepts
REFINE_MAX_ROUNDS = 16                   # XL_DSAC_REFINE_MAX_ROUNDS
# field name -> column (or columns) of a refine_pose_batch row; layout and meaning: include/crossloc_dsac.h.  status, sigma_pos_m,
# sigma_rot_deg, JtJ, cov and cov_center sit where the pose-quality row has them (QUALITY_FIELDS)
REFINE_FIELDS = {
    "n_cells": 0, "n_inliers": 1, "n_inliers_in": 2, "cost_in": 3, "cost_out": 4, "n_bad_sigma": 5, "status": 6,
    "chi": 7, "sigma_pos_m": 8, "sigma_rot_deg": 9,
    "JtJ": slice(10, 31), "cov": slice(31, 52), "cov_center": slice(52, 58),
    "rounds": 58, "evals": 59, "converged": 60, "moved_rot_deg": 61, "moved_pos_m": 62, "n_masked": 63,
}


def _refine_pose(fn, sceneCoordinates, mask, sigma, poses, inlierThreshold, focalLength, ppointX, ppointY, maxReproj, subSampling,
                 sigmaFloorPx, maxRounds, focals, outPoses, w2c):
    """refine_pose_batch (mask None) and refine_pose_masked_batch: the checks, the output tensors and the call"""
    _check_coords(sceneCoordinates, True)
    if fn == "refine_pose_masked_batch":                                           # (a mask of None is refused there)
        mask = _check_mask(fn, sceneCoordinates, mask, poses, "poses")
    if not sceneCoordinates.is_cuda or not isinstance(poses, torch.Tensor) or not poses.is_cuda:
        raise RuntimeError("%s needs CUDA(HIP) tensors; there is no CPU fallback" % fn)
    B, _, Ho, Wo = sceneCoordinates.shape
    if poses.dtype != torch.float32 or tuple(poses.shape) != (B, 4, 4) or not poses.is_contiguous():
        raise RuntimeError("poses must be a contiguous float32 [B,4,4] tensor")
    dev = sceneCoordinates.device
    if poses.device != dev:
        raise RuntimeError("poses must be on the device of sceneCoordinates")
    if sigma is not None:
        if not isinstance(sigma, torch.Tensor) or sigma.dtype != torch.float32 or tuple(sigma.shape) != (B, Ho, Wo):
            raise RuntimeError("sigma must be a float32 [B,Ho,Wo] tensor like sceneCoordinates")
        if sigma.device != dev:
            raise RuntimeError("sigma must be on the device of sceneCoordinates")
    if Ho * Wo > REFINE_MAX_CELLS:
        raise RuntimeError("%s stages an image in the LDS of one CU: Ho*Wo = %d cells exceed the limit of %d"
                           % (fn, Ho * Wo, REFINE_MAX_CELLS))
    if not float(sigmaFloorPx) > 0.0:
        raise RuntimeError("sigmaFloorPx must be positive")
    if not 1 <= int(maxRounds) <= REFINE_MAX_ROUNDS:
        raise RuntimeError("maxRounds must be in 1..%d" % REFINE_MAX_ROUNDS)
    if outPoses is None:
        outPoses = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)        # (the kernel writes all 16 of every pose)
    elif (not isinstance(outPoses, torch.Tensor) or outPoses.dtype != torch.float32 or tuple(outPoses.shape) != (B, 4, 4)
          or not outPoses.is_contiguous() or outPoses.device != dev):
        raise RuntimeError("outPoses must be a contiguous float32 [B,4,4] tensor on the device of sceneCoordinates")
    if w2c is not None and (not isinstance(w2c, torch.Tensor) or w2c.dtype != torch.float64 or tuple(w2c.shape) != (B, 12)
                            or not w2c.is_contiguous() or w2c.device != dev):
        raise RuntimeError("w2c must be a contiguous float64 [B,12] tensor on the device of sceneCoordinates")
    if focals is not None:
        focals = focals.to(device=dev, dtype=torch.float32).contiguous()
        assert focals.numel() == B
    rows = torch.empty((B, REFINE_DOUBLES), dtype=torch.float64, device=dev)       # (the kernel writes all 64 of every row)
    sb, sc, sy, sx = sceneCoordinates.stride()
    gb, gy, gx = sigma.stride() if sigma is not None else (0, 0, 0)
    tail = (_ptr(poses), _ptr(outPoses), _ptr(rows), _ptr(w2c), float(inlierThreshold), float(focalLength), float(ppointX),
            float(ppointY), float(maxReproj), int(subSampling), _ptr(focals), float(sigmaFloorPx), int(maxRounds))
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if mask is None:
            rc = _lib.lib().xl_dsac_refine_pose_batch(_ptr(sceneCoordinates), sb, sc, sy, sx, _ptr(sigma), gb, gy, gx, B, Ho, Wo,
                                                      *tail, stream)
        else:
            rc = _lib.lib().xl_dsac_refine_pose_masked_batch(_ptr(sceneCoordinates), sb, sc, sy, sx, _ptr(sigma), gb, gy, gx,
                                                             B, Ho, Wo, _ptr(mask), *tail, stream)
    _lib.check(rc)
    return outPoses, rows


def refine_pose_batch(sceneCoordinates, sigma, poses, inlierThreshold, focalLength, ppointX, ppointY, maxReproj, subSampling,
                      sigmaFloorPx=1.0, maxRounds=8, focals=None, outPoses=None, w2c=None):
    """Re-fit the poses of B images over their inliers, every cell weighted by its predicted standard deviation: iteratively
    re-weighted Levenberg-Marquardt with the weights 1 / (sigmaFloorPx^2 + (f sigma / z)^2) (model: include/crossloc_dsac.h),
    from the given pose of each image - usually what forward_rgb_batch wrote; enqueue this behind it on the same stream.
    sceneCoordinates [B,3,Ho,Wo] float32 CUDA (any strides, Ho*Wo <= REFINE_MAX_CELLS); sigma [B,Ho,Wo] float32 CUDA (any strides,
    metres; e.g. the channel view pred[:, 3] of the network output) or None for the unweighted re-fit; poses [B,4,4] float32 CUDA
    contiguous cam->world.  outPoses (float32 [B,4,4], may be `poses`) and w2c (float64 [B,12], the refined world->camera pose)
    are optional CUDA contiguous outputs.  Returns (outPoses, rows): the refined poses and a float64 CUDA tensor [B,64]
    (REFINE_FIELDS names the columns), asynchronous on the current stream.  There is no CPU fallback."""
    return _refine_pose("refine_pose_batch", sceneCoordinates, None, sigma, poses, inlierThreshold, focalLength, ppointX, ppointY,
                        maxReproj, subSampling, sigmaFloorPx, maxRounds, focals, outPoses, w2c)


def refine_pose_masked_batch(sceneCoordinates, mask, sigma, poses, inlierThreshold, focalLength, ppointX, ppointY, maxReproj,
                             subSampling, sigmaFloorPx=1.0, maxRounds=8, focals=None, outPoses=None, w2c=None):
    """refine_pose_batch over the cells `mask` admits - usually behind forward_rgb_masked_batch, on the same mask.  mask: uint8 or
    bool [B,Ho,Wo] CUDA contiguous on the device of sceneCoordinates, nonzero = usable; the other arguments and the returns as in
    refine_pose_batch.  A masked-out cell is in no round's inlier set and neither its coordinate nor its sigma enters any
    arithmetic: `n_bad_sigma` counts usable cells only and the masked-out cells are counted in `n_masked`.  The values stored at
    masked-out cells (NaN and Inf included, in the coordinates and in sigma) influence no output bit, and with an all-ones mask
    every output is refine_pose_batch's bit for bit.  An image with fewer than four usable cells has status 1 and keeps its input
    pose bit for bit (behind the masked solver: the identity).  Mask mismatches raise RuntimeError before any device work."""
    return _refine_pose("refine_pose_masked_batch", sceneCoordinates, mask, sigma, poses, inlierThreshold, focalLength, ppointX,
                        ppointY, maxReproj, subSampling, sigmaFloorPx, maxRounds, focals, outPoses, w2c)


BWD_REC = 128                            # XL_DSAC_BWD_REC: doubles per hypothesis in the debug record


def backward_rgb_batch(sceneCoordinates, outSceneCoordinatesGrad, gtPoses, ransacHypotheses, inlierThreshold,
                       focalLength, ppointX, ppointY, wLossRot, wLossTrans, softClamp, inlierAlpha, maxReproj,
                       subSampling, randomSeed, image0=0, image_stride=1, focals=None, max_tries=None, debug=False):
    """DSAC* expected pose loss of B images and its gradient w.r.t. their scene coordinates in one launch sequence.
    sceneCoordinates [B,3,Ho,Wo] and outSceneCoordinatesGrad (same shape, any strides; ACCUMULATED like the
    reference's `+=`) are float32 CUDA tensors, gtPoses [B,4,4] cam->world.  Returns the expected losses as a
    float64 CUDA tensor [B] (asynchronous on the current stream); with debug=True also the per-hypothesis records
    [B,nHyp,BWD_REC] (layout: include/crossloc_dsac.h)."""
    _check_coords(sceneCoordinates, True)
    g = outSceneCoordinatesGrad
    if not sceneCoordinates.is_cuda or not isinstance(g, torch.Tensor) or not g.is_cuda:
        raise RuntimeError("backward_rgb_batch needs CUDA(HIP) tensors; there is no CPU fallback")
    if g.dtype != torch.float32 or tuple(g.shape) != tuple(sceneCoordinates.shape):
        raise RuntimeError("outSceneCoordinatesGrad must be float32 with the shape of sceneCoordinates")
    B, _, Ho, Wo = sceneCoordinates.shape
    dev = sceneCoordinates.device
    gt = gtPoses.to(device=dev, dtype=torch.float32).reshape(B, 16).contiguous()
    if focals is not None:
        focals = focals.to(device=dev, dtype=torch.float32).contiguous()
        assert focals.numel() == B
    loss = torch.zeros((B,), dtype=torch.float64, device=dev)
    rec = torch.zeros((B, ransacHypotheses, BWD_REC), dtype=torch.float64, device=dev) if debug else None
    sb, sc, sy, sx = sceneCoordinates.stride()
    gb, gc, gy, gx = g.stride()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        rc = _lib.lib().xl_dsac_backward_rgb_batch(
            _ptr(sceneCoordinates), sb, sc, sy, sx, B, Ho, Wo, _ptr(g), gb, gc, gy, gx, _ptr(gt), _ptr(loss),
            int(ransacHypotheses), float(inlierThreshold), float(focalLength), float(ppointX), float(ppointY),
            float(wLossRot), float(wLossTrans), float(softClamp), float(inlierAlpha), float(maxReproj),
            int(subSampling), _ptr(focals), int(randomSeed), int(image0), int(image_stride),
            int(MAX_HYPOTHESES_TRIES if max_tries is None else max_tries), ctypes.c_void_p(stream), _ptr(rec))
    _lib.check(rc)
    return (loss, rec) if debug else loss


def backward_rgb_masked_batch(sceneCoordinates, mask, outSceneCoordinatesGrad, gtPoses, ransacHypotheses, inlierThreshold,
                              focalLength, ppointX, ppointY, wLossRot, wLossTrans, softClamp, inlierAlpha, maxReproj,
                              subSampling, randomSeed, image0=0, image_stride=1, focals=None, max_tries=None, debug=False,
                              sampler="reject"):
    """backward_rgb_batch over the cells `mask` admits (mask and sampler: as in forward_rgb_masked_batch, the other arguments as in
    backward_rgb_batch): the hypotheses, scores and soft-max distribution are the masked forward solver's under `sampler`, every hypothesis is
    refined over usable cells only, the score path sums usable cells only, and the gradient at a masked-out cell keeps the
    caller's incoming value bit for bit.  The values stored at masked-out cells (NaN and Inf included) influence no bit of loss,
    record or gradient, and with an all-ones mask and the "reject" sampler all three are backward_rgb_batch's.  An image with fewer than four usable cells
    gets loss 0.0, status 1, zero records and an untouched gradient.  Returns (losses float64 [B], status int32 [B]) on the device
    (asynchronous on the current stream); with debug=True (losses, rec, status).  Shape, dtype and device mismatches raise
    RuntimeError before any device work, an unknown sampler name too."""
    sampler = _sampler_code("backward_rgb_masked_batch", sampler)
    _check_coords(sceneCoordinates, True)
    g = outSceneCoordinatesGrad
    mask = _check_mask("backward_rgb_masked_batch", sceneCoordinates, mask, g, "outSceneCoordinatesGrad")
    if g.dtype != torch.float32 or tuple(g.shape) != tuple(sceneCoordinates.shape):
        raise RuntimeError("outSceneCoordinatesGrad must be float32 with the shape of sceneCoordinates")
    if int(ransacHypotheses) <= 0:
        raise RuntimeError("ransacHypotheses must be positive")
    B, _, Ho, Wo = sceneCoordinates.shape
    dev = sceneCoordinates.device
    gt = gtPoses.to(device=dev, dtype=torch.float32).reshape(B, 16).contiguous()
    if focals is not None:
        focals = focals.to(device=dev, dtype=torch.float32).contiguous()
        if focals.numel() != B:
            raise RuntimeError("expected %d focal lengths, got %d" % (B, focals.numel()))
    loss = torch.zeros((B,), dtype=torch.float64, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)                     # (the first backward kernel writes every entry)
    rec = torch.zeros((B, ransacHypotheses, BWD_REC), dtype=torch.float64, device=dev) if debug else None
    sb, sc, sy, sx = sceneCoordinates.stride()
    gb, gc, gy, gx = g.stride()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        rc = _lib.lib().xl_dsac_backward_rgb_masked_sampled_batch(
            _ptr(sceneCoordinates), sb, sc, sy, sx, B, Ho, Wo, _ptr(mask), sampler, _ptr(g), gb, gc, gy, gx, _ptr(gt), _ptr(loss),
            _ptr(status), int(ransacHypotheses), float(inlierThreshold), float(focalLength), float(ppointX), float(ppointY),
            float(wLossRot), float(wLossTrans), float(softClamp), float(inlierAlpha), float(maxReproj),
            int(subSampling), _ptr(focals), int(randomSeed), int(image0), int(image_stride),
            int(MAX_HYPOTHESES_TRIES if max_tries is None else max_tries), ctypes.c_void_p(stream), _ptr(rec))
    _lib.check(rc)
    return (loss, rec, status) if debug else (loss, status)


def backward_rgb(sceneCoordinates, outSceneCoordinatesGrad, gtPose, ransacHypotheses, inlierThreshold, focalLength,
                 ppointX, ppointY, wLossRot, wLossTrans, softClamp, inlierAlpha, maxReproj, subSampling, randomSeed):
    """dsacstar_rgb_backward (dsacstar.cpp:200-215): pose estimation of ONE image plus the gradient of the expected
    pose loss w.r.t. its scene coordinates, accumulated into outSceneCoordinatesGrad [1,3,H,W]; returns the DSAC
    expectation of the pose loss as a Python float.  Tensors may live on the GPU or (like the reference) the CPU."""
    _check_coords(sceneCoordinates, False)
    g = outSceneCoordinatesGrad
    if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or tuple(g.shape) != tuple(sceneCoordinates.shape):
        raise RuntimeError("outSceneCoordinatesGrad must be float32 with the shape of sceneCoordinates")
    if not isinstance(gtPose, torch.Tensor) or tuple(gtPose.shape) != (4, 4):
        raise RuntimeError("gtPose must be a [4,4] tensor")
    if sceneCoordinates.is_cuda and g.is_cuda:
        loss = backward_rgb_batch(sceneCoordinates, g, gtPose.view(1, 4, 4), ransacHypotheses, inlierThreshold,
                                  focalLength, ppointX, ppointY, wLossRot, wLossTrans, softClamp, inlierAlpha,
                                  maxReproj, subSampling, randomSeed)
        return float(loss.item())
    if sceneCoordinates.is_cuda or g.is_cuda:
        raise RuntimeError("sceneCoordinates and outSceneCoordinatesGrad must be on the same device")
    dev = torch.device("cuda")                       # raises if there is no HIP device: no CPU fallback
    co = sceneCoordinates.to(dev)
    gd = torch.zeros(tuple(g.shape), dtype=torch.float32, device=dev)
    gd.copy_(g)
    loss = backward_rgb_batch(co, gd, gtPose.view(1, 4, 4), ransacHypotheses, inlierThreshold, focalLength, ppointX,
                              ppointY, wLossRot, wLossTrans, softClamp, inlierAlpha, maxReproj, subSampling, randomSeed)
    g.copy_(gd)
    return float(loss.item())


RGBD_DBG_DOUBLES = 16                    # XL_DSAC_RGBD_DBG_DOUBLES: doubles per image in forward_rgbd_batch's debug record
RGBD_MAX_CELLS = 6144                    # XL_DSAC_RGBD_MAX_CELLS: largest Ho*Wo forward_rgbd_batch accepts


def camera_coordinates(depth, focal, image_h, image_w, sub):
    """Camera coordinates [B,3,Ho,Wo] float32 of a depth map [B,Ho,Wo] float32 (depth along the optical axis, 0 = no measurement):
    the ray through the pixel centre (sub*x + sub//2, sub*y + sub//2) of every cell times its depth, principal point
    (image_w/2, image_h/2) - the formula forward_rgbd_batch applies itself when it is given `depth`, with the same bits.
    `focal`: one number or one per image.  The ray factors are computed on the host (correctly rounded float32 division)."""
    if not isinstance(depth, torch.Tensor) or depth.dim() != 3 or depth.dtype != torch.float32:
        raise RuntimeError("depth must be a float32 [B,Ho,Wo] tensor")
    B, Ho, Wo = depth.shape
    f = torch.as_tensor(focal, dtype=torch.float32).reshape(-1).cpu()
    if f.numel() not in (1, B):
        raise RuntimeError("expected 1 or %d focal lengths, got %d" % (B, f.numel()))
    px = (torch.arange(Wo, dtype=torch.int64) * int(sub) + int(sub) // 2).to(torch.float32)
    py = (torch.arange(Ho, dtype=torch.int64) * int(sub) + int(sub) // 2).to(torch.float32)
    rx = ((px - float(image_w / 2))[None, :] / f[:, None]).to(depth.device)              # [1 or B, Wo]
    ry = ((py - float(image_h / 2))[None, :] / f[:, None]).to(depth.device)              # [1 or B, Ho]
    return torch.stack([rx[:, None, :] * depth, ry[:, :, None] * depth, depth], dim=1)


def _rgbd_source(fn, sceneCoordinates, cameraCoordinates, depth, intr, max_cells=None):
    """What the three RGB-D wrappers check alike about where an image comes from: exactly one of cameraCoordinates and depth, its
    dtype and shape, the intrinsics depth needs (intr = focalLength, ppointX, ppointY, subSampling, focals) and the staging
    kernels' cell limit - before any device check."""
    focalLength, ppointX, ppointY, subSampling, focals = intr
    _check_coords(sceneCoordinates, True)
    if (cameraCoordinates is None) == (depth is None):
        raise RuntimeError("%s takes exactly one of cameraCoordinates and depth" % fn)
    B, _, Ho, Wo = sceneCoordinates.shape
    other = cameraCoordinates if depth is None else depth
    if not isinstance(other, torch.Tensor) or other.dtype != torch.float32:
        raise RuntimeError("cameraCoordinates / depth must be a float32 torch.Tensor")
    if depth is None and tuple(other.shape) != (B, 3, Ho, Wo):
        raise RuntimeError("cameraCoordinates must be [B,3,Ho,Wo] like sceneCoordinates, got %s" % (tuple(other.shape),))
    if depth is not None:
        if tuple(other.shape) != (B, Ho, Wo):
            raise RuntimeError("depth must be [B,Ho,Wo] like sceneCoordinates, got %s" % (tuple(other.shape),))
        if (focalLength is None and focals is None) or ppointX is None or ppointY is None or subSampling is None:
            raise RuntimeError("depth needs focalLength (or focals), ppointX, ppointY and subSampling")
        if int(subSampling) <= 0:
            raise RuntimeError("subSampling must be positive")
    if max_cells is not None and Ho * Wo > max_cells:
        raise RuntimeError("%s stages an image in the LDS of one CU: Ho*Wo = %d cells exceed the limit of %d" % (fn, Ho * Wo, max_cells))


def _rgbd_on_device(fn, sceneCoordinates, cameraCoordinates, depth, mine):
    """The device checks of a wrapper: sceneCoordinates, the camera tensor or depth and `mine`, the wrapper's own tensor."""
    other = cameraCoordinates if depth is None else depth
    if not isinstance(mine, torch.Tensor) or not sceneCoordinates.is_cuda or not other.is_cuda or not mine.is_cuda:
        raise RuntimeError("%s needs CUDA(HIP) tensors; there is no CPU fallback" % fn)
    if other.device != sceneCoordinates.device or mine.device != sceneCoordinates.device:
        raise RuntimeError("all tensors must be on the device of sceneCoordinates")


def _rgbd_call_args(sceneCoordinates, cameraCoordinates, depth, intr):
    """What a ctypes call needs of the RGB-D input, after the wrapper's own checks: the pointer/stride prefix up to B, Ho, Wo, the
    intrinsics tail (focal, ppx, ppy, sub, focals), the device, and the converted per-image focals, which must outlive the call."""
    focalLength, ppointX, ppointY, subSampling, focals = intr
    B, _, Ho, Wo = sceneCoordinates.shape
    dev = sceneCoordinates.device
    if focals is not None:
        focals = torch.as_tensor(focals).to(device=dev, dtype=torch.float32).contiguous()
        if focals.numel() != B:
            raise RuntimeError("expected %d focal lengths, got %d" % (B, focals.numel()))
    mb, mc, my, mx = cameraCoordinates.stride() if depth is None else (0, 0, 0, 0)
    db, dy, dx = depth.stride() if depth is not None else (0, 0, 0)
    prefix = (_ptr(sceneCoordinates), *sceneCoordinates.stride(), _ptr(cameraCoordinates), mb, mc, my, mx, _ptr(depth), db, dy, dx,
              B, Ho, Wo)
    tail = (float(focalLength or 0.0), float(ppointX or 0.0), float(ppointY or 0.0), int(subSampling or 1), _ptr(focals))
    return prefix, tail, dev, focals


def forward_rgbd_batch(sceneCoordinates, cameraCoordinates, outPoses, ransacHypotheses, inlierThreshold, inlierAlpha,
                       maxDistError, image0=0, image_stride=1, seed=None, max_tries=None, debug=False, depth=None,
                       focalLength=None, ppointX=None, ppointY=None, subSampling=None, focals=None):
    """RGB-D DSAC* (dsacstar_rgbd_forward, dsacstar.cpp:495-612) for B images in one launch: Kabsch hypotheses from three cells'
    scene and camera coordinates.  sceneCoordinates [B,3,Ho,Wo] float32 CUDA (any strides); EXACTLY ONE of cameraCoordinates
    [B,3,Ho,Wo] float32 CUDA (any strides) and depth [B,Ho,Wo] float32 CUDA (any strides).  With `depth` the camera coordinates
    are formed in the kernel from focalLength (or per-image `focals`), ppointX, ppointY and subSampling, as camera_coordinates
    does.  inlierThreshold and maxDistError are in centimetres.  A cell is valid iff its camera z is nonzero.  outPoses [B,4,4]
    float32 CUDA contiguous, written in place (asynchronous on the current stream).  With debug=True returns a dict of device
    tensors: cells [B,nHyp,3] int32, tries [B,nHyp] int32, scores [B,nHyp] float64, dbg [B,16] float64 (layout:
    include/crossloc_dsac.h)."""
    intr = (focalLength, ppointX, ppointY, subSampling, focals)
    _rgbd_source("forward_rgbd_batch", sceneCoordinates, cameraCoordinates, depth, intr, RGBD_MAX_CELLS)
    _rgbd_on_device("forward_rgbd_batch", sceneCoordinates, cameraCoordinates, depth, outPoses)
    B = sceneCoordinates.shape[0]
    if outPoses.dtype != torch.float32 or tuple(outPoses.shape) != (B, 4, 4) or not outPoses.is_contiguous():
        raise RuntimeError("outPoses must be a contiguous float32 [B,4,4] tensor")
    if int(ransacHypotheses) <= 0:
        raise RuntimeError("ransacHypotheses must be positive")
    prefix, tail, dev, focals = _rgbd_call_args(sceneCoordinates, cameraCoordinates, depth, intr)
    out = None
    cells = tries = scores = dbg = None
    if debug:
        cells = torch.zeros((B, ransacHypotheses, 3), dtype=torch.int32, device=dev)
        tries = torch.zeros((B, ransacHypotheses), dtype=torch.int32, device=dev)
        scores = torch.zeros((B, ransacHypotheses), dtype=torch.float64, device=dev)
        dbg = torch.zeros((B, RGBD_DBG_DOUBLES), dtype=torch.float64, device=dev)
        out = dict(cells=cells, tries=tries, scores=scores, dbg=dbg)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        rc = _lib.lib().xl_dsac_forward_rgbd_batch(
            *prefix, _ptr(outPoses), int(ransacHypotheses), float(inlierThreshold), float(inlierAlpha), float(maxDistError), *tail,
            int(RANSAC_SEED if seed is None else seed), int(image0), int(image_stride),
            int(MAX_HYPOTHESES_TRIES if max_tries is None else max_tries), ctypes.c_void_p(stream),
            _ptr(cells), _ptr(tries), _ptr(scores), _ptr(dbg))
    _lib.check(rc)
    return out


RGBD_BWD_REC = 64                        # XL_DSAC_RGBD_BWD_REC: doubles per hypothesis in backward_rgbd_batch's debug record


def backward_rgbd_batch(sceneCoordinates, cameraCoordinates, outSceneCoordinatesGrad, gtPoses, ransacHypotheses, inlierThreshold,
                        wLossRot, wLossTrans, softClamp, inlierAlpha, maxDistError, randomSeed, image0=0, image_stride=1,
                        max_tries=None, debug=False, depth=None, focalLength=None, ppointX=None, ppointY=None, subSampling=None,
                        focals=None):
    """RGB-D DSAC* backward pass (dsacstar_rgbd_backward, dsacstar.cpp:631-885) for B images: the expected pose loss over the
    hypothesis distribution and its gradient w.r.t. the scene coordinates, Kabsch hypotheses from depth.  Tensor rules as in
    forward_rgbd_batch: sceneCoordinates [B,3,Ho,Wo] float32 CUDA (any strides), EXACTLY ONE of cameraCoordinates [B,3,Ho,Wo] and
    depth [B,Ho,Wo] (float32 CUDA, any strides; depth needs focalLength or focals, ppointX, ppointY, subSampling),
    Ho*Wo <= RGBD_MAX_CELLS, thresholds in centimetres.  outSceneCoordinatesGrad: float32 with the shape of sceneCoordinates, any
    strides, ACCUMULATED (+=) like backward_rgb_batch.  gtPoses [B,4,4] cam->world.  randomSeed is the sampler's seed: with the
    seed and image keys of a forward_rgbd_batch call the hypotheses and scores are that call's, bit for bit.  Returns the expected
    losses as a float64 CUDA tensor [B] (asynchronous on the current stream); with debug=True also the per-hypothesis records
    [B,nHyp,RGBD_BWD_REC] (layout, deviations from the reference and the two guards: include/crossloc_dsac.h)."""
    intr = (focalLength, ppointX, ppointY, subSampling, focals)
    _rgbd_source("backward_rgbd_batch", sceneCoordinates, cameraCoordinates, depth, intr, RGBD_MAX_CELLS)
    B = sceneCoordinates.shape[0]
    g = outSceneCoordinatesGrad
    if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or tuple(g.shape) != tuple(sceneCoordinates.shape):
        raise RuntimeError("outSceneCoordinatesGrad must be float32 with the shape of sceneCoordinates")
    if not isinstance(gtPoses, torch.Tensor) or gtPoses.numel() != B * 16:
        raise RuntimeError("gtPoses must be a [B,4,4] tensor")
    if int(ransacHypotheses) <= 0:
        raise RuntimeError("ransacHypotheses must be positive")
    _rgbd_on_device("backward_rgbd_batch", sceneCoordinates, cameraCoordinates, depth, g)
    prefix, tail, dev, focals = _rgbd_call_args(sceneCoordinates, cameraCoordinates, depth, intr)
    gt = gtPoses.to(device=dev, dtype=torch.float32).reshape(B, 16).contiguous()
    loss = torch.zeros((B,), dtype=torch.float64, device=dev)
    rec = torch.zeros((B, int(ransacHypotheses), RGBD_BWD_REC), dtype=torch.float64, device=dev) if debug else None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        rc = _lib.lib().xl_dsac_backward_rgbd_batch(
            *prefix, _ptr(g), *g.stride(), _ptr(gt), _ptr(loss), int(ransacHypotheses), float(inlierThreshold),
            float(inlierAlpha), float(maxDistError), float(wLossRot), float(wLossTrans), float(softClamp), *tail,
            int(randomSeed), int(image0), int(image_stride),
            int(MAX_HYPOTHESES_TRIES if max_tries is None else max_tries), ctypes.c_void_p(stream), _ptr(rec))
    _lib.check(rc)
    return (loss, rec) if debug else loss


# field name -> column (or columns) of a pose_quality_rgbd_batch row; layout and meaning: include/crossloc_dsac.h.  The columns
# the RGB row shares keep their position (QUALITY_FIELDS); sigma_m takes the place of sigma_px
RGBD_QUALITY_FIELDS = {
    "n_cells": 0, "n_inliers": 1, "soft_score": 2, "sum_err": 3, "sum_err2": 4, "sse": 5, "status": 6,
    "sigma_m": 7, "sigma_pos_m": 8, "sigma_rot_deg": 9,
    "JtJ": slice(10, 31), "cov": slice(31, 52), "cov_center": slice(52, 58), "n_valid": 58, "reserved": slice(59, 64),
}


def pose_quality_rgbd_batch(sceneCoordinates, cameraCoordinates, poses, inlierThreshold, inlierAlpha, maxDistError, depth=None,
                            focalLength=None, ppointX=None, ppointY=None, subSampling=None, focals=None):
    """How far the RGB-D poses of B images can be trusted: inlier statistics of the metric 3-D residuals p - (R X + t), their
    JtJ over the inliers and the covariance of the rigid least-squares fit, at the given pose of each image (usually what
    forward_rgbd_batch wrote; enqueue this behind it on the same stream).  Tensor rules as in forward_rgbd_batch, without its
    cell limit: sceneCoordinates [B,3,Ho,Wo] float32 CUDA (any strides, any grid size), EXACTLY ONE of cameraCoordinates
    [B,3,Ho,Wo] and depth [B,Ho,Wo] (float32 CUDA, any strides; depth needs focalLength or focals, ppointX, ppointY, subSampling),
    thresholds in centimetres; poses [B,4,4] float32 CUDA contiguous cam->world.  Returns a float64 CUDA tensor [B,64]
    (RGBD_QUALITY_FIELDS names the columns), asynchronous on the current stream.  There is no CPU fallback."""
    intr = (focalLength, ppointX, ppointY, subSampling, focals)
    _rgbd_source("pose_quality_rgbd_batch", sceneCoordinates, cameraCoordinates, depth, intr)
    _rgbd_on_device("pose_quality_rgbd_batch", sceneCoordinates, cameraCoordinates, depth, poses)
    B = sceneCoordinates.shape[0]
    if poses.dtype != torch.float32 or tuple(poses.shape) != (B, 4, 4) or not poses.is_contiguous():
        raise RuntimeError("poses must be a contiguous float32 [B,4,4] tensor")
    prefix, tail, dev, focals = _rgbd_call_args(sceneCoordinates, cameraCoordinates, depth, intr)
    rows = torch.empty((B, QUALITY_DOUBLES), dtype=torch.float64, device=dev)      # (the kernel writes all 64 of every row)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        rc = _lib.lib().xl_dsac_pose_quality_rgbd_batch(
            *prefix, _ptr(poses), float(inlierThreshold), float(inlierAlpha), float(maxDistError), *tail,
            _ptr(rows), ctypes.c_void_p(stream))
    _lib.check(rc)
    return rows


# field name -> column (or columns) of a refine_pose_rgbd_batch row; layout and meaning: include/crossloc_dsac.h.  The positions
# of REFINE_FIELDS; chi is metres per axis in the plain form, the costs are r^T W r, and the last column is n_valid
RGBD_REFINE_FIELDS = {
    "n_cells": 0, "n_inliers": 1, "n_inliers_in": 2, "cost_in": 3, "cost_out": 4, "n_bad_sigma": 5, "status": 6,
    "chi": 7, "sigma_pos_m": 8, "sigma_rot_deg": 9,
    "JtJ": slice(10, 31), "cov": slice(31, 52), "cov_center": slice(52, 58),
    "rounds": 58, "evals": 59, "converged": 60, "moved_deg": 61, "moved_m": 62, "n_valid": 63,
}


def _rgbd_sigma_map(name, m, sceneCoordinates):
    """sigma / depthSigma of refine_pose_rgbd_batch: None or a float32 [B,Ho,Wo] tensor on the device of sceneCoordinates"""
    if m is None:
        return (0, 0, 0)
    B, _, Ho, Wo = sceneCoordinates.shape
    if not isinstance(m, torch.Tensor) or m.dtype != torch.float32 or tuple(m.shape) != (B, Ho, Wo):
        raise RuntimeError("%s must be a float32 [B,Ho,Wo] tensor like sceneCoordinates" % name)
    if m.device != sceneCoordinates.device:
        raise RuntimeError("%s must be on the device of sceneCoordinates" % name)
    return m.stride()


def refine_pose_rgbd_batch(sceneCoordinates, cameraCoordinates, sigma, poses, inlierThreshold, maxDistError, depthSigma=None,
                           depthRel=0.0, sigmaFloorM=0.01, maxRounds=8, depth=None, focalLength=None, ppointX=None, ppointY=None,
                           subSampling=None, focals=None, outPoses=None, w2c=None):
    """Ray-aware uncertainty-weighted refinement of the RGB-D poses of B images (model: include/crossloc_dsac.h): Levenberg-
    Marquardt over the inliers of the metric 3-D residuals p - (R X + t) under a 3x3 information matrix per cell, from the given
    pose of each image - usually what forward_rgbd_batch wrote; enqueue this behind it on the same stream.  Tensor rules as in
    pose_quality_rgbd_batch: sceneCoordinates [B,3,Ho,Wo] float32 CUDA (any strides, any grid size), EXACTLY ONE of
    cameraCoordinates [B,3,Ho,Wo] and depth [B,Ho,Wo] (float32 CUDA, any strides; depth needs focalLength or focals, ppointX,
    ppointY, subSampling), thresholds in centimetres; poses [B,4,4] float32 CUDA contiguous cam->world.  sigma [B,Ho,Wo] float32
    CUDA (any strides, metres; e.g. the channel view pred[:, 3] of the network output) or None; depthSigma [B,Ho,Wo] float32 CUDA
    (any strides, metres of depth; e.g. a depth network's uncertainty channel) or None; depthRel: relative depth noise;
    sigmaFloorM: the floor of sigma in metres.  With sigma None, depthSigma None and depthRel 0 it is a plain re-fit over the
    inliers.  outPoses (float32 [B,4,4], may be `poses`) and w2c (float64 [B,12], the refined world->camera pose) are optional
    CUDA contiguous outputs.  Returns (outPoses, rows): the refined poses and a float64 CUDA tensor [B,64] (RGBD_REFINE_FIELDS
    names the columns), asynchronous on the current stream.  There is no CPU fallback."""
    intr = (focalLength, ppointX, ppointY, subSampling, focals)
    _rgbd_source("refine_pose_rgbd_batch", sceneCoordinates, cameraCoordinates, depth, intr)
    _rgbd_on_device("refine_pose_rgbd_batch", sceneCoordinates, cameraCoordinates, depth, poses)
    B = sceneCoordinates.shape[0]
    if poses.dtype != torch.float32 or tuple(poses.shape) != (B, 4, 4) or not poses.is_contiguous():
        raise RuntimeError("poses must be a contiguous float32 [B,4,4] tensor")
    gs = _rgbd_sigma_map("sigma", sigma, sceneCoordinates)
    zs = _rgbd_sigma_map("depthSigma", depthSigma, sceneCoordinates)
    if not float(sigmaFloorM) > 0.0:
        raise RuntimeError("sigmaFloorM must be positive")
    if not 0.0 <= float(depthRel) < float("inf"):
        raise RuntimeError("depthRel must be finite and not negative")
    if not 1 <= int(maxRounds) <= REFINE_MAX_ROUNDS:
        raise RuntimeError("maxRounds must be in 1..%d" % REFINE_MAX_ROUNDS)
    prefix, tail, dev, focals = _rgbd_call_args(sceneCoordinates, cameraCoordinates, depth, intr)
    if outPoses is None:
        outPoses = torch.empty((B, 4, 4), dtype=torch.float32, device=dev)        # (the kernel writes all 16 of every pose)
    elif (not isinstance(outPoses, torch.Tensor) or outPoses.dtype != torch.float32 or tuple(outPoses.shape) != (B, 4, 4)
          or not outPoses.is_contiguous() or outPoses.device != dev):
        raise RuntimeError("outPoses must be a contiguous float32 [B,4,4] tensor on the device of sceneCoordinates")
    if w2c is not None and (not isinstance(w2c, torch.Tensor) or w2c.dtype != torch.float64 or tuple(w2c.shape) != (B, 12)
                            or not w2c.is_contiguous() or w2c.device != dev):
        raise RuntimeError("w2c must be a contiguous float64 [B,12] tensor on the device of sceneCoordinates")
    rows = torch.empty((B, REFINE_DOUBLES), dtype=torch.float64, device=dev)       # (the kernel writes all 64 of every row)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        rc = _lib.lib().xl_dsac_refine_pose_rgbd_batch(
            *prefix[:-3], _ptr(sigma), *gs, _ptr(depthSigma), *zs, *prefix[-3:], _ptr(poses), _ptr(outPoses), _ptr(rows), _ptr(w2c),
            float(inlierThreshold), float(maxDistError), *tail, float(sigmaFloorM), float(depthRel), int(maxRounds),
            ctypes.c_void_p(stream))
    _lib.check(rc)
    return outPoses, rows


def forward_rgbd(*args, **kwargs):
    """dsacstar_rgbd_forward (dsacstar.cpp:495-629): RGB-D variant, no call site in CrossLoc."""
    raise NotImplementedError("dsacstar.forward_rgbd is not on CrossLoc's path and is not implemented")


def backward_rgbd(*args, **kwargs):
    """dsacstar_rgbd_backward (dsacstar.cpp:631-885): RGB-D variant, no call site in CrossLoc."""
    raise NotImplementedError("dsacstar.backward_rgbd is not on CrossLoc's path and is not implemented")
