"""RGB-D scenes shared by tests/test_dsac_rgbd_cpu.py and tests/test_dsac_rgbd_gpu.py — TEST INFRASTRUCTURE ONLY.

A scene of crossloc_amd.synth.make_scene with the depth a sensor at the ground-truth pose would measure: the ground-truth
camera coordinates are R^T (gt - c), the depth is their z (zero where the ray hits nothing), optionally with a seeded share of
cells zeroed (holes) and multiplicative noise.  The camera-coordinate tensor is the depth pushed through the product's
formula in numpy float32 (ray through the pixel centre times depth)."""
import numpy as np

from crossloc_amd import synth


def camera_from_depth(depth, focal, ppx, ppy, sub):
    """[3,Ho,Wo] float32 from depth [Ho,Wo] float32: ((px - ppx) / f) * d, ((py - ppy) / f) * d, d - every step in float32"""
    Ho, Wo = depth.shape
    f = np.float32(focal)
    rx = ((np.arange(Wo) * sub + sub // 2).astype(np.float32) - np.float32(ppx)) / f
    ry = ((np.arange(Ho) * sub + sub // 2).astype(np.float32) - np.float32(ppy)) / f
    return np.stack([rx[None, :] * depth, ry[:, None] * depth, depth]).astype(np.float32)


def rgbd_scene(seed, Ho, Wo, noise=0.0, outlier_ratio=0.3, depth_noise=0.0, holes=0.0, sub=synth.SUBSAMPLE):
    """dict(coords [3,Ho,Wo] f32 predicted scene coordinates, depth [Ho,Wo] f32, cam [3,Ho,Wo] f32, pose [4,4] f64 cam->world,
    focal, ppx, ppy, sub)"""
    s = synth.make_scene(seed, noise=noise, outlier_ratio=outlier_ratio, Ho=Ho, Wo=Wo, sub=sub)
    pose = s["pose"]
    gt = s["gt_coords"].astype(np.float64)
    hit = ~np.all(s["gt_coords"] == np.float32(synth.NODATA), axis=0)
    z = np.einsum("k,khw->hw", pose[:3, 2], gt - pose[:3, 3][:, None, None])          # z row of R^T (gt - c)
    depth = np.where(hit, z, 0.0)
    rng = np.random.default_rng(100003 * seed + 17)
    if depth_noise > 0:
        depth = depth * (1.0 + depth_noise * rng.normal(size=depth.shape))
    if holes > 0:
        idx = rng.choice(Ho * Wo, size=int(round(holes * Ho * Wo)), replace=False)
        depth.reshape(-1)[idx] = 0.0
    depth = depth.astype(np.float32)
    cam = camera_from_depth(depth, s["focal"], s["ppx"], s["ppy"], sub)
    return dict(coords=s["coords"], depth=depth, cam=cam, pose=pose, focal=s["focal"], ppx=s["ppx"], ppy=s["ppy"], sub=sub)


def pose_from_w2c(R, t):
    """cam->world 4x4 float64 of a world->camera (R, t)"""
    T = np.eye(4)
    T[:3, :3] = np.asarray(R).T
    T[:3, 3] = -np.asarray(R).T @ np.asarray(t)
    return T
