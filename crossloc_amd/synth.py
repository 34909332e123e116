"""Synthetic scenes for parity tests and the benchmark.

No datasets or trained weights exist offline, so every workload is generated: a sinusoidal terrain
near the naturescape label mean (utils/learning.py:92-94 of the reference), nadir-ish pinhole
cameras 150-350 m above it, scene-coordinate maps obtained by casting the centre of every output
cell (8x+4, 8y+4) onto the terrain, plus Gaussian noise and a fraction of gross outliers.
Everything is a pure function of the integer seed (numpy PCG64).
"""
import numpy as np

SCENE_MEAN = np.array([-455.934, 417.50, 520.31])   # naturescape coord mean, utils/learning.py:92
FOCAL = 480.0
IMAGE_H, IMAGE_W, SUBSAMPLE = 480, 720, 8
NODATA = -1.0


def terrain_height(x, y):
    """Height field (metres) around SCENE_MEAN[2]; x, y are world coordinates."""
    xr, yr = x - SCENE_MEAN[0], y - SCENE_MEAN[1]
    return SCENE_MEAN[2] - 240.0 + 40.0 * np.sin(xr / 90.0) * np.cos(yr / 70.0) + 15.0 * np.sin(xr / 23.0 + yr / 31.0)


def _rot_xyz(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def random_pose(rng, max_tilt_deg=25.0):
    """cam->world 4x4 (float64). Camera z looks down, x east, y south, then roll/pitch/yaw jitter."""
    nadir = np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])   # columns: camera axes in world
    tilt = np.deg2rad(max_tilt_deg)
    R = _rot_xyz(*(rng.uniform(-tilt, tilt, size=3))) @ nadir
    cx = SCENE_MEAN[0] + rng.uniform(-300, 300)
    cy = SCENE_MEAN[1] + rng.uniform(-300, 300)
    cz = terrain_height(cx, cy) + rng.uniform(150.0, 350.0)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = [cx, cy, cz]
    return T


def raycast(pose, Ho, Wo, sub=SUBSAMPLE, focal=FOCAL, ppx=IMAGE_W / 2, ppy=IMAGE_H / 2):
    """World points hit by the centre ray of every output cell -> [3, Ho, Wo] float64, hit mask."""
    xs = np.arange(Wo) * sub + sub // 2
    ys = np.arange(Ho) * sub + sub // 2
    u, v = np.meshgrid(xs, ys)
    d_cam = np.stack([(u - ppx) / focal, (v - ppy) / focal, np.ones_like(u, float)], 0).reshape(3, -1)
    d = pose[:3, :3] @ d_cam
    o = pose[:3, 3:4]
    hit = d[2] < -1e-3
    dz = np.where(hit, d[2], -1.0)
    lo = (o[2] - (SCENE_MEAN[2] - 240.0 + 56.0)) / -dz
    hi = (o[2] - (SCENE_MEAN[2] - 240.0 - 56.0)) / -dz
    for _ in range(48):
        mid = 0.5 * (lo + hi)
        p = o + d * mid
        above = p[2] > terrain_height(p[0], p[1])
        lo = np.where(above, mid, lo)
        hi = np.where(above, hi, mid)
    p = o + d * (0.5 * (lo + hi))
    return p.reshape(3, Ho, Wo), hit.reshape(Ho, Wo)


def make_scene(seed, noise=0.5, outlier_ratio=0.3, Ho=IMAGE_H // SUBSAMPLE, Wo=IMAGE_W // SUBSAMPLE,
               sub=SUBSAMPLE, focal=FOCAL):
    """One frame: returns dict(coords[3,Ho,Wo] f32 predicted map, gt_coords[3,Ho,Wo] f32 with NODATA,
    pose[4,4] f64 cam->world, focal)."""
    rng = np.random.default_rng(seed)
    ppx, ppy = Wo * sub / 2.0, Ho * sub / 2.0
    pose = random_pose(rng)
    gt, hit = raycast(pose, Ho, Wo, sub, focal, ppx, ppy)
    pred = gt + rng.normal(0.0, noise, size=gt.shape) if noise > 0 else gt.copy()
    n_out = int(round(outlier_ratio * Ho * Wo))
    if n_out > 0:
        idx = rng.choice(Ho * Wo, size=n_out, replace=False)
        lo = np.array([SCENE_MEAN[0] - 750, SCENE_MEAN[1] - 750, SCENE_MEAN[2] - 300])
        hi = np.array([SCENE_MEAN[0] + 750, SCENE_MEAN[1] + 750, SCENE_MEAN[2] - 180])
        pred.reshape(3, -1)[:, idx] = rng.uniform(lo[:, None], hi[:, None], size=(3, n_out))
    gt_lab = np.where(hit[None], gt, NODATA)
    return dict(coords=pred.astype(np.float32), gt_coords=gt_lab.astype(np.float32), pose=pose,
                focal=float(focal), ppx=float(ppx), ppy=float(ppy))


def make_hetero_scene(seed, sigma_range=(0.1, 3.0), outlier_ratio=0.3, Ho=IMAGE_H // SUBSAMPLE, Wo=IMAGE_W // SUBSAMPLE,
                      sub=SUBSAMPLE, focal=FOCAL):
    """One heteroscedastic frame: make_scene's dict plus sigma [Ho,Wo] f32, the standard deviation (metres) an honest network
    would predict for each cell.  sigma is log-uniform in `sigma_range` per cell and the coordinate noise of a cell is Gaussian
    with that sigma per axis; the gross outliers (drawn as in make_scene) keep their drawn sigma.  A function of its own:
    the draws of make_scene do not move."""
    rng = np.random.default_rng(seed)
    ppx, ppy = Wo * sub / 2.0, Ho * sub / 2.0
    pose = random_pose(rng)
    gt, hit = raycast(pose, Ho, Wo, sub, focal, ppx, ppy)
    lo_s, hi_s = float(sigma_range[0]), float(sigma_range[1])
    sigma = np.exp(rng.uniform(np.log(lo_s), np.log(hi_s), size=(Ho, Wo)))
    pred = gt + rng.normal(0.0, 1.0, size=gt.shape) * sigma[None]
    n_out = int(round(outlier_ratio * Ho * Wo))
    if n_out > 0:
        idx = rng.choice(Ho * Wo, size=n_out, replace=False)
        lo = np.array([SCENE_MEAN[0] - 750, SCENE_MEAN[1] - 750, SCENE_MEAN[2] - 300])
        hi = np.array([SCENE_MEAN[0] + 750, SCENE_MEAN[1] + 750, SCENE_MEAN[2] - 180])
        pred.reshape(3, -1)[:, idx] = rng.uniform(lo[:, None], hi[:, None], size=(3, n_out))
    gt_lab = np.where(hit[None], gt, NODATA)
    return dict(coords=pred.astype(np.float32), gt_coords=gt_lab.astype(np.float32), pose=pose,
                focal=float(focal), ppx=float(ppx), ppy=float(ppy), sigma=sigma.astype(np.float32))


def make_decoy_scene(seed, decoy=0.6, noise=0.5, Ho=IMAGE_H // SUBSAMPLE, Wo=IMAGE_W // SUBSAMPLE, sub=SUBSAMPLE, focal=FOCAL):
    """One frame whose larger part is structured garbage: two cameras P and Q are drawn; every cell holds the coordinates camera P
    sees plus Gaussian noise, then the top round(decoy * Ho) rows take EXACTLY the coordinates camera Q would see there - wrong,
    but consistent with each other, which the soft-inlier count cannot tell from the truth.  Returns make_scene's dict (pose = P)
    plus mask [Ho,Wo] uint8 (0 on the decoy rows, 1 elsewhere) and decoy_pose (Q).  A function of its own with a generator of
    its own: the draws of make_scene do not move."""
    rng = np.random.default_rng([seed, 0x4443])
    ppx, ppy = Wo * sub / 2.0, Ho * sub / 2.0
    pose = random_pose(rng)
    decoy_pose = random_pose(rng)
    gt, hit = raycast(pose, Ho, Wo, sub, focal, ppx, ppy)
    pred = gt + rng.normal(0.0, noise, size=gt.shape) if noise > 0 else gt.copy()
    rows = int(round(decoy * Ho))
    other, _ = raycast(decoy_pose, Ho, Wo, sub, focal, ppx, ppy)
    pred[:, :rows] = other[:, :rows]
    mask = np.ones((Ho, Wo), np.uint8)
    mask[:rows] = 0
    gt_lab = np.where(hit[None], gt, NODATA)
    return dict(coords=pred.astype(np.float32), gt_coords=gt_lab.astype(np.float32), pose=pose,
                focal=float(focal), ppx=float(ppx), ppy=float(ppy), mask=mask, decoy_pose=decoy_pose)


def camera_from_depth(depth, focal, ppx, ppy, sub=SUBSAMPLE):
    """Camera coordinates [3,Ho,Wo] float32 of a depth map [Ho,Wo] float32: the ray through the centre of every cell times the
    depth, every step in float32 - the formula the RGB-D solver applies to `depth` itself."""
    Ho, Wo = depth.shape
    f = np.float32(focal)
    rx = ((np.arange(Wo) * sub + sub // 2).astype(np.float32) - np.float32(ppx)) / f
    ry = ((np.arange(Ho) * sub + sub // 2).astype(np.float32) - np.float32(ppy)) / f
    return np.stack([rx[None, :] * depth, ry[:, None] * depth, depth]).astype(np.float32)


def make_hetero_rgbd_scene(seed, sigma_range=(0.02, 0.5), depth_rel=0.01, holes=0.0, outlier_ratio=0.3,
                           Ho=IMAGE_H // SUBSAMPLE, Wo=IMAGE_W // SUBSAMPLE, sub=SUBSAMPLE, focal=FOCAL):
    """One heteroscedastic RGB-D frame: make_hetero_scene's dict (the same draws) plus the depth a sensor at the ground-truth
    pose would measure.  depth [Ho,Wo] f32: the z of the ground-truth camera coordinate times (1 + depth_rel N(0, 1)), zero
    where the ray hits nothing and in a share `holes` of the cells; cam [3,Ho,Wo] f32: that depth through camera_from_depth;
    depth_sigma [Ho,Wo] f32: the standard deviation an honest depth network would predict, depth_rel times the true depth
    (zero where there is no depth).  A function of its own with a generator of its own: no existing draw moves."""
    s = make_hetero_scene(seed, sigma_range=sigma_range, outlier_ratio=outlier_ratio, Ho=Ho, Wo=Wo, sub=sub, focal=focal)
    pose = s["pose"]
    gt = s["gt_coords"].astype(np.float64)
    hit = ~np.all(s["gt_coords"] == np.float32(NODATA), axis=0)
    z = np.einsum("k,khw->hw", pose[:3, 2], gt - pose[:3, 3][:, None, None])          # z row of R^T (gt - c)
    z = np.where(hit, z, 0.0)
    rng = np.random.default_rng([seed, 0x5244])
    depth = z * (1.0 + depth_rel * rng.normal(size=z.shape))
    if holes > 0:
        idx = rng.choice(Ho * Wo, size=int(round(holes * Ho * Wo)), replace=False)
        depth.reshape(-1)[idx] = 0.0
    depth = depth.astype(np.float32)
    s.update(depth=depth, cam=camera_from_depth(depth, s["focal"], s["ppx"], s["ppy"], sub),
             depth_sigma=np.where(depth != 0, depth_rel * z, 0.0).astype(np.float32))
    return s


def make_batch(seed0, count, **kw):
    """`count` frames with seeds seed0, seed0+1, ... stacked: coords [B,3,Ho,Wo], gt [B,3,Ho,Wo], poses [B,4,4]."""
    scenes = [make_scene(seed0 + i, **kw) for i in range(count)]
    return (np.stack([s["coords"] for s in scenes]), np.stack([s["gt_coords"] for s in scenes]),
            np.stack([s["pose"] for s in scenes]))


def pose_error(gt_pose, est_pose):
    """(translation error [m], rotation error [deg]) as utils/evaluation.py:121-132 computes them
    (rotation angle of R_est^T R_gt; the angle is what ||cv2.Rodrigues(.)|| returns)."""
    gt_pose = np.asarray(gt_pose, np.float64)
    est_pose = np.asarray(est_pose, np.float64)
    t_err = float(np.linalg.norm(gt_pose[0:3, 3] - est_pose[0:3, 3]))
    r = est_pose[0:3, 0:3].T @ gt_pose[0:3, 0:3]
    # angle from the skew part and the trace (robust near 0 and near pi)
    s = 0.5 * np.linalg.norm([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
    c = 0.5 * (np.trace(r) - 1.0)
    r_err = float(np.degrees(np.arctan2(s, c)))
    return t_err, r_err
