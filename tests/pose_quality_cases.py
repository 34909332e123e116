"""Inputs shared by tests/test_pose_quality_cpu.py and tests/test_pose_quality_gpu.py: solver parameters, pose helpers and
the hand-made scenes that drive every status code of the pose-quality row."""
import numpy as np

from crossloc_amd import synth

THR, ALPHA, MAX_REPROJ, SUB = 10.0, 100.0, 100.0, 8


def w2c(pose_c2w):
    """float64 world->camera (R, t) of a cam->world 4x4."""
    T = np.asarray(pose_c2w, np.float64)
    R = T[:3, :3].T.copy()
    return R, -R @ T[:3, 3]


def far_point(pose_c2w):
    """A 3-D point that projects ~24000 px off the image at this pose: a gross outlier at any threshold used here."""
    T = np.asarray(pose_c2w, np.float64)
    return T[:3, 3] + T[:3, :3] @ np.array([5000.0, 5000.0, 100.0])


def solver_args(sc, thr=THR, max_reproj=MAX_REPROJ):
    """(thr, focal, ppx, ppy, alpha, max_reproj, sub) of a synth scene."""
    return (thr, sc["focal"], sc["ppx"], sc["ppy"], ALPHA, max_reproj, SUB)


def _keep_only(sc, cells):
    """The scene's coordinates with every cell but `cells` [(y, x), ...] replaced by a gross outlier."""
    co = sc["coords"].copy()
    keep = np.zeros(co.shape[1:], bool)
    for y, x in cells:
        keep[y, x] = True
    co[:, ~keep] = far_point(sc["pose"]).astype(np.float32)[:, None]
    return co


def status_cases(Ho=12, Wo=16):
    """[(name, coords f32 [3,Ho,Wo], pose f32 [4,4] cam->world, solver args, expected status, expected inliers or None)]"""
    sc = synth.make_scene(77, noise=0.5, outlier_ratio=0.0, Ho=Ho, Wo=Wo)
    pose = sc["pose"].astype(np.float32)
    args = solver_args(sc)
    spread = [(1, 2 % Wo), (3, (Wo - 3) % Wo), (Ho - 2, 4 % Wo), (Ho - 4, (Wo - 5) % Wo)]
    cases = [
        ("all_outliers", _keep_only(sc, []), pose, args, 1, 0),
        ("three_inliers", _keep_only(sc, spread[:3]), pose, args, 1, 3),
        ("four_inliers", _keep_only(sc, spread), pose, args, 0, 4),
        ("all_inliers", sc["coords"], pose, args, 0, Ho * Wo),
    ]
    # one cell column holding copies of ONE 3-D point, every other cell a gross outlier: with a threshold wider than the
    # column is long they are all inliers, every inlier has the same Jacobian rows, and JtJ has rank 2
    col = _keep_only(sc, [])
    X = sc["coords"][:, Ho // 2, 1].copy()
    col[:, :, 1] = X[:, None]
    wide = solver_args(sc, thr=float(8 * Ho + 64), max_reproj=float(2 * (8 * Ho + 64)))
    cases.append(("one_point_column", col, pose, wide, 2, Ho))
    bad = pose.copy()
    bad[1, 2] = np.nan
    cases.append(("nan_pose", sc["coords"], bad, args, 3, None))
    return cases


def assert_nan_pattern(row, status):
    """The NaN pattern include/crossloc_dsac.h promises for each status."""
    nan = np.isnan(row)
    if status == 3:
        want = np.ones(64, bool)
        want[[0, 6]] = False
    elif status in (1, 2):
        want = np.zeros(64, bool)
        want[7:10] = True
        want[31:58] = True
    else:
        want = np.zeros(64, bool)
    assert np.array_equal(nan, want), (status, np.flatnonzero(nan != want))
    if status != 3:
        assert np.all(row[58:64] == 0.0)
    assert row[6] == status


def same_bits(a, b):
    """Bitwise equality of float64 arrays; NaNs are compared by position (any payload)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64))


def _log_so3(R):
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    n = np.linalg.norm(s)
    return s if n < 1e-300 else s / n * np.arctan2(n, 0.5 * (np.trace(R) - 1.0))


def calibration_run(qref, oracle, seed, sigma=0.5, outlier_ratio=0.0, draws=200, n_hyp=64):
    """Monte-Carlo calibration of the predicted covariance on the 60x90 scene `seed`: the ground-truth points are moved in the
    camera frame so that the reprojection residual at the ground-truth pose is exactly iid N(0, sigma^2 px^2) per axis,
    X = R^T (z [(u + eu - cx) / f, (v + ev - cy) / f, 1] - t); a fraction `outlier_ratio` of the cells is then replaced by
    points drawn uniformly from the synthetic scene's box (as synth.make_scene draws its outliers).  Every draw goes
    through the oracle's solver and the quality row is taken at its refined double pose.  Returns per-draw arrays
    (sigma_px, status, n_inliers, mahalanobis2, delta [draws,6], var_pred [draws,6]) and `ratio` [6] = mean delta_i^2 over the
    mean predicted variance, with delta = (log(R_est R_gt^T), t_est - t_gt)."""
    from pose_quality_ref import sym
    sc = synth.make_scene(seed, noise=0.0, outlier_ratio=0.0)
    R, t = w2c(sc["pose"])
    f, cx, cy = sc["focal"], sc["ppx"], sc["ppy"]
    args = solver_args(sc)
    _, Ho, Wo = sc["coords"].shape
    X = sc["coords"].reshape(3, -1).T.astype(np.float64)
    ys, xs = np.divmod(np.arange(Ho * Wo), Wo)
    px = np.stack([xs * SUB + SUB // 2, ys * SUB + SUB // 2], 1).astype(np.float64)
    z = (X @ R.T + t)[:, 2]
    lo = np.array([synth.SCENE_MEAN[0] - 750, synth.SCENE_MEAN[1] - 750, synth.SCENE_MEAN[2] - 300])
    hi = np.array([synth.SCENE_MEAN[0] + 750, synth.SCENE_MEAN[1] + 750, synth.SCENE_MEAN[2] - 180])
    n_out = int(round(outlier_ratio * len(z)))
    rng = np.random.default_rng(1000 + seed)
    out = dict(sigma_px=[], status=[], n_inliers=[], mahalanobis2=[], delta=[], var_pred=[])
    for k in range(draws):
        eps = rng.normal(0.0, sigma, size=px.shape)
        ray = np.stack([(px[:, 0] + eps[:, 0] - cx) / f, (px[:, 1] + eps[:, 1] - cy) / f, np.ones(len(z))], 1)
        Xk = (z[:, None] * ray - t) @ R                                   # R^T (z ray - t), row-wise
        if n_out:
            idx = rng.choice(len(z), size=n_out, replace=False)
            Xk[idx] = rng.uniform(lo, hi, size=(n_out, 3))
        coords = np.ascontiguousarray(Xk.T.reshape(sc["coords"].shape).astype(np.float32))
        _, dbg = oracle.forward_rgb(coords, n_hyp, THR, f, cx, cy, ALPHA, MAX_REPROJ, SUB, image=k, debug=True)
        Re, te = dbg["pose1"][:9].reshape(3, 3), dbg["pose1"][9:]
        row = qref.row_w2c(coords, Re, te, *args)
        S = sym(row[31:52], 6)
        d = np.concatenate([_log_so3(Re @ R.T), te - t])
        out["sigma_px"].append(row[7]); out["status"].append(row[6]); out["n_inliers"].append(row[1])
        out["delta"].append(d); out["var_pred"].append(np.diag(S))
        out["mahalanobis2"].append(d @ np.linalg.solve(S, d) if row[6] == 0 else np.nan)
    out = {k: np.asarray(v) for k, v in out.items()}
    out["ratio"] = np.mean(np.square(out["delta"]), 0) / np.mean(out["var_pred"], 0)
    return out
