"""Inputs shared by tests/test_rgbd_quality_cpu.py and tests/test_rgbd_quality_gpu.py — TEST INFRASTRUCTURE ONLY: solver
parameters, the independent numpy restatement of the RGB-D pose-quality row (uncentred normal equations), the hand-made
scenes that drive every status code, and the Monte-Carlo calibration run."""
import numpy as np

import dsac_rgbd_cases as rc
from crossloc_amd import synth
from pose_quality_cases import _log_so3, assert_nan_pattern, same_bits, w2c  # noqa: F401  (re-exported)

ALPHA, SUB = 100.0, 8
THR, MAX_DIST = 10.0, 100.0                # exact inputs: centimetres
NOISY_THR, NOISY_MAX_DIST = 300.0, 3000.0  # 0.5 m coordinate noise
NOISY = dict(noise=0.5, depth_noise=0.01, holes=0.2, outlier_ratio=0.3)


def batch(seed0, B, Ho, Wo, **kw):
    """B scenes of dsac_rgbd_cases.rgbd_scene stacked: dict(coords [B,3,Ho,Wo], cam, depth [B,Ho,Wo], pose [B,4,4] f32, focal)"""
    scs = [rc.rgbd_scene(seed0 + b, Ho, Wo, **kw) for b in range(B)]
    return dict(coords=np.stack([s["coords"] for s in scs]), cam=np.stack([s["cam"] for s in scs]),
                depth=np.stack([s["depth"] for s in scs]), pose=np.stack([s["pose"] for s in scs]).astype(np.float32),
                focal=scs[0]["focal"], ppx=scs[0]["ppx"], ppy=scs[0]["ppy"])


def cross(q):
    """[q]x for q [n,3] -> [n,3,3]"""
    z = np.zeros(len(q))
    return np.stack([np.stack([z, -q[:, 2], q[:, 1]], 1), np.stack([q[:, 2], z, -q[:, 0]], 1), np.stack([-q[:, 1], q[:, 0], z], 1)], 1)


def numpy_row(coords, cam, R, t, thr, alpha, max_dist):
    """The quantities of the row in float64 numpy, independent of the product's header: the residual r = p - (R X + t), the
    float inlier rule, and the UNCENTRED normal equations sum J^T J with J = [[R X]x, -I] per inlier, inverted by numpy.
    Returns dict(n_cells, n_valid, n, inl [N] bool, sum_err, sum_err2, sse, soft, JtJ [6,6], cov [6,6], sigma)."""
    _, Ho, Wo = coords.shape
    X = coords.reshape(3, -1).T.astype(np.float64)
    p = cam.reshape(3, -1).T.astype(np.float64)
    valid = cam.reshape(3, -1)[2] != 0
    q = np.stack([R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1] + R[i, 2] * X[:, 2] for i in range(3)], 1)       # R X
    r = p - (q + t)
    e = (np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]) * 100.0).astype(np.float32)
    e = np.minimum(e, np.float32(max_dist))
    thr32 = np.float32(thr)
    inl = valid & (e < thr32)
    beta = np.float32(5.0) / thr32
    st = (beta * (e[valid] - thr32)).astype(np.float64)
    soft = (1.0 - 1.0 / (1.0 + np.exp(-st))).sum()
    st_inv = np.float64(beta * (np.float32(max_dist) - thr32))
    soft += (Ho * Wo - valid.sum()) * (1.0 - 1.0 / (1.0 + np.exp(-st_inv)))
    fac = np.float32(alpha) / np.float32(Wo) / np.float32(Ho)
    n = int(inl.sum())
    J = np.concatenate([cross(q[inl]), -np.broadcast_to(np.eye(3), (n, 3, 3))], 2)                       # [n,3,6]
    JtJ = np.einsum("nki,nkj->ij", J, J)
    ed = e[inl].astype(np.float64)
    sse = float((r[inl] * r[inl]).sum())
    out = dict(n_cells=Ho * Wo, n_valid=int(valid.sum()), n=n, inl=inl, sum_err=ed.sum(), sum_err2=(ed * ed).sum(), sse=sse,
               soft=soft * np.float64(fac), JtJ=JtJ, r=r, q=q)
    if n >= 3:
        var = sse / (3.0 * n - 6.0)
        out.update(sigma=np.sqrt(var), cov=var * np.linalg.inv(JtJ))
    return out


# ------------------------------------------------------------------------------------------------ status cases

X0 = np.array([40.0, -12.0, 96.0])
LINE = np.array([0.5, 0.25, 1.0])


def _empty(Ho, Wo):
    """scene coordinates X0 everywhere, every cell invalid (camera coordinate 0)"""
    co = np.broadcast_to(X0.astype(np.float32)[:, None, None], (3, Ho, Wo)).copy()
    return co, np.zeros((3, Ho, Wo), np.float32)


def _place(co, cam, cells, points, offset=None):
    """cell (y, x) gets the scene coordinate `point` and, the pose being the identity, the camera coordinate point (+ offset)"""
    for (y, x), pt in zip(cells, points):
        co[:, y, x] = np.asarray(pt, np.float32)
        cam[:, y, x] = np.asarray(pt if offset is None else np.asarray(pt) + offset, np.float32)


def status_cases(Ho=12, Wo=16):
    """[(name, coords f32 [3,Ho,Wo], cam f32 [3,Ho,Wo], pose f32 [4,4] cam->world, expected status, inliers or None, valid or
    None)] at thr 10 cm, maxDist 100 cm.  The pose is the identity and an inlier has p = X in dyadic numbers, so every residual
    is exactly zero and the degeneracies are exact."""
    eye = np.eye(4, dtype=np.float32)
    spread = [(1, 2 % Wo), (3, (Wo - 3) % Wo), (Ho - 2, 1)]
    pts = [X0, X0 + np.array([8.0, 2.0, -4.0]), X0 + np.array([-3.0, 16.0, 32.0])]
    cases = []
    co, cam = _empty(Ho, Wo)
    cases.append(("all_invalid", co, cam, eye, 1, 0, 0))
    co, cam = _empty(Ho, Wo)
    _place(co, cam, spread[:2], pts[:2])
    cases.append(("two_inliers", co, cam, eye, 1, 2, 2))
    co, cam = _empty(Ho, Wo)
    _place(co, cam, spread, pts)
    _place(co, cam, [(Ho - 1, Wo - 1), (0, 0)], [X0, pts[1]], offset=np.array([0.0, 4.0, 64.0]))     # valid, 64 m off
    cases.append(("three_spread_inliers", co, cam, eye, 0, 3, 5))
    co, cam = _empty(Ho, Wo)
    _place(co, cam, [(y, 1) for y in range(Ho)], [X0] * Ho)
    cases.append(("one_point_column", co, cam, eye, 2, Ho, Ho))
    for name, scale in (("collinear", 1.0), ("collinear_far", 16.0)):
        co, cam = _empty(Ho, Wo)
        cells = [divmod((7 * k + 3) % (Ho * Wo), Wo) for k in range(12)]
        assert len(set(cells)) == 12
        _place(co, cam, cells, [scale * X0 + k * LINE for k in range(12)])
        cases.append((name, co, cam, eye, 2, 12, 12))
    sc = rc.rgbd_scene(77, Ho, Wo, noise=0.0, outlier_ratio=0.0)
    bad = sc["pose"].astype(np.float32)
    bad[1, 2] = np.nan
    cases.append(("nan_pose", sc["coords"], sc["cam"], bad, 3, None, None))
    return cases


def assert_status_row(row, status, n_inl, n_valid, Ho, Wo):
    assert row[0] == Ho * Wo and row[6] == status, (row[0], row[6])
    assert_nan_pattern_rgbd(row, status)
    if n_inl is not None:
        assert row[1] == n_inl and row[58] == n_valid, (row[1], row[58])


def assert_nan_pattern_rgbd(row, status):
    """pose_quality_cases.assert_nan_pattern with column 58 holding n_valid: the NaN pattern is the RGB row's, columns
    59..63 are zero and 58 is a count (NaN only under status 3)"""
    r = np.array(row, np.float64)
    if status != 3:
        assert r[58] >= 0 and r[58] == np.floor(r[58])
        r[58] = 0.0
    assert_nan_pattern(r, status)


# ------------------------------------------------------------------------------------------------ calibration

def calibration_run(qref, solver, seed, sigma=0.02, holes=0.0, outlier_ratio=0.0, draws=200, n_hyp=64, thr=50.0, max_dist=500.0):
    """Monte-Carlo calibration of the predicted covariance on the 60x90 scene `seed`: exact scene coordinates X, camera
    coordinates R X + t plus iid N(0, sigma^2) per axis cast to float32; a share `holes` of the cells has no camera coordinate
    and a share `outlier_ratio` has its scene coordinate moved by uniform +-30 m per axis.  Every draw goes through the solver
    restatement (image = draw) and the row is taken at its refined double pose.  Returns per-draw arrays (sigma_m, status,
    n_inliers, n_valid, solver_inliers, mahalanobis2, delta [draws,6], var_pred [draws,6]) and `ratio` [6] = mean delta_i^2 over
    the mean predicted variance, delta = (log(R_est R_gt^T), t_est - t_gt)."""
    from rgbd_quality_ref import sym
    sc = synth.make_scene(seed, noise=0.0, outlier_ratio=0.0)
    R, t = w2c(sc["pose"])
    _, Ho, Wo = sc["coords"].shape
    N = Ho * Wo
    X = sc["coords"].reshape(3, -1).T.astype(np.float64)
    m = X @ R.T + t
    rng = np.random.default_rng(2000 + seed)
    out = dict(sigma_m=[], status=[], n_inliers=[], n_valid=[], solver_inliers=[], mahalanobis2=[], delta=[], var_pred=[])
    for k in range(draws):
        p = (m + rng.normal(0.0, sigma, size=m.shape)).astype(np.float32)
        coords = sc["coords"]
        if holes > 0:
            p[rng.choice(N, size=int(round(holes * N)), replace=False)] = 0.0
        if outlier_ratio > 0:
            idx = rng.choice(N, size=int(round(outlier_ratio * N)), replace=False)
            Xk = X.copy()
            Xk[idx] += rng.uniform(-30.0, 30.0, size=(len(idx), 3))
            coords = np.ascontiguousarray(Xk.T.reshape(3, Ho, Wo).astype(np.float32))
        cam = np.ascontiguousarray(p.T.reshape(3, Ho, Wo))
        dbg = solver.forward(coords, n_hyp, thr, ALPHA, max_dist, cam=cam, image=k)["dbg"]
        Re, te = dbg[4:13].reshape(3, 3), dbg[13:16]
        row = qref.row_w2c(coords, Re, te, thr, ALPHA, max_dist, cam=cam)
        S = sym(row[31:52], 6)
        d = np.concatenate([_log_so3(Re @ R.T), te - t])
        out["sigma_m"].append(row[7]); out["status"].append(row[6]); out["n_inliers"].append(row[1]); out["n_valid"].append(row[58])
        out["solver_inliers"].append(dbg[3])
        out["delta"].append(d); out["var_pred"].append(np.diag(S))
        out["mahalanobis2"].append(d @ np.linalg.solve(S, d) if row[6] == 0 else np.nan)
    out = {k: np.asarray(v) for k, v in out.items()}
    out["ratio"] = np.mean(np.square(out["delta"]), 0) / np.mean(out["var_pred"], 0)
    return out
