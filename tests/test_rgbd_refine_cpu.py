"""The ray-aware pose refinement behind the RGB-D solver without a GPU: the serial C restatement of the kernel
(tests/rgbd_refine_ref.c, over the product's xl_dsac_rgbd_refine_math.h) against an independent numpy implementation of the model
(tests/indep_rgbd_refine.py) and against the SVD Kabsch fit, the pieces of the shared header, every status, the calibration of
its covariance, its accuracy under depth noise and the argument checks of the built library.  The kernel itself:
tests/test_rgbd_refine_gpu.py, bit for bit against the restatement."""
import ctypes

import numpy as np
import pytest

import indep_rgbd_refine as ind
import rgbd_refine_cases as rc
import rgbd_refine_ref
from crossloc_amd import synth


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rgbd_refine_ref.load(tmp_path_factory.mktemp("rgbd_refine_ref"))


def _angle_deg(Ra, Rb):
    D = Ra @ Rb.T
    s = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.degrees(np.arctan2(s, 0.5 * (np.trace(D) - 1.0))))


def _gap(w2c, R, t):
    """(distance of the camera centres [m], angle between the rotations [deg]) of a w2c[12] and a world->camera {R, t}"""
    Rr, tr = w2c[:9].reshape(3, 3), w2c[9:]
    return np.linalg.norm(Rr.T @ tr - R.T @ t), _angle_deg(Rr, R)


# 3 x the largest gap measured over the frames below (see the docstrings of the tests), and the ceiling the issue sets
GAP_MEASURED_M, GAP_MEASURED_DEG = 5.02e-5, 2.74e-6
KABSCH_MEASURED_M, KABSCH_PIN_DEG = 1.33e-6, 1e-6
CEIL_M, CEIL_DEG = 1e-3, 1e-4


def test_restatement_matches_the_independent_implementation(ref):
    """40 heteroscedastic 24x36 frames (sigma 0.02 - 0.5 m, 1 % depth noise, 30 % outliers, gate 300 cm, seeds 300...339), the
    weighted form (sigma + depth_rel 0.01) and the plain form, from starts within 5 cm / 0.01 deg of ground truth.  Where the
    final inlier masks of the two coincide (at most 10 % of the runs may differ; measured: none does) the poses agree.
    Measured largest gap: 5.02e-5 m between the camera centres, 2.74e-6 deg between the rotations: the restatement stops its
    Levenberg-Marquardt at a step of 1.2e-7 of the parameter norm (the solver's FLT_EPSILON stop; |t| is 600 - 1000 m here), the
    independent Gauss-Newton runs on to 1e-13.  The bound is 3 x the measured gap and stays under 1e-3 m / 1e-4 deg."""
    gaps, skipped, runs = [], 0, 0
    for seed in range(300, 340):
        sc = rc.scene(seed)
        start = rc.perturbed(sc["pose"], seed)
        for sigma, k in ((sc["sigma"], 0.01), (None, 0.0)):
            runs += 1
            pose, row, w2c, mask = ref.refine(sc["coords"], start, rc.THR, rc.MAX_DIST, cam=sc["cam"], sigma=sigma, depth_rel=k,
                                              s0=rc.S0, max_rounds=16)
            # the restatement reads its start as float32: the independent implementation starts from the same rounded matrix
            want = rc.indep_fit(sc, start.astype(np.float32).astype(np.float64), sigma, None, k)
            assert row[6] == 0 and want["status"] == 0 and row[60] == 1 and want["converged"], seed
            if not np.array_equal(mask, want["mask"]):
                skipped += 1
                continue
            assert row[1] == want["n"] and row[5] == want["n_bad"] == 0 and row[63] == (sc["depth"] != 0).sum()
            gaps.append(_gap(w2c, want["R"], want["t"]))
            # the cost is flat at its minimum: a pose off by the gap bound g moves a residual of noise s >= 0.02 m by at most g,
            # chi^2 by (g / s)^2 = (1.7e-4 / 0.02)^2 = 7e-5 of itself
            assert abs(row[7] ** 2 - want["chi2"]) < 1e-4 * want["chi2"]
            # JtJ and Sigma in the row's parameters against the UNCENTRED numpy normal equations (condition 1e7 - 1e9)
            J, S = rgbd_refine_ref_sym(row[10:31]), rgbd_refine_ref_sym(row[31:52])
            assert np.abs(J - want["JtJ"]).max() <= 1e-6 * np.abs(want["JtJ"]).max()
            assert np.abs(np.diag(S) / np.diag(want["cov"]) - 1.0).max() <= 1e-4
    gaps = np.array(gaps)
    print("runs compared %d of %d, largest gap %.3g m, %.3g deg" % (len(gaps), runs, gaps[:, 0].max(), gaps[:, 1].max()))
    assert skipped <= runs // 10
    assert gaps[:, 0].max() <= 3 * GAP_MEASURED_M < CEIL_M and gaps[:, 1].max() <= 3 * GAP_MEASURED_DEG < CEIL_DEG


def rgbd_refine_ref_sym(ut):
    M = np.zeros((6, 6))
    M[np.triu_indices(6)] = np.asarray(ut, np.float64)
    return M + np.triu(M, 1).T


def test_plain_form_is_the_kabsch_fit_of_its_final_inlier_set(ref):
    """The 40 frames above, plain form: the pose against the closed-form SVD Kabsch fit of the final inlier set.  The project's
    RGB-D pin of 1e-6 deg holds for the rotations (measured: 3.75e-7 deg); for the camera centres the Levenberg-Marquardt stop
    (a step of 1.2e-7 of a parameter norm of 600 - 1000 m) leaves 1.33e-6 m, so the bound there is 3 x the measured value."""
    gaps = []
    for seed in range(300, 340):
        sc = rc.scene(seed)
        pose, row, w2c, mask = ref.refine(sc["coords"], rc.perturbed(sc["pose"], seed), rc.THR, rc.MAX_DIST, cam=sc["cam"],
                                          max_rounds=16)
        assert row[6] == 0 and row[60] == 1 and mask.sum() == row[1]
        X = sc["coords"].reshape(3, -1).T[mask.reshape(-1)].astype(np.float64)
        p = sc["cam"].reshape(3, -1).T[mask.reshape(-1)].astype(np.float64)
        R, t = ind.kabsch(X, p)
        gaps.append(_gap(w2c, R, t))
        # chi of the plain form is the residual standard deviation per axis of that fit
        sse = np.square(p - (X @ R.T + t)).sum()
        assert abs(row[7] - np.sqrt(sse / (3 * len(X) - 6))) <= 1e-6 * row[7]
    gaps = np.array(gaps)
    print("largest gap to the SVD Kabsch fit %.3g m, %.3g deg" % (gaps[:, 0].max(), gaps[:, 1].max()))
    assert gaps[:, 0].max() <= 3 * KABSCH_MEASURED_M < CEIL_M and gaps[:, 1].max() <= KABSCH_PIN_DEG


def test_information_matrix_and_cell_sums_against_numpy(ref):
    """W against a numpy inverse of a I + b rho rho^T; the 28 sums of one cell against J^T W J, J^T W r and r^T W r formed in
    numpy; b == 0 reduces to the scalar weight 1 / a; a == 1 and b == 0 return the vector itself."""
    sc = rc.scene(21)
    R, t = rc.w2c(sc["pose"])
    rng = np.random.default_rng(5)
    for (y, x) in ((0, 0), (5, 17), (23, 35), (11, 2)):
        xyz = sc["coords"][:, y, x].astype(np.float64)
        p = sc["cam"][:, y, x].astype(np.float64)
        sg, sz, s0, k = 0.3, 0.7, 0.05, 0.01
        a, b, rho, W = ref.noise(p, sg, sz, s0 * s0, k)
        assert abs(a - (s0 * s0 + sg * sg)) <= 1e-15 * a
        assert abs(b - (sz * sz + (k * p[2]) ** 2) * (p @ p) / p[2] ** 2) <= 1e-14 * b
        assert np.abs(rho - p / np.linalg.norm(p)).max() <= 1e-15
        want = np.linalg.inv(a * np.eye(3) + b * np.outer(rho, rho))
        assert np.abs(W - want).max() <= 1e-12 * np.abs(want).max()
        c = R @ xyz + t + rng.normal(size=3) * 40.0
        got = ref.cell_normal_eq(R, t, xyz, p, c, sg, sz, s0 * s0, k)
        m = R @ xyz + t
        r = p - m
        u = m - c
        J = np.hstack([np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]]), -np.eye(3)])
        H, g, cost = J.T @ want @ J, J.T @ want @ r, r @ want @ r
        assert np.abs(rgbd_refine_ref_sym(got[:21]) - H).max() <= 1e-11 * np.abs(H).max()
        assert np.abs(got[21:27] - g).max() <= 1e-11 * np.abs(g).max() and abs(got[27] - cost) <= 1e-11 * cost
        # no depth noise: the scalar weight
        a0, b0, _, W0 = ref.noise(p, sg, 0.0, s0 * s0, 0.0)
        assert b0 == 0.0 and np.array_equal(W0, np.eye(3) / a0)
        # the plain form: the identity, bit for bit
        a1, b1, _, W1 = ref.noise(p, 0.0, 0.0, 1.0, 0.0)
        assert a1 == 1.0 and b1 == 0.0 and np.array_equal(W1, np.eye(3))
        plain = ref.cell_normal_eq(R, t, xyz, p, c, 0.0, 0.0, 1.0, 0.0)
        assert np.abs(rgbd_refine_ref_sym(plain[:21]) - J.T @ J).max() <= 1e-12 * np.abs(J.T @ J).max()
    # the step in (rotation about c, centroid translation): the point c moves by the translation alone
    d = np.array([1e-3, -2e-3, 5e-4, 0.3, -0.2, 0.1])
    c = np.array([10.0, -20.0, 300.0])
    R2, t2 = ref.apply_step(R, t, c, d)
    E = ind.rodrigues(-d[:3])
    assert np.abs(R2 - E @ R).max() <= 1e-15 and np.abs(t2 - (c + E @ (t - c) - d[3:])).max() <= 1e-12
    Xc = R.T @ (c - t)                                                      # the scene point that sits at c
    assert np.abs((R2 @ Xc + t2) - (c - d[3:])).max() <= 1e-11


def test_zero_maps_with_unit_floor_give_the_bits_of_the_plain_form(ref):
    for seed in (31, 32, 33):
        sc = rc.scene(seed)
        start = rc.perturbed(sc["pose"], seed)
        zeros = np.zeros_like(sc["sigma"])
        a = ref.refine(sc["coords"], start, rc.THR, rc.MAX_DIST, cam=sc["cam"])
        b = ref.refine(sc["coords"], start, rc.THR, rc.MAX_DIST, cam=sc["cam"], sigma=zeros, depth_sigma=zeros, s0=1.0)
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and rc.same_bits(a[1], b[1]) and rc.same_bits(a[2], b[2])
        assert np.array_equal(a[3], b[3]) and a[1][6] == 0
        c = ref.refine(sc["coords"], start, rc.THR, rc.MAX_DIST, cam=sc["cam"], s0=0.3)       # the plain form ignores the floor
        assert rc.same_bits(a[1], c[1])
        d = ref.refine(sc["coords"], start, rc.THR, rc.MAX_DIST, depth=sc["depth"], focal=sc["focal"])    # depth form: equal bits
        assert rc.same_bits(a[1], d[1]) and np.array_equal(a[0].view(np.int32), d[0].view(np.int32))


def test_status_and_sigma_edge_cases_of_the_restatement(ref):
    for name, coords, cam, pose, status, n_inl, n_valid in rc.status_cases(12, 16):
        for sigma in (None, np.full((12, 16), 0.5, np.float32)):
            out, row, w2c, mask = ref.refine(coords, pose, 10.0, 100.0, cam=cam, sigma=sigma, depth_rel=0.0 if sigma is None else 0.01)
            rc.assert_status_row(name, row, out, w2c, pose, status, n_inl, n_valid, mask)
    sig, sig_z, n_bad = rc.sigma_status_maps()
    sc = rc.scene(77, 12, 16, outlier_ratio=0.0)
    out, row, _, mask = ref.refine(sc["coords"], sc["pose"], 3000.0, 1e5, cam=sc["cam"], sigma=sig, depth_sigma=sig_z)
    unusable = ~np.isfinite(sig) | (sig < 0) | ~np.isfinite(sig_z) | (sig_z < 0)
    assert unusable.sum() == n_bad and row[6] == 0 and row[5] == n_bad and row[63] == 12 * 16 and row[1] == 12 * 16 - n_bad
    assert not mask[unusable].any()
    holes = sc["cam"].copy()
    holes[:, 1, 3] = 0.0                                                    # an invalid cell is not counted as unusable
    row = ref.refine(sc["coords"], sc["pose"], 3000.0, 1e5, cam=holes, sigma=sig, depth_sigma=sig_z)[1]
    assert row[5] == n_bad - 1 and row[63] == 12 * 16 - 1
    hs = rc.scene(78, 12, 16)
    far = rc.perturbed(hs["pose"], 3, 1.0, 0.2)
    one = ref.refine(hs["coords"], far, rc.THR, rc.MAX_DIST, cam=hs["cam"], sigma=hs["sigma"], depth_rel=0.01, max_rounds=1)[1]
    full = ref.refine(hs["coords"], far, rc.THR, rc.MAX_DIST, cam=hs["cam"], sigma=hs["sigma"], depth_rel=0.01)[1]
    assert one[58] == 1 and one[60] == 0 and full[60] == 1 and 1 <= full[58] <= 8


def _log_so3(R):
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    n = np.linalg.norm(s)
    return s if n < 1e-300 else s / n * np.arctan2(n, 0.5 * (np.trace(R) - 1.0))


@pytest.mark.parametrize("depth_rel", [0.01, 0.0])
def test_covariance_is_calibrated_when_the_gate_does_not_bite(ref, depth_rel):
    """200 noise draws at 24x36 per depth-noise level (1 % and none), sigma 0.02 - 0.5 m, no outliers, gate 30 m, start at ground
    truth.  Each of the six ratios `empirical over mean predicted variance` within [0.6, 1.4] (4 standard deviations of a
    200-draw variance ratio) and the mean chi^2 per degree of freedom within [0.9, 1.1].  Measured: ratios 0.94 - 1.04 (1 %) and
    1.00 - 1.13 (none), mean chi^2 1.002 and 0.997."""
    seed = 11 if depth_rel > 0 else 12
    sc = rc.scene(seed, depth_rel=0.0, outlier_ratio=0.0)
    clean = synth.make_scene(seed, noise=0.0, outlier_ratio=0.0, Ho=24, Wo=36)
    assert np.array_equal(clean["pose"], sc["pose"])                       # the same geometry: gt coordinates without noise
    R, t = rc.w2c(sc["pose"])
    gt = clean["coords"].astype(np.float64)
    z = np.einsum("k,khw->hw", sc["pose"][:3, 2], gt - sc["pose"][:3, 3][:, None, None])
    rng = np.random.default_rng(5100 + seed)
    chi2, delta, var = [], [], []
    for _ in range(200):
        coords = (gt + rng.normal(size=gt.shape) * sc["sigma"][None]).astype(np.float32)
        depth = (z * (1.0 + depth_rel * rng.normal(size=z.shape))).astype(np.float32)
        cam = synth.camera_from_depth(depth, sc["focal"], sc["ppx"], sc["ppy"])
        _, row, w2c, _ = ref.refine(coords, sc["pose"], 3000.0, 1e5, cam=cam, sigma=sc["sigma"], depth_rel=depth_rel, s0=1e-3)
        assert row[6] == 0 and row[1] == row[0]
        chi2.append(row[7] ** 2)
        var.append(np.diag(rgbd_refine_ref_sym(row[31:52])))
        delta.append(np.concatenate([_log_so3(w2c[:9].reshape(3, 3) @ R.T), w2c[9:] - t]))
    ratio = np.mean(np.square(delta), 0) / np.mean(var, 0)
    print("depth_rel %g: mean chi^2 %.4f, ratios %s" % (depth_rel, np.mean(chi2), np.round(ratio, 3)))
    assert 0.9 <= np.mean(chi2) <= 1.1
    assert (ratio >= 0.6).all() and (ratio <= 1.4).all()


def test_weighted_form_beats_the_plain_form_under_depth_noise(ref):
    """48 frames of 24x36 (seeds 100...147) with 1 % depth noise, sigma 0.02 - 0.5 m and 30 % outliers, gate 300 cm, from starts
    within 5 cm of ground truth: the median translation error and the median rotation error of the weighted form (sigma +
    depth_rel 0.01) are each below the plain form's.  Measured: 0.952 -> 0.044 m (0.047 x), 0.204 -> 0.0096 deg (0.047 x); with
    scalar weights (sigma only) 1.236 m: no better than the plain form."""
    gt, got = [], {"plain": [], "sigma": [], "full": []}
    for seed in range(100, 148):
        sc = rc.scene(seed)
        start = rc.perturbed(sc["pose"], seed)
        gt.append(sc["pose"])
        for form, sigma, k in (("plain", None, 0.0), ("sigma", sc["sigma"], 0.0), ("full", sc["sigma"], 0.01)):
            pose, row, _, _ = ref.refine(sc["coords"], start, rc.THR, rc.MAX_DIST, cam=sc["cam"], sigma=sigma, depth_rel=k, s0=rc.S0)
            assert row[6] == 0
            got[form].append(pose)
    med = {form: [np.median(e) for e in rc.errors(gt, poses)] for form, poses in got.items()}
    print("median t / r: plain %.4f m %.4f deg, sigma only %.4f m %.4f deg, along-ray %.4f m %.4f deg (%.3f x, %.3f x)" % (
        *med["plain"], *med["sigma"], *med["full"], med["full"][0] / med["plain"][0], med["full"][1] / med["plain"][1]))
    assert med["full"][0] < med["plain"][0] and med["full"][1] < med["plain"][1]


@pytest.fixture(scope="module")
def hiplib():
    from crossloc_amd import _lib
    return _lib.lib()


def test_argument_checks_come_before_any_device_work(hiplib):
    """XL_ERR_ARG / XL_ERR_GRID are returned before any HIP call: testable without a GPU (the pointers are never followed)."""
    from crossloc_amd import dsacstar as shim
    p = ctypes.c_void_p(4096)

    def call(coords=p, cam=p, depth=None, sigma=p, sigma_z=p, B=1, Ho=60, Wo=90, poses=p, out=p, rows=p, w2c=None, sub=8, s0=0.01,
             k=0.01, rounds=8):
        return hiplib.xl_dsac_refine_pose_rgbd_batch(coords, 16200, 5400, 90, 1, cam, 16200, 5400, 90, 1, depth, 5400, 90, 1,
                                                     sigma, 5400, 90, 1, sigma_z, 5400, 90, 1, B, Ho, Wo, poses, out, rows, w2c,
                                                     300.0, 3000.0, 480.0, 360.0, 240.0, sub, None, s0, k, rounds, None)

    for kw in (dict(coords=None), dict(poses=None), dict(out=None), dict(rows=None), dict(B=0), dict(Ho=0), dict(Wo=-1),
               dict(sub=0), dict(s0=0.0), dict(s0=-1.0), dict(s0=float("nan")), dict(rounds=0), dict(rounds=17),
               dict(cam=None), dict(depth=p), dict(k=-0.01), dict(k=float("nan")), dict(k=float("inf"))):
        assert call(**kw) == -1, kw
    assert call(Ho=2 ** 16, Wo=2 ** 16) == -2                              # the cell index does not fit an int
    f = shim.RGBD_REFINE_FIELDS
    for name in ("n_cells", "n_inliers", "status", "chi", "sigma_pos_m", "sigma_rot_deg", "JtJ", "cov", "cov_center", "rounds",
                 "evals", "converged"):
        assert f[name] == shim.REFINE_FIELDS[name], name
    assert f["n_valid"] == 63 and f["n_bad_sigma"] == 5
    import dsacstar
    assert dsacstar.refine_pose_rgbd_batch is shim.refine_pose_rgbd_batch and dsacstar.RGBD_REFINE_FIELDS is f
    torch = pytest.importorskip("torch")
    co, pose = torch.zeros(1, 3, 6, 9), torch.zeros(1, 4, 4)
    with pytest.raises(RuntimeError):                                      # tensor checks before any device work
        dsacstar.refine_pose_rgbd_batch(co, torch.zeros(1, 3, 6, 9), None, pose, 300.0, 3000.0)
    with pytest.raises(RuntimeError):                                      # both of cam and depth
        dsacstar.refine_pose_rgbd_batch(co, torch.zeros(1, 3, 6, 9), None, pose, 300.0, 3000.0, depth=torch.zeros(1, 6, 9))
    with pytest.raises(RuntimeError):                                      # neither
        dsacstar.refine_pose_rgbd_batch(co, None, None, pose, 300.0, 3000.0)
    from crossloc_amd import evaluation
    with pytest.raises(RuntimeError):
        evaluation._check_refine_mode("rgbd_sigma", None, None)
    with pytest.raises(RuntimeError):
        evaluation._check_refine_mode("sigma", torch.zeros(1, 6, 9), None)
    assert evaluation._check_refine_mode("rgbd_inliers", torch.zeros(1, 6, 9), None)


def test_make_hetero_rgbd_scene_leaves_make_hetero_scene_alone():
    h = synth.make_hetero_scene(100, sigma_range=(0.02, 0.5), Ho=24, Wo=36)
    s = synth.make_hetero_rgbd_scene(100, Ho=24, Wo=36, holes=0.1)
    for k in h:
        assert np.array_equal(h[k], s[k]), k
    assert set(s) == set(h) | {"depth", "cam", "depth_sigma"}
    assert s["depth"].dtype == s["cam"].dtype == s["depth_sigma"].dtype == np.float32 and s["cam"].shape == (3, 24, 36)
    assert (s["depth"] == 0).sum() >= round(0.1 * 24 * 36) and np.array_equal(s["depth_sigma"] == 0, s["depth"] == 0)
    # the camera tensor is the depth through the solver's formula, and the depth is within 6 sigma of the true one
    assert np.array_equal(s["cam"], synth.camera_from_depth(s["depth"], s["focal"], s["ppx"], s["ppy"]))
    R, t = rc.w2c(s["pose"])
    hit = s["depth"] != 0
    z = (np.einsum("ij,jhw->ihw", R, s["gt_coords"].astype(np.float64)) + t[:, None, None])[2]
    assert np.abs(s["depth"][hit] / z[hit] - 1.0).max() < 0.06 and 0.005 < np.std(s["depth"][hit] / z[hit] - 1.0) < 0.015
    assert np.abs(s["depth_sigma"][hit] / (0.01 * z[hit]) - 1.0).max() < 1e-5
    assert np.array_equal(synth.make_hetero_scene(100, sigma_range=(0.02, 0.5), Ho=24, Wo=36)["coords"], h["coords"])
