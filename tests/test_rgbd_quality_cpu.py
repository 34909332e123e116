"""CPU checks of the RGB-D pose-quality pass: the formulas of crossloc_amd/csrc/xl_dsac_rgbd_quality_math.h through the serial
restatement tests/rgbd_quality_ref.c (which the GPU kernel must match bit for bit, tests/test_rgbd_quality_gpu.py) against an
independent uncentred numpy restatement, numeric Jacobians, the solver restatement's scores and a Monte-Carlo calibration;
the status codes, a sanitizer run of the restatement as a program of its own, and the argument validation of the C entry
point, the Python front end and the wiring.  No GPU."""
import ctypes
import subprocess

import numpy as np
import pytest

import dsac_rgbd_cases as rc
import dsac_rgbd_ref
import rgbd_quality_cases as qc
import rgbd_quality_ref
from rgbd_quality_ref import sym


@pytest.fixture(scope="module")
def qref(tmp_path_factory):
    return rgbd_quality_ref.load(tmp_path_factory.mktemp("rgbd_quality_ref"))


@pytest.fixture(scope="module")
def solver(tmp_path_factory):
    return dsac_rgbd_ref.load(tmp_path_factory.mktemp("dsac_rgbd_ref"))


def _params(kw):
    return (qc.NOISY_THR, qc.ALPHA, qc.NOISY_MAX_DIST) if kw.get("noise") else (qc.THR, qc.ALPHA, qc.MAX_DIST)


@pytest.fixture(scope="module")
def posed_scenes(solver):
    """[(scene, params, R, t, what)]: 8x12 and 60x90, exact and noisy, each at ground truth and at the solver restatement's
    refined double pose"""
    out = []
    for seed, Ho, Wo, kw in ((5, 8, 12, dict(noise=0.0, outlier_ratio=0.3)), (6, 60, 90, dict(noise=0.0, outlier_ratio=0.3)),
                             (7, 8, 12, qc.NOISY), (8, 60, 90, qc.NOISY)):
        sc = rc.rgbd_scene(seed, Ho, Wo, **kw)
        par = _params(kw)
        out.append((sc, par) + qc.w2c(sc["pose"]) + ("ground truth %dx%d" % (Ho, Wo),))
        dbg = solver.forward(sc["coords"], 64, *par, cam=sc["cam"])["dbg"]
        out.append((sc, par, dbg[4:13].reshape(3, 3).copy(), dbg[13:16].copy(), "refined %dx%d" % (Ho, Wo)))
    return out


def test_row_matches_the_uncentred_numpy_restatement(qref, posed_scenes):
    """Count, n_valid and column 0 exact; sum e, sum e^2, SSE and the soft score to 1e-12 relative (only the order of the additions
    differs); JtJ within 1e-12 of its maximum; cov within 100 kappa 2^-52 of its maximum, kappa numpy's condition number of the
    uncentred JtJ that the restatement inverts."""
    for sc, par, R, t, what in posed_scenes:
        row = qref.row_w2c(sc["coords"], R, t, *par, cam=sc["cam"])
        want = qc.numpy_row(sc["coords"], sc["cam"], R, t, *par)
        assert row[6] == 0 and want["n"] >= 20, what
        assert row[0] == want["n_cells"] and row[1] == want["n"] and row[58] == want["n_valid"], what
        for col, key in ((2, "soft"), (3, "sum_err"), (4, "sum_err2"), (5, "sse")):
            assert abs(row[col] - want[key]) <= 1e-12 * abs(want[key]), (what, key, row[col], want[key])
        J, S = sym(row[10:31], 6), sym(row[31:52], 6)
        ej = np.abs(J - want["JtJ"]).max() / np.abs(want["JtJ"]).max()
        kappa = np.linalg.cond(want["JtJ"])
        es = np.abs(S - want["cov"]).max() / np.abs(want["cov"]).max()
        print("%s: JtJ %.2e  cov %.2e (kappa %.2e, bound %.2e)" % (what, ej, es, kappa, 100 * kappa * 2.0 ** -52))
        assert ej <= 1e-12, what
        assert es <= 100 * kappa * 2.0 ** -52, what
        assert abs(row[7] - want["sigma"]) <= 1e-12 * want["sigma"]


def test_derived_figures(qref, posed_scenes):
    """sigma_m, the camera-centre covariance (against the numeric Jacobian of C = -R^T t through apply_step), sigma_pos_m and
    sigma_rot_deg follow from SSE, n and cov as in the RGB row"""
    for sc, par, R, t, what in posed_scenes:
        row = qref.row_w2c(sc["coords"], R, t, *par, cam=sc["cam"])
        S, SC = sym(row[31:52], 6), sym(row[52:58], 3)
        assert row[7] == np.sqrt(row[5] / (3.0 * row[1] - 6.0))
        h = 1e-6
        An = np.zeros((3, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            Ru, tu = qref.apply_step(R, t, -d)
            Rd, td = qref.apply_step(R, t, d)
            An[:, k] = (-Ru.T @ tu + Rd.T @ td) / (2 * h)
        assert np.abs(SC - An @ S @ An.T).max() <= 1e-6 * np.abs(SC).max(), what
        assert np.isclose(row[8], np.sqrt(np.trace(SC)), rtol=1e-14)
        assert np.isclose(row[9], np.degrees(np.sqrt(S[0, 0] + S[1, 1] + S[2, 2])), rtol=1e-14)
        assert (np.diag(S) > 0).all() and (np.diag(SC) > 0).all()


def test_jtj_matches_numeric_jacobians(qref, posed_scenes):
    """JtJ of the row == Jn^T Jn with Jn by central differences (h = 1e-5) through apply_step and the residual p - (R X + t):
    |diff| <= 1e-7 max|JtJ| (truncation O(h^2) = 1e-10 relative, rounding 1e-16 / h = 1e-11: three orders of margin)."""
    h = 1e-5
    for sc, par, R, t, what in posed_scenes:
        row = qref.row_w2c(sc["coords"], R, t, *par, cam=sc["cam"])
        inl = qc.numpy_row(sc["coords"], sc["cam"], R, t, *par)["inl"]
        assert row[1] == inl.sum()
        X = sc["coords"].reshape(3, -1).T.astype(np.float64)[inl]
        p = sc["cam"].reshape(3, -1).T.astype(np.float64)[inl]
        Jn = np.zeros((3 * len(X), 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            Ru, tu = qref.apply_step(R, t, -d)                          # pose (+) d: apply_step subtracts
            Rd, td = qref.apply_step(R, t, d)
            Jn[:, k] = (((p - (X @ Ru.T + tu)) - (p - (X @ Rd.T + td))) / (2 * h)).reshape(-1)
        JtJ = sym(row[10:31], 6)
        err = np.abs(JtJ - Jn.T @ Jn).max() / np.abs(JtJ).max()
        print("%s: JtJ vs numeric %.3e" % (what, err))
        assert err <= 1e-7, what


def test_gradient_vanishes_at_the_fit(qref, solver):
    """At the Kabsch fit of its own inlier set (thr wide enough that the set is the same before and after the fit) the pose is
    the least-squares optimum: both gradient parts, sum u x r and sum r, are <= 1e-9 n max|u| max|r|."""
    for seed, kw in ((21, dict(noise=0.5, outlier_ratio=0.0, holes=0.2)), (22, dict(noise=0.5, outlier_ratio=0.3, depth_noise=0.01))):
        sc = rc.rgbd_scene(seed, 60, 90, **kw)
        par = (1000.0, qc.ALPHA, 10000.0)
        R0, t0 = qc.w2c(sc["pose"])
        inl = qc.numpy_row(sc["coords"], sc["cam"], R0, t0, *par)["inl"]
        X = sc["coords"].reshape(3, -1).T.astype(np.float64)
        p = sc["cam"].reshape(3, -1).T.astype(np.float64)
        R, t = solver.kabsch(p[inl], X[inl])
        at = qc.numpy_row(sc["coords"], sc["cam"], R, t, *par)
        assert np.array_equal(at["inl"], inl) and inl.sum() > 3000
        s = qref.sums_w2c(sc["coords"], R, t, *par, cam=sc["cam"])
        assert s["n"] == inl.sum()
        u = (at["q"][inl] + t) - s["c"]
        scale = inl.sum() * np.abs(u).max() * np.abs(at["r"][inl]).max()
        print("gradient: rot %.2e trans %.2e of %.2e" % (np.abs(s["grad_w"]).max(), np.abs(s["grad_t"]).max(), scale))
        assert np.abs(s["grad_w"]).max() <= 1e-9 * scale and np.abs(s["grad_t"]).max() <= 1e-9 * scale
        far = qref.sums_w2c(sc["coords"], R0, t0, *par, cam=sc["cam"])                                   # not at the fit: far from zero
        assert np.abs(far["grad_w"]).max() > 1e-6 * scale


def test_soft_score_is_the_solvers(qref, solver):
    """Column 2 at hypothesis h's pose == scores[h] of the solver restatement to 1e-12 relative (the solver sums the valid list
    x-major in 64 lanes, the pass row-major in 256 threads), for every hypothesis of two scenes with 20 % holes."""
    for seed, Ho, Wo, kw in ((31, 60, 90, qc.NOISY), (32, 33, 17, dict(noise=0.0, outlier_ratio=0.3, holes=0.2))):
        sc = rc.rgbd_scene(seed, Ho, Wo, **kw)
        par = _params(kw)
        res = solver.forward(sc["coords"], 64, *par, cam=sc["cam"])
        assert res["scores"].min() > 0 and len(set(res["scores"])) > 32                   # distinct hypotheses
        for h in range(64):
            row = qref.row_w2c(sc["coords"], res["hyp_poses"][h, :9].reshape(3, 3), res["hyp_poses"][h, 9:], *par, cam=sc["cam"])
            assert abs(row[2] - res["scores"][h]) <= 1e-12 * res["scores"][h], (seed, h, row[2], res["scores"][h])
            assert row[58] == res["dbg"][1]


@pytest.mark.parametrize("seed,holes,outliers", [(3, 0.0, 0.0), (11, 0.0, 0.0), (3, 0.2, 0.0), (3, 0.0, 0.3)])
def test_covariance_is_calibrated(qref, solver, seed, holes, outliers):
    """200 noise draws (sigma = 0.02 m per axis on the camera coordinates, 60x90, thr 50 cm) through the solver restatement: the
    estimated sigma is the true one (mean within 2 %, every draw within 4 % = 7 standard deviations at 16194 degrees of freedom),
    the per-parameter mean squared pose error over the mean predicted variance lies in [0.67, 1.33] (the 99.9 % interval of
    chi^2_200 / 200) and the mean squared Mahalanobis distance in [5.2, 6.8] (6 parameters).  With 20 % holes, and with 30 % of
    the scene coordinates moved by up to 30 m per axis (only the inliers count)."""
    out = qc.calibration_run(qref, solver, seed, sigma=0.02, holes=holes, outlier_ratio=outliers)
    print("seed %d holes %.1f outliers %.1f: ratio %s  mahalanobis^2 %.2f  sigma %.5f..%.5f mean %.5f"
          % (seed, holes, outliers, np.round(out["ratio"], 2), out["mahalanobis2"].mean(), out["sigma_m"].min(), out["sigma_m"].max(),
             out["sigma_m"].mean()))
    assert (out["status"] == 0).all()
    assert np.array_equal(out["n_inliers"], out["solver_inliers"])
    if outliers == 0:
        assert np.array_equal(out["n_inliers"], out["n_valid"])
    else:
        assert (out["n_inliers"] < 0.75 * 5400).all() and (out["n_inliers"] > 0.65 * 5400).all()
    assert abs(out["sigma_m"].mean() - 0.02) <= 0.02 * 0.02
    assert np.abs(out["sigma_m"] - 0.02).max() <= 0.04 * 0.02
    assert (out["ratio"] >= 0.67).all() and (out["ratio"] <= 1.33).all()
    assert 5.2 <= out["mahalanobis2"].mean() <= 6.8


@pytest.mark.parametrize("Ho,Wo", [(12, 16), (200, 4)])
def test_status_cases(qref, Ho, Wo):
    """Every status code with its NaN pattern; the degenerate sets are exact (identity pose, p = X, dyadic coordinates): one point,
    a line, the same line 16 times as far from the origin.  The line's last Cholesky pivot is rounding (far below
    XLQR_PIVOT_REL = 1e-12), the thinnest legitimate set is far above."""
    for name, co, cam, pose, status, n_inl, n_valid in qc.status_cases(Ho, Wo):
        row = qref.row(co, pose, qc.THR, qc.ALPHA, qc.MAX_DIST, cam=cam)
        qc.assert_status_row(row, status, n_inl, n_valid, Ho, Wo)
        if status in (0, 2):
            ratio = qref.sums_w2c(co, *qref.pose_from16(pose), qc.THR, qc.ALPHA, qc.MAX_DIST, cam=cam)["pivot_ratio"]
            print("%s: smallest relative pivot %.3e" % (name, ratio))
            assert ratio > 1e-7 if status == 0 else ratio < 1e-14, (name, ratio)
        if status == 0:
            assert row[7] == 0 and row[5] == 0 and np.isfinite(row).all()      # exact residuals: sigma is zero, not NaN


def test_thin_inlier_sets_stay_far_above_the_pivot_constant(qref):
    """Three neighbouring cells of a row are the thinnest set the pass accepts: over 39 scenes at 8x12, 12x16 and 60x90 their
    smallest relative Cholesky pivot stays five orders above XLQR_PIVOT_REL = 1e-12 (and exactly collinear sets four below it,
    test_status_cases)."""
    worst = np.inf
    for Ho, Wo in ((8, 12), (12, 16), (60, 90)):
        for seed in range(13):
            sc = rc.rgbd_scene(100 + seed, Ho, Wo, noise=0.0, outlier_ratio=0.0)
            R, t = qc.w2c(sc["pose"])
            y = Ho // 2
            xs = [x for x in range(Wo - 2) if (sc["depth"][y, x:x + 3] != 0).all()]
            assert xs
            cam = np.zeros_like(sc["cam"])
            cam[:, y, xs[0]:xs[0] + 3] = sc["cam"][:, y, xs[0]:xs[0] + 3]
            s = qref.sums_w2c(sc["coords"], R, t, qc.THR, qc.ALPHA, qc.MAX_DIST, cam=cam)
            row = qref.row_w2c(sc["coords"], R, t, qc.THR, qc.ALPHA, qc.MAX_DIST, cam=cam)
            assert s["n"] == 3 and row[6] == 0, (Ho, Wo, seed, s["n"], row[6])
            worst = min(worst, s["pivot_ratio"])
    print("smallest relative pivot of three neighbouring cells: %.3e" % worst)
    assert worst >= 1e-7


def test_depth_form_equals_camera_form(qref):
    sc = rc.rgbd_scene(41, 33, 17, **qc.NOISY)
    R, t = qc.w2c(sc["pose"])
    a = qref.row_w2c(sc["coords"], R, t, qc.NOISY_THR, qc.ALPHA, qc.NOISY_MAX_DIST, cam=sc["cam"])
    b = qref.row_w2c(sc["coords"], R, t, qc.NOISY_THR, qc.ALPHA, qc.NOISY_MAX_DIST, depth=sc["depth"], focal=sc["focal"], ppx=sc["ppx"],
                     ppy=sc["ppy"], sub=sc["sub"])
    assert qc.same_bits(a, b) and a[6] == 0
    p32 = sc["pose"].astype(np.float32)
    c = qref.row(sc["coords"], p32, qc.NOISY_THR, qc.ALPHA, qc.NOISY_MAX_DIST, cam=sc["cam"])
    d = qref.row_w2c(sc["coords"], *qref.pose_from16(p32), qc.NOISY_THR, qc.ALPHA, qc.NOISY_MAX_DIST, cam=sc["cam"])
    assert qc.same_bits(c, d)


def _have_static_sanitizers(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text("int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-o", str(tmp_path / "probe"), str(src)],
                       capture_output=True, text=True)
    return r.returncode == 0


def test_sanitizer_run_of_the_restatement(tmp_path):
    """tests/rgbd_quality_ref.c with its own main() under AddressSanitizer + UBSan (runtimes linked statically) on an 8x12 scene,
    a 60x90 scene and an all-invalid one: exit 0, no report"""
    if not _have_static_sanitizers(tmp_path):
        pytest.skip("gcc has no static AddressSanitizer / UBSan runtime here")
    prog = rgbd_quality_ref.build_program(tmp_path, sanitize=True)
    for name, Ho, Wo, thr, max_dist, kw, status in (("exact", 8, 12, 10.0, 100.0, dict(noise=0.0, outlier_ratio=0.3), 0),
                                                    ("noisy", 60, 90, 300.0, 3000.0, qc.NOISY, 0),
                                                    ("invalid", 12, 16, 10.0, 100.0, dict(noise=0.0, outlier_ratio=0.3), 1)):
        sc = rc.rgbd_scene(31, Ho, Wo, **kw)
        cam = sc["cam"] if name != "invalid" else np.zeros_like(sc["cam"])
        path = tmp_path / ("scene_%s.bin" % name)
        with open(path, "wb") as f:
            f.write(np.ascontiguousarray(sc["coords"]).tobytes())
            f.write(np.ascontiguousarray(cam).tobytes())
            f.write(np.ascontiguousarray(sc["pose"], np.float32).tobytes())
        r = subprocess.run([prog, str(path), str(Ho), str(Wo), str(thr), str(max_dist)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        assert "camera form: rc 0 status %d" % status in r.stdout and "depth form: rc 0 status %d" % status in r.stdout, r.stdout
        assert "same row 1" in r.stdout


# --------------------------------------------------------------------------------- argument validation, no GPU

def _abi(coords=8, cam=8, depth=None, B=1, Ho=8, Wo=12, poses=8, rows=8, sub=8):
    from crossloc_amd import _lib
    vp = ctypes.c_void_p
    return _lib.lib().xl_dsac_pose_quality_rgbd_batch(vp(coords), 288, 96, 12, 1, vp(cam), 288, 96, 12, 1, vp(depth), 96, 12, 1,
                                                      B, Ho, Wo, vp(poses), 10.0, 100.0, 100.0, 480.0, 48.0, 32.0, sub, None,
                                                      vp(rows), None)


def test_abi_rejects_bad_arguments_before_any_hip_call():
    """the pointers are never dereferenced: every case returns before the first HIP call"""
    ARG, GRID = -1, -2
    assert _abi(cam=None, depth=None) == ARG                   # neither camera coordinates nor depth
    assert _abi(cam=8, depth=8) == ARG                         # both
    assert _abi(coords=None) == ARG and _abi(poses=None) == ARG and _abi(rows=None) == ARG
    for kw in (dict(B=0), dict(Ho=0), dict(Wo=-3), dict(sub=0), dict(cam=None, depth=8, sub=-1)):
        assert _abi(**kw) == ARG, kw
    assert _abi(Ho=40000, Wo=60000) == GRID                    # the product does not fit an int


def test_python_front_end_rejects_bad_arguments():
    torch = pytest.importorskip("torch")
    import dsacstar
    assert dsacstar.RGBD_QUALITY_FIELDS["n_valid"] == 58 and dsacstar.RGBD_QUALITY_FIELDS["sigma_m"] == 7
    for k in ("n_cells", "n_inliers", "soft_score", "status", "sigma_pos_m", "sigma_rot_deg", "JtJ", "cov", "cov_center"):
        assert dsacstar.RGBD_QUALITY_FIELDS[k] == dsacstar.QUALITY_FIELDS[k], k
    co, cam, depth, poses = torch.zeros(1, 3, 8, 12), torch.zeros(1, 3, 8, 12), torch.zeros(1, 8, 12), torch.zeros(1, 4, 4)
    f = dsacstar.pose_quality_rgbd_batch
    with pytest.raises(RuntimeError, match="exactly one"):
        f(co, None, poses, 10.0, 100.0, 100.0)                                                  # neither
    with pytest.raises(RuntimeError, match="exactly one"):
        f(co, cam, poses, 10.0, 100.0, 100.0, depth=depth)                                      # both
    with pytest.raises(RuntimeError, match="cameraCoordinates must be"):
        f(co, cam[:, :2], poses, 10.0, 100.0, 100.0)                                            # shape
    with pytest.raises(RuntimeError, match="depth must be"):
        f(co, None, poses, 10.0, 100.0, 100.0, depth=depth[:, :4], focalLength=480.0, ppointX=48.0, ppointY=32.0, subSampling=8)
    with pytest.raises(RuntimeError, match="depth needs"):
        f(co, None, poses, 10.0, 100.0, 100.0, depth=depth)                                     # depth without intrinsics
    with pytest.raises(RuntimeError, match="subSampling must be positive"):
        f(co, None, poses, 10.0, 100.0, 100.0, depth=depth, focalLength=480.0, ppointX=48.0, ppointY=32.0, subSampling=0)
    with pytest.raises(RuntimeError, match="float32"):
        f(co, cam.double(), poses, 10.0, 100.0, 100.0)                                          # dtype
    with pytest.raises(RuntimeError, match="expected 4 dims"):
        f(co[0], cam, poses, 10.0, 100.0, 100.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(co, cam, poses, 10.0, 100.0, 100.0)                                                   # CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):                                  # above the solver's cell limit: no limit here
        f(torch.zeros(1, 3, 80, 80), torch.zeros(1, 3, 80, 80), poses, 10.0, 100.0, 100.0)


class _NeverRun:
    num_task_channel = 3
    OUTPUT_SUBSAMPLE = 8

    def __call__(self, images, plan_slot=0):
        raise AssertionError("the quality mode is checked before the network runs")


def test_rgbd_quality_mode_needs_depth_or_camera_coordinates():
    torch = pytest.importorskip("torch")
    from crossloc_amd import evaluation
    images = torch.zeros(1, 3, 64, 96)
    with pytest.raises(RuntimeError, match="needs depth or cam_coords"):
        evaluation.localize_batch(_NeverRun(), images, 16, 480.0, 64, 96, quality="rgbd")
    with pytest.raises(RuntimeError, match="must be False, True or"):
        evaluation.localize_batch(_NeverRun(), images, 16, 480.0, 64, 96, quality="depth", depth=torch.zeros(1, 8, 12))
    evaluation._check_quality_mode(True, None, None)
    evaluation._check_quality_mode(False, None, None)
    evaluation._check_quality_mode("rgbd", torch.zeros(1, 8, 12), None)
    with pytest.raises(RuntimeError, match="needs depth or cam_coords"):
        evaluation._check_quality_mode("rgbd", None, None)
