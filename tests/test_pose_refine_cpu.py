"""The uncertainty-weighted pose refinement without a GPU: the serial C restatement of the kernel (tests/pose_refine_ref.c, over
the product's xl_dsac_refine_math.h) against an independent numpy implementation of the model (tests/indep_pose_refine.py),
its accuracy on heteroscedastic frames, the calibration of its covariance, the pieces of the shared header and the argument
checks of the built library.  The kernel itself: tests/test_pose_refine_gpu.py, bit for bit against the restatement."""
import ctypes

import numpy as np
import pytest

import pose_refine_cases as rc
import pose_refine_ref
from crossloc_amd import synth


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pose_refine_ref.load(tmp_path_factory.mktemp("pose_refine_ref"))


def _angle_deg(Ra, Rb):
    D = Ra @ Rb.T
    s = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.degrees(np.arctan2(s, 0.5 * (np.trace(D) - 1.0))))


# 10 x the largest gap measured over the frames below (see the docstring of the test)
GAP_BOUND_M, GAP_BOUND_DEG = 10 * 4.44e-5, 10 * 3.4e-6


def test_restatement_matches_the_independent_implementation(ref):
    """40 heteroscedastic 24x36 frames (sigma 0.1 - 3 m, 30 % outliers, seeds 300...339), sigma form, from starts within
    0.5 m / 0.1 deg of ground truth.  Where the final inlier masks of the two coincide (at most 10 % of the frames may differ;
    measured: none does) the poses agree.  Measured largest gap: 4.44e-5 m between the camera centres, 3.4e-6 deg between the
    rotations - the order of the solver's own independent check: the restatement stops its Levenberg-Marquardt at a step of
    1.2e-7 of the parameter norm (the solver's FLT_EPSILON stop; |t| is 600 - 1000 m here), the independent Gauss-Newton runs
    on to 1e-13.  The bound is 10 x the measured gap."""
    gaps, skipped = [], 0
    seeds = range(300, 340)
    for seed in seeds:
        sc = rc.hetero(seed)
        start = rc.perturbed(sc["pose"], seed)
        pose, row, w2c, mask = ref.refine(sc["coords"], sc["sigma"], start, *rc.solver_args(sc), max_rounds=16)
        # the restatement reads its start as float32: the independent implementation starts from the same rounded matrix
        want = rc.indep_fit(sc, sc["sigma"], start.astype(np.float32).astype(np.float64))
        assert row[6] == 0 and want["status"] == 0 and row[60] == 1 and want["converged"], seed
        if not np.array_equal(mask, want["mask"]):
            skipped += 1
            continue
        assert row[1] == want["n"]
        R, t = w2c[:9].reshape(3, 3), w2c[9:]
        gaps.append((np.linalg.norm(R.T @ t - want["R"].T @ want["t"]), _angle_deg(R, want["R"])))
        assert abs(row[7] ** 2 - want["chi2"]) < 1e-6 * want["chi2"]
    gaps = np.array(gaps)
    print("frames compared %d of %d, largest gap %.3g m, %.3g deg" % (len(gaps), len(seeds), gaps[:, 0].max(), gaps[:, 1].max()))
    assert skipped <= len(seeds) // 10
    assert gaps[:, 0].max() <= GAP_BOUND_M and gaps[:, 1].max() <= GAP_BOUND_DEG


def test_accuracy_on_heteroscedastic_frames(ref):
    """The 48 frames of the accuracy set, both forms from the independent implementation's unweighted fit.  Measured: the
    independent implementation's median translation error 0.872 m under `inliers` and 0.331 m under `sigma` (0.38 x; rotation
    0.178 -> 0.068 deg); the restatement's four medians over those of the independent implementation: 1.0000 each."""
    frames = rc.accuracy_set()
    gt = [f["sc"]["pose"] for f in frames]
    assert all(f["unweighted"]["status"] == 0 and f["weighted"]["status"] == 0 for f in frames)      # no frame left out
    t_un, r_un = rc.errors(gt, [f["unweighted"]["pose"] for f in frames])
    t_w, r_w = rc.errors(gt, [f["weighted"]["pose"] for f in frames])
    print("independent: median t %.4f -> %.4f m (%.3f x), median r %.4f -> %.4f deg" % (
        np.median(t_un), np.median(t_w), np.median(t_w) / np.median(t_un), np.median(r_un), np.median(r_w)))
    assert np.median(t_w) <= 0.5 * np.median(t_un)
    got = {"inliers": [], "sigma": []}
    for f in frames:
        sc = f["sc"]
        for form, sigma in (("inliers", None), ("sigma", sc["sigma"])):
            pose, row, _, _ = ref.refine(sc["coords"], sigma, f["start"], *rc.solver_args(sc))
            assert row[6] == 0
            got[form].append(pose)
    for form, (t_i, r_i) in (("inliers", (t_un, r_un)), ("sigma", (t_w, r_w))):
        t_r, r_r = rc.errors(gt, got[form])
        print("restatement / independent, %s: t %.4f, r %.4f" % (form, np.median(t_r) / np.median(t_i), np.median(r_r) / np.median(r_i)))
        assert np.median(t_r) <= 1.05 * np.median(t_i) and np.median(r_r) <= 1.05 * np.median(r_i)
        assert np.median(t_i) <= 1.05 * np.median(t_r) and np.median(r_i) <= 1.05 * np.median(r_r)


def _log_so3(R):
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    n = np.linalg.norm(s)
    return s if n < 1e-300 else s / n * np.arctan2(n, 0.5 * (np.trace(R) - 1.0))


def test_covariance_is_calibrated_when_neither_the_gate_nor_the_floor_bites(ref):
    """2 scenes x 200 noise draws at 24x36, no outliers, sigma 0.25 - 2 m (at most ~6 px), s0 = 0.05 px, thr = 40 px, start at
    ground truth.  Mean chi^2 within 1 +- 0.1 and each of the six ratios `empirical over mean predicted variance` within
    1 +- 4 sqrt(2 / 200) = [0.6, 1.4], the sampling interval of a variance estimate from 200 draws.  Measured: mean chi^2
    1.019 and 1.018, ratios 0.92 - 1.34."""
    for seed in (11, 12):
        sc = rc.hetero(seed, sigma_range=(0.25, 2.0), outlier_ratio=0.0)
        clean = synth.make_scene(seed, noise=0.0, outlier_ratio=0.0, Ho=24, Wo=36)
        assert np.array_equal(clean["pose"], sc["pose"])                   # the same geometry: gt coordinates without noise
        R, t = rc.w2c(sc["pose"])
        args = rc.solver_args(sc, thr=40.0)
        rng = np.random.default_rng(5000 + seed)
        gt = clean["coords"].astype(np.float64)
        chi2, delta, var = [], [], []
        for _ in range(200):
            coords = (gt + rng.normal(size=gt.shape) * sc["sigma"][None]).astype(np.float32)
            _, row, w2c, _ = ref.refine(coords, sc["sigma"], sc["pose"], *args, s0=0.05)
            assert row[6] == 0 and row[1] > 0.99 * row[0]
            S = np.zeros((6, 6))
            S[np.triu_indices(6)] = row[31:52]
            chi2.append(row[7] ** 2)
            var.append(np.diag(S))
            delta.append(np.concatenate([_log_so3(w2c[:9].reshape(3, 3) @ R.T), w2c[9:] - t]))
        ratio = np.mean(np.square(delta), 0) / np.mean(var, 0)
        print("scene %d: mean chi^2 %.4f, ratios %s" % (seed, np.mean(chi2), np.round(ratio, 3)))
        assert abs(np.mean(chi2) - 1.0) <= 0.1
        assert (ratio >= 0.6).all() and (ratio <= 1.4).all()


def test_weight_one_gives_the_bits_of_the_unweighted_normal_equations(ref):
    """The weighted and the unweighted accumulator (pnp_cell_normal_eq_w, pnp_cell_normal_eq of xl_dsac_math.h) form the rows
    with one function; what is checked is what they add on top of it: the weight multiplies each product, not the rows, so
    w == 1.0 gives the unweighted bits and a power of two scales exactly.  And the weight itself against its formula."""
    sc = rc.hetero(21)
    R, t = rc.w2c(sc["pose"])
    for (y, x) in ((0, 0), (5, 17), (23, 35), (11, 2)):
        xyz = sc["coords"][:, y, x].astype(np.float64)
        a, q = ref.cell_normal_eq(R, t, xyz, 1.0, y, x, sc["focal"], sc["ppx"], sc["ppy"], rc.SUB)
        assert rc.same_bits(a, q) and np.abs(q).max() > 0
        a, q = ref.cell_normal_eq(R, t, xyz, 0.25, y, x, sc["focal"], sc["ppx"], sc["ppy"], rc.SUB)
        assert rc.same_bits(a, 0.25 * q)                                   # a power of two scales exactly
        z = (R @ xyz + t)[2]
        w = ref.weight(R, t, xyz, 0.7, 0.5, sc["focal"])
        assert abs(w - 1.0 / (0.25 + (sc["focal"] * 0.7 / z) ** 2)) <= 1e-14 * w
        assert ref.weight(R, t, xyz, 0.0, 1.0, sc["focal"]) == 1.0


def test_zero_sigma_with_unit_floor_gives_the_bits_of_the_null_form(ref):
    for seed in (31, 32, 33):
        sc = rc.hetero(seed)
        start = rc.perturbed(sc["pose"], seed)
        a = ref.refine(sc["coords"], None, start, *rc.solver_args(sc), s0=1.0)
        b = ref.refine(sc["coords"], np.zeros_like(sc["sigma"]), start, *rc.solver_args(sc), s0=1.0)
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and rc.same_bits(a[1], b[1]) and rc.same_bits(a[2], b[2])
        assert np.array_equal(a[3], b[3]) and a[1][6] == 0
        c = ref.refine(sc["coords"], None, start, *rc.solver_args(sc), s0=0.3)                # the NULL form ignores the floor
        assert rc.same_bits(a[1], c[1])


def test_pose_to_c2w16_is_the_rigid_inverse(ref):
    for seed in range(5):
        sc = synth.make_scene(seed, Ho=4, Wo=4)
        R, t = rc.w2c(sc["pose"])
        got = ref.pose_to_c2w16(R, t)
        want = np.linalg.inv(np.vstack([np.hstack([R, t[:, None]]), [0, 0, 0, 1]]))
        assert got.dtype == np.float32 and np.array_equal(got[3], [0, 0, 0, 1])
        # float32 rounding of entries up to ~1200 m, plus the float64 error of the inverse
        assert np.abs(got.astype(np.float64) - want)[:3].max() <= 2.0 ** -24 * np.abs(want).max() * 1.01


def test_status_and_sigma_edge_cases_of_the_restatement(ref):
    sig, n_bad = rc.sigma_status_maps()
    for name, coords, pose, qargs, status, n_inl in rc.status_cases(12, 16):
        want = {0: 0, 1: 1, 2: 2, 3: 3}[status]
        args = (qargs[0], qargs[1], qargs[2], qargs[3], qargs[5], qargs[6])
        for sigma in (None, np.full((12, 16), 0.5, np.float32)):
            out, row, w2c, mask = ref.refine(coords, sigma, pose, *args)
            assert row[6] == want, (name, sigma is None, row[6])
            if want != 0:
                assert np.array_equal(out.view(np.int32), pose.view(np.int32)) and not mask.any()
                nan = np.isnan(row)
                expect = np.zeros(64, bool)
                if want == 3:
                    expect[:] = True
                    expect[[0, 6]] = False
                    assert np.isnan(w2c).all()
                else:
                    expect[7:10] = True
                    expect[31:58] = True
                    assert row[1] == row[2] == n_inl and row[3] == row[4] and row[58] == 0 and (row[60:64] == 0).all()
                assert np.array_equal(nan, expect), name
            else:
                assert row[1] == mask.sum() and np.isfinite(row).all()
    sc = synth.make_scene(77, noise=0.5, outlier_ratio=0.0, Ho=12, Wo=16)
    args = rc.solver_args(sc)
    out, row, _, mask = ref.refine(sc["coords"], sig, sc["pose"], *args)
    assert row[6] == 0 and row[5] == n_bad and row[1] == 12 * 16 - n_bad and not mask[np.isnan(sig) | np.isinf(sig) | (sig < 0)].any()
    hs = rc.hetero(78, 12, 16)
    one = ref.refine(hs["coords"], hs["sigma"], rc.perturbed(hs["pose"], 3, 2.0, 0.5), *rc.solver_args(hs), max_rounds=1)[1]
    full = ref.refine(hs["coords"], hs["sigma"], rc.perturbed(hs["pose"], 3, 2.0, 0.5), *rc.solver_args(hs))[1]
    assert one[58] == 1 and one[60] == 0 and full[60] == 1 and 1 <= full[58] <= 8


@pytest.fixture(scope="module")
def hiplib():
    from crossloc_amd import build
    L = ctypes.CDLL(build.build())
    c_i64, c_i32, c_f, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    L.xl_dsac_refine_pose_batch.restype = c_i32
    L.xl_dsac_refine_pose_batch.argtypes = [vp, c_i64, c_i64, c_i64, c_i64, vp, c_i64, c_i64, c_i64, c_i32, c_i32, c_i32,
                                            vp, vp, vp, vp, c_f, c_f, c_f, c_f, c_f, c_i32, vp, c_f, c_i32, vp]
    return L


def test_argument_checks_come_before_any_device_work(hiplib):
    """XL_ERR_ARG / XL_ERR_GRID are returned before any HIP call: testable without a GPU (the pointers are never followed)."""
    from crossloc_amd import dsacstar as shim
    p = ctypes.c_void_p(4096)

    def call(coords=p, sigma=p, B=1, Ho=60, Wo=90, poses=p, out=p, rows=p, w2c=None, sub=8, s0=1.0, rounds=8):
        return hiplib.xl_dsac_refine_pose_batch(coords, 16200, 5400, 90, 1, sigma, 5400, 90, 1, B, Ho, Wo, poses, out, rows, w2c,
                                                10.0, 480.0, 360.0, 240.0, 100.0, sub, None, s0, rounds, None)

    for kw in (dict(coords=None), dict(poses=None), dict(out=None), dict(rows=None), dict(B=0), dict(Ho=0), dict(Wo=-1),
               dict(sub=0), dict(s0=0.0), dict(s0=-1.0), dict(s0=float("nan")), dict(rounds=0), dict(rounds=17)):
        assert call(**kw) == -1, kw
    assert shim.REFINE_MAX_CELLS == 10128 and shim.REFINE_DOUBLES == 64 and shim.REFINE_MAX_ROUNDS == 16
    Ho = shim.REFINE_MAX_CELLS // 100
    assert call(Ho=Ho + 1, Wo=100) == -2 and call(Ho=1, Wo=shim.REFINE_MAX_CELLS + 1) == -2
    assert call(Ho=2 ** 16, Wo=2 ** 16) == -2                              # the product does not fit an int
    f = shim.REFINE_FIELDS
    assert f["status"] == shim.QUALITY_FIELDS["status"] and f["sigma_pos_m"] == shim.QUALITY_FIELDS["sigma_pos_m"]
    assert f["cov"] == shim.QUALITY_FIELDS["cov"] and f["JtJ"] == shim.QUALITY_FIELDS["JtJ"]
    import dsacstar
    assert dsacstar.refine_pose_batch is shim.refine_pose_batch and dsacstar.REFINE_FIELDS is f
    torch = pytest.importorskip("torch")
    with pytest.raises(RuntimeError):                                      # tensor checks before any device work
        dsacstar.refine_pose_batch(torch.zeros(1, 3, 6, 9), None, torch.zeros(1, 4, 4), 10.0, 480.0, 36.0, 24.0, 100.0, 8)


def test_make_hetero_scene_leaves_make_scene_alone():
    a = synth.make_scene(100, Ho=24, Wo=36)
    h = synth.make_hetero_scene(100, Ho=24, Wo=36)
    assert np.array_equal(a["pose"], h["pose"]) and np.array_equal(a["gt_coords"], h["gt_coords"])
    assert h["sigma"].dtype == np.float32 and h["sigma"].shape == (24, 36)
    assert h["sigma"].min() >= 0.1 and h["sigma"].max() <= 3.0 and set(a) | {"sigma"} == set(h)
    # log-uniform: the median sits near the geometric mean of the range
    assert abs(np.log(np.median(h["sigma"])) - 0.5 * (np.log(0.1) + np.log(3.0))) < 0.2
    err = np.linalg.norm(h["coords"].astype(np.float64) - h["gt_coords"], axis=0)
    assert 0.25 < np.mean(err > 50.0) < 0.35                               # the gross outliers
    b = synth.make_scene(100, Ho=24, Wo=36)
    assert np.array_equal(a["coords"], b["coords"])
