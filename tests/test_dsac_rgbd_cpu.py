"""CPU checks of the RGB-D DSAC* solver: the formulas of crossloc_amd/csrc/xl_dsac_rgbd_math.h through the serial restatement
tests/dsac_rgbd_ref.c (which the GPU kernel must match bit for bit, tests/test_dsac_rgbd_gpu.py) against
tests/indep_dsac_rgbd.py (numpy, SVD Kabsch, no shared code), accuracy on exact and noisy inputs, a sanitizer run of the
restatement as a program of its own, and the argument validation of the C entry point and the Python front end.  No GPU."""
import ctypes
import subprocess

import numpy as np
import pytest

import dsac_rgbd_cases as rc
import dsac_rgbd_ref
import indep_dsac_rgbd as indep
from crossloc_amd import synth

N_HYP = 64
GRIDS = [(33, 17), (60, 90)]
SEEDS = (1, 2, 3, 4)
RATIOS = (0.0, 0.3, 0.6)
# the sweep's scenes: 0.1 m coordinate noise (three-point fits then leave residuals of centimetres, so the threshold decides)
SWEEP = dict(noise=0.1, thr=50.0, alpha=100.0, max_dist=1000.0)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return dsac_rgbd_ref.load(tmp_path_factory.mktemp("dsac_rgbd_ref"))


@pytest.fixture(scope="module")
def sweep(ref):
    """the restatement on every (grid, seed, outlier ratio) of the sweep, computed once: key -> (scene, result)"""
    out = {}
    for Ho, Wo in GRIDS:
        for seed in SEEDS:
            for ratio in RATIOS:
                sc = rc.rgbd_scene(seed, Ho, Wo, noise=SWEEP["noise"], outlier_ratio=ratio)
                res = ref.forward(sc["coords"], N_HYP, SWEEP["thr"], SWEEP["alpha"], SWEEP["max_dist"], cam=sc["cam"], image=seed,
                                  rounds=True)
                out[(Ho, Wo, seed, ratio)] = (sc, res)
    return out


def _pairs(sc, cells):
    """camera and scene coordinates [n,3] float64 of the given cells (indices y * Wo + x)"""
    cm = sc["cam"].reshape(3, -1).T.astype(np.float64)
    co = sc["coords"].reshape(3, -1).T.astype(np.float64)
    return cm[cells], co[cells]


def _check_fit(R, t, p, X, what):
    """R proper and orthonormal to 1e-12; objective = the SVD optimum to 1e-9 relative + 1e-12 of the summed squared (centred)
    norms.  R and t are compared with numpy's for EVERY set; a disagreement is an error where sigma_2 > 1e-3 sigma_1, below that
    ratio the set is left out of the pose comparison (returns False).  Thin triangles (sigma_2 / sigma_1 is the squared aspect
    ratio of the point set, below 1e-3 for ~6 % of random triples) are well within the bound and are not left out; repeated
    draws, where the optimal rotation is a one-parameter family, are."""
    assert np.isfinite(R).all() and np.isfinite(t).all(), what
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12, what
    assert abs(np.linalg.det(R) - 1.0) <= 1e-12, what
    Rn, tn, W = indep.kabsch_svd(p, X)
    floor = 1e-12 * (((p - p.mean(0)) ** 2).sum() + ((X - X.mean(0)) ** 2).sum())
    got, want = indep.objective(R, t, p, X), indep.objective(Rn, tn, p, X)
    assert abs(got - want) <= 1e-9 * want + floor, (what, got, want)
    agree = np.abs(R - Rn).max() <= 1e-8 and np.linalg.norm(t - tn) <= 1e-8 * np.linalg.norm(tn)
    assert agree or not W[1] > 1e-3 * W[0], (what, np.abs(R - Rn).max(), t, tn, W)
    return bool(agree)


def test_kabsch_is_optimal_for_every_hypothesis_and_round(sweep):
    """Optimality holds for every accepted hypothesis and every refinement round, whatever the conditioning; the pose itself
    must agree where sigma_2 > 1e-3 sigma_1, and at most 5 % of an image's hypotheses may be left out of that comparison."""
    shares = []
    for key, (sc, res) in sweep.items():
        accepted = np.flatnonzero(res["tries"] > 0)
        assert accepted.size > 0, key
        skipped = 0
        for h in accepted:
            p, X = _pairs(sc, res["cells"][h])
            Rt = res["hyp_poses"][h]
            if not _check_fit(Rt[:9].reshape(3, 3), Rt[9:], p, X, (key, "hypothesis", int(h))):
                skipped += 1
        shares.append(skipped / accepted.size)
        assert skipped <= 0.05 * accepted.size, (key, skipped, accepted.size)
        for r in range(res["round_poses"].shape[0]):
            cells = np.flatnonzero(res["round_masks"][r].reshape(-1))
            p, X = _pairs(sc, cells)
            Rt = res["round_poses"][r]
            assert _check_fit(Rt[:9].reshape(3, 3), Rt[9:], p, X, (key, "round", r)), (key, "ill-conditioned inlier set", r)
    print("share of hypotheses left out of the pose comparison: max %.4f mean %.4f" % (max(shares), float(np.mean(shares))))


def test_kabsch_degenerate_sets(ref):
    """rank 2 (three points), rank 1 (a repeated draw), rank 0 (one point three times), a reflection-optimal set and collinear
    points: finite, deterministic, proper, optimal"""
    rng = np.random.default_rng(5)
    X3 = rng.normal(size=(3, 3)) * 50.0 + np.array([-455.0, 417.0, 280.0])
    Rg = synth._rot_xyz(0.3, -0.2, 1.1)
    p3 = X3 @ Rg.T + np.array([3.0, -2.0, 200.0])
    sets = {
        "three points": (p3, X3),
        "repeated draw": (p3[[0, 1, 1]], X3[[0, 1, 1]]),
        "one point": (p3[[2, 2, 2]], X3[[2, 2, 2]]),
        "collinear": (np.outer([0.0, 1.0, 2.5, 4.0], [1.0, 2.0, 3.0]), np.outer([0.0, 1.0, 2.5, 4.0], [3.0, 1.0, 2.0]) + 7.0),
        "mirror image": (rng.normal(size=(6, 3)) * [1.0, 1.0, -1.0], None),
    }
    m = sets["mirror image"][0]
    sets["mirror image"] = (m, m * [1.0, 1.0, -1.0] + rng.normal(size=m.shape) * 1e-3)
    for name, (p, X) in sets.items():
        R, t = ref.kabsch(p, X)
        R2, t2 = ref.kabsch(p, X)
        assert np.array_equal(R, R2) and np.array_equal(t, t2), name
        if name != "one point":                              # (no spread: the bound's floor is zero there)
            _check_fit(R, t, np.asarray(p, np.float64), np.asarray(X, np.float64), name)
    R, t = ref.kabsch(*sets["one point"])                    # A is zero up to the rounding of the centroid: any rotation is optimal
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12
    assert np.abs(p3[2] - (R @ X3[2] + t)).max() <= 1e-9
    R, t = ref.kabsch(np.array([[1.0, 2.0, 4.0]] * 3), np.array([[8.0, -2.0, 16.0]] * 3))
    assert np.array_equal(R, np.eye(3)) and np.array_equal(t, [-7.0, 4.0, -12.0]), "A == 0 leaves the identity rotation"


def _angle_deg(Ra, Rb):
    r = Ra.T @ Rb
    s = 0.5 * np.linalg.norm([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
    return float(np.degrees(np.arctan2(s, 0.5 * (np.trace(r) - 1.0))))


def test_replay_against_numpy(sweep):
    """The restatement's sampled cells through the numpy implementation: scores to 1e-9 relative, the same winner, the same
    inlier count in every refinement round, the final pose (doubles) within 1e-6 m and 1e-6 degrees.
    Two score comparisons, both at 1e-9 relative.  (1) Scoring, nothing left out: numpy's error map and score at the
    restatement's own pose of EVERY hypothesis (error in cm, float cast, clamp, sigmoid, the invalid cells' term, alpha / Wo /
    Ho) - well conditioned whatever the sampled set.  (2) The whole chain cells -> SVD Kabsch -> score for the sets with
    sigma_2 > 1e-3 sigma_1; below that ratio two correct double-precision fits differ by about eps sigma_1 / sigma_2 in R
    (a repeated draw has a one-parameter family of optimal rotations), which test_kabsch_is_optimal... covers through the
    objective.  The winner must be a set above the ratio."""
    compared = total = 0
    for key, (sc, res) in sweep.items():
        got = indep.solve(sc["coords"], sc["cam"], N_HYP, SWEEP["thr"], SWEEP["alpha"], SWEEP["max_dist"], cells=res["cells"])
        ratio = np.array([(lambda W: W[1] / W[0] if W[0] > 0 else 0.0)(indep.kabsch_svd(*_pairs(sc, c))[2]) for c in res["cells"]])
        well = ratio > 1e-3
        total += N_HYP
        compared += int(well.sum())
        _, Ho, Wo = sc["coords"].shape
        co = sc["coords"].reshape(3, -1).T.astype(np.float64)
        cm = sc["cam"].reshape(3, -1).T.astype(np.float64)
        valid = indep.valid_list(sc["cam"])
        own = np.array([indep.score_of(indep.error_map(Rt[:9].reshape(3, 3), Rt[9:], co, cm, valid, SWEEP["max_dist"]),
                                       SWEEP["thr"], SWEEP["alpha"], Ho, Wo) for Rt in res["hyp_poses"]])
        err = np.abs(res["scores"] - own)
        assert (err <= 1e-9 * np.abs(own)).all(), (key, "scoring at the restatement's poses", (err / np.abs(own)).max())
        err = np.abs(res["scores"] - got["scores"])[well]
        assert (err <= 1e-9 * np.abs(got["scores"][well])).all(), (key, "cells -> SVD -> score", err.max())
        win = int(res["dbg"][0])
        assert well[win] and win == got["winner"], (key, win, got["winner"])
        assert list(res["round_counts"]) == got["round_counts"], (key, res["round_counts"], got["round_counts"])
        R, t = res["dbg"][4:13].reshape(3, 3), res["dbg"][13:16]
        assert np.linalg.norm(-R.T @ t - got["pose"][:3, 3]) <= 1e-6, key
        assert _angle_deg(R, got["R"]) <= 1e-6, key
        assert int(res["dbg"][2]) == len(got["round_counts"]) - 1 and int(res["dbg"][3]) == ([0] + got["round_counts"])[-2], key
    assert compared >= 0.9 * total                            # (thin triangles: ~6 % of random triples are below the ratio)


@pytest.mark.parametrize("Ho,Wo", [(8, 12), (60, 90)])
def test_exact_inputs_give_the_pose(ref, Ho, Wo):
    """No coordinate or depth noise, 30 % outliers, thr 10 cm, maxDist 100 cm: translation < 1e-3 m, rotation < 1e-3 degrees
    (what is left is the float32 rounding of coordinates of several hundred metres)."""
    for seed in (11, 12, 13):
        sc = rc.rgbd_scene(seed, Ho, Wo, noise=0.0, outlier_ratio=0.3)
        res = ref.forward(sc["coords"], N_HYP, 10.0, 100.0, 100.0, cam=sc["cam"], image=seed)
        est = rc.pose_from_w2c(res["dbg"][4:13].reshape(3, 3), res["dbg"][13:16])
        t_err, r_err = synth.pose_error(sc["pose"], est)
        print("exact %dx%d seed %d: %.3g m %.3g deg, %d inliers" % (Ho, Wo, seed, t_err, r_err, res["dbg"][3]))
        assert t_err < 1e-3 and r_err < 1e-3, (seed, t_err, r_err)
        t32, r32 = synth.pose_error(sc["pose"], res["pose"].astype(np.float64))
        assert t32 < 1e-3 and r32 < 1e-3                    # the float32 pose the caller gets


def test_noisy_inputs_stay_within_twice_the_numpy_implementation(ref):
    """60 x 90, 0.5 m coordinate noise, 1 % depth noise, 20 % holes, 30 % outliers, thr 300 cm, maxDist 3000 cm, 8 seeds: the
    restatement's errors against ground truth are within twice the largest error of tests/indep_dsac_rgbd.py (own sampler)
    on the same scenes.  Measured: restatement 0.13 - 0.63 m, 0.020 - 0.105 deg; numpy 0.06 - 0.91 m, 0.011 - 0.151 deg
    (DESIGN.md); the two differ in which hypothesis wins before the refinement."""
    ours, theirs = [], []
    for seed in range(21, 29):
        sc = rc.rgbd_scene(seed, 60, 90, noise=0.5, outlier_ratio=0.3, depth_noise=0.01, holes=0.2)
        res = ref.forward(sc["coords"], N_HYP, 300.0, 100.0, 3000.0, cam=sc["cam"], image=seed)
        assert res["dbg"][1] == 60 * 90 - round(0.2 * 60 * 90)
        ours.append(synth.pose_error(sc["pose"], rc.pose_from_w2c(res["dbg"][4:13].reshape(3, 3), res["dbg"][13:16])))
        got = indep.solve(sc["coords"], sc["cam"], N_HYP, 300.0, 100.0, 3000.0, seed=seed)
        theirs.append(synth.pose_error(sc["pose"], got["pose"]))
    ours, theirs = np.array(ours), np.array(theirs)
    print("restatement t %s r %s" % (np.round(ours[:, 0], 4), np.round(ours[:, 1], 5)))
    print("numpy       t %s r %s" % (np.round(theirs[:, 0], 4), np.round(theirs[:, 1], 5)))
    assert ours[:, 0].max() <= 2.0 * theirs[:, 0].max(), (ours[:, 0], theirs[:, 0])
    assert ours[:, 1].max() <= 2.0 * theirs[:, 1].max(), (ours[:, 1], theirs[:, 1])


def test_depth_form_equals_camera_form(ref):
    """the depth map through the header's formula == the camera tensor built by the same formula in numpy float32, bit for bit;
    an odd width keeps its centre column (x_cam == 0), which the reference's channel-0 test would drop"""
    sc = rc.rgbd_scene(3, 33, 17, noise=0.1, outlier_ratio=0.3, holes=0.2)
    a = ref.forward(sc["coords"], 16, 50.0, 100.0, 1000.0, cam=sc["cam"], image=5, rounds=True)
    b = ref.forward(sc["coords"], 16, 50.0, 100.0, 1000.0, depth=sc["depth"], focal=sc["focal"], ppx=sc["ppx"], ppy=sc["ppy"],
                    sub=sc["sub"], image=5)
    for k in ("pose", "cells", "tries", "scores", "dbg"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["dbg"][1] == (sc["depth"] != 0).sum()
    centre = sc["cam"][0, :, 8]
    assert (centre == 0).all() and (sc["depth"][:, 8] != 0).any()
    for y, x in ((0, 0), (32, 16), (7, 8)):
        assert np.array_equal(ref.cam_from_depth(sc["depth"][y, x], y, x, sc["focal"], sc["ppx"], sc["ppy"], sc["sub"]),
                              sc["cam"][:, y, x])


def test_edge_cases_of_the_restatement(ref):
    sc = rc.rgbd_scene(4, 8, 12, noise=0.0, outlier_ratio=0.3)
    none = ref.forward(sc["coords"], 8, 10.0, 100.0, 100.0, depth=np.zeros((8, 12), np.float32))
    assert np.array_equal(none["pose"], np.eye(4, dtype=np.float32)) and none["dbg"][1] == 0 and (none["tries"] == 0).all()
    assert np.isfinite(none["scores"]).all() and (none["cells"] == -1).all()
    two = np.zeros((8, 12), np.float32)
    two[2, 3], two[6, 9] = sc["depth"][2, 3], sc["depth"][6, 9]
    res = ref.forward(sc["coords"], 8, 10.0, 100.0, 100.0, depth=two)
    assert res["dbg"][1] == 2 and np.isfinite(res["pose"]).all() and np.isfinite(res["scores"]).all()
    assert set(np.unique(res["cells"])) <= {2 * 12 + 3, 6 * 12 + 9}
    hard = rc.rgbd_scene(6, 8, 12, noise=0.0, outlier_ratio=0.9)
    res = ref.forward(hard["coords"], 16, 10.0, 100.0, 100.0, cam=hard["cam"], max_tries=2)
    assert (res["tries"] == -2).any() and np.isfinite(res["scores"]).all() and np.isfinite(res["pose"]).all()


def test_camera_coordinates_matches_the_kernel_formula():
    """dsacstar.camera_coordinates (torch, here on the CPU) == the formula of the shared header, bit for bit, per-image focals"""
    torch = pytest.importorskip("torch")
    import dsacstar
    sc = rc.rgbd_scene(2, 33, 17, holes=0.2)
    depth = torch.from_numpy(np.stack([sc["depth"], sc["depth"] * np.float32(1.25)]))
    focals = [480.0, 517.25]
    got = dsacstar.camera_coordinates(depth, focals, 33 * 8, 17 * 8, 8).numpy()
    assert got.shape == (2, 3, 33, 17) and got.dtype == np.float32
    for b in range(2):
        want = rc.camera_from_depth(depth[b].numpy(), focals[b], 17 * 8 / 2.0, 33 * 8 / 2.0, 8)
        assert got[b].tobytes() == want.tobytes()
    one = dsacstar.camera_coordinates(depth, 480.0, 33 * 8, 17 * 8, 8).numpy()
    assert one[0].tobytes() == got[0].tobytes()
    with pytest.raises(RuntimeError):
        dsacstar.camera_coordinates(depth.double(), 480.0, 264, 136, 8)


def test_sanitizer_run_of_the_restatement(tmp_path):
    """tests/dsac_rgbd_ref.c with its own main() under AddressSanitizer + UBSan on an 8x12 and a 60x90 scene: exit 0, no report"""
    prog = dsac_rgbd_ref.build_program(tmp_path, sanitize=True)
    for Ho, Wo, thr, max_dist, kw in ((8, 12, 10.0, 100.0, dict(noise=0.0)),
                                      (60, 90, 300.0, 3000.0, dict(noise=0.5, depth_noise=0.01, holes=0.2))):
        sc = rc.rgbd_scene(31, Ho, Wo, outlier_ratio=0.3, **kw)
        path = tmp_path / ("scene_%dx%d.bin" % (Ho, Wo))
        with open(path, "wb") as f:
            f.write(np.ascontiguousarray(sc["coords"]).tobytes())
            f.write(np.ascontiguousarray(sc["cam"]).tobytes())
        r = subprocess.run([prog, str(path), str(Ho), str(Wo), "32", str(thr), str(max_dist)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        assert "camera form: status 0" in r.stdout and "depth form: status 0" in r.stdout


# --------------------------------------------------------------------------------- argument validation, no GPU

def _abi(coords=8, cam=8, depth=None, B=1, Ho=8, Wo=12, out=8, n_hyp=8, sub=8, max_tries=10):
    from crossloc_amd import _lib
    vp = ctypes.c_void_p
    return _lib.lib().xl_dsac_forward_rgbd_batch(vp(coords), 288, 96, 12, 1, vp(cam), 288, 96, 12, 1, vp(depth), 96, 12, 1,
                                                 B, Ho, Wo, vp(out), n_hyp, 10.0, 100.0, 100.0, 480.0, 48.0, 32.0, sub, None,
                                                 1305, 0, 1, max_tries, None, None, None, None, None)


def test_abi_rejects_bad_arguments_before_any_hip_call():
    """the pointers are never dereferenced: every case returns before the first HIP call"""
    ARG, GRID = -1, -2
    assert _abi(cam=None, depth=None) == ARG                   # neither camera coordinates nor depth
    assert _abi(cam=8, depth=8) == ARG                         # both
    assert _abi(coords=None) == ARG and _abi(out=None) == ARG
    for kw in (dict(B=0), dict(Ho=0), dict(Wo=-3), dict(n_hyp=0), dict(max_tries=0), dict(max_tries=2 ** 31 - 63), dict(max_tries=2 ** 32 - 1),
               dict(cam=None, depth=8, sub=0)):
        assert _abi(**kw) == ARG, kw
    assert _abi(Ho=64, Wo=97) == GRID                          # 6208 cells > XL_DSAC_RGBD_MAX_CELLS
    assert _abi(Ho=40000, Wo=60000) == GRID                    # the product does not fit an int
    assert _abi(cam=None, depth=8, Ho=100, Wo=100) == GRID


def test_python_front_end_rejects_bad_arguments():
    torch = pytest.importorskip("torch")
    import dsacstar
    co, cam, depth = torch.zeros(1, 3, 8, 12), torch.zeros(1, 3, 8, 12), torch.zeros(1, 8, 12)
    out = torch.zeros(1, 4, 4)
    with pytest.raises(RuntimeError):
        dsacstar.forward_rgbd_batch(co, None, out, 8, 10.0, 100.0, 100.0)                       # neither
    with pytest.raises(RuntimeError):
        dsacstar.forward_rgbd_batch(co, cam, out, 8, 10.0, 100.0, 100.0, depth=depth)           # both
    with pytest.raises(RuntimeError):
        dsacstar.forward_rgbd_batch(co, cam[:, :2], out, 8, 10.0, 100.0, 100.0)                 # shape
    with pytest.raises(RuntimeError):
        dsacstar.forward_rgbd_batch(co, None, out, 8, 10.0, 100.0, 100.0, depth=depth)          # depth without intrinsics
    with pytest.raises(RuntimeError):
        dsacstar.forward_rgbd_batch(co, cam.double(), out, 8, 10.0, 100.0, 100.0)               # dtype
    with pytest.raises(RuntimeError):
        dsacstar.forward_rgbd_batch(co, cam, out, 8, 10.0, 100.0, 100.0)                        # CPU tensors: no fallback
    with pytest.raises(RuntimeError, match="6400 cells exceed the limit of 6144"):
        dsacstar.forward_rgbd_batch(torch.zeros(1, 3, 80, 80), torch.zeros(1, 3, 80, 80), out, 8, 10.0, 100.0, 100.0)
    with pytest.raises(NotImplementedError):
        dsacstar.forward_rgbd()
