"""Inputs shared by tests/test_rgbd_refine_cpu.py and tests/test_rgbd_refine_gpu.py — TEST INFRASTRUCTURE ONLY: solver
parameters, heteroscedastic RGB-D frames, start poses and the hand-made status scenes."""
import numpy as np

import indep_rgbd_refine as ind
import rgbd_quality_cases as qc
from pose_quality_cases import same_bits, w2c                              # noqa: F401  (shared helpers)
from crossloc_amd import synth

SUB = 8
THR, MAX_DIST = 300.0, 3000.0              # centimetres: the gate of the 1 % depth-noise frames
S0 = 0.01                                  # metres
SIGMA_RANGE = (0.02, 0.5)


def scene(seed, Ho=24, Wo=36, depth_rel=0.01, holes=0.0, outlier_ratio=0.3, sigma_range=SIGMA_RANGE):
    return synth.make_hetero_rgbd_scene(seed, sigma_range=sigma_range, depth_rel=depth_rel, holes=holes,
                                        outlier_ratio=outlier_ratio, Ho=Ho, Wo=Wo)


def perturbed(pose_c2w, seed, max_m=0.05, max_deg=0.01):
    """cam->world 4x4 float64 within max_m metres / max_deg degrees of `pose_c2w` (uniform direction, uniform magnitude)"""
    rng = np.random.default_rng(7100 + seed)
    ax = rng.normal(size=3)
    ax *= np.deg2rad(rng.uniform(0.0, max_deg)) / np.linalg.norm(ax)
    dc = rng.normal(size=3)
    dc *= rng.uniform(0.0, max_m) / np.linalg.norm(dc)
    T = np.array(pose_c2w, np.float64)
    T[:3, :3] = ind.rodrigues(ax) @ T[:3, :3]
    T[:3, 3] += dc
    return T


def indep_fit(sc, start_c2w, sigma=None, depth_sigma=None, depth_rel=0.0, thr=THR, max_dist=MAX_DIST, s0=S0):
    """The independent implementation on a scene from a cam->world start -> its result dict plus `pose` (cam->world 4x4)"""
    R, t = w2c(start_c2w)
    out = ind.refine(sc["coords"], sc["cam"], R, t, thr, max_dist, sigma, depth_sigma, depth_rel, s0)
    out["pose"] = ind.c2w(out["R"], out["t"])
    return out


def errors(gt_pose, poses):
    """(translation errors [m], rotation errors [deg]) of cam->world poses against one ground truth each"""
    e = np.array([synth.pose_error(g, p) for g, p in zip(gt_pose, poses)])
    return e[:, 0], e[:, 1]


def status_cases(Ho=12, Wo=16):
    """[(name, coords, cam, pose f32 cam->world, expected status, inliers or None, valid or None)] at thr 10 cm, maxDist 100 cm:
    the exact scenes of the RGB-D quality row (all depth zero: status 1; two inliers: 1; one point / collinear: 2; a NaN pose
    entry: 3; three spread inliers: 0) and `one_grid_row`: twelve inliers in the cells of grid row 5, their points on one line."""
    cases = list(qc.status_cases(Ho, Wo))
    co, cam = qc._empty(Ho, Wo)
    qc._place(co, cam, [(5, x) for x in range(12)], [qc.X0 + k * qc.LINE for k in range(12)])
    cases.append(("one_grid_row", co, cam, np.eye(4, dtype=np.float32), 2, 12, 12))
    return cases


def expected_nan(status):
    expect = np.zeros(64, bool)
    if status == 3:
        expect[:] = True
        expect[[0, 6]] = False
    elif status != 0:
        expect[7:10] = True
        expect[31:58] = True
    return expect


def assert_status_row(name, row, out, w2c_, pose, status, n_inl, n_valid, mask=None):
    """the row, pose and w2c of a status case (restatement or device)"""
    assert row[6] == status, (name, row[6])
    assert np.array_equal(np.isnan(row), expected_nan(status)), name
    if status != 0:
        assert np.array_equal(np.asarray(out, np.float32).view(np.int32).reshape(-1), np.asarray(pose, np.float32).view(np.int32).reshape(-1)), name
        assert mask is None or not mask.any()
    if status == 3:
        assert np.isnan(w2c_).all()
    elif status != 0:
        assert row[1] == row[2] == n_inl and row[3] == row[4] and row[58] == 0 and (row[60:63] == 0).all() and row[63] == n_valid, name
    elif n_inl is not None:
        assert row[1] == n_inl and row[63] == n_valid and np.isfinite(row[:31]).all(), name


def sigma_status_maps(Ho=12, Wo=16):
    """(sigma, sigma_z, unusable cells): sigma with one NaN, one +inf and one negative cell, sigma_z with one -inf, one tiny negative
    and one NaN cell that coincides with sigma's NaN: 5 distinct unusable cells; the rest 0.05 m / 0.5 m"""
    s = np.full((Ho, Wo), 0.05, np.float32)
    z = np.full((Ho, Wo), 0.5, np.float32)
    s[1, 3], s[4, 7], s[7, 9] = np.nan, np.inf, -1.0
    z[5, 0], z[10, 15], z[1, 3] = -np.inf, -1e-30, np.nan
    return s, z, 5
