"""Inputs shared by tests/test_pose_refine_cpu.py and tests/test_pose_refine_gpu.py: solver parameters, heteroscedastic frames,
start poses and the accuracy set of 48 frames with the independent implementation's fits (computed once per process)."""
import functools

import numpy as np

import indep_pose_refine as ind
from pose_quality_cases import same_bits, status_cases, w2c                # noqa: F401  (shared helpers)
from crossloc_amd import synth

THR, MAX_REPROJ, SUB = 10.0, 100.0, 8
ACC_SEEDS = tuple(range(100, 148))                                         # the 48 frames of the accuracy checks
ACC_GRID = (24, 36)


def hetero(seed, Ho=24, Wo=36, sigma_range=(0.1, 3.0), outlier_ratio=0.3):
    return synth.make_hetero_scene(seed, sigma_range=sigma_range, outlier_ratio=outlier_ratio, Ho=Ho, Wo=Wo)


def solver_args(sc, thr=THR, max_reproj=MAX_REPROJ):
    """(thr, focal, ppx, ppy, max_reproj, sub) of a synth scene: the positional tail of refine_pose_batch and of the restatement"""
    return (thr, sc["focal"], sc["ppx"], sc["ppy"], max_reproj, SUB)


def perturbed(pose_c2w, seed, max_m=0.5, max_deg=0.1):
    """cam->world 4x4 float64 within max_m metres / max_deg degrees of `pose_c2w` (uniform direction, uniform magnitude)"""
    rng = np.random.default_rng(7000 + seed)
    ax = rng.normal(size=3)
    ax *= np.deg2rad(rng.uniform(0.0, max_deg)) / np.linalg.norm(ax)
    dc = rng.normal(size=3)
    dc *= rng.uniform(0.0, max_m) / np.linalg.norm(dc)
    T = np.array(pose_c2w, np.float64)
    T[:3, :3] = ind.rodrigues(ax) @ T[:3, :3]
    T[:3, 3] += dc
    return T


def indep_fit(sc, sigma, start_c2w, thr=THR, s0=1.0):
    """The independent implementation on a scene from a cam->world start -> its result dict plus `pose` (cam->world 4x4)"""
    R, t = w2c(start_c2w)
    out = ind.refine(sc["coords"], sigma, R, t, thr, sc["focal"], sc["ppx"], sc["ppy"], SUB, s0=s0)
    out["pose"] = ind.c2w(out["R"], out["t"])
    return out


def errors(gt_pose, poses):
    """(translation errors [m], rotation errors [deg]) of cam->world poses against one ground truth each"""
    e = np.array([synth.pose_error(g, p) for g, p in zip(gt_pose, poses)])
    return e[:, 0], e[:, 1]


@functools.lru_cache(maxsize=None)
def accuracy_set():
    """The 48 heteroscedastic 24x36 frames (sigma 0.1 - 3 m, 30 % outliers) with, per frame, the independent implementation's
    UNWEIGHTED fit from a start within 0.5 m / 0.1 deg of ground truth (`start`: the pose both forms are then run from) and
    its sigma-weighted fit from there.  -> list of dict(sc, start [4,4] f64, unweighted, weighted)"""
    frames = []
    for seed in ACC_SEEDS:
        sc = hetero(seed, *ACC_GRID)
        un = indep_fit(sc, None, perturbed(sc["pose"], seed))
        frames.append(dict(sc=sc, start=un["pose"], unweighted=un, weighted=indep_fit(sc, sc["sigma"], un["pose"])))
    return frames


def sigma_status_maps(Ho=12, Wo=16):
    """A sigma map with one NaN, one +inf, one -inf and two negative cells (5 unusable), the rest 0.5 m"""
    s = np.full((Ho, Wo), 0.5, np.float32)
    s[1, 3], s[4, 7], s[5, 0], s[7, 9], s[10, 15] = np.nan, np.inf, -np.inf, -1.0, -1e-30
    return s, 5
