"""Recorder of tests/golden/rgbd_ref_pin.npz: the bits the three RGB-D restatements (tests/dsac_rgbd_ref.c,
tests/dsac_rgbd_bwd_ref.c, tests/rgbd_quality_ref.c, built by their loaders' load()) produced at commit 09d9aa0 "Add RGB-D
pose quality", BEFORE the block sum, the pose helpers, the input record and the refinement model of the family were each
written once.  Kernels and restatements compile the same xl_dsac_rgbd*_math.h, so a slip that moves both at once is
invisible to the GPU == restatement tests; this fixture pins the restatements, and through those tests the kernels, to the
earlier arithmetic.  The restatements use only + - * / sqrt floor without contraction, so the recorded bits depend neither on
the compiler nor on its optimisation level (recorded at -O2, compared with a -O0 build when recording: identical).

    python tests/golden/make_rgbd_ref_pin.py          # rewrites the fixture from the restatements of the checked-out tree

Re-record only when the arithmetic is changed on purpose.  tests/test_rgbd_ref_pin.py calls compute() and compares.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)

import dsac_rgbd_bwd_ref                        # noqa: E402
import dsac_rgbd_cases as rc                     # noqa: E402
import dsac_rgbd_ref                             # noqa: E402
import rgbd_quality_cases as qc                  # noqa: E402
import rgbd_quality_ref                          # noqa: E402
from crossloc_amd import synth                   # noqa: E402

PATH = os.path.join(HERE, "rgbd_ref_pin.npz")
N_HYP, THR, ALPHA, MAX_DIST = 16, 10.0, 100.0, 100.0
# 8 x 12: fewer cells than one workgroup; 17 x 23 = 391 cells: a partial last wave and a partial second chunk
GRIDS = {"8x12": (8, 12, 61, dict()),
         "17x23": (17, 23, 62, dict(holes=0.2, outlier_ratio=0.3, noise=0.02, depth_noise=0.002))}
FORMS = ("cam", "depth")
FORWARD = ["pose", "cells", "tries", "scores", "dbg", "hyp_poses", "round_counts", "round_poses"]
BACKWARD = ["loss", "rec", "grad"]
QUALITY = ["row", "sums_w2c"]
STATUS_CASE = "three_spread_inliers"
SUMS_KEYS = ["n_valid", "n", "sum_m", "soft", "sum_err", "sum_err2", "sse", "C", "grad_w", "grad_t", "c", "pivot_ratio"]


def moved_pose(pose):
    """as in tests/test_dsac_rgbd_bwd_cpu.py: turned by (0.01, -0.015, 0.02) rad and shifted by (0.3, -0.2, 0.4) m"""
    out = pose.copy()
    out[:3, :3] = out[:3, :3] @ synth._rot_xyz(0.01, -0.015, 0.02)
    out[:3, 3] += [0.3, -0.2, 0.4]
    return out


def _flat_sums(s):
    return np.concatenate([np.asarray(s[k], np.float64).reshape(-1) for k in SUMS_KEYS])


def compute(tmpdir):
    """Everything the fixture holds, computed with the restatements of this tree (compiled into `tmpdir`)."""
    fwd, bwd, qual = dsac_rgbd_ref.load(tmpdir), dsac_rgbd_bwd_ref.load(tmpdir), rgbd_quality_ref.load(tmpdir)
    out = {}
    for grid, (Ho, Wo, seed, kw) in GRIDS.items():
        sc = rc.rgbd_scene(seed, Ho, Wo, **kw)
        out[grid + "_in_coords"], out[grid + "_in_depth"] = sc["coords"], sc["depth"]
        for form in FORMS:
            src = dict(cam=sc["cam"]) if form == "cam" else dict(depth=sc["depth"], focal=sc["focal"], ppx=sc["ppx"], ppy=sc["ppy"],
                                                                 sub=sc["sub"])
            tag = "%s_%s_" % (grid, form)
            f = fwd.forward(sc["coords"], N_HYP, THR, ALPHA, MAX_DIST, image=seed, rounds=True, **src)
            for k in FORWARD:
                out[tag + "f_" + k] = f[k]
            b = bwd.backward(sc["coords"], moved_pose(sc["pose"]), N_HYP, THR, ALPHA, MAX_DIST, image=seed, **src)
            out[tag + "b_loss"], out[tag + "b_rec"], out[tag + "b_grad"] = np.float64(b["loss"]), b["rec"], b["grad"]
            R, t = f["dbg"][4:13].reshape(3, 3), f["dbg"][13:16]
            out[tag + "q_row"] = qual.row(sc["coords"], rc.pose_from_w2c(R, t), THR, ALPHA, MAX_DIST, **src)
            out[tag + "q_sums_w2c"] = _flat_sums(qual.sums_w2c(sc["coords"], R, t, THR, ALPHA, MAX_DIST, **src))
    name, co, cam, pose, status, _, _ = [c for c in qc.status_cases() if c[0] == STATUS_CASE][0]
    out["status_q_row"] = qual.row(co, pose, qc.THR, qc.ALPHA, qc.MAX_DIST, cam=cam)
    assert out["status_q_row"][6] == status
    return out


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        np.savez_compressed(PATH, **compute(tmp))
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))
