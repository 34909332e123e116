"""Monte-Carlo calibration of the pose-quality covariance at a chosen noise level and outlier ratio, on the CPU: the
experiment of tests/test_pose_quality_cpu.py::test_monte_carlo_calibration (tests/pose_quality_cases.calibration_run: the
oracle's solver + the serial restatement of the pass) with its parameters open.  Not a test; no pass/fail threshold.

    python tools/pose_quality_calibration.py                             # 0.5 px, no outliers: what the test asserts
    python tools/pose_quality_calibration.py --outliers 0.3              # chance inliers among gross outliers
    python tools/pose_quality_calibration.py --sigma 2.0
"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_quality_cases as qc                                 # noqa: E402
import pose_quality_ref                                         # noqa: E402
from oracle import dsac_oracle                                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sigma", type=float, default=0.5, help="pixel noise per axis")
    ap.add_argument("--outliers", type=float, default=0.0, help="fraction of cells replaced by uniform gross outliers")
    ap.add_argument("--draws", type=int, default=200)
    ap.add_argument("--seeds", type=int, nargs="+", default=[3, 11])
    opt = ap.parse_args()
    dsac_oracle.build()
    with tempfile.TemporaryDirectory() as tmp:
        qref = pose_quality_ref.load(tmp)
        for seed in opt.seeds:
            m = qc.calibration_run(qref, dsac_oracle, seed, sigma=opt.sigma, outlier_ratio=opt.outliers, draws=opt.draws)
            print("seed %d  sigma %.2f px  outliers %.0f %%  draws %d: sigma_px %.4f  inliers %.0f  variance ratios %s  "
                  "mean Mahalanobis^2 %.3f" % (seed, opt.sigma, 100 * opt.outliers, opt.draws, m["sigma_px"].mean(),
                                               m["n_inliers"].mean(), np.array2string(m["ratio"], precision=3),
                                               np.nanmean(m["mahalanobis2"])))


if __name__ == "__main__":
    main()
