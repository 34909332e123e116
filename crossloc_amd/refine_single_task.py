"""Coord-task evaluation WITH the pose refinement behind the solver: crossloc_amd.test_single_task, run unchanged, with
dsacstar.refine_pose_batch enqueued behind the solver of every batch.

    python -m crossloc_amd.refine_single_task --synthetic 256 --refine sigma --sigma_range 0.1 3 [--sigma_floor_px 1.0]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m crossloc_amd.refine_single_task ...

There is ONE evaluation loop, test_single_task.main(); this module does not restate it (as crossloc_amd.pose_quality_single_task
does not).  main() reaches the harness through the names `evaluation` and `synth`; for the duration of the call they are bound
to views of the two modules in which
  synth.make_scene           with `--sigma_range LO HI` returns a heteroscedastic frame (synth.make_hetero_scene: per-cell
                             coordinate noise log-uniform in [LO, HI] metres in place of `--noise`) and keeps its sigma map,
  evaluation.localize_batch  asks for the refinement and, where the solver consumes the synthetic maps (the solver inputs
                             `synthetic` / `planted`), hands it the kept sigma maps of the batch; main() gets the two values it
                             expects, the first of them the REFINED poses.
Every option of test_single_task is accepted and means the same.  Added:
  --refine {none,inliers,sigma}   default `none`: the report is character for character test_single_task's.  `inliers`: an
                                  unweighted re-fit over the inliers; `sigma`: weighted by the per-cell standard deviation -
                                  the frames' sigma map with --sigma_range, otherwise the network's uncertainty channel
  --sigma_range LO HI             heteroscedastic synthetic frames
  --sigma_floor_px S0             pixel floor of the weights (default 1.0)
"""
import argparse
import sys

import numpy as np
import torch

from . import evaluation, synth, test_single_task


class _SynthWithSigma:
    """crossloc_amd.synth as test_single_task.main() sees it during a run with --sigma_range (see the module docstring)."""

    def __init__(self, sigma_range):
        self.sigma_range = sigma_range
        self.kept = []                                  # sigma maps of the frames made since the last solver call

    def __getattr__(self, name):
        return getattr(synth, name)

    def make_scene(self, seed, noise=0.5, outlier_ratio=0.3, **kw):
        if self.sigma_range is None:
            return synth.make_scene(seed, noise=noise, outlier_ratio=outlier_ratio, **kw)
        sc = synth.make_hetero_scene(seed, sigma_range=self.sigma_range, outlier_ratio=outlier_ratio, **kw)
        self.kept.append(sc["sigma"])
        return sc


class _EvaluationWithRefine:
    """crossloc_amd.evaluation as test_single_task.main() sees it during a refinement run (see the module docstring)."""

    def __init__(self, refine, sigma_floor_px, scenes):
        self.refine, self.sigma_floor_px, self.scenes = refine, sigma_floor_px, scenes

    def __getattr__(self, name):
        return getattr(evaluation, name)

    def localize_batch(self, network, images, *args, **kwargs):
        kept, self.scenes.kept = self.scenes.kept, []
        if self.refine == 'none':
            return evaluation.localize_batch(network, images, *args, **kwargs)
        sigma = None
        if kept and (kwargs.get("scene_coords") is not None or kwargs.get("plant") is not None):
            sigma = torch.from_numpy(np.stack(kept)).to(images.device)
        out = evaluation.localize_batch(network, images, *args, refine=self.refine, sigma=sigma,
                                        sigma_floor_px=self.sigma_floor_px, **kwargs)
        return out[0], out[1]


def main():
    own = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    own.add_argument('--refine', choices=['none', 'inliers', 'sigma'], default='none')
    own.add_argument('--sigma_range', type=float, nargs=2, default=None, metavar=('LO', 'HI'))
    own.add_argument('--sigma_floor_px', type=float, default=1.0)
    opt, rest = own.parse_known_args()                  # test_single_task's parser sees everything else
    scenes = _SynthWithSigma(tuple(opt.sigma_range) if opt.sigma_range is not None else None)
    saved = sys.argv, test_single_task.evaluation, test_single_task.synth
    sys.argv = [sys.argv[0]] + rest
    test_single_task.evaluation = _EvaluationWithRefine(opt.refine, opt.sigma_floor_px, scenes)
    test_single_task.synth = scenes
    try:
        test_single_task.main()
    finally:
        sys.argv, test_single_task.evaluation, test_single_task.synth = saved


if __name__ == '__main__':
    main()
