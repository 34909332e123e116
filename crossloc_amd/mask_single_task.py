"""Coord-task evaluation WITH a per-cell validity mask on the RGB solver: crossloc_amd.test_single_task, run unchanged, with
dsacstar.forward_rgb_masked_batch in place of the plain solver of every batch.

    python -m crossloc_amd.mask_single_task --synthetic 256 --decoy 0.6 --mask truth
    python -m crossloc_amd.mask_single_task --synthetic 256 --decoy 0.6               # the same frames without the mask
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m crossloc_amd.mask_single_task ...

There is ONE evaluation loop, test_single_task.main(); this module does not restate it (as crossloc_amd.refine_single_task does
not).  main() reaches the harness through the names `evaluation` and `synth`; for the duration of the call they are bound to
views of the two modules in which
  synth.make_scene           with `--decoy FRAC` returns a decoy frame (synth.make_decoy_scene: the top FRAC of the rows hold the
                             exact view of a second camera; `--outliers` does not apply) and keeps its mask,
  evaluation.localize_batch  passes the mask of the batch on - the kept masks where the solver consumes the synthetic maps (the
                             solver inputs `synthetic` / `planted`), or `mask_max_sigma` - and hands main() the two values it
                             expects.
Every option of test_single_task is accepted and means the same.  Added:
  --decoy FRAC              synthetic decoy frames
  --mask {none,truth,sigma} default `none`: the report is character for character test_single_task's.  `truth`: the frames' own
                            mask (needs --decoy); `sigma`: cells whose predicted standard deviation is at most --mask_max_sigma
                            (needs a network with an uncertainty channel)
  --mask_max_sigma S        metres (default 1.0)
  --mask_sampler {reject,compact}  the masked solver's sampler (localize_batch's mask_sampler; needs a --mask other than `none`).
                            `compact` draws the cells of a try from the usable cells only
  --refine {none,inliers,sigma}  default `none`: the report is unchanged character for character.  Otherwise the refinement runs
                            behind the solver of every batch and the report is about the refined poses: with a --mask other than
                            `none` over the solver's mask (localize_batch's refine="masked_inliers" / "masked_sigma"), with
                            `--mask none` over every cell ("inliers" / "sigma"), so one command line compares the two.  `sigma`
                            weights by the network's uncertainty channel (the options of crossloc_amd.refine_single_task that
                            shape synthetic sigma maps are not taken here).
A frame the solver reports as dead (fewer than four usable cells) keeps the identity pose it wrote, and counts as such.
"""
import argparse
import sys

import numpy as np
import torch

from . import dsacstar, evaluation, synth, test_single_task


class _SynthWithDecoy:
    """crossloc_amd.synth as test_single_task.main() sees it during a run with --decoy (see the module docstring)."""

    def __init__(self, decoy):
        self.decoy = decoy
        self.kept = []                                  # masks of the frames made since the last solver call

    def __getattr__(self, name):
        return getattr(synth, name)

    def make_scene(self, seed, noise=0.5, outlier_ratio=0.3, **kw):
        if self.decoy is None:
            return synth.make_scene(seed, noise=noise, outlier_ratio=outlier_ratio, **kw)
        sc = synth.make_decoy_scene(seed, decoy=self.decoy, noise=noise, **kw)
        self.kept.append(sc["mask"])
        return sc


class _EvaluationWithMask:
    """crossloc_amd.evaluation as test_single_task.main() sees it during a masked run (see the module docstring)."""

    def __init__(self, mode, max_sigma, scenes, refine='none', sampler='reject'):
        self.mode, self.max_sigma, self.scenes, self.refine, self.sampler = mode, max_sigma, scenes, refine, sampler

    def __getattr__(self, name):
        return getattr(evaluation, name)

    def localize_batch(self, network, images, *args, **kwargs):
        kept, self.scenes.kept = self.scenes.kept, []
        if self.refine != 'none':                       # out[0] is then the refined poses, masked or not
            kwargs["refine"] = self.refine if self.mode == 'none' else "masked_" + self.refine
        if self.mode == 'none':
            return evaluation.localize_batch(network, images, *args, **kwargs)[:2]
        kwargs["mask_sampler"] = self.sampler
        if self.mode == 'sigma':
            out = evaluation.localize_batch(network, images, *args, mask_max_sigma=self.max_sigma, **kwargs)
        else:
            if not kept or (kwargs.get("scene_coords") is None and kwargs.get("plant") is None):
                raise RuntimeError("--mask truth needs --decoy frames that the solver consumes (--solver_input synthetic / planted)")
            mask = torch.from_numpy(np.stack(kept)).to(images.device)
            out = evaluation.localize_batch(network, images, *args, mask=mask, **kwargs)
        return out[0], out[1]


def main():
    own = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    own.add_argument('--decoy', type=float, default=None, metavar='FRAC')
    own.add_argument('--mask', choices=['none', 'truth', 'sigma'], default='none')
    own.add_argument('--mask_max_sigma', type=float, default=1.0)
    own.add_argument('--refine', choices=['none', 'inliers', 'sigma'], default='none')
    own.add_argument('--mask_sampler', choices=list(dsacstar.MASK_SAMPLERS), default='reject')
    opt, rest = own.parse_known_args()                  # test_single_task's parser sees everything else
    if opt.mask_sampler != 'reject' and opt.mask == 'none':
        own.error("--mask_sampler %s is the masked solver's: it needs a --mask other than none" % opt.mask_sampler)
    scenes = _SynthWithDecoy(opt.decoy)
    saved = sys.argv, test_single_task.evaluation, test_single_task.synth
    sys.argv = [sys.argv[0]] + rest
    test_single_task.evaluation = _EvaluationWithMask(opt.mask, opt.mask_max_sigma, scenes, opt.refine, opt.mask_sampler)
    test_single_task.synth = scenes
    try:
        test_single_task.main()
    finally:
        sys.argv, test_single_task.evaluation, test_single_task.synth = saved


if __name__ == '__main__':
    main()
