"""Coord-task evaluation WITH per-frame pose quality: crossloc_amd.test_single_task, run unchanged, with the pose-quality pass
enqueued behind the solver of every batch.

    python -m crossloc_amd.pose_quality_single_task --synthetic 256 --hypotheses 256 [--quality_out rows.npy]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m crossloc_amd.pose_quality_single_task ...

There is ONE evaluation loop, test_single_task.main(); this module does not restate it.  main() reaches the harness through the
name `evaluation`; for the duration of the call that name is bound to a view of crossloc_amd.evaluation in which
  localize_batch        asks for the quality rows too and keeps them (main() gets the two values it expects),
  gather_errors         gathers the kept rows with the same sharding right after the pose errors (every rank calls it once),
  scene_coords_printout prints the usual report, then (it runs on rank 0 only) the selective-accuracy table, and saves the
                        rows [K,64] float64 in dataset order to --quality_out.
Every option of test_single_task is accepted and means the same; `--quality_out FILE.npy` is added and `--pose_quality` is
accepted (it is what this entry point does).  Without this entry point an evaluation is exactly what it was.
"""
import argparse
import sys

import numpy as np
import torch

from . import evaluation, test_single_task
from .dsacstar import QUALITY_DOUBLES, QUALITY_FIELDS


class _EvaluationWithQuality:
    """crossloc_amd.evaluation as test_single_task.main() sees it during a pose-quality run (see the module docstring)."""

    def __init__(self, quality_out, testing_log):
        self.quality_out, self.testing_log = quality_out, testing_log
        self.batches, self.rows = [], None

    def __getattr__(self, name):
        return getattr(evaluation, name)

    def localize_batch(self, *args, **kwargs):
        poses, pred, rows = evaluation.localize_batch(*args, quality=True, **kwargs)
        self.batches.append(rows)
        return poses, pred

    def gather_errors(self, local_vals, num_images, rank, world_size, group=None):
        out = evaluation.gather_errors(local_vals, num_images, rank, world_size, group)
        local = torch.cat(self.batches, 0) if self.batches else \
            torch.empty((0, QUALITY_DOUBLES), dtype=torch.float64, device=local_vals.device)
        self.rows = evaluation.gather_errors(local, num_images, rank, world_size, group).cpu().numpy()
        return out

    def scene_coords_printout(self, t_err_ls, r_err_ls, *args, **kwargs):
        stats = evaluation.scene_coords_printout(t_err_ls, r_err_ls, *args, **kwargs)
        table = evaluation.selective_accuracy_table(t_err_ls, r_err_ls, self.rows[:, QUALITY_FIELDS["sigma_pos_m"]])
        print(table)
        if self.testing_log:
            with open(self.testing_log, 'a') as f:
                f.write(table + '\n')
        if self.quality_out:
            np.save(self.quality_out, self.rows)
        return stats


def main():
    own = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    own.add_argument('--pose_quality', action='store_true')
    own.add_argument('--quality_out', type=str, default=None)
    own.add_argument('--testing_log', type=str, default=None)
    opt, _ = own.parse_known_args()
    # test_single_task's parser sees everything but the two options it does not have
    rest, skip = [], False
    for a in sys.argv[1:]:
        if skip:
            skip = False
        elif a == '--quality_out':
            skip = True
        elif a != '--pose_quality' and not a.startswith('--quality_out='):
            rest.append(a)
    saved = sys.argv, test_single_task.evaluation
    sys.argv = [sys.argv[0]] + rest
    test_single_task.evaluation = _EvaluationWithQuality(opt.quality_out, opt.testing_log)
    try:
        test_single_task.main()
    finally:
        sys.argv, test_single_task.evaluation = saved


if __name__ == '__main__':
    main()
