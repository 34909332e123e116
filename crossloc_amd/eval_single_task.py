"""Task switch of the reference's test_single_task.py (`--task`, :33; loop :328-413) on the MI355X path:

    python -m crossloc_amd.eval_single_task --task depth --uncertainty MLE --scene_dir DIR [--network_in model.net]
    python -m crossloc_amd.eval_single_task --task semantics --fullsize --scene_dir DIR ...
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m crossloc_amd.eval_single_task ...

`--task depth|normal|semantics --scene_dir DIR` evaluates a single-task checkpoint with the reference's metrics
(utils/evaluation.py:247-414) through the fused per-image HIP kernels of csrc/xl_metrics.hip and prints the reference's
report.  `--task coord` (default) is crossloc_amd.test_single_task itself: every other argument is handed to its main()
unchanged, so the coord path is the same code whichever module is started.  Checkpoint and section discovery
(test_single_task.py:118-256), plots and `--save_pred` are out of scope.
"""
import argparse
import os
import sys
import time

import torch

from . import evaluation, test_single_task


def _parse(argv):
    # no -h and no single-dash spellings here: what this parser does not know (`-hyps 8`, `-t 10`) must pass through whole
    p = argparse.ArgumentParser(description="CrossLoc single-task evaluation on MI355X", allow_abbrev=False, add_help=False)
    p.add_argument('--task', choices=['coord', 'depth', 'normal', 'semantics'], default='coord',       # test_single_task.py:33
                   help='depth / normal / semantics: the metrics of utils/evaluation.py:247-414 over --scene_dir')
    p.add_argument('--uncertainty', choices=['none', 'MLE'], default='none',
                   help='depth / normal: the checkpoint has a sigma channel (test_single_task.py:92)')
    p.add_argument('--tiny', action='store_true', help='depth / normal / semantics: the reduced-capacity network')
    p.add_argument('--fullsize', action='store_true', help='full-size output (required by --task semantics)')
    p.add_argument('--section_name', type=str, default='test', help='the section name written to --testing_log')
    opt, rest = p.parse_known_args(argv)
    if opt.task == 'coord':
        given = [o for o in ('--uncertainty', '--tiny', '--fullsize', '--section_name') if o in argv]
        if given:                                                # the coord network is fixed: refuse, do not ignore
            p.error("%s: only with --task depth, normal or semantics" % ', '.join(given))
        return opt, rest
    q = argparse.ArgumentParser(description="CrossLoc %s-task evaluation on MI355X" % opt.task, parents=[p])
    q.add_argument('--network_in', type=str, default=None, help='reference-format state_dict (.net)')
    q.add_argument('--batch', type=int, default=16)
    q.add_argument('--scene_dir', type=str, default=None,
                   help='CrossLoc on-disk scene section (rgb/ calibration/ and the task folder), read by crossloc_amd.dataset')
    q.add_argument('--num_mlr', type=int, default=0, help='3 = CrossLoc three-encoder network')
    q.add_argument('--testing_log', type=str, default=None)
    return q.parse_args(rest, namespace=opt), []


def evaluate_task(opt, rank, world):
    """--task depth / normal / semantics: the loop of test_single_task.py:328-413 on one on-disk section, through
    evaluation.evaluate_section (fused HIP metric rows per batch, one gather), then the reference's report."""
    from .dataset import CamLocDataset
    if not opt.scene_dir:
        raise SystemExit("--task %s needs --scene_dir" % opt.task)
    uncertainty = None if opt.uncertainty == 'none' else opt.uncertainty
    net = evaluation.config_network(opt.task, opt.tiny, False, uncertainty, opt.fullsize, opt.network_in, opt.num_mlr)
    ds = CamLocDataset(opt.scene_dir, mode=1, sparse=True, coord=False, depth=opt.task == 'depth',
                       normal=opt.task == 'normal', semantics=opt.task == 'semantics', augment=False,
                       raw_image=True)                                                  # utils/evaluation.py:64-72
    t0 = time.time()
    rows, metrics = evaluation.evaluate_section(net, ds, opt.task, -1, opt.batch, rank, world)
    elapsed = time.time() - t0
    if rank == 0:
        print("Evaluated %d frames on %d GPU(s) in %.2f s (%.1f images/s incl. loading)" % (
            len(ds), world, elapsed, len(ds) / max(elapsed, 1e-9)))
        if opt.task == 'depth':
            evaluation.depth_printout(metrics[0], metrics[1], opt.testing_log, opt.section_name)
        elif opt.task == 'normal':
            evaluation.normal_printout(metrics, opt.testing_log, opt.section_name)
        else:
            evaluation.semantic_printout([metrics[0]], [metrics[1]], [metrics[2]], opt.testing_log, opt.section_name)


def main():
    opt, rest = _parse(sys.argv[1:])
    if opt.task == 'coord':
        sys.argv = [sys.argv[0]] + rest
        return test_single_task.main()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)
    test_single_task.set_random_seed(2021)                                      # test_single_task.py:265
    evaluate_task(opt, rank, world)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
