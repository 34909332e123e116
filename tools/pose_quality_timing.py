"""Times the pose-quality pass (csrc/xl_dsac_quality.hip through dsacstar.pose_quality_batch) behind the solver, with HIP events
on warm clocks.  Not a test and not part of bench.py; there is no pass/fail threshold.

  95 frames x 256 hypotheses on 60 x 90 (the bench batch) and 1 frame: dsacstar.forward_rgb_batch alone, and followed by
  pose_quality_batch on the same stream at the pose it wrote.

Both sides run alternately in the same process (rounds of `--iters` calls each) after `--warmup` calls; the figure is the median
over rounds of the per-call time, the cost of the pass the difference of the two medians.  The rows are compared with a
separate call before anything is timed.

    python tools/pose_quality_timing.py [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dsacstar                                                 # noqa: E402
from crossloc_amd import synth                                  # noqa: E402

ARGS = (10.0, synth.FOCAL, 360.0, 240.0, 100.0, 100.0, 8)       # threshold, focal, ppx, ppy, alpha, max reprojection, subsampling


def time_pair(a_fn, b_fn, warmup, iters, rounds):
    """median per-call milliseconds of (a_fn, b_fn) and their spreads, alternating rounds; a round ends in an event synchronise"""
    for _ in range(warmup):
        a_fn(); b_fn()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(rounds):
        for k, fn in enumerate((a_fn, b_fn)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / iters)
    return [float(np.median(v)) for v in out], [float(np.max(v) - np.min(v)) for v in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--hypotheses", type=int, default=256)
    ap.add_argument("--json", type=str, default=None)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_quality_timing needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")

    # warm clocks: a second of streaming work before the first timed window
    x = torch.rand(64 << 20, device=dev)
    for _ in range(200):
        x.mul_(1.0000001)
    torch.cuda.synchronize()
    del x

    results = []
    for B in (95, 1):
        coords, _, _ = synth.make_batch(2021, B, noise=0.5, outlier_ratio=0.3)
        co = torch.from_numpy(coords).to(dev)
        poses = torch.zeros((B, 4, 4), dtype=torch.float32, device=dev)

        def solver():
            dsacstar.forward_rgb_batch(co, poses, opt.hypotheses, *ARGS)

        def solver_and_quality():
            dsacstar.forward_rgb_batch(co, poses, opt.hypotheses, *ARGS)
            return dsacstar.pose_quality_batch(co, poses, *ARGS)

        def quality_only():
            return dsacstar.pose_quality_batch(co, poses, *ARGS)

        rows = solver_and_quality()
        again = quality_only()
        torch.cuda.synchronize()
        assert torch.equal(rows.nan_to_num(), again.nan_to_num()) and bool((rows[:, 6] == 0).all())
        (ts, tq), (ss, sq) = time_pair(solver, solver_and_quality, opt.warmup, opt.iters, opt.rounds)
        (tp, _), (sp, _) = time_pair(quality_only, quality_only, opt.warmup, opt.iters * 4, opt.rounds)
        results.append(dict(frames=B, hypotheses=opt.hypotheses, grid=[60, 90], solver_ms=ts, solver_spread_ms=ss,
                            solver_plus_quality_ms=tq, solver_plus_quality_spread_ms=sq, quality_added_ms=tq - ts,
                            quality_added_percent=100.0 * (tq - ts) / ts, quality_alone_ms=tp, quality_alone_spread_ms=sp,
                            solver_launch_form=int(dsacstar._lib.lib().xl_dsac_forward_sub_blocks(B, opt.hypotheses)),
                            median_sigma_pos_m=float(rows[:, 8].median()), median_sigma_rot_deg=float(rows[:, 9].median())))
    for r in results:
        print(json.dumps(r))
    if opt.json:
        os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
        with open(opt.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
