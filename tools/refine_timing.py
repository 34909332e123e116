"""Times the pose refinement (csrc/xl_dsac_refine.hip through dsacstar.refine_pose_batch) behind the solver, with HIP events on
warm clocks.  Not a test and not part of bench.py; there is no pass/fail threshold.

  95 frames x 256 hypotheses on 60 x 90 (the bench batch) and 1 frame, heteroscedastic frames (sigma 0.1 - 3 m, 30 % outliers):
  dsacstar.forward_rgb_batch alone, followed by refine_pose_batch with the sigma map, and followed by it in the NULL form
  (unweighted re-fit), on the same stream at the pose the solver wrote.

The three legs run alternately in the same process (rounds of `--iters` calls each) after `--warmup` calls; the figure of a leg is
the median over rounds of the per-call time, with its spread (max - min over rounds); the cost of the pass is the difference of
two medians.  Rounds and normal-equation evaluations per frame are reported beside it, since the pass is a serial
Levenberg-Marquardt per image and its time follows them.

    python tools/refine_timing.py [--json out.json]
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
RARGS = (10.0, synth.FOCAL, 360.0, 240.0, 100.0, 8)             # the refinement takes no alpha


def time_legs(fns, warmup, iters, rounds):
    """median per-call milliseconds of every leg and their spreads, alternating rounds; a round ends in an event synchronise"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
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
        raise SystemExit("refine_timing needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")

    # warm clocks: a second of streaming work before the first timed window
    x = torch.rand(64 << 20, device=dev)
    for _ in range(200):
        x.mul_(1.0000001)
    torch.cuda.synchronize()
    del x

    results = []
    for B in (95, 1):
        scenes = [synth.make_hetero_scene(2021 + i) for i in range(B)]
        co = torch.from_numpy(np.stack([s["coords"] for s in scenes])).to(dev)
        sg = torch.from_numpy(np.stack([s["sigma"] for s in scenes])).to(dev)
        gt = np.stack([s["pose"] for s in scenes])
        poses = torch.zeros((B, 4, 4), dtype=torch.float32, device=dev)
        refined = torch.zeros((B, 4, 4), dtype=torch.float32, device=dev)

        def solver():
            dsacstar.forward_rgb_batch(co, poses, opt.hypotheses, *ARGS)

        def solver_and_sigma():
            dsacstar.forward_rgb_batch(co, poses, opt.hypotheses, *ARGS)
            return dsacstar.refine_pose_batch(co, sg, poses, *RARGS, outPoses=refined)[1]

        def solver_and_null():
            dsacstar.forward_rgb_batch(co, poses, opt.hypotheses, *ARGS)
            return dsacstar.refine_pose_batch(co, None, poses, *RARGS, outPoses=refined)[1]

        def sigma_only():
            return dsacstar.refine_pose_batch(co, sg, poses, *RARGS, outPoses=refined)[1]

        def null_only():
            return dsacstar.refine_pose_batch(co, None, poses, *RARGS, outPoses=refined)[1]

        rows_n = solver_and_null().clone()
        t_n = [synth.pose_error(g, p)[0] for g, p in zip(gt, refined.cpu().numpy())]
        rows_s = solver_and_sigma().clone()
        t_s = [synth.pose_error(g, p)[0] for g, p in zip(gt, refined.cpu().numpy())]
        torch.cuda.synchronize()
        t_0 = [synth.pose_error(g, p)[0] for g, p in zip(gt, poses.cpu().numpy())]
        assert bool((rows_s[:, 6] == 0).all()) and bool((rows_n[:, 6] == 0).all())
        (ts, tq, tn), (ss, sq, sn) = time_legs((solver, solver_and_sigma, solver_and_null), opt.warmup, opt.iters, opt.rounds)
        (ps, pn), (sps, spn) = time_legs((sigma_only, null_only), opt.warmup, opt.iters * 4, opt.rounds)
        results.append(dict(
            frames=B, hypotheses=opt.hypotheses, grid=[60, 90], solver_ms=ts, solver_spread_ms=ss,
            solver_plus_sigma_ms=tq, solver_plus_sigma_spread_ms=sq, sigma_added_ms=tq - ts, sigma_added_percent=100.0 * (tq - ts) / ts,
            solver_plus_null_ms=tn, solver_plus_null_spread_ms=sn, null_added_ms=tn - ts, null_added_percent=100.0 * (tn - ts) / ts,
            sigma_alone_ms=ps, sigma_alone_spread_ms=sps, null_alone_ms=pn, null_alone_spread_ms=spn,
            solver_launch_form=int(dsacstar._lib.lib().xl_dsac_forward_sub_blocks(B, opt.hypotheses)),
            sigma_rounds_mean=float(rows_s[:, 58].mean()), sigma_rounds_max=float(rows_s[:, 58].max()),
            sigma_evals_mean=float(rows_s[:, 59].mean()), sigma_evals_max=float(rows_s[:, 59].max()),
            null_rounds_mean=float(rows_n[:, 58].mean()), null_evals_mean=float(rows_n[:, 59].mean()),
            null_evals_max=float(rows_n[:, 59].max()), converged_share=float(rows_s[:, 60].mean()),
            median_t_err_solver_m=float(np.median(t_0)), median_t_err_null_m=float(np.median(t_n)),
            median_t_err_sigma_m=float(np.median(t_s)), median_chi=float(rows_s[:, 7].median())))
    for r in results:
        print(json.dumps(r))
    if opt.json:
        os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
        with open(opt.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
