"""Times the RGB-D solver (csrc/xl_dsac_rgbd.hip through dsacstar.forward_rgbd_batch) beside the RGB solver
(dsacstar.forward_rgb_batch) at the same shapes, with HIP events on warm clocks.  Not a test and not part of bench.py.

  95 frames x 256 hypotheses on 60 x 90 (the bench batch) and 1 frame.  RGB-D: camera-tensor form and depth form, 0.5 m
  coordinate noise, 1 % depth noise, 30 % outliers, thr 300 cm, maxDist 3000 cm.  RGB: thr 10 px, the bench's arguments.

The sides run alternately in the same process (rounds of `--iters` calls each) after `--warmup` calls; the figure is the
median over `--rounds` rounds of the per-call time.  The RGB-D poses are checked against ground truth before anything is timed.

    python tools/rgbd_timing.py [--json out.json]

With --backward the two backward passes are timed instead, alternately in the same way: dsacstar.backward_rgbd_batch (camera-tensor
form) beside dsacstar.backward_rgb_batch at 24 frames x 256 hypotheses on 60 x 90 and at 1 frame, pose-loss weights 1 / 100, soft
clamp 100, against the scenes' ground-truth poses.  Each call accumulates into its own gradient tensor.

    python tools/rgbd_timing.py --backward [--json out.json]

With --quality the two pose-quality passes are timed behind their solvers, four sides alternately in the same way:
forward_rgbd_batch (camera-tensor form) alone and with pose_quality_rgbd_batch enqueued behind it, forward_rgb_batch alone and
with pose_quality_batch behind it, at 95 frames x 256 hypotheses on 60 x 90 and at 1 frame.  The cost of a pass is the
difference of the pair.

    python tools/rgbd_timing.py --quality [--json out.json]

With --refine the RGB-D refinement is timed behind its solver, three legs alternately in the same way: forward_rgbd_batch
(camera-tensor form) alone, with the plain refine_pose_rgbd_batch behind it and with the weighted one (sigma + depthRel 0.01)
behind it, at 95 frames x 256 hypotheses on 60 x 90 and at 1 frame; synth.make_hetero_rgbd_scene frames: sigma 0.02 - 0.5 m,
1 % depth noise, 30 % outliers.  The cost of a pass is its leg minus the solver leg of the same run; rounds and evaluations per
frame and the median pose errors of the three legs are reported beside it.

    python tools/rgbd_timing.py --refine [--json out.json]
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

RGB_ARGS = (10.0, synth.FOCAL, 360.0, 240.0, 100.0, 100.0, 8)   # threshold, focal, ppx, ppy, alpha, max reprojection, subsampling
RGBD_ARGS = (300.0, 100.0, 3000.0)                              # threshold [cm], alpha, max distance [cm]


def time_sides(fns, warmup, iters, rounds):
    """median per-call milliseconds of every function and the spread over rounds, alternating; a round ends in an event synchronise"""
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


def depth_of(coords_gt, pose, rng, noise):
    """depth a sensor at `pose` measures of the ground-truth scene coordinates [3,Ho,Wo]: z of R^T (gt - c), multiplicative noise.
    Every ray of these scenes hits the terrain and no holes are cut, so the timed frames have no invalid cells: all 5400 cells
    are staged, sampled from and scored (the most work the kernel does per frame)."""
    z = np.einsum("k,khw->hw", pose[:3, 2], coords_gt.astype(np.float64) - pose[:3, 3][:, None, None])
    return (z * (1.0 + noise * rng.normal(size=z.shape))).astype(np.float32)


def backward_results(opt, dev):
    """one dict per batch size: per-call milliseconds of backward_rgb_batch and backward_rgbd_batch, alternately"""
    results = []
    for B in (24, 1):
        coords, gt, gt_poses = synth.make_batch(2021, B, noise=0.5, outlier_ratio=0.3)
        rng = np.random.default_rng(7)
        depth_np = np.stack([depth_of(gt[b], gt_poses[b], rng, 0.01) for b in range(B)])
        co = torch.from_numpy(coords).to(dev)
        cam = dsacstar.camera_coordinates(torch.from_numpy(depth_np).to(dev), synth.FOCAL, 480, 720, 8)
        poses = torch.from_numpy(np.asarray(gt_poses, np.float32)).to(dev)
        g_rgb, g_rgbd = torch.zeros_like(co), torch.zeros_like(co)
        losses = {}

        def rgb():
            losses["rgb"] = dsacstar.backward_rgb_batch(co, g_rgb, poses, opt.hypotheses, RGB_ARGS[0], RGB_ARGS[1], RGB_ARGS[2],
                                                        RGB_ARGS[3], 1.0, 100.0, 100.0, RGB_ARGS[4], RGB_ARGS[5], RGB_ARGS[6], 1305)

        def rgbd():
            losses["rgbd"] = dsacstar.backward_rgbd_batch(co, cam, g_rgbd, poses, opt.hypotheses, RGBD_ARGS[0], 1.0, 100.0, 100.0,
                                                          RGBD_ARGS[1], RGBD_ARGS[2], 1305)

        rgb(); rgbd()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(g_rgb).all()) and bool(torch.isfinite(g_rgbd).all()) and bool(g_rgbd.abs().max() > 0)
        first = {k: v.cpu().numpy() for k, v in losses.items()}
        (t_rgb, t_rgbd), (s_rgb, s_rgbd) = time_sides((rgb, rgbd), opt.warmup, opt.iters, opt.rounds)
        results.append(dict(mode="backward", frames=B, hypotheses=opt.hypotheses, grid=[60, 90], rounds=opt.rounds, iters=opt.iters,
                            rgb_backward_ms=t_rgb, rgb_backward_spread_ms=s_rgb, rgbd_backward_ms=t_rgbd,
                            rgbd_backward_spread_ms=s_rgbd, rgbd_over_rgb=t_rgbd / t_rgb,
                            rgb_mean_expected_loss=float(first["rgb"].mean()), rgbd_mean_expected_loss=float(first["rgbd"].mean())))
    return results


def quality_results(opt, dev):
    """one dict per batch size: per-call milliseconds of each solver alone and with its pose-quality pass behind it, alternately"""
    results = []
    for B in (95, 1):
        coords, gt, gt_poses = synth.make_batch(2021, B, noise=0.5, outlier_ratio=0.3)
        rng = np.random.default_rng(7)
        depth_np = np.stack([depth_of(gt[b], gt_poses[b], rng, 0.01) for b in range(B)])
        co = torch.from_numpy(coords).to(dev)
        cam = dsacstar.camera_coordinates(torch.from_numpy(depth_np).to(dev), synth.FOCAL, 480, 720, 8)
        poses = [torch.zeros((B, 4, 4), dtype=torch.float32, device=dev) for _ in range(4)]
        rows = {}

        def rgbd():
            dsacstar.forward_rgbd_batch(co, cam, poses[0], opt.hypotheses, *RGBD_ARGS)

        def rgbd_quality():
            dsacstar.forward_rgbd_batch(co, cam, poses[1], opt.hypotheses, *RGBD_ARGS)
            rows["rgbd"] = dsacstar.pose_quality_rgbd_batch(co, cam, poses[1], *RGBD_ARGS)

        def rgb():
            dsacstar.forward_rgb_batch(co, poses[2], opt.hypotheses, *RGB_ARGS)

        def rgb_quality():
            dsacstar.forward_rgb_batch(co, poses[3], opt.hypotheses, *RGB_ARGS)
            rows["rgb"] = dsacstar.pose_quality_batch(co, poses[3], *RGB_ARGS)

        sides = (rgbd, rgbd_quality, rgb, rgb_quality)
        for fn in sides:
            fn()
        torch.cuda.synchronize()
        assert torch.equal(poses[0], poses[1]) and torch.equal(poses[2], poses[3])
        first = {k: v.cpu().numpy() for k, v in rows.items()}
        assert (first["rgbd"][:, 6] == 0).all() and (first["rgb"][:, 6] == 0).all()
        t, sp = time_sides(sides, opt.warmup, opt.iters, opt.rounds)
        results.append(dict(mode="quality", frames=B, hypotheses=opt.hypotheses, grid=[60, 90], rounds=opt.rounds, iters=opt.iters,
                            rgbd_ms=t[0], rgbd_spread_ms=sp[0], rgbd_with_quality_ms=t[1], rgbd_with_quality_spread_ms=sp[1],
                            rgbd_quality_cost_ms=t[1] - t[0],
                            rgb_ms=t[2], rgb_spread_ms=sp[2], rgb_with_quality_ms=t[3], rgb_with_quality_spread_ms=sp[3],
                            rgb_quality_cost_ms=t[3] - t[2],
                            rgbd_median_inliers=float(np.median(first["rgbd"][:, 1])),
                            rgbd_median_sigma_m=float(np.median(first["rgbd"][:, 7])),
                            rgbd_median_sigma_pos_m=float(np.median(first["rgbd"][:, 8])),
                            rgb_median_sigma_pos_m=float(np.median(first["rgb"][:, 8]))))
    return results


def refine_results(opt, dev):
    """one dict per batch size: per-call milliseconds of the RGB-D solver alone, with the plain and with the weighted refinement
    behind it, alternately; rounds and evaluations per frame; the median pose errors of the three legs"""
    results = []
    for B in (95, 1):
        scs = [synth.make_hetero_rgbd_scene(2021 + b, depth_rel=0.01) for b in range(B)]
        co = torch.from_numpy(np.stack([s["coords"] for s in scs])).to(dev)
        cam = torch.from_numpy(np.stack([s["cam"] for s in scs])).to(dev)
        sg = torch.from_numpy(np.stack([s["sigma"] for s in scs])).to(dev)
        gt_poses = [s["pose"] for s in scs]
        poses = [torch.zeros((B, 4, 4), dtype=torch.float32, device=dev) for _ in range(3)]
        refined, rows = {}, {}

        def solver():
            dsacstar.forward_rgbd_batch(co, cam, poses[0], opt.hypotheses, *RGBD_ARGS)

        def plain():
            dsacstar.forward_rgbd_batch(co, cam, poses[1], opt.hypotheses, *RGBD_ARGS)
            refined["plain"], rows["plain"] = dsacstar.refine_pose_rgbd_batch(co, cam, None, poses[1], RGBD_ARGS[0], RGBD_ARGS[2])

        def weighted():
            dsacstar.forward_rgbd_batch(co, cam, poses[2], opt.hypotheses, *RGBD_ARGS)
            refined["weighted"], rows["weighted"] = dsacstar.refine_pose_rgbd_batch(co, cam, sg, poses[2], RGBD_ARGS[0], RGBD_ARGS[2],
                                                                                    depthRel=0.01)

        sides = (solver, plain, weighted)
        for fn in sides:
            fn()
        torch.cuda.synchronize()
        assert torch.equal(poses[0], poses[1]) and torch.equal(poses[0], poses[2])
        first = {k: v.cpu().numpy() for k, v in rows.items()}
        assert (first["plain"][:, 6] == 0).all() and (first["weighted"][:, 6] == 0).all()
        legs = dict(solver=poses[0], plain=refined["plain"], weighted=refined["weighted"])
        errs = {k: np.array([synth.pose_error(gt_poses[b], v[b].cpu().numpy().astype(np.float64)) for b in range(B)])
                for k, v in legs.items()}
        t, sp = time_sides(sides, opt.warmup, opt.iters, opt.rounds)
        r = dict(mode="refine", frames=B, hypotheses=opt.hypotheses, grid=[60, 90], rounds=opt.rounds, iters=opt.iters,
                 rgbd_ms=t[0], rgbd_spread_ms=sp[0], rgbd_with_plain_ms=t[1], rgbd_with_plain_spread_ms=sp[1],
                 rgbd_with_weighted_ms=t[2], rgbd_with_weighted_spread_ms=sp[2],
                 plain_cost_ms=t[1] - t[0], weighted_cost_ms=t[2] - t[0])
        for k in ("plain", "weighted"):
            r.update({k + "_mean_rounds": float(first[k][:, 58].mean()), k + "_mean_evals": float(first[k][:, 59].mean()),
                      k + "_max_evals": float(first[k][:, 59].max()), k + "_converged": float(first[k][:, 60].mean()),
                      k + "_median_chi": float(np.median(first[k][:, 7]))})
        for k, e in errs.items():
            r.update({k + "_median_t_err_m": float(np.median(e[:, 0])), k + "_median_r_err_deg": float(np.median(e[:, 1]))})
        results.append(r)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--hypotheses", type=int, default=256)
    ap.add_argument("--json", type=str, default=None)
    ap.add_argument("--backward", action="store_true", help="time backward_rgbd_batch beside backward_rgb_batch instead")
    ap.add_argument("--quality", action="store_true", help="time each solver alone and with its pose-quality pass behind it instead")
    ap.add_argument("--refine", action="store_true", help="time the RGB-D solver alone and with the plain / weighted refinement behind it instead")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rgbd_timing needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")

    # warm clocks: a second of streaming work before the first timed window
    x = torch.rand(64 << 20, device=dev)
    for _ in range(200):
        x.mul_(1.0000001)
    torch.cuda.synchronize()
    del x

    results = (backward_results(opt, dev) if opt.backward else quality_results(opt, dev) if opt.quality
               else refine_results(opt, dev) if opt.refine else [])
    for B in (() if opt.backward or opt.quality or opt.refine else (95, 1)):
        coords, gt, gt_poses = synth.make_batch(2021, B, noise=0.5, outlier_ratio=0.3)
        rng = np.random.default_rng(7)
        depth_np = np.stack([depth_of(gt[b], gt_poses[b], rng, 0.01) for b in range(B)])
        co = torch.from_numpy(coords).to(dev)
        depth = torch.from_numpy(depth_np).to(dev)
        cam = dsacstar.camera_coordinates(depth, synth.FOCAL, 480, 720, 8)
        poses_rgb = torch.zeros((B, 4, 4), dtype=torch.float32, device=dev)
        poses_cam = torch.zeros((B, 4, 4), dtype=torch.float32, device=dev)
        poses_dep = torch.zeros((B, 4, 4), dtype=torch.float32, device=dev)

        def rgb():
            dsacstar.forward_rgb_batch(co, poses_rgb, opt.hypotheses, *RGB_ARGS)

        def rgbd_cam():
            dsacstar.forward_rgbd_batch(co, cam, poses_cam, opt.hypotheses, *RGBD_ARGS)

        def rgbd_depth():
            dsacstar.forward_rgbd_batch(co, None, poses_dep, opt.hypotheses, *RGBD_ARGS, depth=depth, focalLength=synth.FOCAL,
                                        ppointX=360.0, ppointY=240.0, subSampling=8)

        rgb(); rgbd_cam(); rgbd_depth()
        torch.cuda.synchronize()
        assert torch.equal(poses_cam, poses_dep)
        errs = np.array([synth.pose_error(gt_poses[b], poses_cam[b].cpu().numpy().astype(np.float64)) for b in range(B)])
        errs_rgb = np.array([synth.pose_error(gt_poses[b], poses_rgb[b].cpu().numpy().astype(np.float64)) for b in range(B)])
        assert errs[:, 0].max() < 2.0 and errs[:, 1].max() < 0.5, errs.max(0)
        (t_rgb, t_cam, t_dep), (s_rgb, s_cam, s_dep) = time_sides((rgb, rgbd_cam, rgbd_depth), opt.warmup, opt.iters, opt.rounds)
        results.append(dict(frames=B, hypotheses=opt.hypotheses, grid=[60, 90], rounds=opt.rounds, iters=opt.iters,
                            rgb_ms=t_rgb, rgb_spread_ms=s_rgb, rgbd_camera_ms=t_cam, rgbd_camera_spread_ms=s_cam,
                            rgbd_depth_ms=t_dep, rgbd_depth_spread_ms=s_dep, rgbd_over_rgb=t_cam / t_rgb,
                            rgb_launch_form=int(dsacstar._lib.lib().xl_dsac_forward_sub_blocks(B, opt.hypotheses)),
                            rgbd_median_t_err_m=float(np.median(errs[:, 0])), rgbd_median_r_err_deg=float(np.median(errs[:, 1])),
                            rgb_median_t_err_m=float(np.median(errs_rgb[:, 0])), rgb_median_r_err_deg=float(np.median(errs_rgb[:, 1]))))
    for r in results:
        print(json.dumps(r))
    if opt.json:
        os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
        with open(opt.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
