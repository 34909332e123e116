"""Times the batched augmentation with one rotation per frame (xl_data_batch_augment_frames through data.batch_augment with a
list of angles) against the one-angle kernel it shares its per-pixel code with, and the pose rotation, with HIP events on warm
clocks.  Not a test and not part of bench.py; there is no pass/fail threshold.

  images   [16,3,480,720] -> the same size, bilinear, fill -1
  labels   [16,3,60,90]   -> the same size, nearest, fill -1
  legs     one angle (xl_data_batch_augment, the yardstick), 16 equal angles and 16 distinct angles through the per-frame
           entry point; data.rotate_poses on 16 poses

The legs of a shape run alternately in the same process (rounds of `--iters` calls each) after `--warmup` calls of every leg;
the figure is the median over rounds of the per-call time, the spread is max - min over the rounds of that leg.  The yardstick's
own spread is the margin a difference has to exceed to mean anything.  Results are compared bit for bit before anything is
timed.  Bytes are what the kernel must move (output written once, every input pixel read at most once), from the shapes.

--canvas adds the fixed-size augmentation (xl_data_canvas_augment through data.canvas_augment: a scale and an angle per frame,
one bilinear sample of four taps per image pixel) as further legs on the same tensors, alternating with the per-frame rotation
kernel in the same windows: the 16 distinct angles at scale 1 (the rotation kernel's own work; nearest mode is then bitwise
its output, which is checked), and 16 distinct scales in 2/3 - 3/2 with those angles.

    python tools/augment_timing.py [--canvas] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crossloc_amd import data, synth                            # noqa: E402


def time_legs(legs, warmup, iters, rounds):
    """legs: list of (name, fn, calls per window) -> {name: (median ms per call, max - min over rounds)}; rounds alternate
    over the legs and every window ends in an event synchronise."""
    for _ in range(warmup):
        for _, fn, _ in legs:
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name, _, _ in legs}
    for _ in range(rounds):
        for name, fn, n in legs:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n * iters):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) / (n * iters))
    return {k: (float(np.median(v)), float(np.max(v) - np.min(v))) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--json", type=str, default=None)
    ap.add_argument("--canvas", action="store_true", help="also time data.canvas_augment on the same tensors")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_timing needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(5)
    B = 16
    equal = [12.345] * B
    distinct = [-30.0 + 60.0 * b / (B - 1) for b in range(B)]
    ones = [1.0] * B
    scales = [2 / 3 + (3 / 2 - 2 / 3) * ((5 * b) % B) / (B - 1) for b in range(B)]
    results = []

    # warm clocks: a second of streaming work before the first timed window
    x = torch.rand(64 << 20, device=dev)
    for _ in range(200):
        x.mul_(1.0000001)
    torch.cuda.synchronize()
    del x

    for what, shape, bilinear, per_window in (("images", (B, 3, 480, 720), True, 20), ("labels", (B, 3, 60, 90), False, 100)):
        x = torch.randn(shape, generator=g).to(dev)
        oh, ow = shape[2], shape[3]
        one = data.batch_augment(x, oh, ow, 12.345, -1.0, bilinear)
        assert torch.equal(one, data.batch_augment(x, oh, ow, equal, -1.0, bilinear))
        many = data.batch_augment(x, oh, ow, distinct, -1.0, bilinear)
        for b in (0, 7, B - 1):
            assert torch.equal(many[b:b + 1], data.batch_augment(x[b:b + 1], oh, ow, distinct[b], -1.0, bilinear))
        legs = [("one_angle", lambda: data.batch_augment(x, oh, ow, 12.345, -1.0, bilinear), per_window),
                ("per_frame_equal", lambda: data.batch_augment(x, oh, ow, equal, -1.0, bilinear), per_window),
                ("per_frame_distinct", lambda: data.batch_augment(x, oh, ow, distinct, -1.0, bilinear), per_window)]
        if opt.canvas:
            if not bilinear:                                    # nearest at scale 1 is the rotation kernel's output
                assert torch.equal(many, data.canvas_augment(x, ones, distinct, -1.0, False))
            both = data.canvas_augment(x, scales, distinct, -1.0, bilinear)
            for b in (0, 7, B - 1):
                assert torch.equal(both[b:b + 1], data.canvas_augment(x[b:b + 1], scales[b:b + 1], distinct[b:b + 1], -1.0, bilinear))
            del both
            legs += [("canvas_rotation_only", lambda: data.canvas_augment(x, ones, distinct, -1.0, bilinear), per_window),
                     ("canvas_scale_and_rotation", lambda: data.canvas_augment(x, scales, distinct, -1.0, bilinear), per_window)]
        t = time_legs(legs, opt.warmup, opt.iters, opt.rounds)
        nbytes = 2 * x.numel() * 4
        r = dict(leg=what, shape=list(shape), bilinear=bilinear, bytes=nbytes)
        for k, (ms, spread) in t.items():
            r[k + "_ms"], r[k + "_spread_ms"], r[k + "_GBps"] = ms, spread, nbytes / ms / 1e6
        r["per_frame_equal_minus_one_angle_ms"] = t["per_frame_equal"][0] - t["one_angle"][0]
        r["per_frame_distinct_minus_one_angle_ms"] = t["per_frame_distinct"][0] - t["one_angle"][0]
        if opt.canvas:
            for k in ("canvas_rotation_only", "canvas_scale_and_rotation"):
                r[k + "_minus_per_frame_distinct_ms"] = t[k][0] - t["per_frame_distinct"][0]
        results.append(r)
        del x, one, many

    rng = np.random.default_rng(31)
    poses = torch.from_numpy(np.stack([synth.random_pose(rng) for _ in range(B)]).astype(np.float32)).to(dev)
    got = data.rotate_poses(poses, distinct).cpu().numpy()
    want = np.stack([(poses[b].cpu().numpy().astype(np.float64) @ data.pose_rotation(a)).astype(np.float32)
                     for b, a in enumerate(distinct)])
    assert np.allclose(got, want, rtol=2e-7, atol=0)
    t = time_legs([("rotate_poses", lambda: data.rotate_poses(poses, distinct), 100)], opt.warmup, opt.iters, opt.rounds)
    results.append(dict(leg="rotate_poses", frames=B, launches=1, rotate_poses_ms=t["rotate_poses"][0],
                        rotate_poses_spread_ms=t["rotate_poses"][1]))

    for r in results:
        print(json.dumps(r))
    if opt.json:
        os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
        with open(opt.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
