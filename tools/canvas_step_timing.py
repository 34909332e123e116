"""Times the coord training step (training.make_step: forward, fused loss, backward, fused Adam) at batch 16 on 480x720 frames
that are already on the device, under the three frame paths, as the Trainer drives them (drop_plans_except before each step):

  fixed     no augmentation: the same tensors every step
  batch     the reference's augmentation: one scale and one angle per mini-batch (data.batch_resize); the input size changes
            from step to step, and the network lowers a plan for each new size
  canvas    the fixed-size augmentation: one scale and one angle per frame (data.batch_canvas), per-frame focal lengths to the
            loss, rotated poses; the input size never changes

Not a test and not part of bench.py; there is no pass/fail threshold.  The legs alternate in one process, `--rounds` windows of
`--steps` steps each, after every leg - and every input size of the `batch` leg - has run once.  Host wall-clock around a
window that ends in a device synchronise: planning is host work, which device events would not see.  The figure of a leg is
the median over its windows of the per-step time, the spread max - min over them.  The `batch` leg cycles through `--steps`
scales spread over 2/3 - 3/2, so each window runs the same sizes; its frame path is inside the timed window, like canvas's.

    python tools/canvas_step_timing.py [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crossloc_amd import data, networks, optim, synth, training      # noqa: E402
from crossloc_amd.weights import seeded_state_dict                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=8, help="steps per window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", type=str, default=None)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("canvas_step_timing needs the GPU: a timing taken elsewhere says nothing")
    dev, B = torch.device("cuda"), opt.batch
    net = networks.TransPoseNet(torch.tensor(synth.SCENE_MEAN, dtype=torch.float32), False, False, 2, 2, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=2021))
    net = net.to(dev).train()
    step = training.make_step(net, "coord", optim.Adam(net.parameters(), lr=1e-6), "MLE")
    images = torch.rand(B, 3, 480, 720, device=dev)
    _, gt, poses = synth.make_batch(1, B, noise=0.5, outlier_ratio=0.0)
    gt, poses = torch.from_numpy(gt).to(dev), torch.from_numpy(poses.astype(np.float32)).to(dev)
    focals = [synth.FOCAL] * B
    n = opt.steps
    batch_scales = [2 / 3 + (3 / 2 - 2 / 3) * ((3 * k) % n + 0.5) / n for k in range(n)]
    frame_scales = [[2 / 3 + (3 / 2 - 2 / 3) * ((5 * b + 3 * k) % B + 0.5) / B for b in range(B)] for k in range(n)]
    angles = [[-30.0 + 60.0 * ((7 * b + k) % B) / (B - 1) for b in range(B)] for k in range(n)]

    def run(x, p, lab, focal):
        net.drop_plans_except(x.shape[0], x.shape[2], x.shape[3])
        return step(x, p, lab, focal)

    def fixed(k):
        return run(images, poses, gt, focals[0])

    def batch(k):
        x, lab, f = data.batch_resize(images, gt, focals, batch_scales[k], angles[k][0])
        return run(x, poses, lab, f[0])

    def canvas(k):
        x, lab, p, f = data.batch_canvas(images, gt, poses, focals, frame_scales[k], angles[k])
        return run(x, p, lab, torch.tensor(f, dtype=torch.float64))

    legs = [("fixed", fixed), ("batch", batch), ("canvas", canvas)]
    for _, fn in legs:                                  # every leg and every size once: kernels loaded, allocator warm
        for k in range(n):
            fn(k)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in legs}
    for _ in range(opt.rounds):
        for name, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(n):
                loss, _ = fn(k)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / n * 1e3)
            assert torch.isfinite(loss)
    r = dict(batch_size=B, steps_per_window=n, rounds=opt.rounds, batch_leg_scales=batch_scales)
    for name, v in times.items():
        r[name + "_ms"], r[name + "_spread_ms"] = float(np.median(v)), float(np.max(v) - np.min(v))
    r["canvas_minus_fixed_ms"] = r["canvas_ms"] - r["fixed_ms"]
    r["canvas_minus_batch_ms"] = r["canvas_ms"] - r["batch_ms"]
    print(json.dumps(r))
    if opt.json:
        os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
        with open(opt.json, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
