"""Times the end-to-end DSAC* training step (training.make_e2e_step's sequence) and its parts at batch 16 on 480 x 720 frames
(a 60 x 90 grid), with HIP events on warm clocks.  Not a test and not part of bench.py.

  cnn         forward + backward of the full-size coord network (MLE head, 4 output channels) on a fixed output gradient
  solver      dsacstar.backward_rgb_batch, 64 hypotheses, on the [:, :3] view of a 4-channel output (0.5 m noise, 30 % outliers)
  op          loss.finish_pose_gradient (csrc/xl_e2e.hip, one launch) with clipping on
  eager       the torch restatement of the op (isfinite, norm, clamp, multiply, concatenate) on the same tensors
  step        forward, solver backward, op, backward, fused Adam - the whole step

The network carries seeded weights, which predict nothing: in `step` the coordinate channels of its output are overwritten
with the synthetic ones (one small copy inside the timed window), so the solver works on what it sees in training and not
against its try limit.  The sides run alternately in the same process (rounds of `--iters` calls each) after `--warmup` calls;
a figure is the median over `--rounds` rounds of the per-call time, with the spread over rounds beside it.  The op and its
restatement are compared before anything is timed, and the launches of each are counted with the profiler of torch.

    python tools/e2e_timing.py [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crossloc_amd import dsacstar, loss as xl_loss, optim, synth, training          # noqa: E402
from crossloc_amd.weights import seeded_state_dict                                  # noqa: E402

B, H, W, SUB, HYP, CLIP = 16, 480, 720, 8, 64, 1.0


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


def eager_finish(g, losses, C, weight, clip):
    """The op in eager torch: the same values up to the rounding of the scale (out, per-frame rows, summary row)."""
    n = g.double().flatten(1).norm(dim=1)
    ok = torch.isfinite(g).flatten(1).all(1) & torch.isfinite(losses)
    s = torch.where(ok, (weight / g.shape[0]) * torch.clamp(clip / n, max=1.0), 0.0).float()
    out3 = torch.where(ok[:, None, None, None], g * s[:, None, None, None], 0.0)
    out = torch.cat([out3, out3.new_zeros(g.shape[0], C - 3, *g.shape[2:])], 1)
    okd = ok.double()
    rows = torch.stack([losses, n, s.double(), okd], 1)
    summary = torch.stack([(torch.where(ok, losses, 0.0)).sum() / okd.sum().clamp(min=1.0), okd.sum(),
                           torch.where(ok, n, 0.0).max(), (ok & (n > clip)).double().sum()])
    return out, torch.cat([rows, summary[None]], 0)


def launches(fn):
    """device kernels and memory operations one call of fn enqueues (None where torch's profiler cannot say)"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:                                          # no tracer in this build of torch: not measured
        print("launch count not measured: %s" % (e,), file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--json", type=str, default=None)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("e2e_timing needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")

    # warm clocks: a second of streaming work before the first timed window
    x = torch.rand(64 << 20, device=dev)
    for _ in range(200):
        x.mul_(1.0000001)
    torch.cuda.synchronize()
    del x

    Ho, Wo = H // SUB, W // SUB
    coords, _, gt_poses = synth.make_batch(2021, B, noise=0.5, outlier_ratio=0.3)
    unc = np.ones((B, 1, Ho, Wo), np.float32)
    output = torch.from_numpy(np.concatenate([coords, unc], 1)).to(dev)                  # what the network would hand over
    synthetic = output[:, :3].contiguous()
    poses = torch.from_numpy(np.asarray(gt_poses, np.float32)).to(dev)
    focals = torch.full((B,), synth.FOCAL)
    images = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3)).to(dev)
    net = training.config_network("coord", False, False, "MLE", False, training.get_label_mean("naturescape", "coord"))
    net.load_state_dict(seeded_state_dict(net, seed=7))
    net = net.to(dev).train()
    adam = optim.Adam(net.parameters(), lr=1e-6)
    fixed_grad = torch.randn(B, 4, Ho, Wo, generator=torch.Generator().manual_seed(4)).to(dev)
    g = torch.zeros(B, 3, Ho, Wo, device=dev)
    solver_args = dict(hypotheses=HYP, threshold=10.0, inlier_alpha=100.0, max_pixel_error=100.0, weight_rot=1.0,
                       weight_trans=100.0, soft_clamp=100.0)
    keep = {}

    def cnn():
        net(images).backward(fixed_grad)
        net.zero_grad(set_to_none=True)

    def solver():
        g.zero_()
        keep["losses"] = dsacstar.backward_rgb_batch(output[:, :3], g, poses, HYP, 10.0, 0.0, W / 2, H / 2, 1.0, 100.0, 100.0,
                                                     100.0, 100.0, SUB, 1305, focals=focals, max_tries=xl_loss.E2E_MAX_TRIES)

    def op():
        keep["op"] = xl_loss.finish_pose_gradient(g, keep["losses"], 4, 1.0, CLIP)

    def eager():
        keep["eager"] = eager_finish(g, keep["losses"], 4, 1.0, CLIP)

    def step():
        pred = net(images)
        pred.data[:, :3].copy_(synthetic)
        keep["step"] = xl_loss.expected_pose_loss_and_output_gradient(pred, poses, focals, H, W, seed=1305, clip_norm=CLIP,
                                                                      subsample=SUB, **solver_args)
        pred.backward(keep["step"][2])
        adam.step()
        adam.zero_grad(set_to_none=True)

    solver(); op(); eager(); step()
    torch.cuda.synchronize()
    (o_out, o_stats), (e_out, e_stats) = keep["op"], keep["eager"]
    assert bool(o_stats[B, 1] == B), o_stats[B]
    assert torch.allclose(o_out, e_out, rtol=1e-6, atol=0.0) and torch.allclose(o_stats, e_stats, rtol=1e-6, atol=0.0)
    assert bool(keep["step"][1][B, 1] == B)
    n_op, n_eager = launches(op), launches(eager)

    sides = (cnn, solver, op, eager, step)
    t, sp = time_sides(sides, opt.warmup, opt.iters, opt.rounds)
    result = dict(frames=B, image=[H, W], grid=[Ho, Wo], hypotheses=HYP, rounds=opt.rounds, iters=opt.iters,
                  cnn_forward_backward_ms=t[0], cnn_forward_backward_spread_ms=sp[0],
                  solver_backward_ms=t[1], solver_backward_spread_ms=sp[1],
                  finishing_op_ms=t[2], finishing_op_spread_ms=sp[2], finishing_op_launches=n_op,
                  eager_finishing_ms=t[3], eager_finishing_spread_ms=sp[3], eager_finishing_launches=n_eager,
                  step_ms=t[4], step_spread_ms=sp[4],
                  mean_expected_loss=float(o_stats[B, 0]), max_norm=float(o_stats[B, 2]), clipped=int(o_stats[B, 3]))
    print(json.dumps(result))
    if opt.json:
        os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
        with open(opt.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
