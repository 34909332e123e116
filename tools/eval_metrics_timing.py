"""Times the fused per-image evaluation metrics (csrc/xl_metrics.hip through evaluation.task_metric_rows) against the eager
forms they replace, with HIP events on warm clocks.  Not a test and not part of bench.py; there is no pass/fail threshold.

  semantics  8 and 95 frames of 6 x 480 x 720 logits: task_metric_rows vs evaluation.semantic_eval (eager arg-max, then per
             image a boolean mask, a bincount and a read-back, then the int64 class map copied to the host); and like for
             like, semantic_eval_rows (rows + uint8 class map + read-back) vs semantic_eval, plus that copy on its own
  depth      95 x 60 x 90: task_metric_rows vs the formulas of utils/evaluation.py:247-267 as torch ops on CUDA tensors
  normal     95 x 60 x 90: task_metric_rows vs the formulas of utils/evaluation.py:294-316 as torch ops on CUDA tensors

Both sides of a leg run alternately in the same process (rounds of `--iters` calls each), after `--warmup` calls of every shape;
the figure is the median over rounds of the per-call time.  Results are compared before anything is timed.  Bytes are what the
algorithm must read (logits + labels), computed from the shapes; launches are counted from the code.

    python tools/eval_metrics_timing.py [--json out.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crossloc_amd import evaluation                             # noqa: E402


def eager_depth(depth, gt, nodata):
    """utils/evaluation.py:257-267 without the .cpu()"""
    d = depth.view(depth.size(0), -1)
    g = gt.view(depth.size(0), -1)
    err = torch.abs(d - g)
    m = evaluation.pick_valid_points(g.unsqueeze(1), nodata)
    return (err * m / g).sum() / m.sum(), ((err * m).square().sum() / m.sum()).sqrt()


def eager_normal(logits, gt, nodata):
    """utils/evaluation.py:303-316 with utils/learning.py:417-440, without the .cpu()"""
    B = logits.size(0)
    lg, g = logits.reshape(B, 2, -1), gt.view(B, 3, -1)
    ae = (torch.sigmoid(lg).clamp(min=1.e-7, max=1 - 1.e-7) * 2 - 1.0) * np.pi
    xy = torch.cos(ae[:, 1])
    xyz = torch.nn.functional.normalize(torch.stack([torch.cos(ae[:, 0]) * xy, torch.sin(ae[:, 0]) * xy, torch.sin(ae[:, 1])], 1),
                                        p=2, dim=1)
    ang = torch.acos(torch.nn.functional.cosine_similarity(xyz, g, dim=1).clamp(min=-1 + 1.e-7, max=1 - 1.e-7)) / np.pi * 180.0
    m = evaluation.pick_valid_points(g, nodata)
    return (ang * m).sum() / m.sum()


def time_pair(fused, eager, warmup, iters, rounds, fused_iters=None):
    """median per-call milliseconds of (fused, eager), alternating rounds; each round ends in an event synchronise.
    `fused_iters`: calls per window of the fused side, chosen by the caller so that a window holds tens of milliseconds of work"""
    n_calls = (fused_iters or iters, iters)
    for _ in range(warmup):
        fused(); eager()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(rounds):
        for k, fn in enumerate((fused, eager)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n_calls[k]):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / n_calls[k])
    return [float(np.median(v)) for v in out], [float(np.max(v) - np.min(v)) for v in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", type=str, default=None)
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_metrics_timing needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(5)
    results = []

    # warm clocks: a second of streaming work before the first timed window
    x = torch.rand(64 << 20, device=dev)
    for _ in range(200):
        x.mul_(1.0000001)
    torch.cuda.synchronize()
    del x

    for B in (8, 95):
        H, W = 480, 720
        logits = (torch.randn(B, 6, H, W, generator=g) * 2).to(dev)
        labels = torch.randint(-1, 7, (B, 1, H, W), generator=g).float().to(dev)
        rows = evaluation.task_metric_rows("semantics", logits, labels)
        _, miou, fwiou, acc = evaluation.semantic_eval(logits, labels, mute=True)
        a2, m2, f2 = evaluation.group_metrics("semantics", rows)
        assert np.allclose(m2, miou, rtol=1e-12) and np.allclose(f2, fwiou, rtol=1e-12) and np.allclose(a2, acc, rtol=1e-12)
        it = max(2, opt.iters // (4 if B > 8 else 1))
        (tf, te), (sf, se) = time_pair(lambda: evaluation.task_metric_rows("semantics", logits, labels),
                                       lambda: evaluation.semantic_eval(logits, labels, mute=True), opt.warmup, it, opt.rounds,
                                       fused_iters=opt.iters * 5)
        nbytes = B * H * W * 7 * 4
        # like for like: semantic_eval also returns the class map on the host (int64 [B,H,W], a device-to-host copy of
        # 8*B*H*W bytes); semantic_eval_rows is its replacement with the class map (uint8 on the device, widened on the host)
        # and the read-back, and is timed against it here.  Both sides synchronise with the host in every call.
        (tr, te2), (sr, _) = time_pair(lambda: evaluation.semantic_eval_rows(logits, labels, mute=True),
                                       lambda: evaluation.semantic_eval(logits, labels, mute=True), opt.warmup, it, opt.rounds)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        cls = torch.argmax(logits, dim=1)
        a.record()
        cls.cpu()
        b.record()
        b.synchronize()
        copy_ms = a.elapsed_time(b)
        del cls
        results.append(dict(leg="semantics", frames=B, shape=[6, H, W], fused_ms=tf, eager_ms=te, fused_spread_ms=sf,
                            eager_spread_ms=se, speedup=te / tf, fused_bytes=nbytes, fused_GBps=nbytes / tf / 1e6,
                            fused_launches=2, fused_workgroups=B * math.ceil(H * W / 4096),
                            working_set_MB=nbytes / 1e6, rows_with_map_and_readback_ms=tr, rows_with_map_spread_ms=sr,
                            eager_ms_second_run=te2, eager_class_map_copy_ms=copy_ms, eager_class_map_copy_bytes=B * H * W * 8,
                            eager_form="argmax + per image (mask, index, bincount, read-back): %d host synchronisations, then "
                                       "the int64 class map copied to the host" % B))
        del logits, labels

    B, H, W = 95, 60, 90
    depth = (torch.rand(B, 2, H, W, generator=g) * 300 + 1).to(dev)
    gtd = (torch.rand(B, 1, H, W, generator=g) * 300 + 1)
    gtd[torch.rand(B, 1, H, W, generator=g) < 0.2] = -1
    gtd = gtd.to(dev)
    r = evaluation.depth_eval(depth[:, :1], gtd, -1)
    e = eager_depth(depth[:, :1].contiguous(), gtd, -1)
    assert abs(float(r[0]) / float(e[0]) - 1) < 1e-5 and abs(float(r[1]) / float(e[1]) - 1) < 1e-5
    dc = depth[:, :1].contiguous()
    (tf, te), (sf, se) = time_pair(lambda: evaluation.task_metric_rows("depth", depth[:, :1], gtd, -1),
                                   lambda: eager_depth(dc, gtd, -1), opt.warmup, opt.iters * 5, opt.rounds,
                                   fused_iters=opt.iters * 50)
    results.append(dict(leg="depth", frames=B, shape=[1, H, W], fused_ms=tf, eager_ms=te, fused_spread_ms=sf, eager_spread_ms=se,
                        speedup=te / tf, fused_launches=2, fused_workgroups=B * math.ceil(H * W / 4096),
                        eager_form="the reference's formulas as torch ops on CUDA tensors (fp32), no read-back"))

    nl = (torch.randn(B, 3, H, W, generator=g) * 2).to(dev)
    gn = torch.randn(B, 3, H, W, generator=g)
    gn = gn / gn.norm(dim=1, keepdim=True)
    gn[(torch.rand(B, 1, H, W, generator=g) < 0.2).expand(-1, 3, -1, -1)] = -1
    gn = gn.to(dev)
    r = evaluation.normal_eval(nl[:, :2], gn, -1)
    e = eager_normal(nl[:, :2], gn, -1)
    assert abs(float(r) - float(e)) < 1e-3
    (tf, te), (sf, se) = time_pair(lambda: evaluation.task_metric_rows("normal", nl[:, :2], gn, -1),
                                   lambda: eager_normal(nl[:, :2], gn, -1), opt.warmup, opt.iters * 5, opt.rounds,
                                   fused_iters=opt.iters * 50)
    results.append(dict(leg="normal", frames=B, shape=[2, H, W], fused_ms=tf, eager_ms=te, fused_spread_ms=sf, eager_spread_ms=se,
                        speedup=te / tf, fused_launches=2, fused_workgroups=B * math.ceil(H * W / 4096),
                        eager_form="the reference's formulas as torch ops on CUDA tensors (fp32), no read-back"))

    for r in results:
        print(json.dumps(r))
    if opt.json:
        os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
        with open(opt.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
