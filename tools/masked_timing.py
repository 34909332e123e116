"""Times the masked RGB solver (dsacstar.forward_rgb_masked_batch) against the plain one, with HIP events on warm clocks.  Not
a test and not part of bench.py; no bound is set on the masked legs.

  95 frames x 256 hypotheses on 60 x 90 (the bench batch) and 1 frame.  Legs:
    unmasked       forward_rgb_batch on make_scene frames (0.5 m noise, 30 % outliers)
    all_ones       forward_rgb_masked_batch, all-ones mask, the same frames (the same bits out: what the mask costs by itself)
    half           forward_rgb_masked_batch, a seeded random 50 % mask, the same frames
    decoy_band     forward_rgb_masked_batch on make_decoy_scene frames (top 60 % of the rows a second camera's view) with
                   their band mask - 40 % usable, so about 39 times the tries per hypothesis

The legs run alternately in the same process (rounds of `--iters` calls each) after `--warmup` calls; the figure of a leg is the
median over rounds of the per-call time, with its spread (max - min over rounds).  The mean tries per hypothesis of every leg
are reported beside its time, since the masked solver's cost follows them.

`--unmasked_only` times the first leg alone and needs nothing of this commit's interface: run it under a build of the parent
commit too (XL_TIMING_TREE=<that tree>: the package is imported from there), alternating the two processes, to see that the
unmasked instantiation did not move.
This commit's unmasked time may exceed the parent's by no more than the larger of the two spreads.

`--backward` times the backward passes instead (dsacstar.backward_rgb_masked_batch against backward_rgb_batch): 24 frames x 256
hypotheses on 60 x 90 and 1 frame, the same four legs (ground truth: the frames' own poses; the gradient buffer is accumulated
into and never read), the expected loss of the two decoy legs in place of the pose error.  `--backward --unmasked_only` is
the parent-commit leg as above.

`--quality` / `--refine` time the passes behind the solver (dsacstar.pose_quality_masked_batch / refine_pose_masked_batch against
pose_quality_batch / refine_pose_batch): 95 frames x 256 hypotheses on 60 x 90 and 1 frame.  Every leg is the masked solver plus
the pass behind it, as a masked evaluation runs them: `unmasked` the all-ones solver and the UNMASKED pass, `all_ones`, `half`
and `decoy_band` the solver and the masked pass over that mask (the refinement weighted by a sigma map of 0.5 m, make_scene's
noise).  With `--unmasked_only` the first leg alone, which the parent commit can run too.

`--sampler compact` (forward and `--backward`) adds the compact sampler's legs: every masked leg once more under
sampler="compact" (`<leg>_compact`), and a seeded random 10 % mask under both samplers (`tenth`, `tenth_compact`; max_tries at
its default, so the reject leg does find its hypotheses - at some 10^4 tries each).  What to read off: the compact legs' mean
tries stay at the unmasked leg's whatever the usable fraction; `all_ones_compact` against `all_ones` is the price of the rank
plane and the selection.

    python tools/masked_timing.py [--backward | --quality | --refine] [--sampler compact] [--json out.json] [--unmasked_only]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.environ.get("XL_TIMING_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dsacstar                                                 # noqa: E402
from crossloc_amd import synth                                  # noqa: E402

ARGS = (10.0, synth.FOCAL, 360.0, 240.0, 100.0, 100.0, 8)       # threshold, focal, ppx, ppy, alpha, max reprojection, subsampling
# backward: threshold, focal, ppx, ppy, rotation weight, translation weight, soft clamp, alpha, max reprojection, subsampling, seed
BWD_ARGS = (10.0, synth.FOCAL, 360.0, 240.0, 1.0, 100.0, 100.0, 100.0, 100.0, 8, 1305)


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


def mean_tries(out):
    """mean tries per hypothesis of a debug call (an exhausted hypothesis counts its whole budget)"""
    return float(out["tries"].abs().to(torch.float64).mean())


def backward_rows(opt, dev):
    """the rows of --backward: 24 frames and 1 frame"""
    results = []
    for B in (24, 1):
        scenes = [synth.make_scene(2021 + i) for i in range(B)]
        co = torch.from_numpy(np.stack([s["coords"] for s in scenes])).to(dev)
        gt = torch.from_numpy(np.stack([s["pose"] for s in scenes]).astype(np.float32)).to(dev)
        g = torch.zeros_like(co)

        def unmasked():
            return dsacstar.backward_rgb_batch(co, g, gt, opt.hypotheses, *BWD_ARGS)

        row = dict(solver_pass="backward", frames=B, hypotheses=opt.hypotheses, grid=[60, 90])
        if opt.unmasked_only:
            (tu,), (su,) = time_legs((unmasked,), opt.warmup, opt.iters, opt.rounds)
            row.update(unmasked_ms=tu, unmasked_spread_ms=su)
            results.append(row)
            continue

        decoys = [synth.make_decoy_scene(2021 + i, decoy=0.6) for i in range(B)]
        dco = torch.from_numpy(np.stack([s["coords"] for s in decoys])).to(dev)
        dgt = torch.from_numpy(np.stack([s["pose"] for s in decoys]).astype(np.float32)).to(dev)
        band = torch.from_numpy(np.stack([s["mask"] for s in decoys])).to(dev)
        ones = torch.ones((B, 60, 90), dtype=torch.uint8, device=dev)
        half = torch.from_numpy((np.random.default_rng(2021).random((B, 60, 90)) < 0.5).astype(np.uint8)).to(dev)

        def all_ones():
            return dsacstar.backward_rgb_masked_batch(co, ones, g, gt, opt.hypotheses, *BWD_ARGS)

        def half_mask():
            return dsacstar.backward_rgb_masked_batch(co, half, g, gt, opt.hypotheses, *BWD_ARGS)

        def decoy_band():
            return dsacstar.backward_rgb_masked_batch(dco, band, g, dgt, opt.hypotheses, *BWD_ARGS)

        def sampled(coords, mask, poses, sampler):
            return lambda: dsacstar.backward_rgb_masked_batch(coords, mask, g, poses, opt.hypotheses, *BWD_ARGS, sampler=sampler)

        ga, gb = torch.zeros_like(co), torch.zeros_like(co)
        la = dsacstar.backward_rgb_batch(co, ga, gt, opt.hypotheses, *BWD_ARGS)
        lb, status = dsacstar.backward_rgb_masked_batch(co, ones, gb, gt, opt.hypotheses, *BWD_ARGS)
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and torch.equal(ga, gb) and not status.any(), "identity A: the all-ones mask must give the unmasked pass's bits"
        legs = (("unmasked", unmasked), ("all_ones", all_ones), ("half", half_mask), ("decoy_band", decoy_band))
        if opt.sampler == "compact":
            tenth = torch.from_numpy((np.random.default_rng(2022).random((B, 60, 90)) < 0.1).astype(np.uint8)).to(dev)
            legs += (("all_ones_compact", sampled(co, ones, gt, "compact")), ("half_compact", sampled(co, half, gt, "compact")),
                     ("tenth", sampled(co, tenth, gt, "reject")), ("tenth_compact", sampled(co, tenth, gt, "compact")),
                     ("decoy_band_compact", sampled(dco, band, dgt, "compact")))
        med, spread = time_legs([fn for _, fn in legs], opt.warmup, opt.iters, opt.rounds)
        for (name, _), t, s in zip(legs, med, spread):
            row.update({name + "_ms": t, name + "_spread_ms": s})
        if opt.sampler == "compact":
            row["decoy_band_compact_median_expected_loss"] = float(dict(legs)["decoy_band_compact"]()[0].median())
        row["decoy_band_median_expected_loss"] = float(decoy_band()[0].median())
        row["decoy_unmasked_median_expected_loss"] = float(dsacstar.backward_rgb_batch(dco, g, dgt, opt.hypotheses, *BWD_ARGS).median())
        results.append(row)
    return results


def pass_rows(opt, dev):
    """the rows of --quality / --refine: 95 frames and 1 frame; every leg is the masked solver plus the pass behind it"""
    quality = opt.quality
    intr, tail = ARGS[:4], ((ARGS[4],) if quality else ()) + ARGS[5:]          # the refinement takes no alpha
    results = []
    for B in (95, 1):
        scenes = [synth.make_scene(2021 + i) for i in range(B)]
        co = torch.from_numpy(np.stack([s["coords"] for s in scenes])).to(dev)
        sg = torch.full((B, 60, 90), 0.5, device=dev)                          # make_scene's noise: 0.5 m per axis
        ones = torch.ones((B, 60, 90), dtype=torch.uint8, device=dev)
        poses = torch.zeros((B, 4, 4), dtype=torch.float32, device=dev)

        def behind(coords, mask, solve=True):
            """the solver over `mask`, then the pass: over the same mask, or (mask None: after the all-ones solver) unmasked;
            solve=False: the pass alone, at the poses the last solver call left"""
            if solve:
                dsacstar.forward_rgb_masked_batch(coords, ones if mask is None else mask, poses, opt.hypotheses, *ARGS)
            if quality:
                if mask is None:
                    return dsacstar.pose_quality_batch(coords, poses, *intr, *tail)
                return dsacstar.pose_quality_masked_batch(coords, mask, poses, *intr, *tail)
            if mask is None:
                return dsacstar.refine_pose_batch(coords, sg, poses, *intr, *tail)[1]
            return dsacstar.refine_pose_masked_batch(coords, mask, sg, poses, *intr, *tail)[1]

        row = dict(solver_pass="forward + " + ("quality" if quality else "refine"), frames=B, hypotheses=opt.hypotheses, grid=[60, 90])
        if opt.unmasked_only:
            (tu, tp), (su, sp) = time_legs((lambda: behind(co, None), lambda: behind(co, None, False)), opt.warmup, opt.iters,
                                           opt.rounds)
            row.update(unmasked_ms=tu, unmasked_spread_ms=su, unmasked_pass_ms=tp, unmasked_pass_spread_ms=sp)
            results.append(row)
            continue

        decoys = [synth.make_decoy_scene(2021 + i, decoy=0.6) for i in range(B)]
        dco = torch.from_numpy(np.stack([s["coords"] for s in decoys])).to(dev)
        band = torch.from_numpy(np.stack([s["mask"] for s in decoys])).to(dev)
        half = torch.from_numpy((np.random.default_rng(2021).random((B, 60, 90)) < 0.5).astype(np.uint8)).to(dev)
        ra, rb = behind(co, None), behind(co, ones)
        torch.cuda.synchronize()
        assert torch.equal(ra.nan_to_num(nan=-7.0), rb.nan_to_num(nan=-7.0)), "the all-ones mask must give the unmasked pass's rows"
        legs = (("unmasked", lambda: behind(co, None)), ("all_ones", lambda: behind(co, ones)),
                ("half", lambda: behind(co, half)), ("decoy_band", lambda: behind(dco, band)))
        med, spread = time_legs([fn for _, fn in legs], opt.warmup, opt.iters, opt.rounds)
        for (name, _), t, s in zip(legs, med, spread):
            row.update({name + "_ms": t, name + "_spread_ms": s})
        # the pass alone, at the poses of the all-ones solver: where the mask's own cost shows beside the solver's 2 ms
        behind(co, ones)
        alone = (("unmasked", lambda: behind(co, None, False)), ("all_ones", lambda: behind(co, ones, False)),
                 ("half", lambda: behind(co, half, False)))
        med, spread = time_legs([fn for _, fn in alone], opt.warmup, opt.iters, opt.rounds)
        for (name, _), t, s in zip(alone, med, spread):
            row.update({name + "_pass_ms": t, name + "_pass_spread_ms": s})
        results.append(row)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--hypotheses", type=int, default=256)
    ap.add_argument("--unmasked_only", action="store_true")
    ap.add_argument("--backward", action="store_true", help="time the backward passes (24 frames and 1 frame)")
    ap.add_argument("--quality", action="store_true", help="time the masked solver plus the quality pass behind it")
    ap.add_argument("--refine", action="store_true", help="time the masked solver plus the refinement behind it")
    ap.add_argument("--sampler", choices=("reject", "compact"), default="reject",
                    help="compact: add the compact sampler's legs and the 10 %% mask (forward and --backward)")
    ap.add_argument("--json", type=str, default=None)
    opt = ap.parse_args()
    if opt.backward + opt.quality + opt.refine > 1:
        raise SystemExit("masked_timing: one of --backward, --quality and --refine")
    if opt.sampler != "reject" and (opt.quality or opt.refine or opt.unmasked_only):
        raise SystemExit("masked_timing: --sampler is for the forward and the --backward legs")
    if opt.rounds < 5:
        raise SystemExit("masked_timing: at least 5 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("masked_timing needs the GPU: a timing taken elsewhere says nothing")
    dev = torch.device("cuda")

    # warm clocks: a second of streaming work before the first timed window
    x = torch.rand(64 << 20, device=dev)
    for _ in range(200):
        x.mul_(1.0000001)
    torch.cuda.synchronize()
    del x

    results = backward_rows(opt, dev) if opt.backward else pass_rows(opt, dev) if (opt.quality or opt.refine) else []
    for B in (() if results else (95, 1)):
        co = torch.from_numpy(np.stack([synth.make_scene(2021 + i)["coords"] for i in range(B)])).to(dev)
        poses = torch.zeros((B, 4, 4), dtype=torch.float32, device=dev)

        def unmasked(debug=False):
            return dsacstar.forward_rgb_batch(co, poses, opt.hypotheses, *ARGS, debug=debug)

        row = dict(frames=B, hypotheses=opt.hypotheses, grid=[60, 90],
                   solver_launch_form=int(dsacstar._lib.lib().xl_dsac_forward_sub_blocks(B, opt.hypotheses)))
        if opt.unmasked_only:
            (tu,), (su,) = time_legs((unmasked,), opt.warmup, opt.iters, opt.rounds)
            row.update(unmasked_ms=tu, unmasked_spread_ms=su, unmasked_mean_tries=mean_tries(unmasked(True)))
            results.append(row)
            continue

        decoys = [synth.make_decoy_scene(2021 + i, decoy=0.6) for i in range(B)]
        dco = torch.from_numpy(np.stack([s["coords"] for s in decoys])).to(dev)
        band = torch.from_numpy(np.stack([s["mask"] for s in decoys])).to(dev)
        ones = torch.ones((B, 60, 90), dtype=torch.uint8, device=dev)
        half = torch.from_numpy((np.random.default_rng(2021).random((B, 60, 90)) < 0.5).astype(np.uint8)).to(dev)
        mposes = torch.zeros((B, 4, 4), dtype=torch.float32, device=dev)

        def all_ones(debug=False):
            return dsacstar.forward_rgb_masked_batch(co, ones, mposes, opt.hypotheses, *ARGS, debug=debug)

        def half_mask(debug=False):
            return dsacstar.forward_rgb_masked_batch(co, half, mposes, opt.hypotheses, *ARGS, debug=debug)

        def decoy_band(debug=False):
            return dsacstar.forward_rgb_masked_batch(dco, band, mposes, opt.hypotheses, *ARGS, debug=debug)

        unmasked()
        all_ones()
        torch.cuda.synchronize()
        assert torch.equal(poses, mposes), "identity A: the all-ones mask must give the unmasked solver's poses"
        legs = (("unmasked", unmasked), ("all_ones", all_ones), ("half", half_mask), ("decoy_band", decoy_band))
        if opt.sampler == "compact":
            tenth = torch.from_numpy((np.random.default_rng(2022).random((B, 60, 90)) < 0.1).astype(np.uint8)).to(dev)

            def sampled(coords, mask, sampler):
                return lambda debug=False: dsacstar.forward_rgb_masked_batch(coords, mask, mposes, opt.hypotheses, *ARGS, debug=debug,
                                                                             sampler=sampler)

            legs += (("all_ones_compact", sampled(co, ones, "compact")), ("half_compact", sampled(co, half, "compact")),
                     ("tenth", sampled(co, tenth, "reject")), ("tenth_compact", sampled(co, tenth, "compact")),
                     ("decoy_band_compact", sampled(dco, band, "compact")))
        med, spread = time_legs([fn for _, fn in legs], opt.warmup, opt.iters, opt.rounds)
        for (name, fn), t, s in zip(legs, med, spread):
            row.update({name + "_ms": t, name + "_spread_ms": s, name + "_mean_tries": mean_tries(fn(True))})
        gt = np.stack([s["pose"] for s in decoys])
        if opt.sampler == "compact":
            dict(legs)["decoy_band_compact"]()
            torch.cuda.synchronize()
            row["decoy_band_compact_median_t_err_m"] = float(np.median([synth.pose_error(g, p)[0]
                                                                        for g, p in zip(gt, mposes.cpu().numpy())]))
            truth = np.stack([synth.make_scene(2021 + i)["pose"] for i in range(B)])
            for name in ("tenth", "tenth_compact"):
                dict(legs)[name]()
                torch.cuda.synchronize()
                row[name + "_median_t_err_m"] = float(np.median([synth.pose_error(g, p)[0]
                                                                 for g, p in zip(truth, mposes.cpu().numpy())]))
        decoy_band()
        torch.cuda.synchronize()
        row["decoy_band_median_t_err_m"] = float(np.median([synth.pose_error(g, p)[0] for g, p in zip(gt, mposes.cpu().numpy())]))
        dsacstar.forward_rgb_batch(dco, poses, opt.hypotheses, *ARGS)
        torch.cuda.synchronize()
        row["decoy_unmasked_median_t_err_m"] = float(np.median([synth.pose_error(g, p)[0] for g, p in zip(gt, poses.cpu().numpy())]))
        results.append(row)
    for r in results:
        print(json.dumps(r))
    if opt.json:
        os.makedirs(os.path.dirname(os.path.abspath(opt.json)), exist_ok=True)
        with open(opt.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
