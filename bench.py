#!/usr/bin/env python
"""Benchmark of the CrossLoc localisation hot path on MI355X (BASELINE.json metric: images/s localised,
480x720 frames, 256 RANSAC hypotheses; median pose error in cm / deg).

A step = one batch of synthetic frames through the whole path on one GPU:
    single-task scene-coordinate CNN forward  ->  HIP dsacstar, 256 hypotheses per image.
The CNN computes in fp32: its GEMMs (Winograd F(6x6,3x3) for the 3x3 stride-1 layers, the 1x1 layers, the stride-2 stem) run on
the bf16 matrix pipe with every fp32 operand as an exact sum of three bf16 terms (six MFMA passes, fp32 accumulation).
No trained weights or datasets exist offline: the CNN runs seeded random weights on uniform-random images and
the solver consumes synthetic scene-coordinate maps (ray-cast terrain, 0.5 m noise, 30 % outliers) that are
resident in HBM before the timed region; both stages execute in full for every image of every step.
Multi-GPU: images shard as independent batches (weak scaling, no data-path collective); one RCCL all-gather of the
per-image errors for the median.  One rank per GPU under torch.distributed.run (the driver's launch line); a plain
`python bench.py --gpus N` re-executes itself under torch.distributed.run with N ranks on 127.0.0.1.

Prints ONE JSON line on rank 0 (contract in the task statement) including
    roofline         - the dominant kernel (the 64 batched Winograd GEMMs of a 3x3 512->512 layer) timed with HIP events on
                       its launch stream inside the timed region: executed bf16-MFMA FLOP against the dense bf16 MFMA peak;
    roofline_forward - the whole CNN forward: executed MFMA FLOP per step / CNN time against the same peak, and the
                       algorithmic HBM bytes per step / CNN time against the HBM peak;
    cpu_baseline     - with --full: the CPU oracle (restated reference path: OpenMP C solver + PyTorch-CPU network) on a
                       bounded sample, rank 0 at N=1 only (null otherwise).
A plain run does only what the headline needs: set-up, warm-up, the timed steps, the line.  --full adds, after the timed
region, the CPU baseline and the secondary configurations (secondary_configs: training step vs eager, latency legs, the
3-encoder network, the fp32-MFMA and six-pass bf16 forms, GEMM error figures) in config.  --dump-outputs DIR writes what the
last timed step returned (poses, predictions) as .npy files, for output-for-output comparison of two builds.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import math

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def kernel_source_hash():
    """sha256 (first 16 hex digits) of the sources of the GEMM / conv kernels: ties a traffic record to the code it was
    measured on."""
    import hashlib
    h = hashlib.sha256()
    for name in ("xl_cnn.hip", "xl_gemm_split.hip", "xl_gemm_pair.hip", "xl_stem_split.hip", "xl_common.h"):
        with open(os.path.join(ROOT, "crossloc_amd", "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def lookup_traffic(form, frames):
    """(bytes per launch or None, provenance string) for the dominant kernel in `form` ('wino64', 'wino36', 'direct')."""
    try:
        with open(TRAFFIC_JSON) as f:
            recs = json.load(f)["records"]
    except (OSError, ValueError, KeyError):
        return None, "profiles/traffic.json missing"
    for r in recs:
        if r["form"] == form and r["frames_per_launch"] == frames:
            stale = r.get("kernel_source_sha256_16") != kernel_source_hash()
            return int(r["bytes_per_launch"]), "%s%s" % (r["source"], " (STALE: measured on an older xl_cnn.hip)" if stale else "")
    return None, "no record for %s at %d frames per launch in profiles/traffic.json" % (form, frames)


PEAK_F64_VALU_TFLOPS = 78.65        # fp64 vector FMA: half of the fp32 vector rate (157.3 TFLOP/s, MI355X_MICROARCH.md)


def solver_valu_roofline(frames, n_hyp, cells, ms):
    """The solver against the roof that bounds it - fp64 VALU issue - from the time measured in this run; the issue-side counters
    (share of cycles a SIMD issued VALU work, fp64 share of it) come from the committed PMC record like `dsac_pmc`."""
    flop = float(frames) * n_hyp * cells * 60.0
    achieved = flop / (ms * 1e-3) / 1e12
    pmc = lookup_solver_counters() or {}
    return {"bound": "fp64 VALU issue", "algorithmic_fp64_GFLOP_per_batch": round(flop / 1e9, 3), "achieved": round(achieved, 3),
            "peak": PEAK_F64_VALU_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / PEAK_F64_VALU_TFLOPS, 4),
            "valu_busy_sample_and_score": pmc.get("sample_and_score_valu_busy"),
            "fp64_share_of_valu_instructions": pmc.get("sample_and_score_fp64_share_of_valu"),
            "note": "60 FLOP per (hypothesis, cell) is the useful arithmetic; the kernel's fp64 instruction stream also holds the "
                    "polynomial exp, divisions as Newton steps and the reductions - valu_busy x fp64 share is the issue-side view"}


def lookup_solver_counters():
    """VALU-issue figures of the solver kernels from the committed PMC record (None when there is none)."""
    try:
        with open(TRAFFIC_JSON) as f:
            sv = json.load(f)["solver"]
    except (OSError, ValueError, KeyError):
        return None
    k1 = sv["kernels"].get("xl_dsac_forward_kernel<1>")
    k2 = sv["kernels"].get("xl_dsac_forward_kernel<2>")
    if not k1:
        return None
    return {"sample_and_score_valu_busy": k1["valu_busy"], "sample_and_score_fp64_share_of_valu": k1["fp64_share_of_valu_instructions"],
            "sample_and_score_waves_per_simd": k1["mean_waves_per_simd"], "sample_and_score_lds_conflict_share": k1["lds_conflict_share"],
            "select_and_refine_valu_busy": k2["valu_busy"] if k2 else None, "source": sv["source"]}


def strict(obj):
    """The bench line must parse with a strict (RFC 8259) parser: non-finite floats become null."""
    if isinstance(obj, float):
        return obj if np.isfinite(obj) else None
    if isinstance(obj, dict):
        return {k: strict(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [strict(v) for v in obj]
    if isinstance(obj, np.generic):
        return strict(obj.item())
    return obj


def gather_and_median(local_err, world, dist=None, group=None):
    """Per-image (t_err [m], r_err [deg]) rows of every rank -> (median cm, median deg, rows gathered).  Equal shards
    (each rank localises batch x steps images), ONE all-gather (RCCL on GPU tensors, gloo on CPU tensors in the test);
    the median is not decomposable, hence gather not reduce."""
    import torch
    if world > 1:
        gathered = [torch.empty_like(local_err) for _ in range(world)]
        dist.all_gather(gathered, local_err, group=group)
        allerr = torch.cat(gathered, 0)
    else:
        allerr = local_err
    return (float(torch.median(allerr[:, 0]).item() * 100.0), float(torch.median(allerr[:, 1]).item()),
            int(allerr.shape[0]))


PEAK_F32_MFMA_TFLOPS = 157.3        # /opt/skills/guides/MI355X_MICROARCH.md: fp32-input MFMA = vector fp32 peak
PEAK_BF16_MFMA_TFLOPS = 2500.0      # same guide: dense bf16 MFMA (the 5 PF headline figure includes 2:1 sparsity)
# HBM-side bytes per launch of the dominant kernel cannot be read from inside the process (PMC counters need
# rocprofv3): they come from the committed record profiles/traffic.json, written by tools/traffic_record.py from the
# rocprofv3 PMC passes (FETCH_SIZE doubled per the gfx950 note of MI355X_MICROARCH.md §HBM, + WRITE_SIZE), keyed by
# kernel form and frames per launch, and carrying the hash of the kernel source it was measured on.
TRAFFIC_JSON = os.path.join(ROOT, "profiles", "traffic.json")
WINO_NAME = {16: "F(2x2,3x3)", 36: "F(4x4,3x3)", 64: "F(6x6,3x3)"}
FWD_GFLOP_PER_IMAGE = 295.41        # SURVEY.md §8(d), single-task net, 480x720
FWD_GFLOP_PER_IMAGE_3ENC = 755.96   # SURVEY.md §8(d), CrossLoc 3-encoder net


def plan_work(plan, networks):
    """What one forward of an inference plan executes, from its op list: MFMA FLOP by pipe (an fp16-pair GEMM = three 16-bit
    passes per fp32 product, a split-bf16 one six; useful K only, no tile padding) and the HBM bytes the plan's own tensors imply
    (every op reads its inputs and writes its outputs once; weights once; V / M of the Winograd layers included) - to be set against
    the algorithmic bytes of SURVEY.md 8(d).  `bf16_flop` = everything executed on the 16-bit matrix pipe (fp16 and bf16 MFMAs have
    the same dense peak); `fp32_equivalent_flop` = the fp32 products those passes stand for; `redundant_flop` = executed but not
    useful: conv1 is evaluated once for its GroupNorm statistics alone and again (on 1.16x its pixels: the patch overlap)
    inside the fused stem kernel."""
    bf16 = f32 = eq = redundant = 0.0
    byts = 0.0
    pair_flag = getattr(networks, "CONV_PAIR_F16", 0)
    for op in plan.ops:
        t = op.type
        if t == networks.XL_OP_CONV:
            Z = max(1, op.nchunks2)
            M = op.B * op.Ho * op.Wo
            K = op.ksize * op.ksize * op.Cin
            fl = 2.0 * Z * M * op.Cout * K
            split = bool(op.flags & networks.CONV_SPLIT_BF16)
            pair = bool(op.flags & pair_flag)
            eq += fl
            if split:
                bf16 += (3 if pair else 6) * fl
            else:
                f32 += fl
            act_in = Z * op.B * op.Hi * op.Wi * op.Cin
            if split and not pair and Z > 1 and not (op.flags & getattr(networks, "CONV_SPLIT_ACT", 0)):
                byts += act_in * 6                               # V as three bf16 planes
            else:
                byts += act_in * 4                               # fp32, or fp16 pairs
            byts += Z * M * op.Cout * 4 + Z * op.Cout * K * (4 if (pair or not split) else 6)
        elif t == getattr(networks, "XL_OP_STEM12", -1):
            # conv1 evaluated on the 9 x 33 patch of every 4 x 16 tile of conv2 outputs (1.16x its output pixels), then conv2
            px1 = op.B * (-(-op.Ho // 4)) * (-(-op.Wo // 16)) * 9 * 33
            bf16 += 6 * 2.0 * px1 * 32 * 27 + 6 * 2.0 * op.B * op.Ho * op.Wo * op.Cout * 288
            eq += 2.0 * px1 * 32 * 27 + 2.0 * op.B * op.Ho * op.Wo * op.Cout * 288
            redundant += 6 * 2.0 * (px1 - op.B * op.Hi * op.Wi) * 32 * 27     # the patch overlap
            byts += op.B * op.Hi * op.Wi * 3 * 4 + op.B * op.Ho * op.Wo * op.Cout * 4
        elif t == networks.XL_OP_CONV1:
            px = op.B * op.Hi * op.Wi
            if op.reserved_i == 0 and (op.stats or op.aux2):     # matrix-pipe form, one evaluation per launch
                bf16 += 6 * 2.0 * px * op.Cout * 27
                eq += 2.0 * px * op.Cout * 27
                if op.stats and not op.out:                      # the statistics-only evaluation: nothing but the sums leaves it
                    redundant += 6 * 2.0 * px * op.Cout * 27
            byts += px * 3 * 4 + (px * op.Cout * 4 if op.out else 0)
        elif t == networks.XL_OP_WINO_IN:
            nf = (op.ksize + 2) ** 2
            split = bool(op.flags & networks.CONV_SPLIT_BF16)       # (bf16 planes: 6 bytes; fp32 and fp16 pairs: 4)
            byts += op.B * op.Hi * op.Wi * op.Cin * 4 + nf * op.B * op.Ho * op.Wo * op.Cin * (6 if split else 4)
            if op.out2:                                          # fold: + residual read, + the materialised activation
                byts += op.B * op.Hi * op.Wi * op.Cin * 4 * (2 if op.flags & networks.GN_ADD else 1)
        elif t == networks.XL_OP_WINO_OUT:
            nf = (op.ksize + 2) ** 2
            Th, Tw = -(-op.Hi // op.ksize), -(-op.Wi // op.ksize)
            byts += nf * op.B * Th * Tw * op.Cin * 4 + op.B * op.Hi * op.Wi * op.Cin * 4
        elif t in (networks.XL_OP_GN_STATS, networks.XL_OP_GN_APPLY):
            n = op.B * op.Hi * op.Wi * op.Cin * 4
            byts += n * (1 if t == networks.XL_OP_GN_STATS else 2 + (1 if op.flags & networks.GN_ADD else 0))
        elif t == networks.XL_OP_HEAD:
            byts += op.B * op.Hi * op.Wi * (op.Cin + op.Cout) * 4
    return {"bf16_flop": bf16, "f32_flop": f32, "bytes": byts, "fp32_equivalent_flop": eq, "redundant_flop": redundant}


DUMP_LIMIT = 64 << 20               # bytes --dump-outputs may write in all


def dump_outputs(out_dir, poses, pred):
    """--dump-outputs: the last timed step's poses [B,4,4] and network predictions [B,C,H,W] as float32 .npy files.  Above
    DUMP_LIMIT both keep the same frames, a sample drawn with a fixed seed, so two builds still compare frame for frame."""
    poses, pred = poses.float().cpu().numpy(), pred.float().cpu().numpy()
    per_frame = poses[0].nbytes + pred[0].nbytes
    if len(pred) * per_frame > DUMP_LIMIT:
        keep = np.sort(np.random.default_rng(0).choice(len(pred), DUMP_LIMIT // per_frame, replace=False))
        poses, pred = poses[keep], pred[keep]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "poses.npy"), poses)
    np.save(os.path.join(out_dir, "predictions.npy"), pred)


def respawn_under_torchrun(n, argv):
    """`python bench.py --gpus N` started without a launcher (WORLD_SIZE unset): re-execute the same command line under
    torch.distributed.run with N ranks on this node - what the driver's own launch line does.  Returns the exit status."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: RCCL across processes needs it on this driver
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd, env=env)


def init_ranks(gpus, backend="nccl"):
    """RANK / LOCAL_RANK / WORLD_SIZE from the launcher -> (rank, local_rank, world, dist module or None, ranks in the
    group).  `nccl` IS RCCL on ROCm; one rank per GPU.  A rank without a GPU of its own stops here with a clear message
    (after the spawn, so `--gpus 2` on a one-GPU box says what is missing instead of hanging in the rendezvous)."""
    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != gpus:
        raise SystemExit("bench.py --gpus %d launched with WORLD_SIZE=%d" % (gpus, world))
    if backend == "nccl":
        have = torch.cuda.device_count()
        if have < world:
            raise SystemExit("bench.py --gpus %d needs %d GPUs on this node (one rank per GPU over RCCL); torch sees %d"
                             % (gpus, world, have))
    if world == 1:
        return rank, local_rank, 1, None, 1
    import torch.distributed as dist
    if backend == "nccl":
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        probe = torch.ones(1, device=torch.device("cuda", local_rank))
    else:
        dist.init_process_group(backend)
        probe = torch.ones(1)
    ranks = dist.get_world_size()
    assert dist.get_backend() == backend and ranks == world, (dist.get_backend(), ranks, world)
    dist.all_reduce(probe)                                                    # one collective before the timed region
    assert int(probe.item()) == world, "all-reduce over %d ranks returned %s" % (world, probe.item())
    return rank, local_rank, world, dist, ranks


def timed_steps(dist, sync, run_steps):
    """The contract's timed region: barrier + synchronize, EXACTLY the K steps, synchronize + barrier, MAX over ranks."""
    import torch
    if dist is not None:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    run_steps()
    sync()
    own = time.perf_counter() - t0
    if dist is not None:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    timed_steps.per_rank_s = (own, own)
    if dist is not None:
        dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
        # each rank's own time for its K steps (before the closing barrier): a straggler shows in the first real multi-GPU line
        lo, hi = torch.tensor([own], dtype=torch.float64, device=dev), torch.tensor([own], dtype=torch.float64, device=dev)
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        timed_steps.per_rank_s = (float(lo.item()), float(hi.item()))
    return elapsed


def run_stub(args, rank, world, dist):
    """XL_BENCH_STUB=1 (tests/test_distributed_cpu.py): bench.py's launcher, rank, barrier, max-over-ranks and all-gather
    code on CPU ranks (gloo) around a stand-in localiser that returns the ground-truth pose moved by a known amount per
    global image index.  Not a measurement: the line says so and carries no roofline."""
    import torch
    B, K = args.batch, args.steps
    rows = []

    def run_steps():
        for s in range(K):
            image0 = (s * world + rank) * B                                   # same global image index as the real step
            idx = torch.arange(image0, image0 + B, dtype=torch.float64)
            rows.append(torch.stack([0.01 * (1.0 + idx % 7), 0.001 * (1.0 + idx % 5)], 1))
    elapsed = timed_steps(dist, lambda: None, run_steps)
    local = torch.cat(rows, 0)
    med_t_cm, med_r_deg, n_rows = gather_and_median(local, world, dist)
    assert n_rows == world * B * K
    if rank == 0:
        print(json.dumps({"metric": "images/sec localized (480x720, 256 hyps)", "value": round(n_rows / max(elapsed, 1e-9), 2),
                          "unit": "images/s", "n_gpus": world, "steps": K, "warmup": args.warmup,
                          "ms_per_step": round(elapsed / K * 1e3, 3), "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": "none", "data": "STUB localiser on CPU ranks (plumbing test, not a measurement)",
                          "config": {"workload": "stub", "backend": dist.get_backend() if dist is not None else None,
                                     "ranks": world, "rows_gathered": n_rows, "median_err_cm": med_t_cm,
                                     "median_err_deg": med_r_deg}}))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=None,
                    help="images per step per GPU.  The persistent GEMM kernels walk 256 x 256 tiles with one workgroup per CU, so "
                         "what matters is how evenly the tiles divide over 256 CUs, and every kernel of the ~100 per forward has a "
                         "fixed start-up / tail cost (~0.5 ms per forward in total).  95 frames = 7168 tiles (28.0 rounds) for the 64 "
                         "batched Winograd GEMMs of a 512-channel layer - the 56 row tiles hold 14336 rows, 95 x 150 = 14250 - and 4008 "
                         "tiles (15.7 rounds) for a 1x1 layer; 47 frames (the default until round 4: 14.0 / 7.75 rounds) measures "
                         "1.8-2 %% lower (profiles/r4_bench_b47.json).  Default 95, also with --mlr 3 (47 there: -2.6 %%; 24 until round 4: -9 %%)")
    ap.add_argument("--hyps", type=int, default=256)
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also the CPU baseline and the secondary configurations (N=1 only); a plain "
                         "run measures the headline alone")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned on rank 0 as float32 .npy files: DIR/poses.npy [B,4,4] and "
                         "DIR/predictions.npy [B,C,60,90] (beyond %d MB in all: the same seeded sample of frames in both)"
                         % (DUMP_LIMIT >> 20))
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cnn-streams", type=int, default=1,
                    help="2: a step's CNN forward runs as two sub-batches on two HIP streams (the GEMMs of one overlap the "
                         "HBM-bound passes of the other: +9 %% images/s).  Not the default: kernel durations measured "
                         "while another stream shares the chip are not a roofline measurement")
    ap.add_argument("--mlr", type=int, default=0, choices=[0, 3],
                    help="3: BASELINE configs[4], the 3-encoder CrossLoc network (755.96 GFLOP per frame) instead of "
                         "the single-task one the headline metric is quoted on")
    ap.add_argument("--no-secondary", action="store_true",
                    help="with --full: skip the secondary configurations (BASELINE configs[1] batch-16 training step vs "
                         "PyTorch-ROCm eager, configs[4] 3-encoder network) that N=1 runs report outside the timed region")
    args = ap.parse_args()
    if args.batch is None:
        args.batch = 95

    stub = bool(os.environ.get("XL_BENCH_STUB"))       # tests only: the rank / collective / timing plumbing on CPU (gloo)
    # XL_BENCH_SHARED_GPU=1 (tests/test_multiprocess_gpu.py): the multi-process preflight on a ONE-GPU box.  Every rank runs the
    # real kernels on cuda:0; RCCL refuses two ranks on one device, so the gather and the max-over-ranks go through gloo on CPU
    # tensors and the line says rccl_ranks = 0.  Not a scaling measurement: the ranks share one chip.
    shared = bool(os.environ.get("XL_BENCH_SHARED_GPU"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: become the launcher (one rank per GPU, rendezvous on 127.0.0.1)
        raise SystemExit(respawn_under_torchrun(args.gpus, sys.argv[1:]))

    import torch
    rank, local_rank, world, dist, rccl_ranks = init_ranks(args.gpus, "gloo" if (stub or shared) else "nccl")
    if stub:
        return run_stub(args, rank, world, dist)
    if shared:
        local_rank, rccl_ranks = 0, 0
    from crossloc_amd import networks, synth, evaluation
    from crossloc_amd.weights import seeded_state_dict
    import dsacstar
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)

    B, K, W, H, IMW, NH = args.batch, args.steps, args.warmup, 480, 720, args.hyps
    mean = torch.tensor(synth.SCENE_MEAN, dtype=torch.float32)
    net = networks.TransPoseNet(mean, False, False, 2, 2, 3, 1, num_mlr=args.mlr)   # utils/learning.py:302-305 sizes
    net.load_state_dict(seeded_state_dict(net, seed=2021))
    net = net.to(dev).eval()

    g = torch.Generator(device="cpu").manual_seed(2021 + rank)
    images = torch.rand((B, 3, H, IMW), generator=g).to(dev)             # un-normalised [0,1] RGB at eval
    coords_np, _, poses_np = synth.make_batch(2021 + 1000 * rank, B, noise=0.5, outlier_ratio=0.3)
    coords = torch.from_numpy(coords_np).to(dev)
    gt_poses = torch.from_numpy(poses_np).to(dev)

    # pipeline: the CNN of a step runs as `cnn_streams` sub-batches on their own streams; the latency-bound solver of
    # step s runs on a side stream under the CNN of step s+1 (evaluation.PipelinedLocalizer)
    pipe = evaluation.PipelinedLocalizer(net, NH, synth.FOCAL, H, IMW, cnn_streams=args.cnn_streams)

    # The solver consumes the network's OWN output tensor (the strided NCHW view pred[:, :3], produced on the CNN stream,
    # read on the solver stream) like test_single_task.py:347-363.  Untrained weights do not predict a scene, so the
    # synthetic scene coordinates are written into the coordinate channels of that tensor after the head (`plant`).
    def step(s):
        image0 = (s * world + rank) * B                                   # global image index keys the sampler
        return pipe.submit(images, image0=image0, plant=coords)

    for s in range(W):
        step(s)
    pipe.finish()
    torch.cuda.synchronize()

    L = networks._bind()
    L.xl_cnn_prof_begin.argtypes = [ctypes.c_int]
    L.xl_cnn_prof_end.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    n_sub = min(len(pipe.cnn), B)
    sub_b = [round((i + 1) * B / n_sub) - round(i * B / n_sub) for i in range(n_sub)]
    plan = net._plans[(sub_b[0], H, IMW, dev.index, False, 1)]           # sub-batch 0 (all sub-batches have the same ops)
    n_ops = len(plan.op_array)
    # events only around the launches the roofline object reports (the batched Winograd GEMMs; the conv ops when the
    # plan has none), every op with XL_BENCH_VERBOSE: ~100 extra event pairs per step cost 1.5 % of the step
    has_wino = any(op.type == 1 and op.nchunks2 > 1 for op in plan.ops)
    split_gemm = any(op.type == 1 and op.nchunks2 > 1 and (op.flags & networks.CONV_SPLIT_BF16) for op in plan.ops)
    split_il = any(op.type == 1 and op.nchunks2 > 1 and (op.flags & networks.CONV_SPLIT_IL) for op in plan.ops)
    split_act = any(op.type == 1 and op.nchunks2 > 1 and (op.flags & networks.CONV_SPLIT_ACT) for op in plan.ops)
    pair_gemm = any(op.type == 1 and op.nchunks2 > 1 and (op.flags & networks.CONV_PAIR_F16) for op in plan.ops)
    pair_any = any(op.type == 1 and (op.flags & networks.CONV_PAIR_F16) for op in plan.ops)
    if os.environ.get("XL_BENCH_VERBOSE"):
        L.xl_cnn_prof_filter(-1, 0)
    else:
        L.xl_cnn_prof_filter(1, 0)              # every conv launch (30 per forward: the Winograd GEMMs and the 1x1 layers)
    L.xl_cnn_prof_begin(n_ops * K * n_sub)

    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True),
           torch.cuda.Event(enable_timing=True)) for _ in range(K)]
    all_poses = []
    last = {}

    def run_steps():
        for s in range(K):
            ev[s][0].record(pipe.cnn[0])
            pred, done = pipe.forward_cnn(images, plant=coords)
            last["pred"] = pred
            ev[s][1].record(pipe.cnn[0])                                 # stream 0 joins the others before the concat
            poses = torch.zeros((B, 4, 4), dtype=torch.float32, device=dev)
            for e in done:
                pipe.side.wait_event(e)                                  # solver(s) after CNN(s)
            pipe.side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(pipe.side):
                ev[s][2].record()
                dsacstar.forward_rgb_batch(pred[:, :3], poses, NH, 10.0, synth.FOCAL, IMW / 2.0, H / 2.0, 100.0, 100.0, 8,
                                           image0=(s * world + rank) * B)
                ev[s][3].record()
            pred.record_stream(pipe.side)
            all_poses.append(poses)
        pipe.finish()
    elapsed = timed_steps(dist, torch.cuda.synchronize, run_steps)

    # ---- per-kernel durations from the HIP events recorded inside the timed region
    cap = n_ops * K * n_sub
    idx = (ctypes.c_int32 * cap)()
    typ = (ctypes.c_int32 * cap)()
    ms = (ctypes.c_float * cap)()
    nrec = L.xl_cnn_prof_end(idx, typ, ms, cap)
    conv_ms, by_type, wino, wino_tiles = [], {}, 0, 0
    pw_ms, pw_split = [], False                                          # the 1x1 512 -> 512 layers
    for i in range(max(nrec, 0)):
        op = plan.op_array[idx[i]]
        by_type[typ[i]] = by_type.get(typ[i], 0.0) + ms[i]
        if (typ[i] == networks.XL_OP_CONV and op.Cin == 512 and op.Cout == 512 and op.ksize == 1 and op.nchunks2 <= 1
                and op.Hi == 60):
            pw_ms.append(ms[i])
            pw_split = bool(op.flags & networks.CONV_SPLIT_BF16)
        if typ[i] == networks.XL_OP_CONV and op.Cin == 512 and op.Cout == 512 and op.stride == 1 and (
                (op.ksize == 3 and op.nchunks2 <= 1) or (op.ksize == 1 and op.nchunks2 > 1)):
            conv_ms.append(ms[i])
            wino = int(op.nchunks2) if op.nchunks2 > 1 else 0
            wino_tiles = op.Hi * op.Wi
    if rank == 0 and os.environ.get("XL_BENCH_VERBOSE"):
        per_op = {}
        for i in range(max(nrec, 0)):
            per_op.setdefault(idx[i], []).append(ms[i])
        names = {0: "conv1", 1: "conv", 2: "gn_stats", 3: "gn_apply", 4: "head", 11: "gn_final", 12: "wino_in",
                 13: "wino_out", 19: "stem12"}
        for i in sorted(per_op):
            op = plan.op_array[i]
            sys.stderr.write("op %3d %-8s k%d s%d %4d->%4d %3dx%3d  %.4f ms\n" % (
                i, names[op.type], op.ksize, op.stride, op.Cin, op.Cout, op.Hi, op.Wi, float(np.mean(per_op[i]))))
        sys.stderr.write("by type (ms/step): %s\n" % {names[k]: round(v / K, 3) for k, v in by_type.items()})
    conv_avg_ms = float(np.mean(conv_ms)) if conv_ms else float("nan")
    # dominant kernel: the 3x3 512->512 layers.  Direct form: one implicit GEMM of 2*M*512*4608 FLOP.  Winograd
    # F(2x2,3x3) form (inference plans): one batched launch of 16 GEMMs [M/4 x 512] x [512 x 512]; the FLOPs counted
    # are the ones that launch executes (2.25x fewer multiplies than the direct form for the same layer)
    Bl = sub_b[0]                                    # frames per launch (one sub-batch)
    conv_flop = wino * 2.0 * (Bl * wino_tiles) * 512 * 512 if wino else 2.0 * (Bl * 60 * 90) * 512 * (9 * 512)
    conv_tflops = conv_flop / (conv_avg_ms * 1e-3) / 1e12 if conv_ms else float("nan")
    # split-bf16 GEMMs: every fp32 product is six bf16 MFMA passes; the roofline object counts the bf16 FLOPs the launch
    # executes against the dense bf16 MFMA peak, and also gives the fp32-equivalent rate
    mfma_passes = (3 if pair_gemm else 6) if (wino and split_gemm) else 1
    peak_tflops = PEAK_BF16_MFMA_TFLOPS if mfma_passes > 1 else PEAK_F32_MFMA_TFLOPS
    cnn_ms = float(np.mean([ev[s][0].elapsed_time(ev[s][1]) for s in range(K)]))
    work = plan_work(plan, networks)                 # one sub-batch; the sub-batches of a step have the same ops
    work = {k: v * n_sub for k, v in work.items()}
    dsac_ms = float(np.mean([ev[s][2].elapsed_time(ev[s][3]) for s in range(K)]))

    # ---- pose errors: every image of every step, gathered over ranks with one all-gather
    est = torch.cat(all_poses, 0)
    t_err, r_err = evaluation.pose_errors(gt_poses.repeat(K, 1, 1), est)
    local = torch.stack([t_err, r_err], 1)
    total_imgs = world * B * K
    med_t_cm, med_r_deg, n_rows = gather_and_median(local.cpu() if shared else local, world, dist)
    assert n_rows == total_imgs
    if os.environ.get("XL_BENCH_DUMP_POSES"):          # per-rank poses of every image of every step, in step order (tests)
        np.save("%s.rank%d.npy" % (os.environ["XL_BENCH_DUMP_POSES"], rank), est.cpu().numpy())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, all_poses[-1], last["pred"])

    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(net, images, coords_np, NH, args.mlr)
    secondary = {}
    if args.full and rank == 0 and world == 1 and not args.no_secondary and not args.mlr:
        del pipe, plan
        net.invalidate()
        torch.cuda.empty_cache()
        secondary = secondary_configs(dev, NH, batch=B)

    if rank == 0:
        value = total_imgs / elapsed
        form = ("pairact%d" if (mfma_passes == 3 and split_act) else "pair%d" if mfma_passes == 3 else
                "splitact%d" if (mfma_passes == 6 and split_act) else
                "split%d" if mfma_passes == 6 else "wino%d") % wino if wino else "direct"
        traffic, traffic_source = lookup_traffic(form, Bl)
        if mfma_passes == 3:
            kernel_name = ("pair_conv1x1_kernel<false,false,8,2,256> (256x256 tiles; V read as fp32, fp16 pairs formed inside the kernel)"
                           if split_act else
                           "pair_gemm_kernel<512> (256x256 tiles, persistent, both operands as fp16 pairs by LDS-DMA through a ring of 4 "
                           "stages)") + \
                          " batched x%d: the Winograd %s GEMMs of a 3x3 512->512 layer @60x90 x%d images per launch; an fp32 operand = " \
                          "the fp16 pair {hi, lo} (22 significand bits, power-of-two scaled), three v_mfma_f32_32x32x16_f16 passes " \
                          "(hi*hi, hi*lo, lo*hi), fp32 accumulation" % (wino, WINO_NAME.get(wino, "?"), Bl)
        elif mfma_passes == 6:
            kernel_name = ("split_conv1x1_kernel<false,false,8,2,256> (256x256 tiles; V read as fp32 and split into its three bf16 "
                           "terms inside the kernel, weights as interleaved 3xbf16 planes)" if split_act else
                           "split_gemm_persist_kernel<512> (256x256 tiles, interleaved 3xbf16 operand planes)" if split_il else
                           "split_gemm_kernel (128x128 tiles, separate bf16 planes)") + \
                          " batched x%d: the Winograd %s GEMMs of a 3x3 512->512 layer @60x90 x%d images per launch, every fp32 " \
                          "operand as an exact sum of three bf16 terms, six v_mfma_f32_32x32x16_bf16 passes, fp32 accumulation" % (
                              wino, WINO_NAME.get(wino, "?"), Bl)
        else:
            kernel_name = (("igemm_conv_kernel<1,1,128,512,0,128,1> batched x%d: the Winograd %s GEMMs of a 3x3 "
                            "512->512 layer @60x90" % (wino, WINO_NAME.get(wino, "?")) if wino else
                            "igemm_conv_kernel<3,1,128,512> (3x3 512->512 @60x90") + " x%d images per launch)" % Bl)
        alg_bytes = (wino * (2 * Bl * wino_tiles * 512 + 512 * 512) * 4 if wino else 2 * Bl * 5400 * 512 * 4 + 512 * 4608 * 4)
        if mfma_passes == 6:                         # U as 6 bytes per element (three bf16), M written as fp32, V read as
            v_bytes = 4 if split_act else 6          # fp32 (split inside the kernel) or as three bf16 planes
            alg_bytes = wino * (Bl * wino_tiles * 512 * v_bytes + 512 * 512 * 6 + Bl * wino_tiles * 512 * 4)
        if mfma_passes == 3:                         # V, U as fp16 pairs (4 bytes per element), M written as fp32
            alg_bytes = wino * (Bl * wino_tiles * 512 * 4 + 512 * 512 * 4 + Bl * wino_tiles * 512 * 4)
        out = {
            "metric": "images/sec localized (480x720, 256 hyps)", "value": round(value, 2), "unit": "images/s",
            "n_gpus": world, "steps": K, "warmup": W, "ms_per_step": round(elapsed / K * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": ("f32 (the GEMMs of the 3x3 stride-1 layers - Winograd F(6x6,3x3) - and of the 1x1 layers run with every fp32 "
                      "operand as a power-of-two-scaled fp16 pair {hi, lo} (22 significand bits) and three fp16-MFMA passes hi*hi + "
                      "hi*lo + lo*hi with fp32 accumulation: error against a float64 product of the same operands BELOW the fp32-MFMA "
                      "kernel's own, see split_gemm_err_vs_f64 / f32_mfma_err_vs_f64 in config; the stem's stride-2 layers as exact "
                      "sums of three bf16 terms, six bf16-MFMA passes; everything else fp32; all parity tests at the fp32 "
                      "tolerances; XL_GEMM_PAIR=0 runs the six-pass bf16 form everywhere, XL_GEMM_SPLIT_BF16=0 every GEMM on fp32 MFMA)"
                      if pair_any else
                      "f32 (the GEMMs of the 3x3 stride-1 layers - Winograd F(6x6,3x3) - and of the 1x1 layers run with every fp32 "
                      "operand as an exact sum of three bf16 terms: six bf16-MFMA passes, fp32 accumulation - fp32-class "
                      "accuracy, all parity tests at the fp32 tolerances; everything else fp32, the remaining convolutions on "
                      "fp32 MFMA; XL_GEMM_SPLIT_BF16=0 runs every GEMM on fp32 MFMA)" if split_gemm else "f32"),
            "data": "synthetic",
            "config": {"workload": ("BASELINE configs[4]: CrossLoc 3-encoder (coord+depth+normal) fusion network forward"
                                    if args.mlr else
                                    "BASELINE configs[2]: single-task coord CNN forward (2+2 extra res blocks)")
                                   + " + HIP dsacstar.forward_rgb, 480x720 frames, 60x90 coordinate grid",
                       "hypotheses": NH, "batch_per_gpu": B, "global_batch": B * world,
                       "parallelism": "images sharded over %d GPU(s), no data-path collective" % world,
                       "rccl_ranks": rccl_ranks, "rows_gathered": n_rows,
                       "per_rank_ms_per_step": {"min": round(timed_steps.per_rank_s[0] / K * 1e3, 3),
                                                "max": round(timed_steps.per_rank_s[1] / K * 1e3, 3)},
                       **({"preflight": "XL_BENCH_SHARED_GPU=1: %d ranks share cuda:0 (RCCL refuses two ranks on one device): gloo "
                                        "all-gather / max-over-ranks on CPU tensors, real kernels; not a scaling measurement" % world}
                          if shared else {}),
                       "solver_input": "the network's own output tensor pred[:, :3] (strided NCHW view, CNN stream -> solver "
                                       "stream); untrained seeded weights do not predict a scene, so synthetic scene "
                                       "coordinates (0.5 m noise, 30% outliers) are written into its coordinate channels "
                                       "after the head",
                       "cnn_ms_per_batch": round(cnn_ms, 3), "dsac_ms_per_batch": round(dsac_ms, 3),
                       "pipeline": "CNN of a step as %d sub-batches on %d streams; solver(s) on a side stream under "
                                   "CNN(s+1), ordered by events" % (n_sub, n_sub),
                       # north_star asks for the RANSAC stage against the HBM roofline as well: algorithmic bytes =
                       # nHyp*N*12 B + 64 B per image; the stage is LDS-resident and fp64/latency-bound
                       "dsac_algorithmic_GBps": round(B * (NH * 5400 * 12 + 64) / (dsac_ms * 1e-3) / 1e9, 1),
                       "dsac_hbm_roofline_frac": round(B * (NH * 5400 * 12 + 64) / (dsac_ms * 1e-3) / 8e12, 5),
                       # ... which says little for an LDS-resident fp64 kernel: the VALU-issue fraction from the PMC record
                       "dsac_pmc": lookup_solver_counters(),
                       # the roof that does bound it (round 6): fp64 vector FMA issue.  Algorithmic work = SURVEY.md 8(d)'s scoring count,
                       # nHyp * N * 60 FLOP per image (projection, residual, soft-inlier sigmoid; sampling, P3P and the LM refinement are
                       # not counted), all of it fp64 on the device; peak = 78.65 TFLOP/s (half the fp32 vector rate of the guide:
                       # 157.3 / 2).  Measured on the side stream, i.e. while the next batch's CNN shares the chip
                       "dsac_valu_roofline": solver_valu_roofline(B, NH, 5400, dsac_ms),
                       # direct-convolution FLOP count of the network over the CNN time; with the Winograd
                       # layers fewer multiplies are executed, so this "algorithmic" rate may exceed the MFMA peak
                       "cnn_fwd_algorithmic_tflops": round((FWD_GFLOP_PER_IMAGE_3ENC if args.mlr else FWD_GFLOP_PER_IMAGE) * B / cnn_ms, 2),
                       "conv3x3_s1_algorithm": ("winograd " + WINO_NAME.get(wino, "?")) if wino else "direct implicit GEMM",
                       # the second GEMM family of the forward: ten 1x1 512 -> 512 layers per frame batch
                       "conv1x1_512": {"kernel": "pair_conv1x1_kernel (fp16 pairs formed on load, three passes)" if (pw_split and pair_any)
                                                 else "split_conv1x1_kernel (bf16 pipe, activations split on load)" if pw_split
                                                 else "igemm_conv_kernel<1,1,128,512,...> (fp32 MFMA)",
                                       "avg_launch_ms": round(float(np.mean(pw_ms)), 4) if pw_ms else None,
                                       "launches_timed": len(pw_ms),
                                       "fp32_equivalent_tflops": round(2.0 * Bl * 5400 * 512 * 512 / (float(np.mean(pw_ms)) * 1e-3) / 1e12, 2)
                                       if pw_ms else None},
                       "median_err_cm": round(med_t_cm, 3), "median_err_deg": round(med_r_deg, 5)},
            "roofline": {"bound": "mfma", "kernel": kernel_name,
                         "achieved": round(conv_tflops * mfma_passes, 2), "peak": peak_tflops, "unit": "TFLOP/s",
                         "frac": round(conv_tflops * mfma_passes / peak_tflops, 4),
                         "mfma_dtype": "f16 x f16 -> f32" if mfma_passes == 3 else "bf16 x bf16 -> f32" if mfma_passes == 6 else "f32",
                         "mfma_passes_per_fp32_product": mfma_passes,
                         "fp32_equivalent_tflops": round(conv_tflops, 2),
                         "fp32_equivalent_vs_f32_mfma_peak": round(conv_tflops / PEAK_F32_MFMA_TFLOPS, 4),
                         "traffic": traffic, "traffic_source": traffic_source,
                         "algorithmic_bytes_per_launch": alg_bytes,
                         "avg_launch_ms": round(conv_avg_ms, 4), "launches_timed": len(conv_ms),
                         "algorithmic_gflop_per_launch": round(conv_flop * mfma_passes / 1e9, 2),
                         "fp32_equivalent_gflop_per_launch": round(conv_flop / 1e9, 2)},
            # the whole CNN forward of a step (north_star: ">= 50 % MFMA roofline on the coord-regression forward"): the MFMA
            # FLOP the plan executes (useful K, no tile padding; a split-bf16 product = six bf16 passes) over the CNN time of a
            # step, by pipe; `frac` = the time both pipes would need at their dense peaks / the CNN time.  HBM side: the
            # algorithmic bytes of SURVEY.md 8(d) (668 MB per image + 107 MB of weights) and the bytes the plan's own tensors
            # imply (V and M of the Winograd layers, every remaining GroupNorm pass), both over the same time
            "roofline_forward": {
                "bound": "mfma", "cnn_ms_per_step": round(cnn_ms, 3), "frames_per_step": B,
                "mfma_bf16_tflop_per_step": round(work["bf16_flop"] / 1e12, 3),
                "mfma_f32_tflop_per_step": round(work["f32_flop"] / 1e12, 4),
                "achieved": round(work["bf16_flop"] / (cnn_ms * 1e-3) / 1e12, 1), "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s",
                "frac_bf16_pipe": round(work["bf16_flop"] / (cnn_ms * 1e-3) / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4),
                "frac": round((work["bf16_flop"] / PEAK_BF16_MFMA_TFLOPS + work["f32_flop"] / PEAK_F32_MFMA_TFLOPS) / 1e12
                              / (cnn_ms * 1e-3), 4),
                "fp32_equivalent_tflops": round(work["fp32_equivalent_flop"] / (cnn_ms * 1e-3) / 1e12, 1),
                # executed vs useful: conv1 is evaluated once for its GroupNorm statistics alone and again (on 1.16x its pixels)
                # inside the fused stem kernel - those FLOP are in `achieved`, not in `useful_frac`
                "redundant_tflop_per_step": round(work["redundant_flop"] / 1e12, 3),
                "useful_frac": round(((work["bf16_flop"] - work["redundant_flop"]) / PEAK_BF16_MFMA_TFLOPS + work["f32_flop"] / PEAK_F32_MFMA_TFLOPS)
                                     / 1e12 / (cnn_ms * 1e-3), 4),
                "hbm": {"algorithmic_bytes_per_step": int((668e6 if not args.mlr else 0) * B + 107e6) if not args.mlr else None,
                        "algorithmic_TBps": round((668e6 * B + 107e6) / (cnn_ms * 1e-3) / 1e12, 3) if not args.mlr else None,
                        "plan_bytes_per_step": int(work["bytes"]),
                        "plan_TBps": round(work["bytes"] / (cnn_ms * 1e-3) / 1e12, 3),
                        "plan_over_algorithmic": round(work["bytes"] / (668e6 * B + 107e6), 2) if not args.mlr else None,
                        "peak_TBps": 8.0}},
            "cpu_baseline": cpu,
        }
        out["config"].update(secondary)
        print(json.dumps(strict(out), allow_nan=False))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def _eager_forward(sd, x, enc_add=2, dec_add=2, groups=32):
    """The single-task graph of networks/networks.py:221-256, 328-360 in plain PyTorch ops on the GPU (PyTorch-ROCm eager:
    MIOpen convolutions, native GroupNorm) - the BASELINE configs[1] comparison point, not part of the product path."""
    import torch
    import torch.nn.functional as F

    def cgr(t, conv, norm, stride=1, relu=True):
        w = sd[conv + ".weight"]
        t = F.conv2d(t, w, sd[conv + ".bias"], stride=stride, padding=w.shape[2] // 2)
        t = F.group_norm(t, groups, sd[norm + ".weight"], sd[norm + ".bias"], 1e-5)
        return F.relu(t) if relu else t

    def block(t, prefix):
        y = cgr(t, prefix + ".0", prefix + ".1")
        y = cgr(y, prefix + ".3", prefix + ".4")
        y = cgr(y, prefix + ".6", prefix + ".7")
        return F.relu(t + y)
    e = "encoder."
    t = cgr(x, e + "conv1", e + "norm1")
    t = cgr(t, e + "conv2", e + "norm2", 2)
    t = cgr(t, e + "conv3", e + "norm3", 2)
    res = cgr(t, e + "conv4", e + "norm4", 2)
    t = cgr(res, e + "res1_conv1", e + "res1_norm1")
    t = cgr(t, e + "res1_conv2", e + "res1_norm2")
    t = cgr(t, e + "res1_conv3", e + "res1_norm3")
    res = F.relu(res + t)
    t = cgr(res, e + "res2_conv1", e + "res2_norm1")
    t = cgr(t, e + "res2_conv2", e + "res2_norm2")
    t = cgr(t, e + "res2_conv3", e + "res2_norm3")
    res = F.relu(cgr(res, e + "res2_skip", e + "res2_skip_norm", relu=False) + t)
    for i in range(enc_add):
        res = block(res, e + "enc_add_res_block%d" % (i + 1))
    d = "decoder."
    for i in range(dec_add):
        res = block(res, d + "dec_add_res_block%d" % (i + 1))
    t = cgr(res, d + "res3_conv1", d + "res3_norm1")
    t = cgr(t, d + "res3_conv2", d + "res3_norm2")
    t = cgr(t, d + "res3_conv3", d + "res3_norm3")
    res = F.relu(res + t)
    t = cgr(res, d + "fc1", d + "fc1_norm")
    t = cgr(t, d + "fc2", d + "fc2_norm")
    sc = F.conv2d(t, sd[d + "fc3.weight"], sd[d + "fc3.bias"])
    coords = sc[:, :3] + sd[d + "mean"][None, :, None, None]
    sigma = torch.exp(F.hardtanh(sc[:, 3:], -16.10, 13.82))
    return coords, sigma


def _eager_coord_loss(sc, unc, poses, gt, focal=480.0, W=720, H=480):
    """loss/coord.py:87-188 (MLE mode, default clamps) in plain PyTorch ops, for the eager baseline."""
    import torch
    B = sc.shape[0]
    X, G = sc.reshape(B, 3, -1), gt.reshape(B, 3, -1)
    P = torch.linalg.inv(poses)[:, :3, :]
    one = torch.ones(B, 1, X.shape[2], device=sc.device)
    Xc, Gc = torch.bmm(P, torch.cat([X, one], 1)), torch.bmm(P, torch.cat([G, one], 1))
    d = torch.norm(Xc - Gc, dim=1)
    K = torch.tensor([[focal, 0, W / 2.0], [0, focal, H / 2.0], [0, 0, 1.0]], device=sc.device)
    p = torch.bmm(K.expand(B, 3, 3), Xc)
    uv = p[:, :2] / torch.clamp(p[:, 2:], min=0.1)
    ys, xs = torch.meshgrid(torch.arange(H // 8, device=sc.device) * 8.0 + 4, torch.arange(W // 8, device=sc.device) * 8.0 + 4,
                            indexing="ij")
    e = (uv - torch.stack([xs, ys]).reshape(1, 2, -1)).norm(dim=1).clamp(min=1e-7)
    g = (G == -1).sum(1) == 0
    m = ~(Xc[:, 2] < 0.1) & ~(e > 1000.0) & ~((d > 50.0) & g)
    ep = e * m
    lr = (ep * (ep <= 100.0)).clamp(min=1e-7) + torch.sqrt(100.0 * (ep * (ep > 100.0)).clamp(min=1e-7) + 1e-7).clamp(min=1e-7)
    s = unc.reshape(B, -1).clamp(min=1e-7)
    lu = 3.0 * torch.log(s) + d.square().clamp(min=1e-7) / (2.0 * s.square().clamp(min=1e-7))
    return (lu * g + lr).sum() / g.numel()


def inference_leg(dev, env, n_hyp, batch=95, steps=5, warmup=2):
    """The headline step (CNN forward + solver through PipelinedLocalizer, 480x720, `batch` frames) under the environment
    switches `env` (read when a plan is lowered), outside the headline's timed region: wall clock over `steps` steps between
    synchronisations, and the launches of the 3x3 512 -> 512 layers timed by HIP events on their own stream like the headline.
    Returns (images/s, average launch ms of the dominant kernel, launches timed, Z of that launch)."""
    import torch
    from crossloc_amd import evaluation, networks, synth
    from crossloc_amd.weights import seeded_state_dict
    H, W = 480, 720
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        net = networks.TransPoseNet(torch.tensor(synth.SCENE_MEAN, dtype=torch.float32), False, False, 2, 2, 3, 1)
        net.load_state_dict(seeded_state_dict(net, seed=2021))
        net = net.to(dev).eval()
        images = torch.rand((batch, 3, H, W), generator=torch.Generator().manual_seed(2021)).to(dev)
        coords = torch.from_numpy(synth.make_batch(2021, batch, noise=0.5, outlier_ratio=0.3)[0]).to(dev)
        pipe = evaluation.PipelinedLocalizer(net, n_hyp, synth.FOCAL, H, W)
        for s_ in range(warmup):
            pipe.submit(images, image0=s_ * batch, plant=coords)
        pipe.finish()
        torch.cuda.synchronize()
        plan = [p for k, p in net._plans.items() if k[0] == batch][0]
        L = networks._bind()
        L.xl_cnn_prof_begin.argtypes = [ctypes.c_int]
        L.xl_cnn_prof_end.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.xl_cnn_prof_filter(1, 0)
        cap = len(plan.op_array) * steps
        L.xl_cnn_prof_begin(cap)
        t0 = time.perf_counter()
        for s_ in range(steps):
            pipe.submit(images, image0=s_ * batch, plant=coords)
        pipe.finish()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        idx, typ, ms = (ctypes.c_int32 * cap)(), (ctypes.c_int32 * cap)(), (ctypes.c_float * cap)()
        n = L.xl_cnn_prof_end(idx, typ, ms, cap)
        dom, z = [], 0
        for i in range(max(n, 0)):
            op = plan.op_array[idx[i]]
            if typ[i] == networks.XL_OP_CONV and op.Cin == 512 and op.Cout == 512 and op.stride == 1 and (
                    (op.ksize == 3 and op.nchunks2 <= 1) or (op.ksize == 1 and op.nchunks2 > 1)):
                dom.append(ms[i])
                z = int(op.nchunks2) if op.nchunks2 > 1 else 0
        del pipe, plan, net
        torch.cuda.empty_cache()
        return batch * steps / dt, (float(np.mean(dom)) if dom else None), len(dom), z
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def gemm_error_leg(dev, frames=95):
    """What justifies `dtype: f32` for the split-bf16 GEMMs, measured on the bench box: the 64 batched [7050 x 512] x [512 x 512]
    products of a Winograd layer at `frames` frames on random fp32 operands, through the split kernel (six bf16-MFMA passes) and
    through the fp32-MFMA kernel, both against a float64 product of the SAME fp32 operands (torch.matmul in float64 on the GPU - a
    checker, not part of the product path).  Returns max |M - M64| / max |M64| for both."""
    import torch
    from crossloc_amd import networks
    Z, T, C, N = 64, frames * 150, 512, 512
    g = torch.Generator(device="cpu").manual_seed(99)
    V = torch.randn((Z, T, C), generator=g).to(dev)
    U = (torch.randn((Z, N, C), generator=g) * (1.0 / C) ** 0.5).to(dev)
    planes = networks._Plan.split_bf16_interleaved(U, C)
    L = networks._bind()
    il = networks.CONV_SPLIT_BF16 | networks.CONV_SPLIT_IL
    # fp16 pairs: V through the same split the input transform applies, with a scale 64 times looser than the data needs (a plan's
    # scale comes from a bound, not from the data); the weights one matrix at a time (one power-of-two scale each)
    vmax = float(V.abs().max().item())
    sexp = 14 - math.frexp(vmax)[1] - 6
    ascale = torch.tensor([math.ldexp(1.0, sexp), math.ldexp(1.0, -sexp)], dtype=torch.float32, device=dev)
    Vp = torch.empty(Z * T * C * 2, dtype=torch.int16, device=dev)
    networks._check(L.xl_cnn_pair_activation(V.data_ptr(), Vp.data_ptr(), Z * T, C, ascale.data_ptr(), None))
    Up = torch.zeros(2 * Z * N * C + 4 * Z, dtype=torch.int16, device=dev)
    one = torch.zeros(2 * N * C + 4, dtype=torch.int16, device=dev)
    for z in range(Z):
        networks._check(L.xl_cnn_pair_weight(U[z].contiguous().data_ptr(), one.data_ptr(), N, C, 1, None))
        Up[2 * z * N * C:2 * (z + 1) * N * C] = one[:2 * N * C]
        Up[2 * Z * N * C:].view(torch.float32)[Z + z] = one[2 * N * C:].view(torch.float32)[1]
    out = {}
    for name, flags, w, vin in (("pair", il | networks.CONV_PAIR_F16, Up, Vp), ("split", il | networks.CONV_SPLIT_ACT, planes, V), ("f32", 0, U, V)):
        Mb = torch.empty((Z, T, N), dtype=torch.float32, device=dev)
        op = networks.XlOp()
        op.type = networks.XL_OP_CONV
        op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout = frames, 10, 15, C, 10, 15, N
        op.ksize, op.stride, op.ld_in, op.ld_out, op.nchunks2, op.flags = 1, 1, C, N, Z, flags
        op.reserved_i = 256 if flags else 0
        op.in_, op.w, op.out, op.scale = vin.data_ptr(), w.data_ptr(), Mb.data_ptr(), ascale.data_ptr()
        arr = (networks.XlOp * 1)(op)
        networks._check(networks._bind().xl_cnn_run(arr, 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        err = scale = 0.0
        for z0 in range(0, Z, 8):                                            # float64 reference, 8 products at a time
            ref = torch.matmul(V[z0:z0 + 8].double(), U[z0:z0 + 8].double().transpose(1, 2))
            err = max(err, (Mb[z0:z0 + 8].double() - ref).abs().max().item())
            scale = max(scale, ref.abs().max().item())
        out[name] = err / scale
        del Mb
    del V, U, planes, Vp, Up
    torch.cuda.empty_cache()
    return out["pair"], out["split"], out["f32"]


def secondary_configs(dev, n_hyp, train_batch=16, mlr_batch=95, steps=5, batch=95):
    """Outside the timed region of the headline, N=1 only - the other single-GPU BASELINE configurations, so that their
    figures are driver-visible:
      configs[1]  batch-16 480x720 coord network forward + MLE coordinate loss + backward (train_single_task.py:245-301
                  without the optimizer), HIP path vs PyTorch-ROCm eager on the same graph, weights and inputs;
      configs[4]  the 3-encoder CrossLoc network forward + HIP dsacstar at 256 hypotheses (single-GPU share of it)."""
    import torch
    from crossloc_amd import evaluation, loss as xl_loss, networks, synth
    from crossloc_amd.weights import seeded_state_dict
    out = {}
    mean = torch.tensor(synth.SCENE_MEAN, dtype=torch.float32)
    H, W = 480, 720

    def timed(fn, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3, r

    # ---- configs[1]
    B = train_batch
    net = networks.TransPoseNet(mean, False, False, 2, 2, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=2021))
    net = net.to(dev).train()
    images = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(16)).to(dev)
    _, gt, poses = synth.make_batch(1, B, noise=0.5, outlier_ratio=0.0)
    gt_t, poses_t = torch.from_numpy(gt).to(dev), torch.from_numpy(poses.astype(np.float32)).to(dev)
    grid, cam = xl_loss.get_pixel_grid(8), xl_loss.get_cam_mat(W, H, synth.FOCAL)

    def hip_step():
        net.zero_grad(set_to_none=True)
        pred = net(images)
        sc, unc = torch.split(pred, [3, 1], dim=1)                          # train_single_task.py:269
        loss, _ = xl_loss.scene_coords_regression_loss(0.1, 100.0, 1000.0, 50.0, "MLE", grid, -1, cam, sc, unc,
                                                       poses_t, gt_t)
        loss.backward()
        return loss
    ms, loss = timed(hip_step)
    out["train16_ms_per_step"] = round(ms, 2)
    out["train16_loss"] = round(float(loss.item()), 4)
    out["train16_fwd_bwd_algorithmic_tflops"] = round(885.64 * B / ms, 1)     # 885.64 GFLOP per image
    sd = {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point and not k.endswith("mean"))
          for k, v in net.state_dict().items()}
    # the training step as the reference runs it (train_single_task.py:298-300, utils/learning.py:390-396): forward + MLE
    # coordinate loss + backward + optimizer.step() (fused Adam, one launch), and - because the weights changed - the re-pack
    # of every convolution operand before the next forward (Winograd transforms in float64 + the bf16 splits: HIP kernels,
    # csrc/xl_pack.hip).  Consecutive steps, so each timed step contains one of everything.
    from crossloc_amd import optim as xl_optim
    opt = xl_optim.Adam(net.parameters(), lr=1e-4)

    def full_step():
        loss, _ = xl_optim.train_step(net, opt, images, poses_t, gt_t, grid, cam)
        return loss
    fms, floss = timed(full_step)
    out["train16_full_step_ms"] = round(fms, 2)
    out["train16_full_step_loss_after_%d_steps" % (steps + 2)] = round(float(floss.item()), 4)
    del net, opt
    torch.cuda.empty_cache()

    def eager_step():
        for v in sd.values():
            v.grad = None
        sc, unc = _eager_forward(sd, images)
        loss = _eager_coord_loss(sc, unc, poses_t, gt_t)
        loss.backward()
        return loss
    try:
        ems, eloss = timed(eager_step)
        out["train16_eager_ms"] = round(ems, 2)
        out["train16_eager_loss"] = round(float(eloss.item()), 4)
        out["train16_speedup_vs_eager"] = round(ems / ms, 2)
    except RuntimeError as e:                                                 # MIOpen unavailable / out of workspace
        out["train16_eager_ms"] = None
        out["train16_eager_error"] = str(e)[:200]
    del sd
    torch.cuda.empty_cache()

    # ---- the reference's own API shape: batch 1 (test_single_task.py:347-363), and 8 frames per step.  Plans of <= 8 frames
    # replay their op list as one HIP graph; launches whose 256 x 256 tiles cannot fill the chip use 256 x 128 or 128 x 128
    # tiles, or 256 x 128 tiles for the last partial round of the 256 CUs (networks._Plan.split_tile_form).
    net = networks.TransPoseNet(mean, False, False, 2, 2, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=2021))
    net = net.to(dev).eval()
    for nb, key in ((1, "latency_b1_ms"), (8, "b8_images_per_s")):
        imgs = torch.rand((nb, 3, H, W), generator=torch.Generator().manual_seed(nb)).to(dev)
        c_np, _, _ = synth.make_batch(7000, nb, noise=0.5, outlier_ratio=0.3)
        c_t = torch.from_numpy(c_np).to(dev)
        pipe = evaluation.PipelinedLocalizer(net, n_hyp, synth.FOCAL, H, W)

        def small_step():
            pipe.submit(imgs, image0=0, plant=c_t)
        for _ in range(5):
            small_step()
        pipe.finish()
        torch.cuda.synchronize()
        n_it = 200 if nb == 1 else 60
        reps = []
        for _ in range(3):                                                    # median of three timed runs of n_it steps
            t0 = time.perf_counter()
            for _ in range(n_it):
                small_step()
            pipe.finish()
            torch.cuda.synchronize()
            reps.append((time.perf_counter() - t0) / n_it * 1e3)
        ms_small = sorted(reps)[1]
        out[key] = round(ms_small, 3) if nb == 1 else round(nb / ms_small * 1e3, 1)
        if nb == 1:
            out["latency_b1_images_per_s"] = round(1e3 / ms_small, 1)
        plan = [p for k, p in net._plans.items() if k[0] == nb][0]
        out["latency_b%d_hip_graph" % nb] = bool(getattr(plan, "graph", None))
        del pipe
    # ---- the drop-in call pattern itself (round 5): what a maintainer who only swaps the imports gets.  The literal sequence of
    # test_single_task.py:347-363 + utils/evaluation.py:156-172 per frame: `network(image.cuda())` on the DEFAULT stream,
    # torch.split, `scene_coords.cpu()`, `out_pose = torch.zeros((4, 4))` on the host, blocking `dsacstar.forward_rgb` with the
    # positional argument list of the reference.  64 frames, median of three passes.
    import dsacstar
    net.invalidate()
    frames = torch.rand((64, 1, 3, H, W), generator=torch.Generator().manual_seed(64))
    c_np, _, _ = synth.make_batch(9000, 64, noise=0.5, outlier_ratio=0.3)
    planted = torch.from_numpy(c_np).to(dev)

    def dropin_pass():
        with torch.no_grad():
            for i in range(64):
                predictions = net(frames[i].cuda())                          # [1, 4, 60, 90], default stream
                predictions, _unc = torch.split(predictions, [3, 1], dim=1)
                predictions = predictions.clone()
                predictions.copy_(planted[i:i + 1])                          # (untrained weights predict no scene: plant one)
                out_pose = torch.zeros((4, 4))
                scene_coords = predictions.cpu()
                dsacstar.forward_rgb(scene_coords, out_pose, n_hyp, 10.0, synth.FOCAL, float(W / 2), float(H / 2), 100.0, 100.0, 8)
        return out_pose
    dropin_pass()
    reps = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dropin_pass()
        torch.cuda.synchronize()
        reps.append((time.perf_counter() - t0) / 64 * 1e3)
    out["dropin_b1_ms"] = round(sorted(reps)[1], 3)
    out["dropin_b1_images_per_s"] = round(1e3 / sorted(reps)[1], 1)
    plan = [p for k, p in net._plans.items() if k[0] == 1][0]
    out["dropin_b1_hip_graph_on_default_stream"] = bool(getattr(plan, "graph", None))
    out["dropin_b1_sequence"] = ("per frame: net(image.cuda()) on the default stream, torch.split, .cpu(), out_pose = torch.zeros(4, 4), "
                                 "blocking dsacstar.forward_rgb(coords_cpu, out_pose, 256, 10, f, 360, 240, 100, 100, 8) - "
                                 "test_single_task.py:347-363 / utils/evaluation.py:156-172 of the reference, upload of the frame included")
    del net
    torch.cuda.empty_cache()

    # ---- configs[4], single-GPU share
    B = mlr_batch
    net = networks.TransPoseNet(mean, False, False, 2, 2, 3, 1, num_mlr=3)
    net.load_state_dict(seeded_state_dict(net, seed=2021))
    net = net.to(dev).eval()
    images = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(24)).to(dev)
    coords_np, _, poses_np = synth.make_batch(5000, B, noise=0.5, outlier_ratio=0.3)
    coords = torch.from_numpy(coords_np).to(dev)
    pipe = evaluation.PipelinedLocalizer(net, n_hyp, synth.FOCAL, H, W)
    last = {}

    def mlr_step():
        last["poses"], _ = pipe.submit(images, image0=0, plant=coords)
    ms, _ = timed(lambda: mlr_step())
    pipe.finish()
    torch.cuda.synchronize()
    t_err, r_err = evaluation.pose_errors(torch.from_numpy(poses_np).to(dev), last["poses"])
    out["mlr3_images_per_s"] = round(B / ms * 1e3, 1)
    out["mlr3_batch"] = B
    out["mlr3_ms_per_step"] = round(ms, 2)
    out["mlr3_fwd_algorithmic_tflops"] = round(FWD_GFLOP_PER_IMAGE_3ENC * B / ms, 1)
    out["mlr3_median_err_cm"] = round(float(torch.median(t_err).item()) * 100.0, 3)
    del pipe, net
    torch.cuda.empty_cache()

    # ---- the strict fp32-MFMA form of the headline (every GEMM on v_mfma_f32_32x32x2_f32, XL_GEMM_SPLIT_BF16=0) and the GEMM
    # error figures that justify calling the split-bf16 form f32: driver-visible, not builder-run files
    ips, dom_ms, n_dom, z = inference_leg(dev, {"XL_GEMM_SPLIT_BF16": "0"}, n_hyp, batch=batch)
    out["f32_mfma_images_per_s"] = round(ips, 1)
    if dom_ms:
        flop = (z * 2.0 * (batch * 150) * 512 * 512) if z else 2.0 * (batch * 5400) * 512 * 4608
        out["f32_mfma_dominant_kernel"] = {"avg_launch_ms": round(dom_ms, 4), "launches_timed": n_dom,
                                           "tflops": round(flop / (dom_ms * 1e-3) / 1e12, 2), "peak": PEAK_F32_MFMA_TFLOPS,
                                           "frac": round(flop / (dom_ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)}
    # ... and the six-pass bf16 form of the headline (XL_GEMM_PAIR=0, the round-4 kernels) for the same-session A/B
    ips6, dom6, n6, _ = inference_leg(dev, {"XL_GEMM_PAIR": "0"}, n_hyp, batch=batch)
    out["six_pass_bf16_images_per_s"] = round(ips6, 1)
    if dom6:
        out["six_pass_bf16_dominant_kernel_ms"] = round(dom6, 4)
    epair, esix, e32 = gemm_error_leg(dev, frames=batch)
    pair_on = os.environ.get("XL_GEMM_PAIR", "1") not in ("", "0")
    esp = epair if pair_on else esix                                      # the kernel the headline runs
    out["split_gemm_err_vs_f64"] = float("%.3e" % esp)
    out["split_gemm_kernel"] = "fp16 pairs, three passes (pair_gemm_kernel)" if pair_on else "three bf16 terms, six passes"
    out["f32_mfma_err_vs_f64"] = float("%.3e" % e32)
    out["split_gemm_err_over_f32_mfma_err"] = round(esp / max(e32, 1e-30), 2)
    out["six_pass_bf16_gemm_err_vs_f64"] = float("%.3e" % esix)
    out["fp16_pair_gemm_err_vs_f64"] = float("%.3e" % epair)
    return out


def host_cpu_info():
    """(model string, hardware threads this process may use, physical cores among them) from /proc/cpuinfo + affinity."""
    allowed = sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else list(range(os.cpu_count() or 1))
    model, cores, cur = "unknown", set(), {}
    try:
        with open("/proc/cpuinfo") as f:
            for line in f.read().split("\n") + [""]:
                if ":" in line:
                    k, v = [t.strip() for t in line.split(":", 1)]
                    cur[k] = v
                elif cur:
                    if "model name" in cur and model == "unknown":
                        model = cur["model name"]
                    if int(cur.get("processor", "-1")) in allowed:
                        cores.add((cur.get("physical id", "0"), cur.get("core id", cur.get("processor", "0"))))
                    cur = {}
    except (OSError, ValueError):
        pass
    return model, len(allowed), max(1, len(cores))


def cpu_baseline(net, images, coords_np, n_hyp, num_mlr=0, frames=5):
    """The restated reference CPU path on this box's host cores: PyTorch-CPU fp32 network with all
    physical cores + the C/OpenMP solver at OMP_NUM_THREADS = 1 and = the physical cores; the same synthetic frames and
    seeds as the GPU run, `frames` frames each after a warm-up, MEDIAN per-frame time.  Bounded (well under a minute)."""
    import torch
    from oracle import cnn_oracle, dsac_oracle
    dsac_oracle.build()
    model, threads, phys = host_cpu_info()
    # more threads than physical cores (or than 64) oversubscribe both OpenMP runtimes badly on a 2-socket host
    # (measured 22 s per frame at 256 threads): physical cores, at most 64, reported as `cores`
    cores = max(1, min(phys, 64))
    torch.set_num_threads(cores)
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    frames = min(frames, images.shape[0], coords_np.shape[0])
    xs = [images[b:b + 1].detach().cpu() for b in range(frames)]
    cnn_oracle.transposenet_forward(sd, xs[0], num_mlr, 2, 2)            # warm-up
    t_cnn = []
    for x in xs:
        t0 = time.perf_counter()
        cnn_oracle.transposenet_forward(sd, x, num_mlr, 2, 2)
        t_cnn.append(time.perf_counter() - t0)

    def solver(nthreads):
        dsac_oracle.set_num_threads(nthreads)
        dsac_oracle.forward_rgb(coords_np[0], n_hyp, 10.0, 480.0, 360.0, 240.0, 100.0, 100.0, 8)   # warm-up
        ts = []
        for b in range(frames):
            t0 = time.perf_counter()
            dsac_oracle.forward_rgb(coords_np[b], n_hyp, 10.0, 480.0, 360.0, 240.0, 100.0, 100.0, 8, image=b)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))
    t_dsac_1 = solver(1)
    t_dsac_n = solver(cores)
    t_cnn = float(np.median(t_cnn))

    # BASELINE configs[0]: ONE 480x720 frame, coord regression forward + forward_rgb with 64 hypotheses on the CPU path
    def solver64(nthreads):
        dsac_oracle.set_num_threads(nthreads)
        dsac_oracle.forward_rgb(coords_np[0], 64, 10.0, 480.0, 360.0, 240.0, 100.0, 100.0, 8)
        ts = []
        for b in range(frames):
            t0 = time.perf_counter()
            dsac_oracle.forward_rgb(coords_np[b], 64, 10.0, 480.0, 360.0, 240.0, 100.0, 100.0, 8, image=b)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))
    t64_1, t64_n = solver64(1), solver64(cores)
    return {"value": round(1.0 / (t_cnn + t_dsac_n), 3), "unit": "images/s", "cores": cores, "kind": "port",
            "sample": "median of %d frames each, after one warm-up frame: CNN forward (PyTorch CPU fp32, batch 1, %d threads) + "
                      "oracle dsacstar %d hyps (C/OpenMP, %d threads); reference binary unbuildable (needs OpenCV)" % (
                          frames, cores, n_hyp, cores),
            "cpu_model": model, "hardware_threads": threads, "physical_cores": phys,
            "cnn_s_per_image": round(t_cnn, 4), "dsac_s_per_image": round(t_dsac_n, 5),
            "dsac_s_per_image_omp1": round(t_dsac_1, 5),
            "value_omp1_solver": round(1.0 / (t_cnn + t_dsac_1), 3),
            "configs0_single_image_64hyps": {
                "workload": "BASELINE configs[0]: one 480x720 frame, CNN forward (PyTorch CPU fp32) + forward_rgb with 64 "
                            "hypotheses (C/OpenMP restatement), no GPU",
                "latency_s": round(t_cnn + t64_n, 4), "images_per_s": round(1.0 / (t_cnn + t64_n), 3),
                "cnn_s": round(t_cnn, 4), "dsac_s": round(t64_n, 5), "dsac_s_omp1": round(t64_1, 5),
                "latency_s_omp1_solver": round(t_cnn + t64_1, 4)}}


if __name__ == "__main__":
    main()
