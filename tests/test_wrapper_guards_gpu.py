"""GPU: the kernel families behind the Python wrappers - losses, evaluation metrics, frame preparation, augmentation, the fused
Adam step and the pose solvers (through the ctypes shim crossloc_amd.dsacstar; the compiled binding allocates in C++) - with
every tensor the wrapper allocates between guard bands (tests/guarded.py).  One ragged case each, taken from the parameter
lists of the family's own test module.  Every case runs the wrapper as always, then again with `torch` proxied in the owning
module (tensors the CALLER hands in to be written - poses, gradients, parameters, a class map - come from the registry too),
requires the results to be bitwise those of the first call, and every guard band intact."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import eval_inputs                                                               # noqa: E402
import dsac_rgbd_cases as rc                                                     # noqa: E402
import guarded                                                                   # noqa: E402
import rgbd_quality_cases as qc                                                  # noqa: E402
from crossloc_amd import data, dsacstar as shim, evaluation, loss as xl_loss, optim, synth     # noqa: E402

pytestmark = pytest.mark.gpu


def _same_bits(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        if not isinstance(a, torch.Tensor):
            assert a == b or (a != a and b != b), (what, i, a, b)
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, (what, i, a.dtype, b.dtype, a.shape, b.shape)
        x, y = (t.detach().contiguous().reshape(-1).view(torch.uint8) for t in (a, b))
        differ = int((x != y).sum())
        assert differ == 0, "%s: result %d of the guarded call differs from the unguarded one in %d of %d bytes" % (what, i, differ, x.numel())


def _twice(monkeypatch, module, fn, what):
    """fn(alloc) -> list of results; `alloc` (torch, then the proxy) allocates what the caller hands in to be written."""
    want = fn(torch)
    torch.cuda.synchronize()
    proxy = guarded.guard_modules(monkeypatch, module)
    try:
        got = fn(proxy)
        n = guarded.handed_out()
        print("%s: %d buffers between guard bands" % (what, n))
        assert n > 0
        _same_bits(got, want, what)
        guarded.assert_intact()
    finally:
        guarded.stop()


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


# ---- losses: the RAGGED shapes of tests/test_loss_gpu.py, reduction=None (70 images: past the finaliser's 64-entry table)

RAGGED = [(1, 1, 1), (1, 7, 9), (3, 61, 91), (70, 5, 7)]


def _loss_inputs(kind, B, Ho, Wo):
    rng = np.random.default_rng(2 + B * Ho)
    unc = np.exp(rng.uniform(-2, 3, size=(B, 1, Ho, Wo))).astype(np.float32)
    if kind == "coord":
        coords, gt, poses = synth.make_batch(900 + B, B, noise=3.0, outlier_ratio=0.1, Ho=Ho, Wo=Wo)
        return coords, unc, gt, poses.astype(np.float32)
    if kind == "depth":
        gd = rng.uniform(100, 300, size=(B, 1, Ho, Wo)).astype(np.float32)
        pd = gd + rng.normal(0, 4, size=gd.shape).astype(np.float32)
        gd[rng.uniform(size=gd.shape) < 0.1] = -1.0
        return pd, unc, gd, None
    if kind == "normal":
        gn = rng.normal(size=(B, 3, Ho, Wo)).astype(np.float32)
        gn /= np.linalg.norm(gn, axis=1, keepdims=True)
        gn[:, :, rng.uniform(size=(Ho, Wo)) < 0.05] = -1.0
        return rng.normal(0, 2, size=(B, 2, Ho, Wo)).astype(np.float32), unc, gn, None
    logits = (rng.normal(size=(B, 6, Ho, Wo)) * 3).astype(np.float32)
    return logits, None, rng.integers(0, 6, size=(B, 1, Ho, Wo)).astype(np.float32), None


@pytest.mark.parametrize("B,Ho,Wo", RAGGED)
@pytest.mark.parametrize("kind", ["coord", "depth", "normal", "semantics"])
def test_losses_between_guard_bands(monkeypatch, kind, B, Ho, Wo):
    pred, unc, gt, poses = _loss_inputs(kind, B, Ho, Wo)
    w = torch.linspace(0.5, 1.5, B).cuda()

    def fn(alloc):
        p = _dev(pred).requires_grad_(True)
        u = _dev(unc).requires_grad_(True) if unc is not None else None
        if kind == "coord":
            loss, rate = xl_loss.scene_coords_regression_loss(0.1, 100.0, 1000.0, 50.0, "MLE", xl_loss.get_pixel_grid(8), -1,
                                                              xl_loss.get_cam_mat(8 * Wo, 8 * Ho, synth.FOCAL), p, u, _dev(poses),
                                                              _dev(gt), reduction=None)
        elif kind == "depth":
            loss, rate = xl_loss.depth_regression_loss(0.1, 10.0, "MLE", -1, p, u, _dev(gt), reduction=None)
        elif kind == "normal":
            loss, rate = xl_loss.normal_regression_loss(10.0, "MLE", -1, p, u, _dev(gt), reduction=None)
        else:
            loss, rate = xl_loss.semantics_classification_loss(None, p, None, _dev(gt), xl_loss.CrossEntropyLoss2d(), None)
        assert tuple(loss.shape) == (B,)
        (loss * w).sum().backward()
        return [loss, float(rate), p.grad] + ([u.grad] if u is not None else [])
    _twice(monkeypatch, xl_loss, fn, "%s loss %dx%dx%d" % (kind, B, Ho, Wo))


# ---- evaluation metrics: the one-cell case and one CASES entry per task

def test_metrics_of_one_cell_between_guard_bands(monkeypatch):
    d = torch.tensor([[[[3.0]]], [[[7.0]]]], device="cuda")
    g = torch.tensor([[[[2.0]]], [[[-1.0]]]], device="cuda")
    _twice(monkeypatch, evaluation, lambda alloc: [evaluation.task_metric_rows("depth", d, g, -1)], "depth metrics of one cell")


@pytest.mark.parametrize("task", ["depth", "normal", "semantics"])
def test_metric_rows_between_guard_bands(monkeypatch, task):
    tag, nt = "b3_37x53", {"depth": 1, "normal": 2, "semantics": 6}[task]
    case = {"depth": eval_inputs.depth_inputs, "normal": eval_inputs.normal_inputs, "semantics": eval_inputs.semantics_case}[task](tag)
    out, gt = _dev(case[0]), _dev(case[1])
    B, _, H, W = out.shape

    def fn(alloc):
        if task != "semantics":
            return [evaluation.task_metric_rows(task, out[:, :nt], gt, -1)]        # (the strided view of the [B,nt+1,H,W] output)
        cmap = alloc.full((B, H, W), 99, dtype=torch.uint8, device="cuda")
        return [evaluation.task_metric_rows("semantics", out[:, :6], gt, class_map=cmap), cmap]
    _twice(monkeypatch, evaluation, fn, "%s metrics %s" % (task, tag))


# ---- frame preparation and augmentation

def test_prepare_images_between_guard_bands(monkeypatch):
    frames = torch.from_numpy(np.random.default_rng(300 + 451 + 3).integers(0, 256, (2, 300, 451, 3), dtype=np.uint8)).cuda()
    jitter = [(0.93, 1.07, 0.0), (1.08, 0.91, 1.0)]
    _twice(monkeypatch, data, lambda alloc: [data.prepare_images(frames, 480, jitter=jitter, normalize=True)], "prepare_images 300x451x3")


def test_batch_augment_between_guard_bands(monkeypatch):
    scale, angle = 1.2345, 12.345
    g = torch.Generator().manual_seed(int(scale * 100))
    x = torch.randn(3, 3, 96, 144, generator=g).cuda()
    lab = torch.randn(3, 3, 12, 18, generator=g).cuda()
    oh, ow = math.ceil(96 * scale), math.ceil(144 * scale)

    def fn(alloc):
        return [data.batch_augment(x, oh, ow, angle, -1.0, True),
                data.batch_augment(lab, math.ceil(oh / 8), math.ceil(ow / 8), angle, -1.0, False)]
    _twice(monkeypatch, data, fn, "batch_augment 1.2345 / 12.345")


# ---- the fused Adam step: the shape list of test_fused_adam_matches_torch_adam (70001 and 1 elements: the chunk tails)

def test_adam_step_between_guard_bands(monkeypatch):
    g = torch.Generator().manual_seed(0)
    shapes = [(512, 512, 3, 3), (512,), (70001,), (4, 512, 1, 1), (1,)]
    values = [torch.randn(s, generator=g) for s in shapes]
    grads = [torch.randn(s, generator=g).cuda() for s in shapes]

    def fn(alloc):
        ps = []
        for v in values:                                    # the kernel writes the parameters in place: guarded as well
            p = alloc.empty(v.shape, dtype=torch.float32, device="cuda")
            p.copy_(v)
            ps.append(p.requires_grad_(True))
        opt = optim.Adam(ps, lr=1e-3)
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt.step()
        torch.cuda.synchronize()
        return [p.detach() for p in ps] + [opt.state[p][k] for p in ps for k in ("exp_avg", "exp_avg_sq")]
    _twice(monkeypatch, optim, fn, "Adam step")


# ---- the pose solvers through the ctypes shim

@pytest.mark.parametrize("Ho,Wo", [(7, 13), (33, 17)])
def test_forward_rgb_batch_between_guard_bands(monkeypatch, Ho, Wo):
    sc = synth.make_scene(50, noise=0.2, outlier_ratio=0.2, Ho=Ho, Wo=Wo)
    co = _dev(sc["coords"][None])

    def fn(alloc):
        poses = alloc.zeros((1, 4, 4), dtype=torch.float32, device="cuda")
        d = shim.forward_rgb_batch(co, poses, 16, 10.0, synth.FOCAL, sc["ppx"], sc["ppy"], 100.0, 100.0, 8, debug=True)
        return [poses] + [d[k] for k in ("cells", "tries", "scores", "dbg")]
    _twice(monkeypatch, shim, fn, "forward_rgb_batch %dx%d" % (Ho, Wo))


def test_backward_rgb_batch_between_guard_bands(monkeypatch):
    coords, _, poses = synth.make_batch(77, 3, noise=0.5, outlier_ratio=0.3)
    co, gt = _dev(coords), _dev(poses)

    def fn(alloc):
        g = alloc.zeros(tuple(co.shape), dtype=torch.float32, device="cuda")
        loss, rec = shim.backward_rgb_batch(co, g, gt, 64, 10.0, synth.FOCAL, 360.0, 240.0, 1.0, 1.0, 100.0, 100.0, 100.0, 8, 5,
                                            image0=20, debug=True)
        return [loss, rec, g]
    _twice(monkeypatch, shim, fn, "backward_rgb_batch B=3")


def test_rgbd_solver_between_guard_bands(monkeypatch):
    """Forward at 5 x 7 with holes (21 valid cells: a partial wave), backward at 17 x 23 (391 cells) with B = 3, the quality rows
    at 7 x 9 (63 cells: less than a wave) - the smallest ragged cases of the three families' own tests."""
    sc = rc.rgbd_scene(7, 5, 7, noise=0.1, outlier_ratio=0.3, holes=0.4)
    co, cam = _dev(sc["coords"][None]), _dev(sc["cam"][None])

    def forward(alloc):
        poses = alloc.full((1, 4, 4), float("nan"), dtype=torch.float32, device="cuda")
        d = shim.forward_rgbd_batch(co, cam, poses, 3, 50.0, 100.0, 1000.0, image0=3, debug=True)
        return [poses] + [d[k] for k in ("cells", "tries", "scores", "dbg")]
    _twice(monkeypatch, shim, forward, "forward_rgbd_batch 5x7")

    scs = [rc.rgbd_scene(90 + b, 17, 23, noise=0.05, outlier_ratio=0.3, holes=0.2) for b in range(3)]
    for s in scs:
        s["gt"] = s["pose"].copy()
        s["gt"][:3, 3] += [0.3, -0.2, 0.4]
    bco, bcam, bgt = (_dev(np.stack([np.asarray(s[k], np.float32) for s in scs])) for k in ("coords", "cam", "gt"))

    def backward(alloc):
        g = alloc.zeros(tuple(bco.shape), dtype=torch.float32, device="cuda")
        loss, rec = shim.backward_rgbd_batch(bco, bcam, g, bgt, 64, 10.0, 1.0, 100.0, 1e6, 100.0, 100.0, 1305, image0=5,
                                             image_stride=2, debug=True)
        return [loss, rec, g]
    _twice(monkeypatch, shim, backward, "backward_rgbd_batch 17x23 B=3")

    bt = qc.batch(4021, 6, 7, 9, **qc.NOISY)
    qco, qcam, qpose = _dev(bt["coords"]), _dev(bt["cam"]), _dev(bt["pose"])
    _twice(monkeypatch, shim, lambda alloc: [shim.pose_quality_rgbd_batch(qco, qcam, qpose, qc.NOISY_THR, qc.ALPHA, qc.NOISY_MAX_DIST)],
           "pose_quality_rgbd_batch 7x9")


def test_pose_quality_batch_between_guard_bands(monkeypatch):
    coords, _, poses = synth.make_batch(2021, 3, noise=0.5, outlier_ratio=0.3, Ho=7, Wo=13)
    co, po = _dev(coords), _dev(poses)
    _twice(monkeypatch, shim, lambda alloc: [shim.pose_quality_batch(co, po, 10.0, synth.FOCAL, 52.0, 28.0, 100.0, 100.0, 8)],
           "pose_quality_batch 7x13")
