"""GPU: one rotation per frame in the batched augmentation (xl_data_batch_augment_frames) against the one-angle kernel it
shares its per-pixel code with, the pose rotation that goes with it (xl_data_rotate_poses) against the float64 product, the
collate path with rotate_poses on and off, the convention through the solver, and the end-to-end step and driver on
rotated frames."""
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import guarded                                                                                       # noqa: E402
from crossloc_amd import data, dataset, dsacstar, networks, optim, synth, train_e2e, training        # noqa: E402
from crossloc_amd.weights import seeded_state_dict                                                   # noqa: E402
from oracle import data_oracle as do                                                                 # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _guarded_again(monkeypatch, fn, want):
    """fn() once more with every tensor data.py allocates between guard bands: the same bits, every band intact."""
    torch.cuda.synchronize()
    guarded.guard_modules(monkeypatch, data)
    try:
        got = fn()
        assert guarded.handed_out() > 0
        assert len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
        guarded.assert_intact()
    finally:
        guarded.stop()


# ---------------------------------------------------------------------------------------------- the per-frame op

ANGLES = (0.0, -30.0, 12.345)


def _frames():
    g = torch.Generator().manual_seed(123)
    x = torch.randn(3, 3, 96, 144, generator=g)
    lab = torch.randn(3, 3, 12, 18, generator=g)
    lab[:, :, 2, 3] = -1.0
    return x.cuda(), lab.cuda()


@pytest.mark.parametrize("scale", [1.2345, 2 / 3])
def test_frame_b_is_the_one_angle_call_on_that_frame(monkeypatch, scale):
    x, lab = _frames()
    oh, ow = math.ceil(96 * scale), math.ceil(144 * scale)
    ch, cw = math.ceil(oh / 8), math.ceil(ow / 8)

    def fn():
        return [data.batch_augment(x, oh, ow, list(ANGLES), -1.0, True), data.batch_augment(lab, ch, cw, ANGLES, -1.0, False),
                data.batch_augment(x, oh, ow, [12.345] * 3, -1.0, True), data.batch_augment(lab, ch, cw, [-30.0] * 3, -1.0, False)]
    img, lb, img_eq, lb_eq = out = fn()
    assert img.shape == (3, 3, oh, ow) and lb.shape == (3, 3, ch, cw)
    for b, angle in enumerate(ANGLES):
        assert _same(img[b:b + 1], data.batch_augment(x[b:b + 1], oh, ow, angle, -1.0, True)), b
        assert _same(lb[b:b + 1], data.batch_augment(lab[b:b + 1], ch, cw, angle, -1.0, False)), b
    assert not torch.equal(img[1], data.batch_augment(x[1:2], oh, ow, 12.345, -1.0, True)[0])        # (the angles matter)
    assert _same(img_eq, data.batch_augment(x, oh, ow, 12.345, -1.0, True))
    assert _same(lb_eq, data.batch_augment(lab, ch, cw, -30.0, -1.0, False))
    with pytest.raises(RuntimeError):
        data.batch_augment(x, oh, ow, [1.0, 2.0], -1.0, True)
    with pytest.raises(RuntimeError):
        data.batch_augment(x.cpu(), oh, ow, list(ANGLES), -1.0, True)
    _guarded_again(monkeypatch, fn, out)


def test_more_frames_than_one_argument_pack(monkeypatch):
    """The rotation records ride in the kernel arguments, 64 frames per launch: 70 frames run as two launches."""
    x = torch.randn(70, 3, 16, 24, generator=torch.Generator().manual_seed(5)).cuda()
    angles = [-30.0 + 60.0 * b / 69 for b in range(70)]

    def fn():
        return [data.batch_augment(x, 20, 30, angles, -1.0, True), data.batch_augment(x, 13, 19, angles, -1.0, False)]
    img, lb = out = fn()
    for b in (0, 63, 64, 69):
        assert _same(img[b:b + 1], data.batch_augment(x[b:b + 1], 20, 30, angles[b], -1.0, True)), b
        assert _same(lb[b:b + 1], data.batch_augment(x[b:b + 1], 13, 19, angles[b], -1.0, False)), b
    _guarded_again(monkeypatch, fn, out)


# ---------------------------------------------------------------------------------------------- rotate_poses

POSE_ANGLES = (0.0, 30.0, -30.0, 12.345, 1e-3)


def _within_one_ulp(got, P, angles):
    """got float32 [B,4,4] against (P float32 -> float64) @ pose_rotation(angle) rounded to float32 once."""
    P = np.asarray(P, np.float32)
    want = np.stack([(P[b].astype(np.float64) @ data.pose_rotation(a)).astype(np.float32) for b, a in enumerate(angles)])
    assert got.dtype == np.float32 and got.shape == want.shape
    off = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (off <= np.spacing(np.abs(want)).astype(np.float64)).all(), off.max()
    return want


def test_rotate_poses_is_the_float64_product_rounded_once(monkeypatch):
    rng = np.random.default_rng(31)
    P = np.stack([synth.random_pose(rng) for _ in POSE_ANGLES]).astype(np.float32)
    dev = torch.from_numpy(P).cuda()
    got = data.rotate_poses(dev, POSE_ANGLES)
    assert got.is_cuda and got.dtype == torch.float32 and got.data_ptr() != dev.data_ptr()
    assert torch.equal(dev.cpu(), torch.from_numpy(P))                                   # the input is left alone
    g = got.cpu().numpy()
    _within_one_ulp(g, P, POSE_ANGLES)
    assert g[0].tobytes() == P[0].tobytes()                                              # angle 0: bit for bit
    assert g[:, 3, :].tobytes() == P[:, 3, :].tobytes() and g[:, :, 2:].tobytes() == P[:, :, 2:].tobytes()
    assert not np.array_equal(g[4, :3, :2], P[4, :3, :2])                                # 1e-3 degrees is not nothing
    # any strides: a transposed view and a slice of a wider tensor
    wide = torch.zeros(5, 4, 6, device="cuda")
    wide[:, :, 1:5] = dev
    assert _same(data.rotate_poses(wide[:, :, 1:5], POSE_ANGLES), got)
    t = dev.transpose(1, 2)
    assert not t.is_contiguous() and _same(data.rotate_poses(t, POSE_ANGLES), data.rotate_poses(t.contiguous(), POSE_ANGLES))
    with pytest.raises(RuntimeError):
        data.rotate_poses(dev.cpu(), POSE_ANGLES)
    with pytest.raises(RuntimeError):
        data.rotate_poses(dev, POSE_ANGLES[:4])
    many = dev.repeat(14, 1, 1)                                                          # 70 poses: two argument packs
    angles = [POSE_ANGLES[i % 5] for i in range(70)]
    assert _same(data.rotate_poses(many, angles), got.repeat(14, 1, 1))
    _guarded_again(monkeypatch, lambda: [data.rotate_poses(dev, POSE_ANGLES), data.rotate_poses(many, angles)],
                   [got, got.repeat(14, 1, 1)])


# ---------------------------------------------------------------------------------------------- the collate path

def test_collate_gpu_with_rotated_poses_follows_the_draws_frame_by_frame(tmp_path):
    """CamLocDataset(rotate_poses=True).collate_gpu against the oracle pipeline driven by the same `random` stream, each frame
    with its own angle."""
    root = dataset.write_synthetic_scene(str(tmp_path / "scene"), 3, seed=21)
    ds = dataset.CamLocDataset(root, augment=True, batch=True, rotate_poses=True)
    items = [ds[i] for i in range(3)]
    random.seed(11)
    images, poses, labels, focals, files = ds.collate_gpu(items)
    random.seed(11)
    jit = [data.draw_jitter(0.1, 0.1) for _ in items]
    scale = random.uniform(2 / 3, 3 / 2)
    angles = [random.uniform(-30, 30) for _ in items]
    assert len(set(angles)) == 3
    oh, ow = math.ceil(480 * scale), math.ceil(720 * scale)
    assert images.shape == (3, 3, oh, ow) and images.is_cuda and poses.is_cuda
    for i, it in enumerate(items):
        ref = torch.from_numpy(do.prepare_image(it[0].numpy(), 480, jit[i], data.MEAN, data.STD))[None]
        ref = do.batch_resize_images(ref, scale, angles[i])
        assert torch.allclose(images[i:i + 1].cpu(), ref, rtol=0, atol=2e-4)       # (test_data_gpu.py: the bilinear weights)
        rl = do.batch_resize_labels(it[2][None], math.ceil(oh / 8), math.ceil(ow / 8), angles[i])
        assert torch.equal(labels[i:i + 1].cpu(), rl)
    _within_one_ulp(poses.cpu().numpy(), np.stack([it[1].numpy() for it in items]), angles)
    assert focals.dtype == torch.float64 and np.allclose(focals.numpy(), 480.0 * scale)
    assert len(files) == 3


def test_collate_gpu_without_the_option_is_batch_resize_by_hand(tmp_path):
    root = dataset.write_synthetic_scene(str(tmp_path / "scene"), 3, seed=21)
    ds = dataset.CamLocDataset(root, augment=True, batch=True)
    items = [ds[i] for i in range(3)]
    random.seed(11)
    images, poses, labels, focals, files = ds.collate_gpu(items)
    after = random.getstate()
    random.seed(11)
    jit = [data.draw_jitter(0.1, 0.1) for _ in items]
    scale = random.uniform(2 / 3, 3 / 2)
    angle = random.uniform(-30, 30)
    assert random.getstate() == after
    frames = torch.stack([it[0] for it in items]).cuda()
    lab = torch.stack([it[2] for it in items]).cuda()
    ri, rl, rf = data.batch_resize(data.prepare_images(frames, 480, jitter=jit, normalize=True), lab, [it[3] for it in items],
                                   scale, angle)
    assert _same(images, ri) and _same(labels, rl)
    assert _same(poses.cpu(), torch.stack([it[1] for it in items]))
    assert torch.equal(focals, torch.tensor(rf, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------- the solver

def test_the_solver_finds_the_rotated_pose_on_rotated_coordinates():
    """Exact 60 x 90 coordinate maps rotated by the per-frame op: the solver's pose is the rotated pose, not the original one.
    |angle| / 4 tells the conventions apart (the error against the unrotated pose is then above 3 |angle| / 4); it is no
    accuracy claim."""
    angles = (20.0, -30.0, 20.0, -30.0)
    _, gt, P = synth.make_batch(100, 4, noise=0, outlier_ratio=0, Ho=60, Wo=90)
    rotated = data.batch_augment(torch.from_numpy(gt).cuda(), 60, 90, angles, -1.0, False)
    want = data.rotate_poses(torch.from_numpy(P.astype(np.float32)).cuda(), angles).cpu().numpy()
    out = torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda")
    dsacstar.forward_rgb_batch(rotated, out, 64, 10.0, 480.0, 360.0, 240.0, 100.0, 100.0, 8)
    got = out.cpu().numpy()
    for b, angle in enumerate(angles):
        t_err, r_err = synth.pose_error(want[b], got[b])
        print("frame %d: %.4f m, %.4f deg from the rotated pose; %.2f deg from the original" % (
            b, t_err, r_err, synth.pose_error(P[b], got[b])[1]))
        assert r_err < abs(angle) / 4
        assert synth.pose_error(P[b], got[b])[1] > 3 * abs(angle) / 4


# ---------------------------------------------------------------------------------------------- the step and the driver

B, H, W, SUB, HYP, FOCAL = 2, 64, 96, 8, 16, 60.0          # the batch of tests/test_e2e_step_gpu.py


def _net():
    net = networks.TransPoseNet(torch.tensor(synth.SCENE_MEAN, dtype=torch.float32), True, False, 0, 0, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=11))
    return net.cuda().train()


def _step(images, poses, gt, focals):
    opt = train_e2e._config_parser(["naturescape", "--network_in", "unused", "--uncertainty", "MLE", "--hypotheses", str(HYP),
                                    "--seed", "5"])
    net = _net()
    step = training.make_e2e_step(net, optim.Adam(net.parameters(), lr=1e-4), opt)
    loss, summary = step(images, poses, gt, focals, 4, image0=3)
    return loss, summary, [p.detach() for p in net.parameters()]


def test_step_on_rotated_frames():
    _, gt, poses = synth.make_batch(10, B, noise=0.5, outlier_ratio=0.0, Ho=H // SUB, Wo=W // SUB, focal=FOCAL)
    gt, poses = torch.from_numpy(gt).cuda(), torch.from_numpy(poses.astype(np.float32)).cuda()
    focals = torch.tensor([FOCAL, FOCAL * 1.01])
    images = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(2)).cuda()

    loss, summary, params = _step(images, poses, gt, focals)
    loss0, summary0, params0 = _step(images, data.rotate_poses(poses, [0, 0]), gt, focals)
    assert _same(loss, loss0) and _same(summary, summary0)
    assert all(_same(a, b) for a, b in zip(params, params0))

    ri, rl, rp, rf = data.batch_resize_posed(images, gt, poses, focals.tolist(), 1.0, (20.0, -20.0))
    assert ri.shape == images.shape and rl.shape == gt.shape and not torch.equal(rp, poses)
    loss, summary, params = _step(ri, rp, rl, torch.tensor(rf))
    assert torch.isfinite(loss).all() and all(torch.isfinite(p).all() for p in params)
    assert float(summary[1]) == B
    assert any(not torch.equal(a, b) for a, b in zip(params, params0))


def test_driver_trains_with_rotation(tmp_path):
    scene = tmp_path / "scene"
    dataset.write_synthetic_scene(str(scene / "train_sim"), 8)
    net = training.config_network("coord", True, False, "MLE", False, training.get_label_mean("naturescape", "coord"))
    net.load_state_dict(seeded_state_dict(net, seed=11))
    model = tmp_path / "init.net"
    torch.save(training.state_dict(net), model)
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "crossloc_amd.train_e2e", "naturescape", "--scene_dir", str(scene), "--real_data_chunk", "0.0",
           "--output_dir", str(out), "--network_in", str(model), "--tiny", "--uncertainty", "MLE", "--batch_size", "2",
           "--hypotheses", "16", "--learningrate", "1e-4", "--log_interval", "1", "--max_steps", "2", "--aug_rotation", "30"]
    env = dict(os.environ, XL_TRAIN_WORKERS="0", PYTHONPATH=ROOT)
    proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    with open(os.path.join(out, "output.log")) as f:
        log = f.read()
    assert "aug_rotation=30.0" in log
    lines = re.findall(r"Pose loss: (\S+), Accepted: (\d+)/(\d+),", log)
    assert len(lines) == 2
    for pose_loss, accepted, of in lines:
        assert np.isfinite(float(pose_loss)) and (int(accepted), int(of)) == (2, 2)
