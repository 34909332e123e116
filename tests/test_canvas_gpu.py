"""GPU: the fixed-size augmentation - xl_data_canvas_augment against its host restatement (tests/canvas_ref.py) bit for bit and
against the per-frame rotation kernel at scale 1, data.batch_canvas, the geometry through the solver, the coord loss with one
focal length per frame (xl_loss_coord_frames_ld) against single-frame calls of the existing entry, and the training steps in
canvas mode.  Every call of the new entry points runs once more with its tensors between guard bands."""
import math
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import canvas_ref                                                                                    # noqa: E402
import guarded                                                                                       # noqa: E402
from crossloc_amd import data, dataset, dsacstar, loss as xl_loss, networks, optim, synth, train_e2e, training   # noqa: E402
from crossloc_amd import train_single_task as ts                                                     # noqa: E402
from crossloc_amd.weights import seeded_state_dict                                                   # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _guarded_again(monkeypatch, fn, want, *modules):
    """fn() once more with every tensor the modules (default: data.py) allocate between guard bands: the same bits, every
    band intact."""
    torch.cuda.synchronize()
    guarded.guard_modules(monkeypatch, *(modules or (data,)))
    try:
        got = fn()
        assert guarded.handed_out() > 0
        assert len(got) == len(want) and all(_same(g, w) for g, w in zip(got, want))
        guarded.assert_intact()
    finally:
        guarded.stop()


# ---------------------------------------------------------------------------------------------- the kernel

SCALES = (1.0, 2 / 3, 1.2345)
ANGLES = (0.0, -30.0, 12.345)


def _frames():
    g = torch.Generator().manual_seed(123)
    x = torch.randn(3, 3, 96, 144, generator=g)
    lab = torch.randn(3, 3, 12, 18, generator=g)
    lab[:, :, 2, 3] = -1.0
    return x, lab


def _against_restatement(x, scales, angles, fill, bilinear):
    got = data.canvas_augment(x.cuda(), scales, angles, fill, bilinear)
    want = canvas_ref.canvas_augment(x.numpy(), scales, angles, fill, bilinear)
    assert got.shape == x.shape and got.dtype == torch.float32 and got.is_cuda
    g = got.cpu().numpy()
    assert g.tobytes() == want.tobytes(), "%d of %d values differ, max %.3g" % (
        (g != want).sum(), g.size, np.abs(g.astype(np.float64) - want).max())
    return got


def test_kernel_is_the_restatement_bit_for_bit(monkeypatch):
    x, lab = _frames()
    img = _against_restatement(x, SCALES, ANGLES, -1.0, True)
    lb = _against_restatement(lab, SCALES, ANGLES, -1.0, False)
    assert (img[1] == -1.0).any() and (lb[1] == -1.0).any() and not _same(img[2], x[2].cuda())
    g = torch.Generator().manual_seed(9)
    odd, deep = torch.randn(2, 1, 7, 11, generator=g), torch.randn(1, 6, 5, 9, generator=g)     # odd sizes: the centre on a half pixel
    outs = [img, lb]
    for bilinear in (True, False):
        outs.append(_against_restatement(odd, (1.5, 0.8), (20.0, -7.5), 0.0, bilinear))
        outs.append(_against_restatement(deep, (0.75,), (-30.0,), -1.0, bilinear))
    # the other pairings of the scales and angles, the pure zooms and the pure rotations among them
    for s in SCALES + (1.5,):
        _against_restatement(x, (s,) * 3, ANGLES, -1.0, True)
        _against_restatement(lab, (s,) * 3, ANGLES, -1.0, False)

    def fn():
        r = [data.canvas_augment(x.cuda(), SCALES, ANGLES, -1.0, True), data.canvas_augment(lab.cuda(), SCALES, ANGLES, -1.0, False)]
        for bilinear in (True, False):
            r.append(data.canvas_augment(odd.cuda(), (1.5, 0.8), (20.0, -7.5), 0.0, bilinear))
            r.append(data.canvas_augment(deep.cuda(), (0.75,), (-30.0,), -1.0, bilinear))
        return r
    _guarded_again(monkeypatch, fn, outs)


def test_wrong_counts_and_host_tensors_are_refused():
    x = torch.randn(3, 1, 8, 12)
    with pytest.raises(RuntimeError):
        data.canvas_augment(x, SCALES, ANGLES, -1.0, True)                   # a host tensor
    with pytest.raises(RuntimeError):
        data.canvas_augment(x.cuda(), SCALES[:2], ANGLES, -1.0, True)
    with pytest.raises(RuntimeError):
        data.canvas_augment(x.cuda(), SCALES, ANGLES + (1.0,), -1.0, False)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            data.canvas_augment(x.cuda(), (1.0, bad, 1.0), ANGLES, -1.0, False)


def test_nearest_mode_at_scale_one_is_the_per_frame_rotation(monkeypatch):
    _, lab = _frames()
    lab = lab.cuda()
    x = torch.randn(3, 2, 20, 30, generator=torch.Generator().manual_seed(2)).cuda()

    def fn():
        return [data.canvas_augment(lab, (1.0,) * 3, ANGLES, -1.0, False), data.canvas_augment(x, (1.0,) * 3, ANGLES, 0.0, False)]
    a, b = out = fn()
    for i, angle in enumerate(ANGLES):
        assert _same(a[i:i + 1], data.batch_augment(lab[i:i + 1], 12, 18, angle, -1.0, False)), i
        assert _same(b[i:i + 1], data.batch_augment(x[i:i + 1], 20, 30, angle, 0.0, False)), i
    assert _same(a, data.batch_augment(lab, 12, 18, list(ANGLES), -1.0, False))
    _guarded_again(monkeypatch, fn, out)


def test_identity_returns_the_input_bits(monkeypatch):
    x, lab = _frames()
    x, lab = x.cuda(), lab.cuda()
    x[0, 0, 0, 0], x[1, 1, 5, 7], lab[2, 0, 1, 1] = -0.0, float("nan"), float("inf")       # bits, not values

    def fn():
        return [data.canvas_augment(x, (1.0,) * 3, (0.0,) * 3, -1.0, True), data.canvas_augment(lab, (1.0,) * 3, (0.0,) * 3, -1.0, False),
                data.canvas_augment(x, (1.0, 1.2, 1.0), (0.0, 0.0, 5.0), -1.0, True)]
    a, b, c = out = fn()
    assert _same(a, x) and _same(b, lab) and a.data_ptr() != x.data_ptr()
    assert _same(c[0], x[0]) and not _same(c[1], x[1]) and not _same(c[2], x[2])        # the branch is per frame
    _guarded_again(monkeypatch, fn, out)


def test_frame_b_of_a_batch_is_the_single_frame_call(monkeypatch):
    x, lab = _frames()
    x, lab = x.cuda(), lab.cuda()
    img, lb = data.canvas_augment(x, SCALES, ANGLES, -1.0, True), data.canvas_augment(lab, SCALES, ANGLES, -1.0, False)

    def singles():
        return ([data.canvas_augment(x[b:b + 1], SCALES[b:b + 1], ANGLES[b:b + 1], -1.0, True) for b in range(3)]
                + [data.canvas_augment(lab[b:b + 1], SCALES[b:b + 1], ANGLES[b:b + 1], -1.0, False) for b in range(3)])
    out = singles()
    for b in range(3):
        assert _same(img[b:b + 1], out[b]) and _same(lb[b:b + 1], out[3 + b]), b
    _guarded_again(monkeypatch, singles, out)
    assert not _same(img[1:2], data.canvas_augment(x[1:2], SCALES[2:3], ANGLES[1:2], -1.0, True))    # (the scales matter)


def test_more_frames_than_one_argument_pack(monkeypatch):
    """The records ride in the kernel arguments, 64 frames per launch: 70 frames run as two launches."""
    x = torch.randn(70, 3, 16, 24, generator=torch.Generator().manual_seed(5)).cuda()
    scales = [2 / 3 + (3 / 2 - 2 / 3) * b / 69 for b in range(70)]
    angles = [-30.0 + 60.0 * b / 69 for b in range(70)]
    assert len(set(zip(scales, angles))) == 70

    def fn():
        return [data.canvas_augment(x, scales, angles, -1.0, True), data.canvas_augment(x, scales, angles, -1.0, False)]
    img, lb = out = fn()
    for b in (0, 1, 35, 63, 64, 65, 69):
        assert _same(img[b:b + 1], data.canvas_augment(x[b:b + 1], scales[b:b + 1], angles[b:b + 1], -1.0, True)), b
        assert _same(lb[b:b + 1], data.canvas_augment(x[b:b + 1], scales[b:b + 1], angles[b:b + 1], -1.0, False)), b
    _guarded_again(monkeypatch, fn, out)


# ---------------------------------------------------------------------------------------------- batch_canvas

def test_batch_canvas(monkeypatch):
    g = torch.Generator().manual_seed(8)
    images = torch.randn(3, 3, 64, 96, generator=g).cuda()
    coord = torch.randn(3, 3, 8, 12, generator=g).cuda()
    depth = torch.rand(3, 1, 8, 12, generator=g).cuda()
    sem = torch.randint(0, 6, (3, 1, 64, 96), generator=g).float().cuda()
    rng = np.random.default_rng(31)
    poses = torch.from_numpy(np.stack([synth.random_pose(rng) for _ in range(3)]).astype(np.float32)).cuda()
    focals = [60.0, 61.5, 59.25]
    scales, angles = [1.25, 0.7, 1.0], [10.0, -25.0, 0.0]

    def fn():
        im, lb, ps, fo = data.batch_canvas(images, coord, poses, focals, scales, angles)
        _, d, _, _ = data.batch_canvas(images, {"coord": coord, "depth": depth, "other": None}, poses, focals, scales, angles)
        _, s, _, _ = data.batch_canvas(images, sem, poses, focals, scales, angles, semantics=True)
        assert fo == [f * s_ for f, s_ in zip(focals, scales)] and d["other"] == 0
        return [im, lb, ps, d["coord"], d["depth"], s]
    im, lb, ps, dc, dd, s = out = fn()
    assert im.shape == images.shape and lb.shape == coord.shape and dd.shape == depth.shape and s.shape == sem.shape
    assert _same(im, data.canvas_augment(images, scales, angles, -1.0, True))
    assert _same(lb, data.canvas_augment(coord, scales, angles, -1.0, False)) and _same(dc, lb)
    assert _same(dd, data.canvas_augment(depth, scales, angles, -1.0, False))
    assert _same(ps, data.rotate_poses(poses, angles))
    assert _same(s, data.canvas_augment(sem, scales, angles, 0.0, False))
    assert (s[1] == 0).all(0).any() and not (s == -1).any() and (lb[1] == -1).all(0).any()       # fill 0 / fill -1
    assert _same(im[2], images[2]) and _same(ps[2], poses[2])
    with pytest.raises(RuntimeError):
        data.batch_canvas(images, coord, poses, focals[:2], scales, angles)
    _guarded_again(monkeypatch, fn, out)


# ---------------------------------------------------------------------------------------------- the solver

def test_the_solver_finds_the_rotated_pose_under_the_scaled_focal(monkeypatch):
    """Exact 60 x 90 coordinate maps warped by (1.3, 20 degrees): with focal f sigma the solver's pose is P Rz(theta); with
    focal f it is not.  Thresholds: tests/test_pose_rotation_gpu.py tells its conventions apart at |angle| / 4 on cells that
    nearest resampling displaced by up to half a cell; here the displacement is sigma times that, hence sigma |angle| / 4.
    A wrong focal length shows in the translation: a camera that looks down from d metres and images the scene at focal
    f sigma is, to a solver told f, a camera at about d / sigma - off by d (1 - 1 / sigma) along the optical axis.  Half of
    that at the SMALLEST depth of the frame tells the two apart; neither is an accuracy claim."""
    sigma, angle, B = 1.3, 20.0, 3
    _, gt, P = synth.make_batch(100, B, noise=0, outlier_ratio=0, Ho=60, Wo=90)
    gt_dev, P_dev = torch.from_numpy(gt).cuda(), torch.from_numpy(P.astype(np.float32)).cuda()
    warped = data.canvas_augment(gt_dev, [sigma] * B, [angle] * B, -1.0, False)
    rotated = data.rotate_poses(P_dev, [angle] * B)
    _guarded_again(monkeypatch, lambda: [data.canvas_augment(gt_dev, [sigma] * B, [angle] * B, -1.0, False),
                                         data.rotate_poses(P_dev, [angle] * B)], [warped, rotated])
    want = rotated.cpu().numpy()

    def solve(focal):
        out = torch.zeros((B, 4, 4), dtype=torch.float32, device="cuda")
        dsacstar.forward_rgb_batch(warped, out, 64, 10.0, focal, 360.0, 240.0, 100.0, 100.0, 8)
        return out.cpu().numpy()
    right, wrong = solve(synth.FOCAL * sigma), solve(synth.FOCAL)
    for b in range(B):
        hit = (gt[b] != synth.NODATA).all(0)
        depth = np.einsum("c,chw->hw", P[b][:3, 2], gt[b].astype(np.float64) - P[b][:3, 3][:, None, None])[hit]
        far = 0.5 * depth.min() * (1 - 1 / sigma)
        t_ok, r_ok = synth.pose_error(want[b], right[b])
        t_bad, r_bad = synth.pose_error(want[b], wrong[b])
        print("frame %d: %.3f m, %.3f deg with f sigma; %.3f m, %.3f deg with f (far: %.1f m); %.2f deg from the original pose" % (
            b, t_ok, r_ok, t_bad, r_bad, far, synth.pose_error(P[b], right[b])[1]))
        assert r_ok < sigma * abs(angle) / 4 and t_ok < far
        assert synth.pose_error(P[b], right[b])[1] > 3 * abs(angle) / 4
        assert t_bad > far


# ---------------------------------------------------------------------------------------------- the loss

LOSS_ARGS = (0.1, 100.0, 1000.0, 50.0)          # min_depth, soft_clamp, hard_clamp, init_tolerance


def _loss_batch(Ho, Wo, focals):
    """Three frames, each a scene seen at its own focal length; predictions 3 m off, 10 % outliers, an uncertainty channel."""
    sc = [synth.make_scene(700 + b, noise=3.0, outlier_ratio=0.1, Ho=Ho, Wo=Wo, focal=f) for b, f in enumerate(focals)]
    unc = np.exp(np.random.default_rng(1).uniform(-2, 3, size=(len(sc), 1, Ho, Wo))).astype(np.float32)
    return (torch.from_numpy(np.stack([s["coords"] for s in sc])).cuda(), torch.from_numpy(unc).cuda(),
            torch.from_numpy(np.stack([s["pose"] for s in sc]).astype(np.float32)).cuda(),
            torch.from_numpy(np.stack([s["gt_coords"] for s in sc])).cuda())


# kT = 256 cells per workgroup (csrc/xl_loss.hip): 8 x 12 is part of one tile, 23 x 37 = 851 is three tiles and 83 cells
@pytest.mark.parametrize("mode", ["MLE", None])
@pytest.mark.parametrize("Ho,Wo", [(8, 12), (23, 37)])
def test_coord_loss_with_one_focal_length_per_frame(monkeypatch, Ho, Wo, mode):
    H, W = Ho * 8, Wo * 8
    f0 = 0.625 * W                                                   # the field of view of the 480 x 720 camera at focal 450
    focals = [f0, f0 * 0.8, f0 * 1.3]
    pred, unc, poses, gt = _loss_batch(Ho, Wo, focals)
    grid = xl_loss.get_pixel_grid(8)

    def call(p, u, ps, g, reduction, focal=f0, per_frame=None):
        p, u = p.clone().requires_grad_(True), u.clone().requires_grad_(True)
        loss, rate = xl_loss.scene_coords_regression_loss(*LOSS_ARGS, mode, grid, -1, xl_loss.get_cam_mat(W, H, focal), p, u, ps, g,
                                                          reduction=reduction, focals=per_frame)
        loss.sum().backward()
        return [loss.detach(), rate, p.grad] + ([u.grad] if mode else [])

    # per-image losses and gradients: three single-frame calls of the existing function, each with its frame's cam_mat
    got = call(pred, unc, poses, gt, None, focal=1.0, per_frame=focals)
    for b, f in enumerate(focals):
        one = call(pred[b:b + 1], unc[b:b + 1], poses[b:b + 1], gt[b:b + 1], None, focal=f)
        assert float(one[1]) > 0                                                    # (valid cells: the reprojection term counts)
        assert _same(got[0][b:b + 1], one[0]), b
        for a, o in zip(got[2:], one[2:]):
            assert _same(a[b:b + 1], o), b
    assert not _same(got[0], call(pred, unc, poses, gt, None, focal=f0)[0])         # (the focal lengths matter)
    # a tensor of focal lengths, float64 as the dataset returns them, is the list
    assert all(_same(a, o) for a, o in zip(got, call(pred, unc, poses, gt, None, focal=1.0,
                                                     per_frame=torch.tensor(focals, dtype=torch.float64))))

    # all focal lengths equal: the existing call, for both reductions and for the step's form
    for reduction in ("mean", None):
        old, new = call(pred, unc, poses, gt, reduction), call(pred, unc, poses, gt, reduction, focal=7.0, per_frame=[f0] * 3)
        assert all(_same(a, o) for a, o in zip(new, old)), reduction
    out = torch.cat([pred, unc], 1) if mode else pred.clone()
    cam = xl_loss.get_cam_mat(W, H, f0)
    old = xl_loss.task_loss_and_output_gradient("coord", mode, out, 3, gt, poses, grid, cam)
    new = xl_loss.task_loss_and_output_gradient("coord", mode, out, 3, gt, poses, grid, cam, focals=[f0] * 3)
    assert all(_same(a, o) for a, o in zip(new, old))
    step = xl_loss.task_loss_and_output_gradient("coord", mode, out, 3, gt, poses, grid, cam, focals=focals)
    mean = call(pred, unc, poses, gt, "mean", focal=1.0, per_frame=focals)
    assert _same(step[0], mean[0]) and _same(step[1], mean[1]) and _same(step[2][:, :3], mean[2])
    if mode:
        assert _same(step[2][:, 3:], mean[3])

    # the mean over the batch: float64 finalisation, one rounding - against the float64 mean of the rounded per-image values
    want = got[0].double().mean().item()
    ulp = float(np.spacing(np.float32(abs(want))))
    print("mean loss %.9g, float64 mean of the per-image losses %.9g, %.3f ulp apart" % (
        mean[0].item(), want, abs(mean[0].item() - want) / ulp))
    assert abs(mean[0].item() - want) <= 2 * ulp

    with pytest.raises(RuntimeError):
        call(pred, unc, poses, gt, None, per_frame=focals[:2])
    with pytest.raises(RuntimeError):
        xl_loss.task_loss_and_output_gradient("coord", mode, out, 3, gt, poses, grid, cam, focals=focals + [1.0])
    _guarded_again(monkeypatch, lambda: call(pred, unc, poses, gt, None, focal=1.0, per_frame=focals)
                   + list(xl_loss.task_loss_and_output_gradient("coord", mode, out, 3, gt, poses, grid, cam, focals=focals)),
                   got + list(step), xl_loss)


# ---------------------------------------------------------------------------------------------- the steps

H, W, SUB, FOCAL = 64, 96, 8, 60.0          # the frame of tests/test_e2e_step_gpu.py


def _net():
    net = networks.TransPoseNet(torch.tensor(synth.SCENE_MEAN, dtype=torch.float32), True, False, 0, 0, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=11))
    return net.cuda().train()


def _small_scene(root, count):
    """write_synthetic_scene's files with the labels of a 64 x 96 camera: 8 x 12 coordinate maps and their poses, and the
    calibration of the stored 480 x 720 frame that makes the focal length of the 64 x 96 frame FOCAL."""
    import os
    dataset.write_synthetic_scene(root, count)
    for i in range(count):
        sc = synth.make_scene(40 + i, noise=0.0, outlier_ratio=0.0, Ho=H // SUB, Wo=W // SUB, focal=FOCAL)
        name = "frame_%05d" % i
        np.savetxt(os.path.join(root, "poses", name + ".txt"), sc["pose"])
        np.savetxt(os.path.join(root, "calibration", name + ".txt"), [FOCAL * synth.IMAGE_H / H])
        torch.save(torch.from_numpy(sc["gt_coords"]), os.path.join(root, "init", name + ".dat"))
    return root


def test_training_steps_in_canvas_mode_keep_one_size_and_hand_over_every_focal_length(tmp_path, monkeypatch):
    monkeypatch.setenv("XL_TRAIN_WORKERS", "0")
    root = _small_scene(str(tmp_path / "scene"), 6)
    ds = dataset.CamLocDataset(root, augment=True, canvas=True, image_height=H)
    opt = ts._config_parser(["naturescape", "--task", "coord", "--uncertainty", "MLE", "--tiny", "--batch_size", "2", "--max_steps", "3",
                             "--log_interval", "1", "--learningrate", "1e-4", "--aug_canvas"])
    net, hand = _net(), _net()
    out = str(tmp_path / "out")
    import os
    os.makedirs(out)
    tr = training.Trainer(net, ds, "coord", opt, out, out, torch.device("cuda"), num_workers=0)
    real, seen, direct = tr.step_fn, [], []
    grid = xl_loss.get_pixel_grid(SUB)

    def spy(images, gt_poses, gt_labels, focal_length):
        seen.append((tuple(images.shape), tuple(gt_labels.shape), focal_length))
        if len(seen) == 1:                                   # the same weights, the same batch: the loss called directly
            pred = hand(images).detach().contiguous()
            direct.append(xl_loss.task_loss_and_output_gradient(
                "coord", "MLE", pred, 3, gt_labels, gt_poses, grid, xl_loss.get_cam_mat(W, H, 1.0), -1, opt.mindepth, opt.softclamp,
                opt.hardclamp, opt.inittolerance, focals=focal_length)[0].clone())
            one = xl_loss.task_loss_and_output_gradient(
                "coord", "MLE", pred, 3, gt_labels, gt_poses, grid, xl_loss.get_cam_mat(W, H, float(focal_length[0])), -1,
                opt.mindepth, opt.softclamp, opt.hardclamp, opt.inittolerance)[0]
            direct.append(one.clone())
        return real(images, gt_poses, gt_labels, focal_length)
    tr.step_fn = spy
    random.seed(3)
    tr.run()
    assert len(seen) == 3 and len(tr.recent) == 3
    for shape, lshape, focal in seen:
        assert shape == (2, 3, H, W) and lshape == (2, 3, H // SUB, W // SUB)
        assert isinstance(focal, torch.Tensor) and focal.shape == (2,) and focal.dtype == torch.float64
        ratio = (focal / FOCAL).tolist()
        assert all(2 / 3 - 1e-9 <= r <= 3 / 2 + 1e-9 for r in ratio) and ratio[0] != ratio[1]
    losses = [l for l, _ in tr.recent]
    assert all(torch.isfinite(l) for l in losses)
    assert _same(losses[0], direct[0]) and not _same(losses[0], direct[1])     # each frame's own focal, not the first frame's

    # the frame path of a batch and the loss on it, once more between guard bands
    items = [ds[i] for i in (0, 1)]

    def fn():
        random.seed(29)
        images, poses, labels, focals, _ = ds.collate_gpu(items)
        pred = torch.cat([labels + 0.5, torch.ones_like(labels[:, :1])], 1)
        loss, rate, grad = xl_loss.task_loss_and_output_gradient("coord", "MLE", pred, 3, labels, poses, grid,
                                                                 xl_loss.get_cam_mat(W, H, 1.0), focals=focals)
        return [images, poses, labels, focals, loss, rate, grad]
    want = fn()
    assert want[0].shape == (2, 3, H, W) and want[3].shape == (2,)
    _guarded_again(monkeypatch, fn, want, data, xl_loss)


class _FixedOutput(torch.nn.Module):
    """Stands in for the network in a step: its 'output' is a parameter, so a step runs on chosen coordinates."""
    OUTPUT_SUBSAMPLE, num_task_channel = SUB, 3

    def __init__(self, out):
        super().__init__()
        self.out = torch.nn.Parameter(out.clone())

    def forward(self, images):
        return self.out * 1.0


@pytest.mark.parametrize("init_weight", [0.0, 0.5])
def test_one_rgbd_end_to_end_step_in_canvas_mode(tmp_path, monkeypatch, init_weight):
    """--mode rgbd --aug_canvas on coordinates 0.5 m off the truth (the setting of tests/test_e2e_step_gpu.py) at 60 x 90: the
    grid stays 60 x 90 at the drawn scales, the frames are accepted, the gradient is not zero, and the --init_weight coord
    term reads each frame's own focal length."""
    B = 2
    opt = train_e2e._config_parser(["naturescape", "--network_in", "unused", "--uncertainty", "MLE", "--hypotheses", "16", "--seed", "5",
                                    "--mode", "rgbd", "--aug_canvas", "--aug_rotation", "30", "--init_weight", str(init_weight)])
    (tmp_path / "rgb").mkdir()
    ds = dataset.CamLocDataset(str(tmp_path), augment=True, **train_e2e.dataset_options(opt))
    random.seed(17)
    scales, angles = ds.draw_geometry(B)
    assert all(2 / 3 <= s <= 3 / 2 and s != 1 for s in scales) and all(-30 <= a <= 30 and a != 0 for a in angles)

    coords, gt, poses = synth.make_batch(10, B, noise=0.5, outlier_ratio=0.0, Ho=60, Wo=90)
    z = np.einsum("bc,bchw->bhw", poses[:, :3, 2], gt.astype(np.float64) - poses[:, :3, 3][:, :, None, None])
    depth = np.where((gt != synth.NODATA).all(1), z, synth.NODATA).astype(np.float32)[:, None]
    unc = np.random.default_rng(1).uniform(0.5, 2.0, size=(B, 1, 60, 90)).astype(np.float32)
    images = torch.zeros(B, 3, synth.IMAGE_H, synth.IMAGE_W, device="cuda")
    labels = {"coord": torch.from_numpy(gt).cuda(), "depth": torch.from_numpy(depth).cuda()}
    raw, poses_dev = (images, labels), torch.from_numpy(poses.astype(np.float32)).cuda()
    images, labels, gt_poses, focals = data.batch_canvas(images, labels, poses_dev, [synth.FOCAL] * B, scales, angles)
    if init_weight == 0.0:

        def again():
            im, lb, ps, _ = data.batch_canvas(*raw, poses_dev, [synth.FOCAL] * B, scales, angles)
            return [im, lb["coord"], lb["depth"], ps]
        _guarded_again(monkeypatch, again, [images, labels["coord"], labels["depth"], gt_poses])
    assert labels["coord"].shape == (B, 3, 60, 90) and labels["depth"].shape == (B, 1, 60, 90)
    assert 60 * 90 <= dsacstar.RGBD_MAX_CELLS and images.shape == (B, 3, synth.IMAGE_H, synth.IMAGE_W)
    pred = torch.cat([data.canvas_augment(torch.from_numpy(coords).cuda(), scales, angles, -1.0, False),
                      torch.from_numpy(unc).cuda()], 1)

    net = _FixedOutput(pred).cuda()
    step = training.make_e2e_step(net, torch.optim.SGD(net.parameters(), lr=1.0), opt)
    loss, summary = step(images, gt_poses, labels, torch.tensor(focals, dtype=torch.float64), 4, image0=3)
    assert torch.isfinite(loss) and float(summary[1]) == B, summary.tolist()
    delta = pred - net.out.detach()                               # lr 1: the gradient the step applied
    assert torch.isfinite(delta).all() and delta[:, :3].any()

    grad, beta = None, 0.0
    if init_weight:
        _, _, grad = xl_loss.task_loss_and_output_gradient(
            "coord", "MLE", pred, 3, labels["coord"], gt_poses, xl_loss.get_pixel_grid(SUB),
            xl_loss.get_cam_mat(synth.IMAGE_W, synth.IMAGE_H, 1.0), -1, opt.mindepth, opt.softclamp, opt.hardclamp,
            opt.inittolerance, focals=focals)
        beta = init_weight
    ref_loss, ref_stats, ref = xl_loss.expected_pose_loss_and_output_gradient(
        pred, gt_poses, torch.tensor(focals), synth.IMAGE_H, synth.IMAGE_W, opt.hypotheses, opt.threshold, opt.inlieralpha,
        opt.maxpixelerror, opt.weightrot, opt.weighttrans, opt.softclamp, opt.seed + 4, image0=3, clip_norm=opt.clip_norm,
        grad=grad, beta=beta, depth=labels["depth"][:, 0].clamp_min(0.0), rgbd_threshold=opt.threshold,
        max_dist_error=opt.maxpixelerror, subsample=SUB)
    assert _same(loss, ref_loss) and _same(summary, ref_stats[B])
    assert torch.equal(net.out.detach(), pred - ref)
    if init_weight:
        assert delta[:, 3].any()                                  # the coord term reaches the uncertainty channel
