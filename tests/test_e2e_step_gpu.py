"""GPU: the chain of end-to-end DSAC* training from the solver to the parameters - the output-gradient form against its
parts, one make_e2e_step step against the same step driven by hand, and the train_e2e.py driver with resume."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from crossloc_amd import dataset, dsacstar, loss as xl_loss, networks, optim, synth, train_e2e, training     # noqa: E402
from crossloc_amd.weights import seeded_state_dict                                                           # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN = torch.tensor(synth.SCENE_MEAN, dtype=torch.float32)
B, H, W, SUB, HYP, FOCAL = 2, 64, 96, 8, 16, 60.0
SOLVER = dict(hypotheses=HYP, threshold=10.0, inlier_alpha=100.0, max_pixel_error=100.0, weight_rot=1.0, weight_trans=100.0,
              soft_clamp=100.0)


@pytest.fixture(scope="module")
def batch():
    """Two frames on the 8 x 12 grid: a 4-channel 'network output' (coordinates 0.5 m off the truth + an uncertainty channel),
    labels, poses, per-frame focal lengths and the depth of the true points along the optical axis."""
    coords, gt, poses = synth.make_batch(10, B, noise=0.5, outlier_ratio=0.0, Ho=H // SUB, Wo=W // SUB, focal=FOCAL)
    assert (gt != synth.NODATA).all()
    unc = np.random.default_rng(1).uniform(0.5, 2.0, size=(B, 1, H // SUB, W // SUB)).astype(np.float32)
    z = np.einsum("bc,bchw->bhw", poses[:, :3, 2], gt.astype(np.float64) - poses[:, :3, 3][:, :, None, None])
    return dict(pred=torch.from_numpy(np.concatenate([coords, unc], 1)).cuda(), gt=torch.from_numpy(gt).cuda(),
                poses=torch.from_numpy(poses.astype(np.float32)).cuda(), focals=torch.tensor([FOCAL, FOCAL * 1.01]),
                depth=torch.from_numpy(z.astype(np.float32)).cuda())


def _pose_form(batch, **kw):
    args = dict(SOLVER, seed=5, image0=3)
    args.update(kw)
    return xl_loss.expected_pose_loss_and_output_gradient(batch["pred"], batch["poses"], batch["focals"], H, W, **args)


def test_output_gradient_is_the_solver_followed_by_the_op(batch):
    mean_loss, stats, grad = _pose_form(batch, clip_norm=0.5)
    g = torch.zeros(B, 3, H // SUB, W // SUB, device="cuda")
    losses = dsacstar.backward_rgb_batch(batch["pred"][:, :3], g, batch["poses"], HYP, 10.0, 0.0, W / 2, H / 2, 1.0, 100.0,
                                         100.0, 100.0, 100.0, SUB, 5, image0=3, focals=batch["focals"],
                                         max_tries=xl_loss.E2E_MAX_TRIES)
    ref_grad, ref_stats = xl_loss.finish_pose_gradient(g, losses, 4, 1.0, 0.5)
    assert torch.equal(grad, ref_grad) and torch.equal(stats, ref_stats)
    assert grad.shape == batch["pred"].shape and not grad[:, 3].any() and grad[:, :3].any()
    assert torch.isfinite(losses).all() and stats[B, 1] == B
    assert mean_loss.dim() == 0 and mean_loss.is_cuda and float(mean_loss) == float((losses[0] + losses[1]) / 2)
    assert torch.equal(stats[:B, 0], losses)


def test_solver_reads_the_strided_view_like_a_contiguous_copy(batch):
    _, stats, _ = _pose_form(batch)
    g = torch.zeros(B, 3, H // SUB, W // SUB, device="cuda")
    direct = dsacstar.backward_rgb_batch(batch["pred"][:, :3].contiguous(), g, batch["poses"], HYP, 10.0, 0.0, W / 2, H / 2, 1.0,
                                         100.0, 100.0, 100.0, 100.0, SUB, 5, image0=3, focals=batch["focals"],
                                         max_tries=xl_loss.E2E_MAX_TRIES)
    assert torch.equal(stats[:B, 0], direct)
    # the keys of the call are image0 + b: the same frames keyed through image_keys
    _, stats_k, _ = _pose_form(batch, image_keys=[3, 4])
    assert torch.equal(stats_k, stats)
    _, stats_o, _ = _pose_form(batch, image0=4)
    assert not torch.equal(stats_o[:B, 0], stats[:B, 0])
    with pytest.raises(ValueError):
        _pose_form(batch, image_keys=[3, 9, 4])


def test_joint_mode_adds_the_pose_gradient_onto_the_weighted_coord_gradient(batch):
    grid, cam = xl_loss.get_pixel_grid(SUB), xl_loss.get_cam_mat(W, H, FOCAL)
    _, _, cg = xl_loss.task_loss_and_output_gradient("coord", "MLE", batch["pred"], 3, batch["gt"], batch["poses"], grid, cam)
    _, _, pg = _pose_form(batch)
    _, _, grad = _pose_form(batch, grad=cg.clone(), beta=0.5)
    assert cg[:, 3].any()
    assert torch.equal(grad[:, 3], 0.5 * cg[:, 3])
    assert torch.equal(grad[:, :3], 0.5 * cg[:, :3] + pg[:, :3])


def test_rgbd_form_is_the_rgbd_solver_followed_by_the_op(batch):
    mean_loss, stats, grad = _pose_form(batch, depth=batch["depth"], rgbd_threshold=10.0, max_dist_error=100.0)
    g = torch.zeros(B, 3, H // SUB, W // SUB, device="cuda")
    losses = dsacstar.backward_rgbd_batch(batch["pred"][:, :3], None, g, batch["poses"], HYP, 10.0, 1.0, 100.0, 100.0, 100.0,
                                          100.0, 5, image0=3, max_tries=xl_loss.E2E_MAX_TRIES, depth=batch["depth"],
                                          ppointX=W / 2, ppointY=H / 2, subSampling=SUB, focals=batch["focals"])
    ref_grad, ref_stats = xl_loss.finish_pose_gradient(g, losses, 4)
    assert torch.equal(grad, ref_grad) and torch.equal(stats, ref_stats)
    assert torch.isfinite(losses).all() and stats[B, 1] == B and grad[:, :3].any()
    _, stats_rgb, _ = _pose_form(batch)
    assert not torch.equal(stats_rgb[:B, 0], losses)                    # (it is the other solver)


def _net():
    net = networks.TransPoseNet(MEAN, True, False, 0, 0, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=11))
    return net.cuda().train()


@pytest.mark.parametrize("init_weight", [0.0, 0.5])
def test_one_step_equals_the_step_driven_by_hand(batch, init_weight):
    opt = train_e2e._config_parser(["naturescape", "--network_in", "unused", "--uncertainty", "MLE", "--hypotheses", str(HYP),
                                    "--seed", "5", "--init_weight", str(init_weight)])
    images = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(2)).cuda()
    net, hand = _net(), _net()
    before = [p.detach().clone() for p in net.parameters()]
    step = training.make_e2e_step(net, optim.Adam(net.parameters(), lr=1e-4), opt)
    loss, summary = step(images, batch["poses"], batch["gt"], batch["focals"], 4, image0=3)

    adam = optim.Adam(hand.parameters(), lr=1e-4)
    pred = hand(images)
    grad, beta = None, 0.0
    if init_weight:
        grid, cam = xl_loss.get_pixel_grid(SUB), xl_loss.get_cam_mat(W, H, float(batch["focals"][0]))
        _, _, grad = xl_loss.task_loss_and_output_gradient("coord", "MLE", pred, 3, batch["gt"], batch["poses"], grid, cam)
        beta = init_weight
    ref_loss, ref_stats, grad = xl_loss.expected_pose_loss_and_output_gradient(
        pred, batch["poses"], batch["focals"], H, W, seed=5 + 4, image0=3, grad=grad, beta=beta, **SOLVER)
    pred.backward(grad)
    adam.step()

    assert torch.equal(loss, ref_loss) and torch.equal(summary, ref_stats[B])
    assert summary.is_cuda and summary.shape == (4,)
    for a, b in zip(net.parameters(), hand.parameters()):
        assert torch.equal(a, b)
    assert any(not torch.equal(a, b) for a, b in zip(net.parameters(), before))
    if init_weight == 0.0:
        assert float(summary[1]) == B, "a rejected frame: the pose gradient of this step is not exercised"


# ---------------------------------------------------------------------------------------------------------- the driver
def _driver(scene, out, model, steps, *extra):
    cmd = [sys.executable, "-m", "crossloc_amd.train_e2e", "naturescape", "--scene_dir", str(scene), "--real_data_chunk", "0.0",
           "--output_dir", str(out), "--network_in", str(model), "--tiny", "--uncertainty", "MLE", "--batch_size", "2",
           "--hypotheses", "16", "--learningrate", "1e-4", "--log_interval", "1", "--max_steps", str(steps), *extra]
    env = dict(os.environ, XL_TRAIN_WORKERS="0", PYTHONPATH=ROOT)
    proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    with open(os.path.join(out, "output.log")) as f:
        return re.findall(r"Pose loss: (\S+), Accepted: (\d+)/(\d+), Max norm: (\S+), Clipped: (\d+)", f.read())


def test_driver_trains_resumes_bitwise_and_logs_accepted_frames(tmp_path):
    scene = tmp_path / "scene"
    dataset.write_synthetic_scene(str(scene / "train_sim"), 8)
    net = training.config_network("coord", True, False, "MLE", False, training.get_label_mean("naturescape", "coord"))
    net.load_state_dict(seeded_state_dict(net, seed=11))
    model = tmp_path / "init.net"
    torch.save(training.state_dict(net), model)

    lines = _driver(scene, tmp_path / "a", model, 3, "--auto_resume")
    assert len(lines) == 3
    for pose_loss, accepted, of, max_norm, clipped in lines:
        assert np.isfinite(float(pose_loss)) and np.isfinite(float(max_norm))
        assert (int(accepted), int(of), int(clipped)) == (2, 2, 0)
    for f in ("model.net", "resume.pt"):
        assert os.path.exists(tmp_path / "a" / f), f
    three = torch.load(tmp_path / "a" / "model.net", map_location="cpu")
    init = torch.load(model, map_location="cpu")
    assert any(not torch.equal(three[k], init[k]) for k in init)

    assert len(_driver(scene, tmp_path / "a", model, 5, "--auto_resume")) == 5          # the log is appended to: 3 + 2 lines
    assert len(_driver(scene, tmp_path / "b", model, 5)) == 5
    resumed = torch.load(tmp_path / "a" / "model.net", map_location="cpu")
    straight = torch.load(tmp_path / "b" / "model.net", map_location="cpu")
    assert list(resumed) == list(straight)
    diff = [k for k in straight if not torch.equal(resumed[k], straight[k])]
    assert not diff, diff
    assert any(not torch.equal(resumed[k], three[k]) for k in three)
