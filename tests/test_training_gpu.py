"""GPU: the training entry points end to end on a synthetic on-disk scene at 480x720 - every task learns, checkpoints load
strictly, decoder fine-tuning keeps frozen encoders bitwise, and a resumed run continues bitwise."""
import os

import numpy as np
import pytest
import torch

from crossloc_amd import dataset, networks, training
from crossloc_amd import finetune_decoder_single_task as ft
from crossloc_amd import train_single_task as ts

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _workers(monkeypatch):
    monkeypatch.setenv("XL_TRAIN_WORKERS", "0")         # PNG decoding in the main process unless a test says otherwise


def write_scene(root, count=8, semantics=True):
    """A naturescape-like scene section with coord, depth and normal labels (and raw semantics maps)."""
    sec = os.path.join(root, "train_sim")
    dataset.write_synthetic_scene(sec, count, semantics=semantics)
    os.makedirs(os.path.join(sec, "depth"), exist_ok=True)
    os.makedirs(os.path.join(sec, "normal"), exist_ok=True)
    rng = np.random.default_rng(5)
    for name in sorted(os.listdir(os.path.join(sec, "init"))):
        stem = name[:-4]
        gt = torch.load(os.path.join(sec, "init", name)).numpy()             # [3, 60, 90], nodata -1
        pose = np.loadtxt(os.path.join(sec, "poses", stem + ".txt"))
        valid = (gt != -1).any(0)
        cam = np.linalg.inv(pose) @ np.concatenate([gt.reshape(3, -1), np.ones((1, gt[0].size))])
        depth = np.where(valid, np.abs(cam[2].reshape(gt.shape[1:])), -1).astype(np.float32)
        n = rng.normal(size=gt.shape) * 0.2 + np.array([0.0, 0.0, 1.0])[:, None, None]
        n = n / np.linalg.norm(n, axis=0, keepdims=True)
        normal = np.where(valid[None], n, -1).astype(np.float32)
        torch.save(torch.from_numpy(depth), os.path.join(sec, "depth", stem + ".dat"))
        torch.save(torch.from_numpy(normal), os.path.join(sec, "normal", stem + ".dat"))
    return root


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    return write_scene(str(tmp_path_factory.mktemp("scene")))


def _train(scene, out, task, steps, *extra):
    args = ["naturescape", "--task", task, "--scene_dir", scene, "--real_data_chunk", "0.0", "--output_dir", str(out),
            "--batch_size", "2", "--max_steps", str(steps), "--log_interval", "5"]
    if task == "semantics":
        args += ["--fullsize"]
    else:
        args += ["--uncertainty", "MLE"]
    return ts.main(args + list(extra))


@pytest.mark.parametrize("task", ["coord", "depth", "normal", "semantics"])
def test_twenty_steps_lower_the_loss_and_checkpoints_load(scene, tmp_path, task):
    tr = _train(scene, tmp_path, task, 20, "--learningrate", "1e-3")
    losses = [float(l) for l, _ in tr.recent]
    assert len(losses) == 20 and all(np.isfinite(losses))
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses
    for f in ("model.net", "resume.pt", "ckpt_iter_0000002.net"):
        assert os.path.exists(tmp_path / f), f
    assert not os.path.exists(tmp_path / "FLAG_training_done.nodata")      # stopped by --max_steps
    fresh = training.config_network(task, False, False, None if task == "semantics" else "MLE", task == "semantics",
                                    training.get_label_mean("naturescape", task))
    sd = torch.load(tmp_path / "model.net", map_location="cpu")
    fresh.load_state_dict(sd, strict=True)
    live = tr.network.state_dict()
    assert all(torch.equal(sd[k], live[k].cpu()) for k in sd)


def test_a_whole_run_writes_the_done_flag(scene, tmp_path):
    _train(scene, tmp_path, "coord", 100, "--epochs", "1")
    assert os.path.exists(tmp_path / "FLAG_training_done.nodata")


@pytest.fixture(scope="module")
def encoders(scene, tmp_path_factory):
    root = tmp_path_factory.mktemp("encoders")
    paths = {}
    for task in ("coord", "depth", "normal"):
        _train(scene, root / task, task, 2)
        paths[task] = str(root / task / "model.net")
    return paths


@pytest.mark.parametrize("reuse,unfreeze", [(False, False), (True, False), (True, True)])
def test_finetuning_keeps_frozen_encoders(scene, tmp_path, encoders, reuse, unfreeze, monkeypatch):
    captured = {}
    real = training.Trainer.run

    def run(self):                      # the network as the loop receives it, before the first step
        captured["before"] = {k: v.detach().cpu().clone() for k, v in self.network.state_dict().items()}
        return real(self)
    monkeypatch.setattr(training.Trainer, "run", run)
    args = ["naturescape", "--task", "coord", "--scene_dir", scene, "--real_data_chunk", "0.0", "--sim_data_chunk", "1.0",
            "--output_dir", str(tmp_path), "--batch_size", "2", "--max_steps", "5", "--uncertainty", "MLE",
            "--encoders", "coord", "depth", "normal", "--coord_weight", encoders["coord"], "--depth_weight",
            encoders["depth"], "--normal_weight", encoders["normal"], "--semantics_weight", encoders["normal"],
            "--learningrate", "1e-3"]
    args += ["--reuse_coord_encoder"] if reuse else []
    args += ["--unfreeze_coord_encoder"] if unfreeze else []
    tr = ft.main(args)
    before = captured["before"]
    after = {k: v.detach().cpu() for k, v in tr.network.state_dict().items()}
    coord = torch.load(encoders["coord"], map_location="cpu")
    for k, v in coord.items():
        if k.startswith("decoder."):
            assert torch.equal(before[k], v), k                        # decoder initialised from the coord checkpoint
    frozen = {n for n, p in tr.network.named_parameters() if not p.requires_grad}
    assert frozen
    for n in frozen:
        assert torch.equal(before[n], after[n]), n
    coord_enc = [k for k in after if k.startswith("mlr_encoder_1.")] if reuse else []
    changed = any(not torch.equal(before[k], after[k]) for k in coord_enc)
    assert changed == unfreeze
    assert any(not torch.equal(before[k], after[k]) for k in after if k.startswith("decoder.fc3"))


def _adam_state(tr):
    st = tr.optimizer.state
    return [(st[p]["exp_avg"].cpu(), st[p]["exp_avg_sq"].cpu(), st[p]["step"]) for p in tr.network.parameters()
            if p in st]


@pytest.mark.parametrize("workers", [0, 2])
def test_resume_continues_bitwise(scene, tmp_path, workers, monkeypatch):
    """--auto_resume as every reference script passes it: the first run starts fresh, the second continues from the
    output folder.  workers = 2: PNG decoding in DataLoader workers (collate_host, pin_memory, to_gpu in the loop)."""
    monkeypatch.setenv("XL_TRAIN_WORKERS", str(workers))
    straight = _train(scene, tmp_path / "a", "coord", 6)
    first = _train(scene, tmp_path / "b", "coord", 3, "--auto_resume")
    assert first.state["steps"] == 3
    resumed = _train(scene, tmp_path / "b", "coord", 6, "--auto_resume")
    assert resumed.state["steps"] == 6 and resumed.state["iteration"] == straight.state["iteration"]
    a, b = straight.network.state_dict(), resumed.network.state_dict()
    diff = [k for k in a if not torch.equal(a[k].cpu(), b[k].cpu())]
    assert not diff, diff
    for (m1, v1, s1), (m2, v2, s2) in zip(_adam_state(straight), _adam_state(resumed)):
        assert torch.equal(m1, m2) and torch.equal(v1, v2) and s1 == s2
    assert [float(l) for l, _ in straight.recent][3:] == [float(l) for l, _ in resumed.recent]


def test_gradient_buffer_holds_every_gradient():
    torch.manual_seed(0)
    net = training.config_network("coord", False, False, "MLE", False, torch.zeros(3)).cuda().train()
    x = torch.rand(1, 3, 64, 96, device="cuda")
    net(x).sum().backward()
    flat = networks.gradient_buffer(net)
    for p in net.parameters():
        g = p.grad
        assert g.untyped_storage().data_ptr() == flat.data_ptr()
    before = [p.grad.clone() for p in net.parameters()]
    flat.mul_(2)
    assert all(torch.equal(p.grad, 2 * b) for p, b in zip(net.parameters(), before))
    p0 = next(net.parameters())
    p0.grad = p0.grad.clone()
    with pytest.raises(RuntimeError):
        networks.gradient_buffer(net)


def test_rccl_average_on_a_one_rank_group():
    """The device path of the gradient all-reduce (ReduceOp.AVG through RCCL) on a one-rank group."""
    import socket
    import torch.distributed as dist
    if dist.is_initialized():
        pytest.skip("a default process group already exists in this process")
    with socket.socket() as sck:
        sck.bind(("127.0.0.1", 0))
        port = sck.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        torch.manual_seed(0)
        net = training.config_network("coord", False, False, "MLE", False, torch.zeros(3)).cuda().train()
        net(torch.rand(1, 3, 64, 96, device="cuda")).sum().backward()
        before = [p.grad.clone() for p in net.parameters()]
        training.allreduce_flat_gradients(net, 1, dist.group.WORLD)
        torch.cuda.synchronize()
        assert all(torch.equal(p.grad, b) for p, b in zip(net.parameters(), before))
    finally:
        dist.destroy_process_group()


def test_step_at_the_largest_augmentation_scale():
    """3/2 of a 480x720 frame: the conv1 weight gradient stages 1082-pixel rows (68 KiB of LDS)."""
    from crossloc_amd import optim, synth
    torch.manual_seed(0)
    net = training.config_network("coord", False, False, "MLE", False, torch.zeros(3)).cuda().train()
    opt = optim.Adam(net.parameters(), lr=1e-4)
    step = training.make_step(net, "coord", opt, "MLE", -1)
    images = torch.rand(1, 3, 720, 1080, device="cuda")
    _, gt, poses = synth.make_batch(1, 1, noise=0.5, outlier_ratio=0.0)
    gt = torch.nn.functional.interpolate(torch.from_numpy(gt), size=(90, 135), mode="nearest").cuda()
    w0 = net.encoder.conv1.weight.detach().clone()
    loss, rate = step(images, torch.from_numpy(poses.astype(np.float32)).cuda(), gt, synth.FOCAL * 1.5)
    assert np.isfinite(float(loss))
    assert not torch.equal(w0, net.encoder.conv1.weight.detach())


def test_output_gradient_form_equals_the_autograd_losses():
    """loss.task_loss_and_output_gradient (the step's form: the network output read in place, one gradient tensor) against
    the split + autograd functions the reference calls, bit for bit."""
    from crossloc_amd import loss as L
    from crossloc_amd import synth
    g = torch.Generator().manual_seed(3)
    B, H, W = 2, 60, 90
    _, gt, poses = synth.make_batch(5, B, noise=0.5, outlier_ratio=0.0)
    gt, poses = torch.from_numpy(gt).cuda(), torch.from_numpy(poses.astype(np.float32)).cuda()
    grid, cam = L.get_pixel_grid(8), L.get_cam_mat(720, 480, synth.FOCAL)
    cases = {
        "coord": (3, lambda a, u: L.scene_coords_regression_loss(0.1, 100, 1000, 50, "MLE", grid, -1, cam, a, u, poses, gt)),
        "depth": (1, lambda a, u: L.depth_regression_loss(0.1, 1000, "MLE", -1, a, u, gt[:, 2:3].abs())),
        "normal": (2, lambda a, u: L.normal_regression_loss(1000, "MLE", -1, a, u, gt / gt.norm(dim=1, keepdim=True))),
    }
    for task, (nt, fn) in cases.items():
        base = torch.randn(B, nt + 1, H, W, generator=g) * (100 if task == "coord" else 1)
        if task == "coord":
            base[:, :3] += gt.cpu()
        base[:, nt] = base[:, nt].abs() + 0.5
        x = base.cuda().requires_grad_(True)
        a, u = torch.split(x, [nt, 1], 1)
        ref_loss, ref_rate = fn(a, u)
        ref_loss.backward()
        labels = {"coord": gt, "depth": gt[:, 2:3].abs(), "normal": gt / gt.norm(dim=1, keepdim=True)}[task]
        loss, rate, grad = L.task_loss_and_output_gradient(task, "MLE", base.cuda(), nt, labels, poses, grid, cam, -1,
                                                           0.1, 100, 1000, 50)
        assert torch.equal(loss, ref_loss.detach()) and torch.equal(rate, ref_rate), task
        assert torch.equal(grad, x.grad), task
    logits = torch.randn(B, 6, 32, 48, generator=g).cuda().requires_grad_(True)
    lab = torch.randint(0, 6, (B, 1, 32, 48), generator=g).float().cuda()
    ref_loss, ref_rate = L.semantics_classification_loss(None, logits, None, lab, L.CrossEntropyLoss2d(), 'mean')
    ref_loss.backward()
    loss, rate, grad = L.task_loss_and_output_gradient("semantics", None, logits.detach(), 6, lab)
    assert torch.equal(loss, ref_loss.detach()) and torch.equal(rate, ref_rate) and torch.equal(grad, logits.grad)
