"""GPU: data-parallel training through the entry point - two ranks sharing cuda:0 (the driver's XL_TRAIN_SHARED_GPU mode:
gloo reduces a host copy of the flat gradient buffer), per-rank batch 2, 3 steps - against one process that runs the same
two half-batches, sums their flat gradients, halves the sum and takes the Adam step.  With two ranks (a + b) / 2 is the
same float operation both ways: the result must match bit for bit."""
import os
import random
import signal
import socket
import subprocess
import sys

import pytest
import torch

from crossloc_amd import dataset as xl_dataset
from crossloc_amd import loss as xl_loss
from crossloc_amd import networks, optim, training

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_training_gpu import write_scene  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _replay(scene, steps, batch, world):
    training.set_random_seed(2021)
    net = training.config_network("coord", False, False, "MLE", False,
                                  training.get_label_mean("naturescape", "coord")).cuda().train()
    ds = xl_dataset.CamLocDataset([os.path.join(scene, "train_sim")], coord=True, augment=True)
    opt = optim.Adam(net.parameters(), lr=2e-4)
    grid = xl_loss.get_pixel_grid(8)
    per_epoch = len(training.epoch_batches(len(ds), 0, batch, 0, world))
    for s in range(steps):
        epoch, b = divmod(s, per_epoch)
        state, flats = random.getstate(), []
        for rank in range(world):
            random.setstate(state)                       # every rank draws the same augmentation parameters
            idx = training.epoch_batches(len(ds), epoch, batch, rank, world)[b]
            images, poses, gt, focals, _ = ds.collate_gpu([ds[i] for i in idx])
            pred = net(images)
            sc, unc = torch.split(pred, [3, 1], dim=1)
            cam = xl_loss.get_cam_mat(images.size(3), images.size(2), float(focals[0]))
            loss, _ = xl_loss.scene_coords_regression_loss(0.1, 100, 1000, 50.0, "MLE", grid, -1, cam, sc, unc, poses, gt)
            loss.backward()
            flats.append(networks.gradient_buffer(net).cpu())
            if rank < world - 1:
                net.zero_grad(set_to_none=True)
        networks.gradient_buffer(net).copy_((flats[0] + flats[1]) / 2)
        opt.step()
        opt.zero_grad(set_to_none=True)
    return net, opt


def test_two_ranks_on_one_gpu_equal_the_one_process_step(tmp_path):
    scene = write_scene(str(tmp_path / "scene"), count=8, semantics=False)
    with socket.socket() as sck:
        sck.bind(("127.0.0.1", 0))
        port = sck.getsockname()[1]
    env = dict(os.environ, XL_TRAIN_SHARED_GPU="1", XL_TRAIN_WORKERS="0")
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", "crossloc_amd.train_single_task", "naturescape", "--task", "coord",
           "--scene_dir", scene, "--real_data_chunk", "0.0", "--uncertainty", "MLE", "--batch_size", "2",
           "--max_steps", "3", "--output_dir", str(out), "--no_lr_scheduling"]
    # own process group: on a time-out the ranks go with the launcher instead of staying on the device
    proc = subprocess.Popen(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                            start_new_session=True)
    try:
        _, err = proc.communicate(timeout=600)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.communicate()
        raise
    assert proc.returncode == 0, err[-4000:]
    net, opt = _replay(scene, 3, 2, 2)
    got = torch.load(out / "model.net", map_location="cpu")
    ref = net.state_dict()
    diff = [k for k in got if not torch.equal(got[k], ref[k].cpu())]
    assert not diff, diff
    res = torch.load(out / "resume.pt", map_location="cpu", weights_only=False)
    assert res["state"]["steps"] == 3 and res["state"]["iteration"] == 12
    mine = opt.state_dict()["state"]
    for i, st in res["optimizer"]["state"].items():
        assert torch.equal(st["exp_avg"].cpu(), mine[i]["exp_avg"].cpu()) and torch.equal(
            st["exp_avg_sq"].cpu(), mine[i]["exp_avg_sq"].cpu()), i
