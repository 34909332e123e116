"""GPU parity of the pose-quality pass: xl_dsac_pose_quality_batch (through dsacstar.pose_quality_batch) against the serial
C restatement tests/pose_quality_ref.c.  Every comparison is bitwise on all 64 doubles of a row (NaNs by position): the two
sides compile the same header, so this checks the kernel's orchestration - the cell walk, the strides, the butterfly and
wave order - and that gcc and hipcc agree.  The formulas themselves: tests/test_pose_quality_cpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pose_quality_cases as qc
import pose_quality_ref
from crossloc_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def qref(tmp_path_factory):
    return pose_quality_ref.load(tmp_path_factory.mktemp("pose_quality_ref"))


def _rows(coords, poses, args, focals=None):
    """coords: torch CUDA [B,3,Ho,Wo] (any strides) or numpy; poses numpy / torch [B,4,4] -> numpy [B,64]"""
    import dsacstar
    if not isinstance(coords, torch.Tensor):
        coords = torch.from_numpy(np.ascontiguousarray(coords)).cuda()
    if not isinstance(poses, torch.Tensor):
        poses = torch.from_numpy(np.ascontiguousarray(poses, np.float32)).cuda()
    out = dsacstar.pose_quality_batch(coords, poses, *args, focals=focals)
    torch.cuda.synchronize()
    assert out.dtype == torch.float64 and tuple(out.shape) == (coords.shape[0], 64)
    return out.cpu().numpy()


def _args(ppx, ppy, focal=synth.FOCAL, thr=qc.THR, max_reproj=qc.MAX_REPROJ):
    return (thr, focal, ppx, ppy, qc.ALPHA, max_reproj, qc.SUB)


def _assert_rows(qref, got, coords, poses, args, frames, what):
    for b in frames:
        want = qref.row(coords[b], poses[b], *args)
        assert qc.same_bits(got[b], want), (what, b, np.flatnonzero(got[b] != want))


@pytest.mark.parametrize("Ho,Wo", [(60, 90), (37, 53), (7, 9), (129, 128)])
def test_rows_bit_exact_at_grid_sizes(qref, Ho, Wo):
    """5400 cells; 1961 (no multiple of 64); 63 (less than a wave, most threads idle); 16512 (above the solver's limit:
    ground-truth poses only).  Frames 0, 2 and 5 of a batch of 6, at the pose forward_rgb_batch wrote and at ground truth."""
    import dsacstar
    B, frames = 6, (0, 2, 5)
    coords, _, gt = synth.make_batch(2021, B, noise=0.5, outlier_ratio=0.3, Ho=Ho, Wo=Wo)
    ppx, ppy = Wo * qc.SUB / 2.0, Ho * qc.SUB / 2.0
    args = _args(ppx, ppy)
    gt32 = gt.astype(np.float32)
    got = _rows(coords, gt32, args)
    _assert_rows(qref, got, coords, gt32, args, frames, "ground truth")
    assert (got[:, 0] == Ho * Wo).all() and (got[:, 6] == 0).all()
    assert (got[:, 1] > 0.55 * Ho * Wo).all() and (got[:, 1] < 0.8 * Ho * Wo).all()       # ~70 % inliers
    if Ho * Wo > 16384:
        return
    co = torch.from_numpy(coords).cuda()
    est = torch.zeros((B, 4, 4), dtype=torch.float32, device="cuda")
    dbg = dsacstar.forward_rgb_batch(co, est, 64, qc.THR, synth.FOCAL, ppx, ppy, qc.ALPHA, qc.MAX_REPROJ, qc.SUB, debug=True)
    got = _rows(co, est, args)
    est_np = est.cpu().numpy()
    _assert_rows(qref, got, coords, est_np, args, frames, "solver pose")
    if Ho * Wo >= 1000:
        # the refinement's last inlier count belongs to the pose before its last step, and the row re-reads the pose from
        # float32: the counts agree to a few cells, not exactly
        assert np.abs(got[:, 1] - dbg["dbg"][:, 2].cpu().numpy()).max() <= 0.01 * Ho * Wo
        assert (got[:, 6] == 0).all() and (got[:, 8] < 1.0).all() and (got[:, 9] < 0.5).all()


@pytest.fixture(scope="module")
def one_batch():
    coords, _, gt = synth.make_batch(3100, 6, noise=0.5, outlier_ratio=0.3, Ho=37, Wo=53)
    args = _args(53 * qc.SUB / 2.0, 37 * qc.SUB / 2.0)
    return coords, gt.astype(np.float32), args, _rows(coords, gt.astype(np.float32), args)


def test_strided_inputs_give_the_bits_of_the_contiguous_copy(qref, one_batch):
    coords, poses, args, base = one_batch
    _assert_rows(qref, base, coords, poses, args, range(6), "contiguous")
    co = torch.from_numpy(coords).cuda()
    B, _, Ho, Wo = co.shape
    pred = torch.randn((B, 4, Ho, Wo), device="cuda")
    pred[:, :3] = co
    view = pred[:, :3]                                                   # the network output's coordinate channels
    assert not view.is_contiguous()
    assert qc.same_bits(_rows(view, poses, args), base)
    cl = co.contiguous(memory_format=torch.channels_last)
    assert cl.stride(1) == 1 and not cl.is_contiguous()
    assert qc.same_bits(_rows(cl, poses, args), base)
    wide = torch.full((B, 3, Ho + 3, Wo + 11), float("nan"), device="cuda")
    wide[:, :, 2:2 + Ho, 5:5 + Wo] = co
    pitched = wide[:, :, 2:2 + Ho, 5:5 + Wo]                             # padded row pitch
    assert pitched.stride(2) == Wo + 11
    assert qc.same_bits(_rows(pitched, poses, args), base)


def test_slot_independence(one_batch):
    coords, poses, args, base = one_batch
    alone = _rows(coords[3:4], poses[3:4], args)
    assert qc.same_bits(alone[0], base[3])
    first = np.concatenate([coords[3:4], coords[:3], coords[4:]])
    got = _rows(first, np.concatenate([poses[3:4], poses[:3], poses[4:]]), args)
    assert qc.same_bits(got[0], base[3]) and qc.same_bits(got[1], base[0])
    last = np.concatenate([coords[:3], coords[4:], coords[3:4]])
    got = _rows(last, np.concatenate([poses[:3], poses[4:], poses[3:4]]), args)
    assert qc.same_bits(got[5], base[3]) and qc.same_bits(got[4], base[5])


def test_per_image_focals_match_the_scalar_form(qref):
    scenes = [synth.make_scene(40 + i, noise=0.5, outlier_ratio=0.3, Ho=20, Wo=30, focal=f)
              for i, f in enumerate((480.0, 455.5, 512.25))]
    coords = np.stack([s["coords"] for s in scenes])
    poses = np.stack([s["pose"] for s in scenes]).astype(np.float32)
    focals = torch.tensor([s["focal"] for s in scenes])
    got = _rows(coords, poses, _args(120.0, 80.0, focal=1.0), focals=focals)              # the scalar is ignored
    for b, s in enumerate(scenes):
        args = _args(120.0, 80.0, focal=s["focal"])
        assert qc.same_bits(got[b], _rows(coords[b:b + 1], poses[b:b + 1], args)[0])
        assert qc.same_bits(got[b], qref.row(coords[b], poses[b], *args))
    assert (got[:, 6] == 0).all() and len(set(got[:, 7])) == 3


@pytest.mark.parametrize("Ho,Wo", [(12, 16), (200, 4)])
def test_status_cases(qref, Ho, Wo):
    for name, coords, pose, args, status, n_inl in qc.status_cases(Ho, Wo):
        got = _rows(coords[None], pose[None], args)[0]
        assert got[6] == status and (n_inl is None or got[1] == n_inl), (name, got[6], got[1])
        qc.assert_nan_pattern(got, status)
        assert qc.same_bits(got, qref.row(coords, pose, *args)), name


class _PlantNet(torch.nn.Module):
    """Stand-in for the network in the wiring tests: the solver's input is given by the caller (`scene_coords`)."""
    num_task_channel = 3
    OUTPUT_SUBSAMPLE = qc.SUB

    def forward(self, images, plan_slot=0):
        return torch.zeros((images.shape[0], 4, 60, 90), device=images.device)


def test_localize_batch_and_pipelined_localizer_wiring():
    import dsacstar
    from crossloc_amd import evaluation
    coords, _, _ = synth.make_batch(5200, 4, noise=0.5, outlier_ratio=0.3)
    co = torch.from_numpy(coords).cuda()
    images = torch.zeros((4, 3, 480, 720), device="cuda")
    net = _PlantNet()
    args = _args(360.0, 240.0)
    plain = evaluation.localize_batch(net, images, 64, synth.FOCAL, 480, 720, image0=3, scene_coords=co)
    assert len(plain) == 2
    out = evaluation.localize_batch(net, images, 64, synth.FOCAL, 480, 720, image0=3, scene_coords=co, quality=True)
    assert len(out) == 3
    torch.cuda.synchronize()
    assert torch.equal(out[0], plain[0])                                 # the poses are what they were
    sep = dsacstar.pose_quality_batch(co, out[0], *args)
    torch.cuda.synchronize()
    assert qc.same_bits(out[2].cpu().numpy(), sep.cpu().numpy()) and (out[2][:, 6] == 0).all()

    loc = evaluation.PipelinedLocalizer(net, 64, synth.FOCAL, 480, 720)
    p_plain = loc.submit(images, image0=3, scene_coords=co)
    p_out = loc.submit(images, image0=3, scene_coords=co, quality=True)
    loc.finish()
    torch.cuda.synchronize()
    assert len(p_plain) == 2 and len(p_out) == 3
    assert torch.equal(p_plain[0], plain[0]) and torch.equal(p_out[0], plain[0])
    assert qc.same_bits(p_out[2].cpu().numpy(), sep.cpu().numpy())


def test_single_task_driver_writes_rows_and_prints_the_table(tmp_path):
    """crossloc_amd.pose_quality_single_task runs test_single_task.main() itself: same frames, same report, plus the table and
    the rows; test_single_task without it prints no table."""
    out = tmp_path / "quality.npy"
    common = ["--synthetic", "16", "--batch", "8"]

    def run(module, extra):
        res = subprocess.run([sys.executable, "-m", module] + common + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        return res.stdout

    with_q = run("crossloc_amd.pose_quality_single_task", ["--pose_quality", "--quality_out", str(out)])
    plain = run("crossloc_amd.test_single_task", [])
    assert "Selective accuracy" in with_q and "Selective accuracy" not in plain
    report = plain[plain.index("Accuracy:"):].strip()
    assert "Median Error" in report and report in with_q                 # the usual report, character for character
    assert with_q.index(report) < with_q.index("Selective accuracy")
    rows = np.load(out)
    assert rows.shape == (16, 64) and rows.dtype == np.float64 and np.isfinite(rows).all()
    assert (rows[:, 0] == 5400).all() and (rows[:, 6] == 0).all() and (rows[:, 8] < 1.0).all()
