"""GPU: the fused per-image evaluation metrics (csrc/xl_metrics.hip, include/crossloc_metrics.h) and what is built on them in
crossloc_amd/evaluation.py and crossloc_amd/eval_single_task.py, against the values recorded from the reference's own
functions (tests/golden/eval_metrics.npz) and the float64 restatement of tests/eval_refs.py (pinned to the same fixture by
tests/test_eval_metrics_cpu.py).

Bounds.  Semantics counts are integers: exact; derived metrics 1e-12.  Depth and normal against the reference's float64
result: 1e-10 relative (depth), 1e-8 degrees (normal) - with float64 per-cell arithmetic only the rounding of the device's
exp / sin / cos / acos remains, which acos amplifies by at most 1/sin(theta) ~ 2.2e3 at the cosine clamp (~1e-12 rad).  Against
the reference's fp32 result: |ours - ref32| <= |ref32 - ref64| + that bound (not further from the reference than the reference
is from the truth).  Every figure is printed before it is asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import eval_inputs                                              # noqa: E402
import eval_refs                                                # noqa: E402

from crossloc_amd import evaluation                             # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(HERE, "golden", "eval_metrics.npz"))
NT = {"depth": 1, "normal": 2, "semantics": 6}
DEPTH_REL, NORMAL_DEG = 1e-10, 1e-8
_cache = {}


def _inputs(task, tag):
    """(network-shaped output [B,nt+1,H,W], label) of a case, generated once per session and never modified"""
    if (task, tag) not in _cache:
        fn = {"depth": eval_inputs.depth_inputs, "normal": eval_inputs.normal_inputs, "semantics": eval_inputs.semantics_case}[task]
        _cache[(task, tag)] = fn(tag)
    return _cache[(task, tag)]


def _rows(task, out, gt, **kw):
    """rows of the kernels, read through the strided [:, :nt] view of the [B,nt+1,H,W] tensor"""
    t = torch.from_numpy(np.ascontiguousarray(out)).cuda()
    view = t[:, :NT[task]]
    assert not view.is_contiguous() or t.shape[0] == 1
    return evaluation.task_metric_rows(task, view, torch.from_numpy(np.ascontiguousarray(gt)).cuda(), -1, **kw)


def _hold(name, ours, ref64, ref32, bound, relative):
    ours, ref64, ref32 = (np.asarray(v, np.float64) for v in (ours, ref64, ref32))
    tol = bound * (np.abs(ref64) if relative else 1.0)                           # relative bounds as |a - b| <= bound * |b|
    d64, d32, own = np.abs(ours - ref64), np.abs(ours - ref32), np.abs(ref32 - ref64)
    print("%s: |ours-ref64| %s  |ours-ref32| %s  |ref32-ref64| %s  allowed %s (%.0e%s)" % (
        name, d64, d32, own, tol, bound, " relative" if relative else " deg"))
    assert np.all(d64 <= tol), (name, d64, tol)
    assert np.all(d32 <= own + tol), (name, d32, own, tol)


def _hold64(name, ours, ref, bound, relative):
    ours, ref = np.asarray(ours, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(ours), np.isnan(ref)), (name, ours, ref)
    ok = ~np.isnan(ref)
    d = np.abs(ours - ref)[ok]
    tol = bound * (np.abs(ref)[ok] if relative else np.ones(d.shape))
    print("%s: |ours-ref64| max %.3e, largest share of the allowance %.3g (bound %.0e%s)" % (
        name, d.max() if d.size else 0.0, (d / np.maximum(tol, 1e-300)).max() if d.size else 0.0, bound,
        " relative" if relative else " deg"))
    assert np.all(d <= tol), (name, d, tol)


@pytest.mark.parametrize("tag", list(eval_inputs.CASES))
def test_depth_rows_match_the_reference(tag):
    out, gt = _inputs("depth", tag)
    rows = _rows("depth", out, gt).cpu().numpy()
    ref = eval_refs.depth_rows(out[:, :1], gt)
    assert rows.dtype == np.float64 and rows.shape == ref.shape
    assert np.array_equal(rows[:, 2], ref[:, 2])                                  # valid-cell counts: exact
    assert np.array_equal(rows[eval_inputs.EMPTY_IMAGE], np.zeros(3))
    s = rows.sum(0)
    _hold(tag + " depth [abs_rel, rms]", [s[0] / s[2], np.sqrt(s[1] / s[2])], GOLD[tag + "_depth64"], GOLD[tag + "_depth32"],
          DEPTH_REL, True)
    _hold64(tag + " depth per image", np.stack(evaluation.group_metrics("depth", rows, 1), 1), GOLD[tag + "_depth64_img"],
            DEPTH_REL, True)
    _hold64(tag + " depth per group of 4", np.stack(evaluation.group_metrics("depth", rows, 4), 1), GOLD[tag + "_depth64_grp"],
            DEPTH_REL, True)
    _hold64(tag + " depth sums vs restatement", rows[:, :2], ref[:, :2], DEPTH_REL, True)


@pytest.mark.parametrize("tag", list(eval_inputs.CASES))
def test_normal_rows_match_the_reference(tag):
    out, gt = _inputs("normal", tag)
    rows = _rows("normal", out, gt).cpu().numpy()
    ref = eval_refs.normal_rows(out[:, :2], gt)
    assert rows.dtype == np.float64 and rows.shape == ref.shape
    assert np.array_equal(rows[:, 1], ref[:, 1])
    assert np.array_equal(rows[eval_inputs.EMPTY_IMAGE], np.zeros(2))
    s = rows.sum(0)
    _hold(tag + " normal mean angle", s[0] / s[1], GOLD[tag + "_normal64"], GOLD[tag + "_normal32"], NORMAL_DEG, False)
    _hold64(tag + " normal per image", evaluation.group_metrics("normal", rows, 1), GOLD[tag + "_normal64_img"], NORMAL_DEG, False)
    _hold64(tag + " normal per group of 4", evaluation.group_metrics("normal", rows, 4), GOLD[tag + "_normal64_grp"],
            NORMAL_DEG, False)


@pytest.mark.parametrize("tag", list(eval_inputs.SEM_CASES))
def test_semantics_counts_and_class_map(tag):
    out, lab, (tb, tc, tcls) = _inputs("semantics", tag)
    B, _, H, W = out.shape
    cmap = torch.full((B, H, W), 99, dtype=torch.uint8, device="cuda")
    t = torch.from_numpy(out).cuda()
    rows = evaluation.task_metric_rows("semantics", t[:, :6], torch.from_numpy(lab).cuda(), class_map=cmap)
    assert rows.dtype == torch.int64
    assert np.array_equal(rows.cpu().numpy().reshape(B, 6, 6), GOLD[tag + "_cm"])             # exact
    acc, miou, fwiou = evaluation.group_metrics("semantics", rows)
    _hold64(tag + " semantics [miou, fwiou, acc]", np.stack([miou, fwiou, acc]), GOLD[tag + "_sem64"], 1e-12, True)
    _hold64(tag + " semantics vs the reference's fp32 run", np.stack([miou, fwiou, acc]), GOLD[tag + "_sem32"], 1e-12, True)
    # the class map: torch.argmax wherever there is no tie, the lowest index on the planted ties
    top2 = torch.topk(t[:, :6], 2, dim=1).values
    clear = top2[:, 0] > top2[:, 1]
    assert int((~clear).sum()) >= 12
    assert torch.equal(cmap[clear].long(), torch.argmax(t[:, :6], dim=1)[clear])
    assert np.array_equal(cmap.reshape(B, -1).cpu().numpy()[tb, tc], tcls)
    assert np.array_equal(cmap.cpu().numpy(), eval_refs.class_map(out[:, :6]))
    # without a class map the counts are the same, and as_float hands the gather exact float64 counts
    again = evaluation.task_metric_rows("semantics", t[:, :6], torch.from_numpy(lab).cuda(), as_float=True)
    assert again.dtype == torch.float64 and torch.equal(again, rows.double())


@pytest.mark.parametrize("task,tag", [(k, t) for k in ("depth", "normal", "semantics") for t in eval_inputs.CASES])
def test_a_frames_row_is_bitwise_the_same_alone_and_in_any_slot(task, tag):
    """The chunking depends on n_cells only and the cell -> lane mapping not on alignment: frame f alone (an aligned base) and
    in slots 0 and B-1 of a batch (bases that are not 16-byte aligned when n_cells is odd) give the same bits."""
    out, gt = _inputs(task, tag)[:2]
    B = out.shape[0]
    batch = _rows(task, out, gt)
    for f in (0, B - 1):
        alone = _rows(task, out[f:f + 1], gt[f:f + 1])
        assert torch.equal(alone[0], batch[f]), (task, tag, f)
        order = [f] + [b for b in range(B) if b != f] + [f]                      # f in slot 0 and in slot B (the last)
        moved = _rows(task, out[order], gt[order])
        assert torch.equal(moved[0], alone[0]) and torch.equal(moved[-1], alone[0]), (task, tag, f)
        assert torch.equal(moved[1:-1], batch[[b for b in range(B) if b != f]])


def test_one_cell_and_contiguous_inputs():
    """n_cells = 1 and a [B,nt,H,W] tensor without a sigma channel (contiguous, image stride nt*n)"""
    d = torch.tensor([[[[3.0]]], [[[7.0]]]], device="cuda")
    g = torch.tensor([[[[2.0]]], [[[-1.0]]]], device="cuda")
    rows = evaluation.task_metric_rows("depth", d, g, -1).cpu().numpy()
    assert np.array_equal(rows, np.array([[0.5, 1.0, 1.0], [0.0, 0.0, 0.0]]))
    out, gt = _inputs("normal", "b3_37x53")
    a = evaluation.task_metric_rows("normal", torch.from_numpy(out[:, :2].copy()).cuda(), torch.from_numpy(gt).cuda(), -1)
    assert torch.equal(a, _rows("normal", out, gt))


@pytest.mark.parametrize("tag", list(eval_inputs.CASES))
def test_reference_named_functions_on_cuda_tensors(tag):
    out, gt = _inputs("depth", tag)
    t = torch.from_numpy(out).cuda()
    abs_rel, rms = evaluation.depth_eval(t[:, :1], torch.from_numpy(gt).cuda(), -1)
    _hold(tag + " depth_eval", [float(abs_rel), float(rms)], GOLD[tag + "_depth64"], GOLD[tag + "_depth32"], DEPTH_REL, True)
    out, gt = _inputs("normal", tag)
    t = torch.from_numpy(out).cuda()
    err = evaluation.normal_eval(t[:, :2], torch.from_numpy(gt).cuda(), -1)
    _hold(tag + " normal_eval", float(err), GOLD[tag + "_normal64"], GOLD[tag + "_normal32"], NORMAL_DEG, False)
    out, lab, _ = _inputs("semantics", tag)
    t = torch.from_numpy(out).cuda()
    cls, miou, fwiou, acc = evaluation.semantic_eval_rows(t[:, :6], torch.from_numpy(lab).cuda(), mute=True)
    assert cls.dtype == torch.int64 and not cls.is_cuda and np.array_equal(cls.numpy(), eval_refs.class_map(out[:, :6]))
    _hold64(tag + " semantic_eval_rows", np.stack([miou, fwiou, acc]), GOLD[tag + "_sem64"], 1e-12, True)


# ------------------------------------------------------------------------------------------ the section loop and the entry point

FRAMES, BATCH = 8, 3


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from crossloc_amd.dataset import write_synthetic_scene
    return write_synthetic_scene(str(tmp_path_factory.mktemp("eval_scene")), FRAMES, depth=True, normal=True, semantics=True)


def _direct(task, scene, fullsize, uncertainty=None):
    """network(...) on the same batches, then the float64 restatement on the host: rows [K,D].  With uncertainty='MLE' the
    network output has nt+1 channels and pred[:, :nt] is the sigma split (a strided view)."""
    from crossloc_amd.dataset import CamLocDataset
    net = evaluation.config_network(task, True, False, uncertainty, fullsize)
    ds = CamLocDataset(scene, coord=False, depth=task == "depth", normal=task == "normal", semantics=task == "semantics",
                       raw_image=True)
    assert len(ds) == FRAMES
    fn = {"depth": eval_refs.depth_rows, "normal": eval_refs.normal_rows, "semantics": eval_refs.semantics_rows}[task]
    rows = []
    for s in range(0, FRAMES, BATCH):
        items = [ds[i] for i in range(s, min(FRAMES, s + BATCH))]
        with torch.no_grad():
            pred = net(torch.stack([it[0] for it in items]).cuda())
        assert pred.shape[1] == NT[task] + (uncertainty is not None)
        rows.append(fn(pred[:, :NT[task]].cpu().numpy(), torch.stack([it[2] for it in items]).numpy()))
    return net, ds, np.concatenate(rows).astype(np.float64)


def _run_entry(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "crossloc_amd.eval_single_task"] + args, cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_depth_section_and_entry_point(scene, tmp_path, capsys):
    net, ds, ref_rows = _direct("depth", scene, False, "MLE")
    rows, (abs_rel, rms) = evaluation.evaluate_section(net, ds, "depth", -1, BATCH, 0, 1)
    assert rows.shape == (FRAMES, 3) and np.array_equal(rows[:, 2], ref_rows[:, 2]) and rows[:, 2].sum() > 0
    ra, rr = eval_refs.group("depth", ref_rows)
    assert abs_rel.shape == (2,)                                                  # 8 frames: two groups of 4
    _hold64("section depth abs_rel", abs_rel, ra, DEPTH_REL, True)
    _hold64("section depth rms", rms, rr, DEPTH_REL, True)
    # sharded over 2 "ranks" by hand: the interleaved rows are the single-rank rows, bit for bit (batch-independent rows)
    parts = []
    for r in range(2):
        sub = torch.utils.data.Subset(ds, list(range(r, FRAMES, 2)))
        parts.append(evaluation.evaluate_section(net, sub, "depth", -1, 2, 0, 1)[0])
    inter = np.empty_like(rows)
    inter[0::2], inter[1::2] = parts
    assert np.array_equal(inter, rows)
    expect = evaluation.depth_printout(ra, rr)
    capsys.readouterr()
    log = str(tmp_path / "depth.log")
    text = _run_entry(["--task", "depth", "--uncertainty", "MLE", "--scene_dir", scene, "--tiny", "--batch", str(BATCH), "--testing_log", log,
                       "--section_name", "val_drone_sim"])
    assert expect in text, text
    logged = open(log).read()
    assert logged == "{:s} Evaluation on section val_drone_sim {:s}\n".format('=' * 20, '=' * 20) + expect + "\n"


def test_semantics_section_and_entry_point(scene, tmp_path, capsys):
    net, ds, ref_rows = _direct("semantics", scene, True)
    rows, (acc, miou, fwiou) = evaluation.evaluate_section(net, ds, "semantics", -1, BATCH, 0, 1)
    assert rows.shape == (FRAMES, 36) and np.array_equal(rows, ref_rows) and rows.sum() > 0      # counts: exact
    racc, rmiou, rfw = eval_refs.group("semantics", ref_rows)
    _hold64("section semantics", np.stack([acc, miou, fwiou]), np.stack([racc, rmiou, rfw]), 1e-12, True)
    expect = evaluation.semantic_printout([racc], [rmiou], [rfw])
    capsys.readouterr()
    log = str(tmp_path / "sem.log")
    text = _run_entry(["--task", "semantics", "--fullsize", "--scene_dir", scene, "--tiny", "--batch", str(BATCH),
                       "--testing_log", log, "--section_name", "test_drone_real"])
    assert expect in text, text
    assert open(log).read() == "{:s} Evaluation on section test_drone_real {:s}\n".format('=' * 20, '=' * 20) + expect + "\n\n"


def test_normal_section(scene):
    net, ds, ref_rows = _direct("normal", scene, False, "MLE")
    rows, err = evaluation.evaluate_section(net, ds, "normal", -1, BATCH, 0, 1)
    assert np.array_equal(rows[:, 1], ref_rows[:, 1]) and rows[:, 1].sum() > 0
    _hold64("section normal", err, eval_refs.group("normal", ref_rows), NORMAL_DEG, False)
