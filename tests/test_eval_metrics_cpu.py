"""CPU: the depth / normal / semantics evaluation metrics without a GPU - the float64 restatement (tests/eval_refs.py) against
the values recorded from the reference's own functions (tests/golden/eval_metrics.npz, written by
tests/golden/make_eval_golden.py), argument validation of the C ABI, the frame grouping and the report text."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import eval_inputs                                              # noqa: E402
import eval_refs                                                # noqa: E402

from crossloc_amd import evaluation                             # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "eval_metrics.npz"))


def _close(a, b, rel):
    """|a - b| <= rel * |b| element-wise, NaN matching NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all(np.abs(a - b)[~np.isnan(b)] <= rel * np.abs(b)[~np.isnan(b)]))


@pytest.mark.parametrize("tag", list(eval_inputs.CASES))
def test_depth_restatement_reproduces_the_reference(tag):
    out, gt = eval_inputs.depth_inputs(tag)
    assert eval_inputs.checksum(out, gt) == float(GOLD[tag + "_depth_checksum"])
    rows = eval_refs.depth_rows(out[:, :1], gt)
    assert rows[eval_inputs.EMPTY_IMAGE, 2] == 0 and (np.delete(rows[:, 2], eval_inputs.EMPTY_IMAGE) > 0).all()
    s = rows.sum(0)
    assert _close([s[0] / s[2], np.sqrt(s[1] / s[2])], GOLD[tag + "_depth64"], 1e-12)
    assert _close(np.stack(eval_refs.group("depth", rows, 1), 1), GOLD[tag + "_depth64_img"], 1e-12)
    assert _close(np.stack(eval_refs.group("depth", rows, 4), 1), GOLD[tag + "_depth64_grp"], 1e-12)


@pytest.mark.parametrize("tag", list(eval_inputs.CASES))
def test_normal_restatement_reproduces_the_reference(tag):
    out, gt = eval_inputs.normal_inputs(tag)
    assert eval_inputs.checksum(out, gt) == float(GOLD[tag + "_normal_checksum"])
    B = out.shape[0]
    # the planted cells do what they are there for: both sigmoid clamps and both cosine clamps bind on valid cells
    ang = eval_refs.normal_angles(out[:, :2].reshape(B, 2, -1), gt.reshape(B, 3, -1))
    valid = (gt.reshape(B, 3, -1) == -1).sum(1) == 0
    lo, hi = np.arccos(1 - 1e-7) / np.pi * 180.0, np.arccos(-1 + 1e-7) / np.pi * 180.0
    assert (ang[valid] == lo).sum() >= 4 and (ang[valid] == hi).sum() >= 4
    assert (out[:, :2] == 40).any() and (out[:, :2] == -40).any()
    rows = eval_refs.normal_rows(out[:, :2], gt)
    s = rows.sum(0)
    assert abs(s[0] / s[1] - float(GOLD[tag + "_normal64"])) <= 1e-9
    for size, key in ((1, "_normal64_img"), (4, "_normal64_grp")):
        mine, ref = eval_refs.group("normal", rows, size), GOLD[tag + key]
        assert np.array_equal(np.isnan(mine), np.isnan(ref)) and np.nanmax(np.abs(mine - ref)) <= 1e-9


@pytest.mark.parametrize("tag", list(eval_inputs.SEM_CASES))
def test_semantics_restatement_reproduces_the_reference(tag):
    out, lab, (tb, tc, tcls) = eval_inputs.semantics_case(tag)
    assert eval_inputs.checksum(out, lab) == float(GOLD[tag + "_sem_checksum"])
    B = out.shape[0]
    for v in (-1.0, 6.0, 255.0, 4.5):
        assert (lab == v).any()
    cls = eval_refs.class_map(out[:, :6]).reshape(B, -1)
    assert np.array_equal(cls[tb, tc], tcls)                                     # ties take the lowest index
    rows = eval_refs.semantics_rows(out[:, :6], lab)
    assert np.array_equal(rows.reshape(B, 6, 6), GOLD[tag + "_cm"])              # exact
    acc, miou, fwiou = eval_refs.group("semantics", rows)
    for key in ("_sem64", "_sem32"):
        assert _close(np.stack([miou, fwiou, acc]), GOLD[tag + key], 1e-12)
    # the product's own host-side metrics agree with the restatement
    acc2, miou2, fwiou2 = evaluation.group_metrics("semantics", rows)
    assert _close(np.stack([miou2, fwiou2, acc2]), GOLD[tag + "_sem64"], 1e-12)


@pytest.fixture(scope="module")
def hiplib():
    from crossloc_amd import build
    return ctypes.CDLL(build.build())


def test_abi_validation_needs_no_gpu(hiplib):
    """Arguments are checked before any HIP call: every bad call returns XL_ERR_ARG (-1) on a machine without a GPU."""
    vp, i64, ci, cf = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    L = hiplib
    L.xl_metrics_workspace_bytes.restype = i64
    L.xl_metrics_workspace_bytes.argtypes = [ci, ci]
    assert L.xl_metrics_workspace_bytes(4, 5400) == 4 * 2 * 144
    assert L.xl_metrics_workspace_bytes(1, 4096) == 144 and L.xl_metrics_workspace_bytes(1, 4097) == 288
    assert L.xl_metrics_workspace_bytes(0, 5400) == 0 and L.xl_metrics_workspace_bytes(1, 0) == 0
    for name in ("xl_metrics_depth", "xl_metrics_normal"):
        fn = getattr(L, name)
        fn.restype = ci
        fn.argtypes = [vp, i64, i64, vp, ci, ci, cf, vp, vp, vp]
        p = vp(4096)                                                 # never dereferenced: validation fails first
        assert fn(None, 10, 5, p, 1, 5, -1.0, p, p, None) == -1      # null prediction
        assert fn(p, 10, 5, None, 1, 5, -1.0, p, p, None) == -1      # null label
        assert fn(p, 10, 5, p, 1, 5, -1.0, None, p, None) == -1      # null workspace
        assert fn(p, 10, 5, p, 1, 5, -1.0, p, None, None) == -1      # null rows
        assert fn(p, 10, 5, p, 0, 5, -1.0, p, p, None) == -1         # B <= 0
        assert fn(p, 10, 5, p, -3, 5, -1.0, p, p, None) == -1
        assert fn(p, 10, 5, p, 65536, 5, -1.0, p, p, None) == -1     # B > XL_METRICS_MAX_BATCH (the grid's y extent)
        assert fn(p, 10, 5, p, 1, 0, -1.0, p, p, None) == -1         # n_cells <= 0
        assert fn(p, -10, 5, p, 1, 5, -1.0, p, p, None) == -1        # negative stride
    fn = L.xl_metrics_semantics
    fn.restype = ci
    fn.argtypes = [vp, i64, i64, ci, vp, ci, ci, vp, vp, vp, vp]
    p = vp(4096)
    assert fn(None, 30, 5, 6, p, 1, 5, p, p, None, None) == -1
    assert fn(p, 30, 5, 6, None, 1, 5, p, p, None, None) == -1
    assert fn(p, 30, 5, 6, p, 1, 5, None, p, None, None) == -1
    assert fn(p, 30, 5, 6, p, 1, 5, p, None, None, None) == -1
    assert fn(p, 30, 5, 6, p, 0, 5, p, p, None, None) == -1
    assert fn(p, 30, 5, 6, p, 65536, 5, p, p, None, None) == -1
    assert fn(p, 30, 5, 6, p, 1, 0, p, p, None, None) == -1
    for C in (0, 5, 7):
        assert fn(p, 30, 5, C, p, 1, 5, p, p, None, None) == -1      # channel count


def test_python_entry_points_refuse_cpu_tensors_and_bad_shapes():
    with pytest.raises(RuntimeError):
        evaluation.task_metric_rows("depth", torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))   # no CPU fallback
    with pytest.raises(NotImplementedError):
        evaluation.task_metric_rows("coord", torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4))
    with pytest.raises(NotImplementedError):
        evaluation.config_network("semantics", True, False, None, False)
    with pytest.raises(NotImplementedError):
        evaluation.config_network("semantics", True, False, "MLE", True)
    with pytest.raises(ValueError):
        evaluation.group_metrics("depth", np.zeros((4, 2)))


def _rows10(task):
    rng = np.random.default_rng(7)
    if task == "depth":
        rows = np.stack([rng.uniform(1, 50, 10), rng.uniform(1, 900, 10), rng.integers(1, 5400, 10).astype(np.float64)], 1)
    elif task == "normal":
        rows = np.stack([rng.uniform(1, 9e4, 10), rng.integers(1, 5400, 10).astype(np.float64)], 1)
    else:
        rows = rng.integers(0, 900, size=(10, 36)).astype(np.float64)
    return rows


@pytest.mark.parametrize("task", ["depth", "normal", "semantics"])
def test_group_metrics_groups_of_four_and_sharding_round_trip(task):
    rows = _rows10(task)
    got = evaluation.group_metrics(task, rows)
    ref = eval_refs.group(task, rows)
    got, ref = (got, ref) if isinstance(got, tuple) else ((got,), (ref,))
    n = 10 if task == "semantics" else 3                                         # groups of 4, 4 and 2
    for g, r in zip(got, ref):
        assert g.shape == (n,) and _close(g, r, 1e-12)
    if task == "depth":
        s = rows[8:10].sum(0)                                                    # the shorter last group
        assert got[0][2] == pytest.approx(s[0] / s[2], rel=1e-15) and got[1][2] == pytest.approx(np.sqrt(s[1] / s[2]), rel=1e-15)
    # frames sharded i % 3, padded to ceil(10/3) rows with NaN and interleaved back, as gather_errors does
    shards = [torch.from_numpy(rows[r::3]) for r in range(3)]
    per = 4
    padded = []
    for r in range(3):
        # gather_errors with world-size-1 semantics pads one shard to `per` rows: rows beyond the shard are NaN
        one = evaluation.gather_errors(shards[r], per, 0, 1)
        assert one.shape == (per, rows.shape[1]) and torch.isnan(one[len(shards[r]):]).all()
        padded.append(one)
    back = torch.empty((per * 3, rows.shape[1]), dtype=torch.float64)
    for r in range(3):
        back[r::3] = padded[r]
    back = back[:10].numpy()
    assert np.array_equal(back, rows)
    again = evaluation.group_metrics(task, back)
    again = again if isinstance(again, tuple) else (again,)
    for g, a in zip(got, again):
        assert np.array_equal(g, a)


def test_a_group_without_valid_cells_is_nan():
    rows = _rows10("depth")
    rows[4:8] = 0.0
    a, r = evaluation.group_metrics("depth", rows)
    assert np.isnan(a[1]) and np.isnan(r[1]) and not np.isnan(a[[0, 2]]).any() and not np.isnan(r[[0, 2]]).any()
    rows = _rows10("normal")
    rows[8:10] = 0.0
    e = evaluation.group_metrics("normal", rows)
    assert np.isnan(e[2]) and not np.isnan(e[:2]).any()
    acc, miou, fwiou = evaluation.group_metrics("semantics", np.zeros((1, 36)))
    assert np.isnan(acc[0]) and np.isnan(miou[0]) and fwiou[0] == 0.0


def test_printouts_match_the_reference_format(tmp_path, capsys):
    log = str(tmp_path / "log.txt")
    s = evaluation.depth_printout([0.0512, 0.1, 0.07], [3.456, 10.0, 1.0], log, "val_drone_sim")
    assert s == ("Depth accuracy:\nabsolute relative error, mean: 7.37%, median: 7.00%"
                 "\nRMS error, mean: 4.82m, median: 3.46m")
    s = evaluation.normal_printout([10.04, 30.0, 12.26], log, "val_drone_sim")
    assert s == "Surface normal accuracy:\nangular prediction error, mean: 17.4 deg, median: 12.3 deg"
    s = evaluation.semantic_printout([np.array([0.5, 0.7]), np.array([0.9])], [np.array([0.25, 0.35]), np.array([0.3])],
                                     [np.array([0.4, 0.6]), np.array([0.8])], log, "val_drone_sim")
    assert s == ("Pixel accuracy, mean: 70.00, median: 70.00\nMean IoU, mean: 30.00, median: 30.00\n"
                 "Frequency weighted IoU, mean: 60.00, median: 60.00")
    printed = capsys.readouterr().out
    assert "Depth accuracy:" in printed and "Surface normal accuracy:" in printed and "Mean IoU, mean: 30.00" in printed
    head = "{:s} Evaluation on section {:s} {:s}".format('=' * 20, "val_drone_sim", '=' * 20)
    text = open(log).read()
    assert text.count(head + "\n") == 3
    assert text.startswith(head + "\nDepth accuracy:\nabsolute relative error, mean: 7.37%, median: 7.00%\n")
    assert text.endswith("Frequency weighted IoU, mean: 60.00, median: 60.00\n\n")       # the reference's blank line (:484)
    assert text.count("\n\n") == 1
    evaluation.normal_printout([1.0])                                            # the log is optional


def test_write_synthetic_scene_optional_folders(tmp_path):
    from crossloc_amd.dataset import CamLocDataset, write_synthetic_scene
    root = write_synthetic_scene(str(tmp_path / "s"), 2, depth=True, normal=True)
    d = CamLocDataset(root, coord=False, depth=True, raw_image=True)[1][2]
    n = CamLocDataset(root, coord=False, normal=True, raw_image=True)[1][2]
    c = CamLocDataset(root, coord=True, raw_image=True)[1][2]
    assert tuple(d.shape) == (1, 60, 90) and tuple(n.shape) == (3, 60, 90)
    hit = (c != -1).all(0)
    assert hit.any() and (d[0][hit] >= 1).all() and torch.equal(d[0] == -1, ~hit)
    assert torch.allclose(n[:, hit].norm(dim=0), torch.ones(int(hit.sum())), atol=1e-6)
    plain = write_synthetic_scene(str(tmp_path / "p"), 1)
    assert sorted(os.listdir(plain)) == ["calibration", "init", "poses", "rgb"]      # defaults unchanged


def test_entry_point_options(monkeypatch):
    from crossloc_amd import eval_single_task, test_single_task
    opt, rest = eval_single_task._parse(["--task", "semantics", "--fullsize", "--tiny", "--scene_dir", "S", "--batch", "3",
                                         "--uncertainty", "MLE", "--section_name", "val_sim", "--testing_log", "L"])
    assert rest == [] and (opt.task, opt.fullsize, opt.tiny, opt.scene_dir, opt.batch, opt.uncertainty, opt.section_name,
                           opt.testing_log, opt.network_in, opt.num_mlr) == ("semantics", True, True, "S", 3, "MLE", "val_sim",
                                                                             "L", None, 0)
    with pytest.raises(SystemExit):                                              # coord-only options are refused, not ignored
        eval_single_task._parse(["--task", "depth", "--scene_dir", "S", "--hypotheses", "8"])
    for extra in (["--tiny"], ["--fullsize"], ["--uncertainty", "MLE"], ["--section_name", "x"]):
        with pytest.raises(SystemExit):                                          # task-only options are refused with --task coord
            eval_single_task._parse(["--synthetic", "4"] + extra)
    # --task coord (and no --task): every other argument reaches test_single_task.main() as given
    coord = ["--synthetic", "4", "-t", "10", "-hyps", "8", "--testing_log", "L"]
    seen = []
    monkeypatch.setattr(test_single_task, "main", lambda: seen.append(list(sys.argv[1:])))
    for head in ([], ["--task", "coord"]):
        monkeypatch.setattr(sys, "argv", ["eval_single_task"] + head + coord)
        eval_single_task.main()
    assert seen == [coord, coord]
