"""CPU checks of the pose-quality pass: the formulas of crossloc_amd/csrc/xl_dsac_quality_math.h through the serial
restatement tests/pose_quality_ref.c (which the GPU kernel must match bit for bit, tests/test_pose_quality_gpu.py), the
pure-numpy selective_accuracy, and the argument validation of the C entry point.  No GPU."""
import ctypes

import numpy as np
import pytest

import pose_quality_cases as qc
import pose_quality_ref
from crossloc_amd import synth
from pose_quality_ref import sym


@pytest.fixture(scope="module")
def qref(tmp_path_factory):
    return pose_quality_ref.load(tmp_path_factory.mktemp("pose_quality_ref"))


def _project(R, t, X, f, cx, cy):
    """double pixel of points X [n,3] at the world->camera pose {R, t}"""
    Xc = X @ R.T + t
    return np.stack([Xc[:, 0] / Xc[:, 2] * f + cx, Xc[:, 1] / Xc[:, 2] * f + cy], 1)


def _step(qref, R, t, delta):
    """pose (+) delta in the row's parametrisation: R' = Exp(w) R, t' = t + d, through apply_step (which subtracts)"""
    return qref.apply_step(R, t, -np.asarray(delta, np.float64))


def _cells(sc):
    """scene coordinates [n,3] float64 and cell-centre pixels [n,2] in cell order"""
    _, Ho, Wo = sc["coords"].shape
    X = sc["coords"].reshape(3, -1).T.astype(np.float64)
    ys, xs = np.divmod(np.arange(Ho * Wo), Wo)
    return X, np.stack([xs * qc.SUB + qc.SUB // 2, ys * qc.SUB + qc.SUB // 2], 1).astype(np.float64)


@pytest.fixture(scope="module")
def small_scenes(qref):
    """three 20x30 scenes (noise 0.5, no outliers) with their row at the ground-truth pose"""
    out = []
    for seed in (1, 2, 3):
        sc = synth.make_scene(seed, noise=0.5, outlier_ratio=0.0, Ho=20, Wo=30)
        R, t = qc.w2c(sc["pose"])
        out.append((sc, R, t, qref.row_w2c(sc["coords"], R, t, *qc.solver_args(sc))))
    return out


def test_jtj_matches_numeric_jacobians(qref, small_scenes):
    """JtJ of the row == Jn^T Jn with Jn by central differences (h = 1e-5) through apply_step and the projection:
    |diff| <= 1e-7 max|JtJ| (truncation O(h^2) = 1e-10 relative, rounding 1e-16 / h = 1e-11: three orders of margin)."""
    h = 1e-5
    for sc, R, t, row in small_scenes:
        X, px = _cells(sc)
        f, cx, cy = sc["focal"], sc["ppx"], sc["ppy"]
        inl = np.linalg.norm(_project(R, t, X, f, cx, cy) - px, axis=1) < qc.THR
        assert row[1] == inl.sum() and row[6] == 0
        Jn = np.zeros((2 * int(inl.sum()), 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            up = _project(*_step(qref, R, t, d), X[inl], f, cx, cy)
            dn = _project(*_step(qref, R, t, -d), X[inl], f, cx, cy)
            Jn[:, k] = ((up - dn) / (2 * h)).reshape(-1)
        JtJ = sym(row[10:31], 6)
        err = np.abs(JtJ - Jn.T @ Jn).max() / np.abs(JtJ).max()
        print("JtJ vs numeric: %.3e" % err)
        assert err <= 1e-7


def test_covariance_and_derived_figures(qref, small_scenes):
    for sc, R, t, row in small_scenes:
        JtJ, S, SC = sym(row[10:31], 6), sym(row[31:52], 6), sym(row[52:58], 3)
        var = row[5] / (2.0 * row[1] - 6.0)
        assert row[7] == np.sqrt(var)
        resid = np.abs(S @ JtJ - var * np.eye(6)).max() / var
        print("Sigma JtJ - sigma^2 I: %.3e" % resid)
        assert resid <= 1e-9
        ok, inv = qref.inv6(row[10:31])
        assert ok and np.array_equal(inv, inv.T) and (np.diag(inv) > 0).all() and (np.diag(S) > 0).all()
        assert np.array_equal(S, var * inv)
        # covariance of the camera centre C = -R^T t against the numeric Jacobian of C through apply_step
        h = 1e-6
        An = np.zeros((3, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            Ru, tu = _step(qref, R, t, d)
            Rd, td = _step(qref, R, t, -d)
            An[:, k] = (-Ru.T @ tu + Rd.T @ td) / (2 * h)
        errc = np.abs(SC - An @ S @ An.T).max() / np.abs(SC).max()
        print("Sigma_C vs numeric: %.3e" % errc)
        assert errc <= 1e-6
        assert np.isclose(row[8], np.sqrt(np.trace(SC)), rtol=1e-14)
        assert np.isclose(row[9], np.degrees(np.sqrt(S[0, 0] + S[1, 1] + S[2, 2])), rtol=1e-14)
        # a frame seen from 150-350 m with 0.5 m noise: centimetres to decimetres, hundredths of a degree
        assert 1e-3 < row[8] < 1.0 and 1e-4 < row[9] < 0.5


def test_inlier_count_and_sums_against_the_oracle(qref, oracle):
    """Count, sum e, sum e^2, SSE and the soft score at a double pose against a float64 numpy restatement built on the
    oracle's per-cell error (resid_row returns the double norm of the float pixel difference that cell_err rounds and clamps) and
    against oracle.score.  The count is exact; the sums differ only in the order of at most 5400 additions."""
    sc = synth.make_scene(5, noise=0.5, outlier_ratio=0.3)
    R, t = qc.w2c(sc["pose"])
    args = qc.solver_args(sc)
    row = qref.row_w2c(sc["coords"], R, t, *args)
    X, px = _cells(sc)
    f, cx, cy = sc["focal"], sc["ppx"], sc["ppy"]
    e = np.array([oracle.resid_row(R, t, np.zeros(3), X[i], px[i, 0], px[i, 1], f, cx, cy, 1e30)[0] for i in range(len(X))])
    e = np.minimum(e.astype(np.float32), np.float32(qc.MAX_REPROJ))
    inl = e < np.float32(qc.THR)
    assert 0.6 * len(X) < inl.sum() < 0.8 * len(X)
    assert row[0] == len(X) and row[1] == inl.sum()
    ed = e[inl].astype(np.float64)
    assert np.isclose(row[3], ed.sum(), rtol=1e-12) and np.isclose(row[4], (ed * ed).sum(), rtol=1e-12)
    r = _project(R, t, X[inl], f, cx, cy) - px[inl]
    assert np.isclose(row[5], (r * r).sum(), rtol=1e-12)
    want = oracle.score(sc["coords"], R, t, qc.THR, qc.ALPHA, qc.MAX_REPROJ, f, cx, cy, qc.SUB)
    assert want > 0 and abs(row[2] - want) <= 1e-12 * want


def test_normal_equation_sums_are_the_solvers_bit_for_bit(qref, oracle, tmp_path):
    """The pass and the solver's refinement accumulate the same function per inlier (pnp_cell_normal_eq of xl_dsac_math.h), so
    the per-cell arithmetic agrees by construction.  What is held together here is what each builds on top of it: the inlier
    set, the walk of the 256 virtual threads over the cells and the order of the additions.  The pass's 28 normal-equation sums
    equal the oracle's own xo_normal_eq (which the solver kernels match bitwise) over the refinement's inlier set at the same
    pose, bit for bit - at ground truth and at the oracle's refined pose, with outliers, on a full and on a ragged grid."""
    ne = pose_quality_ref.load_oracle_normal_eq(tmp_path)
    for seed, Ho, Wo in ((5, 60, 90), (6, 37, 53), (7, 7, 9)):
        sc = synth.make_scene(seed, noise=0.5, outlier_ratio=0.3, Ho=Ho, Wo=Wo)
        args = qc.solver_args(sc)
        _, dbg = oracle.forward_rgb(sc["coords"], 64, qc.THR, sc["focal"], sc["ppx"], sc["ppy"], qc.ALPHA, qc.MAX_REPROJ, qc.SUB,
                                    debug=True)
        for R, t in (qc.w2c(sc["pose"]), (dbg["pose1"][:9].reshape(3, 3), dbg["pose1"][9:])):
            sums = qref.sums_w2c(sc["coords"], R, t, *args)
            want = ne.normal_eq(sc["coords"], R, t, *args)
            assert sums[28] > 0.5 * Ho * Wo and np.abs(want[:21]).max() > 0
            assert qc.same_bits(sums[:28], want), (seed, np.flatnonzero(sums[:28] != want))
            row = qref.row_w2c(sc["coords"], R, t, *args)
            assert qc.same_bits(row[10:31], want[:21]) and qc.same_bits(row[5], want[27])


@pytest.mark.parametrize("seed", [3, 11])
def test_monte_carlo_calibration(qref, oracle, seed):
    """The predicted covariance describes the solver's actual scatter.  Ground-truth points of a 60x90 scene are moved in
    the camera frame so that the reprojection residual at the ground-truth pose is exactly iid N(0, 0.5^2 px^2) per axis;
    200 draws go through the oracle's solver (64 hypotheses) and the row is taken at its refined double pose.
      sigma_px: its mean over the draws is within 2 % of 0.5, and every single draw within 4 % (one draw estimates it from 10794
                degrees of freedom: standard deviation 0.5 / sqrt(2 * 10794) = 0.68 %, so 2 % is 2.9 of them - among 400 draws
                one or two would miss it by chance - and 4 % is 5.9: no wrong row hides in the mean);
      per parameter: mean of delta_i^2 over the mean predicted variance in [0.67, 1.33], the 99.9 % interval of chi2_200 / 200;
      mean squared Mahalanobis distance in [5.2, 6.8]: 6 +- 3.3 sqrt(12 / 200).
    Measured figures: DESIGN.md (pose quality); other noise levels and outlier ratios: tools/pose_quality_calibration.py."""
    sigma = 0.5
    m = qc.calibration_run(qref, oracle, seed, sigma=sigma, outlier_ratio=0.0, draws=200)
    assert (m["status"] == 0).all() and (m["n_inliers"] == 5400).all()
    print("seed %d: sigma_px mean %.4f, per draw %.4f .. %.4f  variance ratios %s  mean Mahalanobis^2 %.3f" % (
        seed, m["sigma_px"].mean(), m["sigma_px"].min(), m["sigma_px"].max(), np.array2string(m["ratio"], precision=3),
        m["mahalanobis2"].mean()))
    assert abs(m["sigma_px"].mean() - sigma) <= 0.02 * sigma
    assert (np.abs(m["sigma_px"] - sigma) <= 0.04 * sigma).all()          # every single draw: 5.9 standard deviations
    assert (m["ratio"] >= 0.67).all() and (m["ratio"] <= 1.33).all()
    assert 5.2 <= m["mahalanobis2"].mean() <= 6.8


def test_status_paths(qref):
    seen = set()
    for Ho, Wo in ((12, 16), (200, 4)):
        for name, coords, pose, args, status, n_inl in qc.status_cases(Ho, Wo):
            row = qref.row(coords, pose, *args)
            assert row[6] == status, (name, Ho, Wo, row[6], row[1])
            assert row[0] == Ho * Wo
            if n_inl is not None:
                assert row[1] == n_inl, (name, row[1])
            qc.assert_nan_pattern(row, status)
            seen.add((name, int(row[1]) if status != 3 else -1))
    assert ("one_point_column", 200) in seen and ("three_inliers", 3) in seen and ("four_inliers", 4) in seen


def test_float_pose_entry_reads_the_pose_like_the_backward_pass(qref):
    """A 4x4 cam->world matrix means what it means in backward_rgb: gt_from_pose16's {R2, t2}, and the float32 entry is the
    double entry at that pose."""
    sc = synth.make_scene(9, noise=0.5, outlier_ratio=0.3, Ho=20, Wo=30)
    pose = sc["pose"].astype(np.float32)
    R, t = qref.pose_from16(pose)
    Rw, tw = qc.w2c(pose)
    assert np.abs(R - Rw).max() < 1e-6 and np.abs(t - tw).max() < 1e-3 and np.abs(R @ R.T - np.eye(3)).max() < 1e-14
    args = qc.solver_args(sc)
    assert qc.same_bits(qref.row(sc["coords"], pose, *args), qref.row_w2c(sc["coords"], R, t, *args))


def test_selective_accuracy():
    from crossloc_amd import evaluation
    #                 0     1     2     3      4     5     6     7
    t = np.array([1.0, 40.0, 2.0, 4.0, 100.0, 0.5, 6.0, 2.5])
    r = np.array([1.0, 20.0, 2.0, 4.0, 50.0, 0.5, 6.0, 2.5])
    s = np.array([0.3, 0.9, 0.1, 0.3, np.nan, 0.2, 0.5, 0.05])
    # ascending sigma, ties by index, NaN last: 7, 2, 5, 0, 3, 6, 1, 4
    out = evaluation.selective_accuracy(t, r, s, keep=(1.0, 0.9, 0.75, 0.5))
    assert [(frac, n) for frac, n, _ in out] == [(1.0, 8), (0.9, 8), (0.75, 6), (0.5, 4)]
    for (_, n, st), idx in zip(out, ([7, 2, 5, 0, 3, 6, 1, 4],) * 2 + ([7, 2, 5, 0, 3, 6], [7, 2, 5, 0])):
        want, _ = evaluation.accuracy_report(t[idx], r[idx])
        assert st == want
    assert out[3][2]["3m3deg"] == 100.0 and out[3][2]["median_t"] == 1.5
    assert out[2][2]["5m5deg"] == pytest.approx(100.0 * 5 / 6) and out[0][2]["30m10deg"] == 75.0
    # the tie (frames 0 and 3, sigma 0.3) is broken by index: keeping 4 of 8 takes frame 0, not frame 3
    assert out[3][2]["mean_t"] == pytest.approx(np.mean([2.5, 2.0, 0.5, 1.0]))
    assert "Selective accuracy" in evaluation.selective_accuracy_table(t, r, s)


def test_driver_runs_test_single_task_itself(monkeypatch, tmp_path, capsys):
    """crossloc_amd.pose_quality_single_task restates nothing: it calls test_single_task.main() with its own two options taken out
    of argv and `evaluation` bound to a view that adds the quality rows to localize_batch, gather_errors and the printout."""
    import sys
    import torch
    from crossloc_amd import evaluation, pose_quality_single_task as drv, test_single_task
    out = tmp_path / "rows.npy"
    seen = {}

    def fake_main():
        seen["argv"] = list(sys.argv[1:])
        ev = test_single_task.evaluation
        assert isinstance(ev, drv._EvaluationWithQuality) and ev.accuracy_report is evaluation.accuracy_report
        rows = torch.zeros((3, 64), dtype=torch.float64)
        rows[:, 8] = torch.tensor([0.3, float("nan"), 0.1], dtype=torch.float64)
        ev.batches += [rows[:2], rows[2:]]
        errs = torch.tensor([[1.0, 1.0], [50.0, 20.0], [2.0, 2.0]], dtype=torch.float64)
        allv = ev.gather_errors(errs, 3, 0, 1).numpy()
        assert np.array_equal(allv, errs.numpy())
        ev.scene_coords_printout(allv[:, 0], allv[:, 1], None, [np.array([1.0, 2.0])], testing_log=None)

    monkeypatch.setattr(test_single_task, "main", fake_main)
    argv = ["x", "--synthetic", "16", "--pose_quality", "--quality_out", str(out), "--batch", "8", "-hyps", "32"]
    monkeypatch.setattr(sys, "argv", list(argv))
    drv.main()
    assert seen["argv"] == ["--synthetic", "16", "--batch", "8", "-hyps", "32"]
    assert sys.argv == argv and test_single_task.evaluation is evaluation          # both restored
    text = capsys.readouterr().out
    assert text.index("Median Error") < text.index("Selective accuracy")
    rows = np.load(out)
    assert rows.shape == (3, 64) and np.isnan(rows[1, 8]) and rows[2, 8] == 0.1
    monkeypatch.setattr(sys, "argv", ["x", "--quality_out=" + str(out), "--batch", "4"])
    drv.main()
    assert seen["argv"] == ["--batch", "4"]


def test_python_surface_without_a_gpu():
    import torch
    import dsacstar
    import crossloc_amd.dsacstar as shim
    assert dsacstar.pose_quality_batch is shim.pose_quality_batch and dsacstar.QUALITY_FIELDS is shim.QUALITY_FIELDS
    cols = np.zeros(64, int)
    for v in shim.QUALITY_FIELDS.values():
        cols[v] += 1
    assert (cols == 1).all()                                          # the names cover the 64 columns once
    assert shim.QUALITY_FIELDS["status"] == 6 and shim.QUALITY_FIELDS["cov"] == slice(31, 52)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dsacstar.pose_quality_batch(torch.zeros(1, 3, 6, 9), torch.zeros(1, 4, 4), 10.0, 480.0, 36.0, 24.0, 100.0, 100.0, 8)
    with pytest.raises(RuntimeError):
        dsacstar.pose_quality_batch(torch.zeros(3, 6, 9), torch.zeros(1, 4, 4), 10.0, 480.0, 36.0, 24.0, 100.0, 100.0, 8)


def test_c_entry_point_refuses_bad_arguments_before_any_hip_call():
    from crossloc_amd import build
    L = ctypes.CDLL(build.build())
    fn = L.xl_dsac_pose_quality_batch
    i64, i32, f32, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    fn.restype = i32
    fn.argtypes = [vp, i64, i64, i64, i64, i32, i32, i32, vp, f32, f32, f32, f32, f32, f32, i32, vp, vp, vp]
    buf = (ctypes.c_double * 64)()                                   # host memory standing in for a device pointer: never read
    p = ctypes.cast(buf, vp)

    def call(coords=p, poses=p, rows=p, B=1, Ho=60, Wo=90, sub=8):
        return fn(coords, 16200, 5400, 90, 1, B, Ho, Wo, poses, 10.0, 480.0, 360.0, 240.0, 100.0, 100.0, sub, None, rows, None)

    for kw in (dict(coords=None), dict(poses=None), dict(rows=None), dict(B=0), dict(B=-3), dict(Ho=0), dict(Ho=-1),
               dict(Wo=0), dict(sub=0)):
        assert call(**kw) == -1, kw                                  # XL_ERR_ARG
    assert call(Ho=1 << 16, Wo=1 << 15) == -2                        # XL_ERR_GRID: the cell index would not fit an int
