"""CPU checks of the RGB-D DSAC* backward pass: the formulas of crossloc_amd/csrc/xl_dsac_rgbd_bwd_math.h through the serial
restatement tests/dsac_rgbd_bwd_ref.c (which the GPU kernels must match bit for bit, tests/test_dsac_rgbd_bwd_gpu.py) against
tests/indep_dsac_rgbd_bwd.py (numpy SVD Kabsch, central differences, no shared code); a sanitizer run of the restatement as a
program of its own; the argument validation of the C entry point and the Python front end.  No GPU.

Ground truth of the gradient scenes.  The ground-truth pose handed to the backward pass is the scene's pose moved by about one
degree and half a metre.  At the scene's own pose and exact inputs the estimate equals the ground truth to rounding: the
rotation angle is ~1e-8 rad, 3 - trace(R1 R2^T) is at the rounding of the trace, and d acos - in dLoss and in any numeric
derivative alike - is not determined to better than per cent there (xl_dsac_math.h notes the same at the end of dloss).  A
comparison to 1e-5 of the gradient needs a loss that is a function of the pose in double precision."""
import ctypes
import subprocess

import numpy as np
import pytest

import dsac_rgbd_bwd_ref as bref
import dsac_rgbd_cases as rc
import indep_dsac_rgbd_bwd as indep
from crossloc_amd import synth

THR, ALPHA, MAX_DIST = 10.0, 100.0, 100.0
W_ROT, W_TRANS, NO_CLAMP = 1.0, 100.0, 1.0e6
STEP = 1.0e-6                                  # metres: below the residuals |d| of exact float32 inputs (2e-6 m and up), where the error has its kink
# (grid, hypotheses, coordinate noise) -> scene seed; 30 % outliers, 20 % holes everywhere
CASES = [(8, 12, 16, 0.0, 70), (8, 12, 16, 0.05, 71), (8, 12, 64, 0.0, 72), (8, 12, 64, 0.05, 73),
         (17, 23, 16, 0.0, 74), (17, 23, 16, 0.05, 75), (17, 23, 64, 0.0, 76), (17, 23, 64, 0.05, 77)]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return bref.load(tmp_path_factory.mktemp("dsac_rgbd_bwd_ref"))


def moved_pose(pose):
    """the scene's cam->world pose turned by (0.01, -0.015, 0.02) rad and shifted by (0.3, -0.2, 0.4) m"""
    out = pose.copy()
    out[:3, :3] = out[:3, :3] @ synth._rot_xyz(0.01, -0.015, 0.02)
    out[:3, 3] += [0.3, -0.2, 0.4]
    return out


def scene_of(Ho, Wo, noise, seed):
    sc = rc.rgbd_scene(seed, Ho, Wo, noise=noise, outlier_ratio=0.3, holes=0.2)
    sc["gt"] = moved_pose(sc["pose"])
    return sc


def frozen_of(res):
    """the discrete choices and constants of a run of the restatement, for the independent surrogate"""
    rec = res["rec"]
    return dict(cells=res["cells"], masks=res["masks"], active=rec[:, bref.ACTIVE] > 0, rounds_fitted=rec[:, bref.INLIERS] > 0,
                guard1=rec[:, bref.GUARD_I] > 0, guard2=rec[:, bref.GUARD_II] > 0,
                const_pose=(res["hyp_poses"][:, :9].reshape(-1, 3, 3).copy(), res["hyp_poses"][:, 9:].copy()),
                const_score=res["scores"].copy(), const_loss=rec[:, bref.LOSS].copy())


@pytest.fixture(scope="module")
def runs(ref):
    """the restatement and the independent surrogate on every case, computed once: case -> (scene, result, surrogate)"""
    out = {}
    for Ho, Wo, n_hyp, noise, seed in CASES:
        sc = scene_of(Ho, Wo, noise, seed)
        res = ref.backward(sc["coords"], sc["gt"], n_hyp, THR, ALPHA, MAX_DIST, W_ROT, W_TRANS, NO_CLAMP, cam=sc["cam"], image=seed)
        sur = indep.Surrogate(sc["coords"], sc["cam"], sc["gt"], frozen_of(res), THR, ALPHA, MAX_DIST, W_ROT, W_TRANS, NO_CLAMP)
        out[(Ho, Wo, n_hyp, noise)] = (sc, res, sur)
    return out


# --------------------------------------------------------------------------------- 1. the Kabsch adjoint against SVD

def _point_sets():
    rng = np.random.default_rng(11)
    Rg = synth._rot_xyz(0.3, -0.2, 1.1)
    sets = {}
    for n in (3, 4, 7, 200):
        X = rng.normal(size=(n, 3)) * 30.0 + np.array([-455.0, 417.0, 280.0])
        sets["%d points" % n] = (X @ Rg.T + np.array([3.0, -2.0, 200.0]) + rng.normal(size=(n, 3)) * 0.05, X)
    X = np.array([[0.0, 0.0, 0.0], [40.0, 0.0, 0.0], [20.0, 0.4, 0.0]]) @ synth._rot_xyz(0.5, 0.1, -0.3).T + [100.0, -50.0, 20.0]
    sets["thin triangle"] = (X @ Rg.T + np.array([3.0, -2.0, 200.0]) + rng.normal(size=(3, 3)) * 0.01, X)       # aspect 1 : 100
    return sets


@pytest.mark.parametrize("name", ["3 points", "4 points", "7 points", "200 points", "thin triangle"])
def test_adjoint_against_central_differences_of_svd_kabsch(ref, name):
    """dL/dX of L = <G_R, R> + g_t . t for random G_R, g_t: the header's closed form against central differences of numpy's SVD
    Kabsch; tolerance 10 x the step-halving self-consistency of the differences, measured here"""
    p, X = _point_sets()[name]
    rng = np.random.default_rng(5)
    for trial in range(3):
        GR, gt = rng.normal(size=(3, 3)), rng.normal(size=3)
        got, R, t, gap, guard = ref.adjoint(p, X, GR, gt)
        Rn, tn = indep.kabsch_svd(p, X)
        assert not guard and gap > 1e-8 and np.abs(R - Rn).max() < 1e-9
        a, b = indep.numeric_adjoint(p, X, GR, gt, 1e-4), indep.numeric_adjoint(p, X, GR, gt, 5e-5)
        own = np.abs(a - b).max()
        err = np.abs(got - b).max()
        print("%s trial %d: |grad| %.3g, error %.3g, self-consistency %.3g, gap %.3g" % (name, trial, np.abs(b).max(), err, own, gap))
        assert err <= 10.0 * own, (name, trial, err, own)


def test_adjoint_guard_on_degenerate_sets(ref):
    """collinear and repeated points: the fit is not unique, the guard fires, the gradient is finite and exactly zero"""
    rng = np.random.default_rng(7)
    s = np.array([0.0, 1.0, 2.5, 4.0])
    X3 = rng.normal(size=(3, 3)) * 30.0
    p3 = X3 @ synth._rot_xyz(0.3, -0.2, 1.1).T + [3.0, -2.0, 200.0]
    sets = {"collinear": (np.outer(s, [1.0, 2.0, 3.0]), np.outer(s, [3.0, 1.0, 2.0]) + 7.0),
            "repeated draw": (p3[[0, 1, 1]], X3[[0, 1, 1]]),
            "one point": (p3[[2, 2, 2]], X3[[2, 2, 2]])}
    for name, (p, X) in sets.items():
        got, R, t, gap, guard = ref.adjoint(p, X, rng.normal(size=(3, 3)), rng.normal(size=3))
        assert guard, (name, gap)
        assert np.isfinite(got).all() and not got.any(), name
        assert np.isfinite(R).all() and np.isfinite(gap), name


# --------------------------------------------------------------------------------- 2. / 3. whole gradient, expected loss

@pytest.mark.parametrize("Ho,Wo,n_hyp,noise", [c[:4] for c in CASES])
def test_gradient_against_numeric(runs, Ho, Wo, n_hyp, noise):
    """The restatement's gradient against central differences of the independent surrogate: every cell at 8 x 12, the support
    cells plus 40 seeded cells at 17 x 23.  Tolerance: 10 x the step-halving self-consistency of the differences on the same
    scene, as a fraction of the gradient's maximum.  Measured (error / self-consistency, fractions of the maximum): 2e-6 / 2e-6,
    1e-6 / 1e-6, 4e-6 / 4e-6, 3e-7 / 3e-7 at 8 x 12 and 3e-5 / 3e-5, 2e-6 / 3e-6, 2e-5 / 2e-5, 2e-6 / 2e-6 at 17 x 23:
    the differences themselves limit the comparison."""
    sc, res, sur = runs[(Ho, Wo, n_hyp, noise)]
    rec = res["rec"]
    act = rec[:, bref.ACTIVE] > 0
    flagged = (rec[act, bref.GUARD_I] > 0) | (rec[act, bref.GUARD_II] > 0)
    assert act.sum() >= 1 and flagged.sum() <= 0.25 * act.sum(), (act.sum(), flagged.sum())
    N = Ho * Wo
    if N <= 96:
        cells = np.arange(N)
    else:
        support = res["cells"][act].reshape(-1)
        cells = np.unique(np.concatenate([support[support >= 0], np.random.default_rng(3).choice(N, 40, replace=False)]))
    a, b = sur.gradient(cells, STEP), sur.gradient(cells, STEP / 2)
    got = res["grad"].reshape(3, -1).T[cells].astype(np.float64)
    top = np.abs(b).max()
    own, err = np.abs(a - b).max() / top, np.abs(got - b).max() / top
    print("%dx%d %d hyp noise %.2f: %d active, %d flagged, max |grad| %.4g, error %.3g, self-consistency %.3g of it"
          % (Ho, Wo, n_hyp, noise, act.sum(), flagged.sum(), top, err, own))
    assert top > 0 and np.isfinite(got).all()
    assert err <= 10.0 * own, (err, own)
    invalid = sc["cam"][2].reshape(-1) == 0
    assert invalid.any() and not res["grad"].reshape(3, -1)[:, invalid].any()          # holes get nothing


@pytest.mark.parametrize("Ho,Wo,n_hyp,noise", [c[:4] for c in CASES])
def test_expected_loss_against_numpy(runs, Ho, Wo, n_hyp, noise):
    """sum_h softmax(score)_h loss_h from numpy (SVD Kabsch on the triples and the final inlier sets, float32 error as the solver
    defines its score) to 1e-9 relative"""
    _, res, sur = runs[(Ho, Wo, n_hyp, noise)]
    want = sur.value()
    assert abs(res["loss"] - want) <= 1e-9 * abs(want), (res["loss"], want)
    prob, loss, _ = sur.parts(sur.X0, cast=True)
    assert np.abs(prob - res["rec"][:, bref.PROB]).max() <= 1e-9
    assert abs(res["rec"][:, bref.PROB].sum() - 1.0) <= 1e-12


# --------------------------------------------------------------------------------- 4. descent

@pytest.mark.parametrize("soft_clamp", [NO_CLAMP, 20.0])
def test_a_small_step_against_the_gradient_lowers_the_expected_loss(ref, soft_clamp):
    """soft clamp inactive and active (the expected loss of these scenes is ~55, so 20 puts every hypothesis on the sqrt branch)"""
    for Ho, Wo, noise, seed in ((8, 12, 0.05, 81), (17, 23, 0.0, 82)):
        sc = scene_of(Ho, Wo, noise, seed)
        kw = dict(cam=sc["cam"], image=seed)
        r0 = ref.backward(sc["coords"], sc["gt"], 16, THR, ALPHA, MAX_DIST, W_ROT, W_TRANS, soft_clamp, **kw)
        g = r0["grad"]
        assert np.isfinite(g).all() and np.abs(g).max() > 0
        if soft_clamp < NO_CLAMP:
            assert (r0["rec"][:, bref.LOSS] > soft_clamp).all()          # sqrt(cut * loss) > cut iff loss > cut: every one is clamped
        step = 1e-3 / np.abs(g).max()                       # the largest coordinate moves by a millimetre
        moved = (sc["coords"] - np.float32(step) * g).astype(np.float32)
        r1 = ref.backward(moved, sc["gt"], 16, THR, ALPHA, MAX_DIST, W_ROT, W_TRANS, soft_clamp, **kw)
        predicted = step * float((g.astype(np.float64) ** 2).sum())
        print("%dx%d clamp %g: loss %.9g -> %.9g, first order predicts -%.3g" % (Ho, Wo, soft_clamp, r0["loss"], r1["loss"], predicted))
        assert r1["loss"] < r0["loss"], (r0["loss"], r1["loss"])


# --------------------------------------------------------------------------------- 5. edge cases

def test_edge_cases_of_the_restatement(ref):
    sc = scene_of(8, 12, 0.0, 4)
    ident = np.eye(3).reshape(9), np.zeros(3)
    # no valid cell: the loss of the identity pose, a zero gradient, no NaN
    none = ref.backward(sc["coords"], sc["gt"], 8, THR, ALPHA, MAX_DIST, depth=np.zeros((8, 12), np.float32))
    assert none["loss"] == pytest.approx(ref.pose_loss(*ident, sc["gt"], 1.0, 100.0, 1e6), rel=1e-12)
    assert not none["grad"].any() and np.isfinite(none["rec"]).all() and (none["cells"] == -1).all()
    # a single hypothesis: probability 1, soft-max gradient 0
    one = ref.backward(sc["coords"], sc["gt"], 1, THR, ALPHA, MAX_DIST, cam=sc["cam"])
    assert one["rec"][0, bref.PROB] == 1.0 and one["rec"][0, bref.SOG] == 0.0 and one["rec"][0, bref.ACTIVE] == 1.0
    assert np.isfinite(one["grad"]).all() and one["grad"].any()
    # the sampling budget exhausted (90 % outliers, 128 tries for a threshold of 1 mm): still returns, finite
    hard = rc.rgbd_scene(6, 8, 12, noise=0.5, outlier_ratio=0.9)
    res = ref.backward(hard["coords"], moved_pose(hard["pose"]), 16, 0.1, ALPHA, MAX_DIST, cam=hard["cam"], max_tries=128)
    assert np.isfinite(res["loss"]) and np.isfinite(res["grad"]).all() and np.isfinite(res["rec"]).all()
    # an all-inactive tail: with noisy coordinates few hypotheses carry the probability mass, the last ones none of it
    noisy = scene_of(8, 12, 0.05, 73)
    many = ref.backward(noisy["coords"], noisy["gt"], 64, THR, ALPHA, MAX_DIST, cam=noisy["cam"], image=73)
    act = many["rec"][:, bref.ACTIVE] > 0
    assert act.any() and not act[-4:].any(), np.flatnonzero(act)
    assert (many["rec"][~act, bref.PROB] < 1e-3).all() and not many["rec"][~act, 2:].any()
    assert np.isfinite(many["loss"]) and np.isfinite(many["grad"]).all()
    # accumulation into a nonzero gradient
    base = ref.backward(sc["coords"], sc["gt"], 16, THR, ALPHA, MAX_DIST, cam=sc["cam"])
    acc = ref.backward(sc["coords"], sc["gt"], 16, THR, ALPHA, MAX_DIST, cam=sc["cam"], grad=np.full((3, 8, 12), 0.125, np.float32))
    valid = sc["cam"][2] != 0
    assert (acc["grad"][:, ~valid] == 0.125).all()
    assert np.abs(acc["grad"][:, valid] - (base["grad"][:, valid] + 0.125)).max() <= 16 * 2.0 ** -23 * np.abs(base["grad"]).max()
    # the depth form and the camera form give the same bits
    dep = ref.backward(sc["coords"], sc["gt"], 16, THR, ALPHA, MAX_DIST, depth=sc["depth"], focal=sc["focal"], ppx=sc["ppx"],
                       ppy=sc["ppy"], sub=sc["sub"])
    for k in ("grad", "rec", "cells", "scores"):
        assert dep[k].tobytes() == base[k].tobytes(), k
    assert dep["loss"] == base["loss"]


# --------------------------------------------------------------------------------- 6. argument validation, no GPU

def _abi(coords=8, cam=8, depth=None, B=1, Ho=8, Wo=12, grad=8, gt=8, loss=8, n_hyp=8, sub=8, max_tries=10):
    from crossloc_amd import _lib
    vp = ctypes.c_void_p
    return _lib.lib().xl_dsac_backward_rgbd_batch(vp(coords), 288, 96, 12, 1, vp(cam), 288, 96, 12, 1, vp(depth), 96, 12, 1,
                                                  B, Ho, Wo, vp(grad), 288, 96, 12, 1, vp(gt), vp(loss), n_hyp, 10.0, 100.0, 100.0,
                                                  1.0, 100.0, 100.0, 480.0, 48.0, 32.0, sub, None, 1305, 0, 1, max_tries, None, None)


def test_abi_rejects_bad_arguments_before_any_hip_call():
    """the pointers are never dereferenced: every case returns before the first HIP call"""
    ARG, GRID = -1, -2
    assert _abi(cam=None, depth=None) == ARG                   # neither camera coordinates nor depth
    assert _abi(cam=8, depth=8) == ARG                         # both
    for name in ("coords", "grad", "gt", "loss"):
        assert _abi(**{name: None}) == ARG, name
    for kw in (dict(B=0), dict(Ho=0), dict(Wo=-3), dict(n_hyp=0), dict(max_tries=0), dict(max_tries=2 ** 31 - 63),
               dict(max_tries=2 ** 32 - 1), dict(cam=None, depth=8, sub=0)):
        assert _abi(**kw) == ARG, kw
    assert _abi(Ho=64, Wo=97) == GRID                          # 6208 cells > XL_DSAC_RGBD_MAX_CELLS
    assert _abi(Ho=40000, Wo=60000) == GRID                    # the product does not fit an int
    assert _abi(cam=None, depth=8, Ho=100, Wo=100) == GRID
    assert _abi(B=70000) == GRID                               # images ride on the grid's y dimension


def test_python_front_end_rejects_bad_arguments():
    torch = pytest.importorskip("torch")
    import dsacstar
    co, cam, depth = torch.zeros(1, 3, 8, 12), torch.zeros(1, 3, 8, 12), torch.zeros(1, 8, 12)
    g, gt = torch.zeros(1, 3, 8, 12), torch.eye(4)[None]
    tail = (8, 10.0, 1.0, 100.0, 100.0, 100.0, 100.0, 1305)
    with pytest.raises(RuntimeError):
        dsacstar.backward_rgbd_batch(co, None, g, gt, *tail)                                     # neither
    with pytest.raises(RuntimeError):
        dsacstar.backward_rgbd_batch(co, cam, g, gt, *tail, depth=depth)                         # both
    with pytest.raises(RuntimeError):
        dsacstar.backward_rgbd_batch(co, cam[:, :2], g, gt, *tail)                               # shape
    with pytest.raises(RuntimeError):
        dsacstar.backward_rgbd_batch(co, None, g, gt, *tail, depth=depth)                        # depth without intrinsics
    with pytest.raises(RuntimeError):
        dsacstar.backward_rgbd_batch(co, cam.double(), g, gt, *tail)                             # dtype
    with pytest.raises(RuntimeError):
        dsacstar.backward_rgbd_batch(co, cam, g[:, :, :4], gt, *tail)                            # gradient shape
    with pytest.raises(RuntimeError):
        dsacstar.backward_rgbd_batch(co, cam, g.double(), gt, *tail)                             # gradient dtype
    with pytest.raises(RuntimeError):
        dsacstar.backward_rgbd_batch(co, cam, g, torch.eye(4), 0, *tail[1:])                     # no hypotheses
    with pytest.raises(RuntimeError):
        dsacstar.backward_rgbd_batch(co, cam, g, torch.zeros(2, 4, 4), *tail)                    # one pose per image
    with pytest.raises(RuntimeError):
        dsacstar.backward_rgbd_batch(co, cam, g, gt, *tail)                                      # CPU tensors: no fallback
    big = torch.zeros(1, 3, 80, 80)
    with pytest.raises(RuntimeError, match="6400 cells exceed the limit of 6144"):
        dsacstar.backward_rgbd_batch(big, big, big, gt, *tail)
    with pytest.raises(NotImplementedError):
        dsacstar.backward_rgbd()
    assert dsacstar.RGBD_BWD_REC == bref.REC


# --------------------------------------------------------------------------------- 7. sanitizer run

def test_sanitizer_run_of_the_restatement(tmp_path):
    """tests/dsac_rgbd_bwd_ref.c with its own main() under AddressSanitizer + UBSan on an 8x12 and a 17x23 scene: exit 0, no
    report.  Only this stand-alone program is sanitized."""
    prog = bref.build_program(tmp_path, sanitize=True)
    for Ho, Wo, noise in ((8, 12, 0.0), (17, 23, 0.05)):
        sc = scene_of(Ho, Wo, noise, 31)
        path = tmp_path / ("scene_%dx%d.bin" % (Ho, Wo))
        with open(path, "wb") as f:
            f.write(np.ascontiguousarray(sc["coords"]).tobytes())
            f.write(np.ascontiguousarray(sc["cam"]).tobytes())
            f.write(np.ascontiguousarray(sc["gt"], np.float32).tobytes())
        r = subprocess.run([prog, str(path), str(Ho), str(Wo), "32", str(THR), str(MAX_DIST)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        assert "camera form: status 0" in r.stdout and "depth form: status 0" in r.stdout
