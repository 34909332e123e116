"""CPU: the fixed-size augmentation (xl_data_canvas_augment: a scale and a rotation per frame onto a canvas of the frame's own
size) through its host restatement tests/canvas_ref.py - the geometry it implies for the focal length and the pose, the set of
cells it fills - the refusals of the two new entry points, the random draws of CamLocDataset(canvas=True), and the options
that switch it on (--aug_canvas in the common parser and in train_e2e)."""
import ctypes
import math
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import canvas_ref                                       # noqa: E402
from crossloc_amd import data, dataset, synth          # noqa: E402

SUB = 8
SCALES = (2 / 3, 1.0, 1.2345, 1.5)
ANGLES = (0.0, 20.0, -30.0, 7.5)
GRIDS = ((60, 90), (8, 12), (7, 11))


def _bound(scale):
    """Nearest resampling moves the content of a cell by at most half a SOURCE cell per axis; a source cell is 8 sigma output
    pixels wide: 4 sqrt(2) sigma px.  The slack is the one tests/test_pose_rotation_cpu.py derives (float32 coordinates of
    magnitude ~500 m seen from 150-350 m at focal 480: about 1e-4 px)."""
    return 4.0 * math.sqrt(2.0) * scale + 1e-3


def _reprojection_errors(label, pose, focal):
    """label [3,Ho,Wo] float32 with -1 fill, pose float64 cam->world: the distance in px of every non-fill cell's reprojection
    from its cell centre, in float64."""
    Ho, Wo = label.shape[1:]
    keep = (label != synth.NODATA).all(0)
    X = label.astype(np.float64)[:, keep]
    cam = pose[:3, :3].T @ (X - pose[:3, 3:4])
    v, u = np.nonzero(keep)
    du = focal * cam[0] / cam[2] + Wo * SUB / 2.0 - (u * SUB + SUB // 2)
    dv = focal * cam[1] / cam[2] + Ho * SUB / 2.0 - (v * SUB + SUB // 2)
    assert (cam[2] > 0).all()
    return np.hypot(du, dv)


@pytest.fixture(scope="module")
def scenes():
    """Exact coordinate maps, two seeds per grid size; computed once, never modified."""
    return {(Ho, Wo): [synth.make_scene(seed, noise=0, outlier_ratio=0, Ho=Ho, Wo=Wo) for seed in (100, 101)] for Ho, Wo in GRIDS}


@pytest.mark.parametrize("angle", ANGLES)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("Ho,Wo", GRIDS)
def test_warped_labels_reproject_under_the_scaled_focal_and_the_rotated_pose_only(scenes, Ho, Wo, scale, angle):
    for sc in scenes[(Ho, Wo)]:
        gt = sc["gt_coords"]
        lab, inside = canvas_ref.canvas_frame(gt, scale, angle, -1.0, False)
        filled = (lab != synth.NODATA).all(0)
        assert not filled[~inside].any() and filled.mean() > 0.3
        pose, focal = sc["pose"] @ data.pose_rotation(angle), sc["focal"] * scale
        err = _reprojection_errors(lab, pose, focal)
        assert err.max() <= _bound(scale), (scale, angle, err.max())
        if (Ho, Wo) != (60, 90):
            continue                                     # the border is far enough from the centre at 60 x 90 only
        # wrong geometry must fail: the unscaled focal length where the scale is far from 1 (at scale 1 it is the right one),
        # the unrotated and the counter-rotated pose where the angle is far from 0 (at angle 0 they are the right one)
        if abs(scale - 1) >= 0.25:
            assert _reprojection_errors(lab, pose, sc["focal"]).max() > 2 * _bound(scale)
        if abs(angle) >= 20:
            for wrong in (sc["pose"], sc["pose"] @ data.pose_rotation(-angle)):
                assert _reprojection_errors(lab, wrong, focal).max() > 2 * _bound(scale)


# The pairs are chosen so that the float64 prediction leaves at most 1 % of the grid undecided (asserted below: a condition of
# the comparison, checked on the prediction alone).  Left out are the pairs whose source coordinates hit rounding ties by
# arithmetic: scale 3/2 at angle 0 (column j maps to (j - 44.5) / 1.5 + 44.5: every third column is a tie), and on some
# grids sin(30 deg) = 1/2 and cos(30 deg) * 3/2 = 1.2990 with the rational scales.  On the 8 x 12 and 7 x 11 grids 1 % is less
# than one cell, so only pairs without any undecided cell qualify there.
_BIG = ([(s, a) for s in SCALES for a in (20.0, 7.5, 12.345)]
        + [(2 / 3, 0.0), (1.0, 0.0), (1.2345, 0.0), (1.0, -30.0), (1.2345, -30.0), (1.5, -30.0)])
_SMALL = [(s, 20.0) for s in SCALES] + [(1.0, 0.0), (1.2345, 0.0), (2 / 3, 7.5), (1.0, 7.5), (1.5, 7.5), (1.2345, -30.0), (1.5, -30.0)]
SET_CASES = ([(60, 90, s, a) for s, a in _BIG] + [(96, 144, s, a) for s, a in _BIG]
             + [(8, 12, s, a) for s, a in _SMALL] + [(7, 11, s, a) for s, a in _SMALL])


@pytest.mark.parametrize("H,W,scale,angle", SET_CASES)
def test_the_filled_cells_are_the_geometric_prediction(H, W, scale, angle):
    x = np.random.default_rng(3).uniform(1.0, 2.0, size=(1, H, W)).astype(np.float32)
    want, undecided = canvas_ref.predicted_inside(H, W, scale, angle, 1e-3)
    assert undecided.mean() <= 0.01, undecided.mean()
    for bilinear in (False, True):
        out, inside = canvas_ref.canvas_frame(x, scale, angle, -1.0, bilinear)
        assert ((out[0] != -1.0) == inside).all()
        assert (inside == want)[~undecided].all()
    if scale == 1.0 and angle == 0.0:
        assert inside.all() and out.tobytes() == x.tobytes()


def test_the_restatement_at_scale_one_is_the_rotation_oracle():
    """Nearest mode with scale 1 is the per-frame rotation of the batched augmentation: the restatement against the oracle of
    that path (oracle/data_oracle.py, pinned against torchvision) on a label map."""
    from oracle import data_oracle as do
    lab = torch.randn(1, 3, 12, 18, generator=torch.Generator().manual_seed(4))
    for angle in (-30.0, 12.345, 20.0):
        want = do.batch_resize_labels(lab, 12, 18, angle, -1.0)[0].numpy()
        got = canvas_ref.canvas_frame(lab[0].numpy(), 1.0, angle, -1.0, False)[0]
        assert got.tobytes() == want.tobytes(), angle


def test_the_new_entry_points_refuse_bad_arguments_before_any_gpu_call():
    from crossloc_amd import build
    lib = ctypes.CDLL(build.build())
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    buf = ctypes.cast((ctypes.c_float * 64)(), vp)
    other = ctypes.cast((ctypes.c_float * 64)(), vp)
    d2 = ctypes.c_double * 2
    scales, angles = d2(1.2, 0.8), d2(10.0, -20.0)
    fn = lib.xl_data_canvas_augment
    fn.restype, fn.argtypes = ci, [vp, vp, ci, ci, ci, ci, vp, vp, cf, ci, vp]
    assert fn(None, other, 2, 1, 2, 2, scales, angles, -1.0, 0, None) == -1
    assert fn(buf, None, 2, 1, 2, 2, scales, angles, -1.0, 0, None) == -1
    assert fn(buf, buf, 2, 1, 2, 2, scales, angles, -1.0, 0, None) == -1                 # in place: a gather cannot be
    assert fn(buf, other, 2, 1, 2, 2, None, angles, -1.0, 0, None) == -1
    assert fn(buf, other, 2, 1, 2, 2, scales, None, -1.0, 1, None) == -1
    for bad in ((0, 1, 2, 2), (2, 0, 2, 2), (2, 1, 0, 2), (2, 1, 2, 0), (-1, 1, 2, 2)):
        assert fn(buf, other, *bad, scales, angles, -1.0, 0, None) == -1
    for s in (0.0, -1.5, float("nan"), float("inf"), -float("inf")):
        for at in (0, 1):
            bad = [1.2, 0.8]
            bad[at] = s
            for bilinear in (0, 1):
                assert fn(buf, other, 2, 1, 2, 2, d2(*bad), angles, -1.0, bilinear, None) == -1, (s, at)
    assert fn(buf, other, 2, 1, 2, 2, scales, d2(10.0, float("nan")), -1.0, 0, None) == -1

    fn = lib.xl_loss_coord_frames_ld
    fn.restype = ci
    fn.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, cf, cf, cf, cf, cf, cf, cf, cf, ci, ci, vp, vp, vp, vp, vp]
    tail = (48.0, 32.0, 8.0, 0.1, 100.0, 1000.0, 50.0, -1.0)

    def call(pred=buf, unc=buf, poses=buf, gt=buf, B=1, Ho=2, Wo=2, ldp=4, ldu=4, focals=buf, mode=1, ws=buf, out=buf):
        return fn(pred, unc, poses, gt, B, Ho, Wo, ldp, ldu, focals, *tail, mode, 0, buf, buf, ws, out, None)
    for kw in (dict(pred=None), dict(poses=None), dict(gt=None), dict(focals=None), dict(ws=None), dict(out=None),
               dict(unc=None), dict(B=0), dict(Ho=0), dict(Wo=0), dict(B=-2), dict(ldp=2), dict(ldu=0)):
        assert call(**kw) == -1, kw
    assert call(focals=None, mode=0, unc=None) == -1


def _dataset(tmp_path, **kw):
    (tmp_path / "rgb").mkdir(exist_ok=True)
    return dataset.CamLocDataset(str(tmp_path), augment=True, **kw)


@pytest.mark.parametrize("rotation", [30, 12.5, 0])
def test_draw_geometry_with_canvas_draws_a_scale_and_an_angle_per_frame(tmp_path, rotation):
    ds = _dataset(tmp_path, canvas=True, aug_rotation=rotation)
    assert ds.canvas is True and ds.rotate_poses is False
    for n in (1, 3, 16):
        random.seed(7)
        scales, angles = ds.draw_geometry(n)
        after = random.getstate()
        random.seed(7)
        want_s, want_a = [], []
        for _ in range(n):                                                      # frame by frame: scale, then angle
            want_s.append(random.uniform(2 / 3, 3 / 2))
            want_a.append(random.uniform(-rotation, rotation))
        assert random.getstate() == after                                       # 2 n draws, also at aug_rotation = 0
        assert scales == want_s and angles == want_a and len(scales) == len(angles) == n
        assert all(2 / 3 <= s <= 3 / 2 for s in scales) and all(-rotation <= a <= rotation for a in angles)
        random.seed(7)
        assert ds.draw_geometry(n) == (scales, angles)
    assert len(set(scales)) == 16
    assert (len(set(angles)) == 16) if rotation else (angles == [0.0] * 16)


@pytest.mark.parametrize("k", [0, 11])
def test_draw_geometry_without_canvas_is_what_it_was(tmp_path, k):
    ds = _dataset(tmp_path)
    assert ds.canvas is False
    random.seed(k)
    got = ds.draw_geometry(5)
    after = random.getstate()
    random.seed(k)
    assert got == (random.uniform(2 / 3, 3 / 2), random.uniform(-30, 30)) and random.getstate() == after
    ds = _dataset(tmp_path, rotate_poses=True)
    random.seed(k)
    got = ds.draw_geometry(3)
    random.seed(k)
    assert got == (random.uniform(2 / 3, 3 / 2), [random.uniform(-30, 30) for _ in range(3)])


def test_canvas_needs_the_batched_augmenting_path(tmp_path):
    (tmp_path / "rgb").mkdir()
    for kw in (dict(augment=False), dict(augment=True, batch=False)):
        with pytest.raises((ValueError, NotImplementedError)):
            dataset.CamLocDataset(str(tmp_path), canvas=True, **kw)


def _e2e(*extra):
    from crossloc_amd import train_e2e
    return train_e2e._config_parser(["naturescape", "--network_in", "model.net", *extra])


@pytest.mark.parametrize("mode", ["rgb", "rgbd"])
def test_train_e2e_aug_canvas(mode, tmp_path):
    from crossloc_amd import train_e2e
    off = _e2e("--mode", mode)
    assert off.aug_canvas is False and "-canvas" not in train_e2e.get_output_path(off)
    ds = _dataset(tmp_path, **train_e2e.dataset_options(off))
    assert ds.canvas is False
    if mode == "rgbd":
        assert ds.aug_scale_min == ds.aug_scale_max == 1                        # without the flag: scale 1, as it was
    opt = _e2e("--mode", mode, "--aug_canvas")
    on = train_e2e.dataset_options(opt)
    assert on == dict(coord=True, depth=mode == "rgbd", aug_rotation=0, canvas=True)
    ds = _dataset(tmp_path, **on)
    assert ds.canvas and ds.aug_rotation == 0 and not ds.rotate_poses and ds.depth == (mode == "rgbd")
    assert (ds.aug_scale_min, ds.aug_scale_max) == (2 / 3, 3 / 2)               # the grid stays 60 x 90: rgbd scales again
    path = train_e2e.get_output_path(opt)
    assert path.endswith("-canvas") and "-rot" not in path
    both = _e2e("--mode", mode, "--aug_canvas", "--aug_rotation", "30", "--tiny")
    assert train_e2e.dataset_options(both) == dict(on, aug_rotation=30.0)
    assert "-rot30-canvas-tiny" in train_e2e.get_output_path(both)


def test_aug_canvas_in_the_common_parser_is_for_every_task():
    from crossloc_amd import finetune_decoder_single_task, train_single_task
    weights = ["--encoders", "coord", "--coord_weight", "c", "--depth_weight", "d", "--normal_weight", "n",
               "--semantics_weight", "s"]
    for mod, more in ((train_single_task, []), (finetune_decoder_single_task, weights)):
        for task in ("coord", "depth", "normal"):
            assert mod._config_parser(["naturescape", "--task", task] + more).aug_canvas is False
            assert mod._config_parser(["naturescape", "--task", task, "--aug_canvas"] + more).aug_canvas is True
        assert mod._config_parser(["naturescape", "--task", "semantics", "--fullsize", "--aug_canvas"] + more).aug_canvas is True
