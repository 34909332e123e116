"""CPU: the convention of the pose rotation that goes with the frame rotation of the batched augmentation
(data.pose_rotation, the host restatement of xl_data_rotate_poses), the random draws of CamLocDataset.draw_geometry, and
the options that switch it on (train_e2e --aug_rotation, common_parser --rotate_poses)."""
import math
import random

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from crossloc_amd import data, dataset, synth          # noqa: E402
from oracle import data_oracle as do                    # noqa: E402

SUB = 8
# nearest-neighbour resampling moves the content of a cell by at most half a cell (4 px) per axis: 4 sqrt(2) px.  The slack
# covers the float32 coordinates (magnitude ~500 m, seen from 150-350 m at focal 480: about 1e-4 px).
BOUND = 4.0 * math.sqrt(2.0) + 1e-3


def _reprojection_errors(label, pose, focal):
    """label [3,Ho,Wo] float32 with -1 fill, pose float64 cam->world: (distance in px of every non-fill cell's
    reprojection from its cell centre, in float64; the share of non-fill cells)."""
    Ho, Wo = label.shape[1:]
    keep = (label != synth.NODATA).all(0)
    X = label.astype(np.float64)[:, keep]
    cam = pose[:3, :3].T @ (X - pose[:3, 3:4])
    v, u = np.nonzero(keep)
    du = focal * cam[0] / cam[2] + Wo * SUB / 2.0 - (u * SUB + SUB // 2)
    dv = focal * cam[1] / cam[2] + Ho * SUB / 2.0 - (v * SUB + SUB // 2)
    assert (cam[2] > 0).all()
    return np.hypot(du, dv), keep.mean()


@pytest.mark.parametrize("angle", [20.0, -30.0, 7.5])
@pytest.mark.parametrize("Ho,Wo", [(60, 90), (8, 12), (7, 11)])
def test_rotated_labels_reproject_under_the_rotated_pose_only(Ho, Wo, angle):
    for seed in range(100, 104):
        sc = synth.make_scene(seed, noise=0, outlier_ratio=0, Ho=Ho, Wo=Wo)
        rot = do.batch_resize_labels(torch.from_numpy(sc["gt_coords"])[None], Ho, Wo, angle, -1.0)[0].numpy()
        err, share = _reprojection_errors(rot, sc["pose"] @ data.pose_rotation(angle), sc["focal"])
        assert share >= 0.8, (seed, share)
        assert err.max() <= BOUND, (seed, err.max())
        if abs(angle) >= 20:
            for wrong in (sc["pose"], sc["pose"] @ data.pose_rotation(-angle)):
                assert _reprojection_errors(rot, wrong, sc["focal"])[0].max() > 2 * BOUND


def test_pose_rotation_is_rz():
    r = data.pose_rotation(30.0)
    assert r.dtype == np.float64 and r.shape == (4, 4)
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    assert np.array_equal(r, np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]))
    assert np.array_equal(data.pose_rotation(0.0), np.eye(4))


def test_the_new_entry_points_refuse_bad_arguments_before_any_gpu_call():
    import ctypes
    from crossloc_amd import build
    lib = ctypes.CDLL(build.build())
    angles = (ctypes.c_double * 2)(10.0, 20.0)
    buf = ctypes.cast((ctypes.c_float * 32)(), ctypes.c_void_p)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.xl_data_rotate_poses.argtypes = [vp, vp, ci, vp, vp]
    assert lib.xl_data_rotate_poses(None, buf, 2, angles, None) == -1
    assert lib.xl_data_rotate_poses(buf, None, 2, angles, None) == -1
    assert lib.xl_data_rotate_poses(buf, buf, 2, None, None) == -1
    assert lib.xl_data_rotate_poses(buf, buf, 0, angles, None) == -1
    lib.xl_data_batch_augment_frames.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp, ctypes.c_float, ci, vp]
    assert lib.xl_data_batch_augment_frames(None, buf, 2, 1, 2, 2, 2, 2, angles, -1.0, 0, None) == -1
    assert lib.xl_data_batch_augment_frames(buf, None, 2, 1, 2, 2, 2, 2, angles, -1.0, 0, None) == -1
    assert lib.xl_data_batch_augment_frames(buf, buf, 2, 1, 2, 2, 2, 2, None, -1.0, 0, None) == -1
    for bad in ((0, 1, 2, 2, 2, 2), (2, 0, 2, 2, 2, 2), (2, 1, 0, 2, 2, 2), (2, 1, 2, 0, 2, 2), (2, 1, 2, 2, 0, 2), (2, 1, 2, 2, 2, 0)):
        assert lib.xl_data_batch_augment_frames(buf, buf, *bad, angles, -1.0, 0, None) == -1


def _dataset(tmp_path, **kw):
    (tmp_path / "rgb").mkdir(exist_ok=True)
    return dataset.CamLocDataset(str(tmp_path), augment=True, **kw)


@pytest.mark.parametrize("k", [0, 11, 2021])
def test_draw_geometry_off_is_the_two_draws_of_the_reference(tmp_path, k):
    ds = _dataset(tmp_path)
    assert ds.rotate_poses is False
    random.seed(k)
    got = ds.draw_geometry(5)
    after = random.getstate()
    random.seed(k)
    want = (random.uniform(2 / 3, 3 / 2), random.uniform(-30, 30))
    assert got == want and isinstance(got[1], float)
    assert random.getstate() == after


def test_draw_geometry_on_draws_one_angle_per_frame(tmp_path):
    ds = _dataset(tmp_path, rotate_poses=True, aug_rotation=12.5)
    for n in (1, 3, 16):
        random.seed(7)
        scale, angles = ds.draw_geometry(n)
        after = random.getstate()
        random.seed(7)
        want_scale = random.uniform(2 / 3, 3 / 2)
        want = [random.uniform(-12.5, 12.5) for _ in range(n)]
        assert random.getstate() == after                                   # 1 + n draws
        assert scale == want_scale and angles == want and len(angles) == n
        assert all(-12.5 <= a <= 12.5 for a in angles)
        random.seed(7)
        assert ds.draw_geometry(n) == (scale, angles)
    assert len(set(angles)) == 16


def _e2e(*extra):
    from crossloc_amd import train_e2e
    return train_e2e._config_parser(["naturescape", "--network_in", "model.net", *extra])


@pytest.mark.parametrize("mode", ["rgb", "rgbd"])
def test_train_e2e_aug_rotation(mode, tmp_path):
    from crossloc_amd import train_e2e
    off = train_e2e.dataset_options(_e2e("--mode", mode))
    want = dict(coord=True, depth=mode == "rgbd", aug_rotation=0)
    if mode == "rgbd":
        want.update(aug_scale_min=1, aug_scale_max=1)
    assert off == want and _e2e("--mode", mode).aug_rotation == 0                   # the default: what it was
    assert "-rot" not in train_e2e.get_output_path(_e2e("--mode", mode))
    opt = _e2e("--mode", mode, "--aug_rotation", "30")
    on = train_e2e.dataset_options(opt)
    assert on == dict(want, aug_rotation=30.0, rotate_poses=True)
    assert "-rot30" in train_e2e.get_output_path(opt)
    ds = _dataset(tmp_path, **on)
    assert ds.rotate_poses and ds.aug_rotation == 30.0
    if mode == "rgbd":
        assert ds.aug_scale_min == ds.aug_scale_max == 1 and ds.depth
    with pytest.raises(SystemExit):
        _e2e("--aug_rotation", "-5")


def test_rotate_poses_option_is_for_the_coord_task():
    from crossloc_amd import finetune_decoder_single_task, train_single_task
    assert train_single_task._config_parser(["naturescape", "--task", "coord"]).rotate_poses is False
    assert train_single_task._config_parser(["naturescape", "--task", "coord", "--rotate_poses"]).rotate_poses is True
    assert train_single_task._config_parser(["naturescape", "--task", "depth"]).rotate_poses is False
    for mod in (train_single_task, finetune_decoder_single_task):
        for task in ("depth", "normal", "semantics"):
            with pytest.raises((ValueError, SystemExit)):
                mod._config_parser(["naturescape", "--task", task, "--rotate_poses"])
