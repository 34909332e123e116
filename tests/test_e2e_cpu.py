"""CPU-side checks of end-to-end DSAC* training: the finishing op's argument validation (before any HIP call, so it runs
without a GPU), the options of train_e2e.py, the augmentation it asks for, and the keys of a step."""
import ctypes

import pytest

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def op():
    from crossloc_amd import build
    L = ctypes.CDLL(build.build())
    c_i64, c_i32, c_f, c_vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    L.xl_e2e_pose_gradient.restype = c_i32
    L.xl_e2e_pose_gradient.argtypes = [c_vp, c_i64, c_i64, c_i64, c_i64, c_vp, c_i32, c_i32, c_i32, c_i32, c_f, c_f, c_f,
                                       c_vp, c_vp, c_vp]
    return L.xl_e2e_pose_gradient


def test_the_op_refuses_bad_arguments_before_any_hip_call(op):
    """Host buffers stand in for device memory: a call that got past the checks would launch on them (and fail for want of
    a device here); every case below must come back XL_ERR_ARG (-1) from the checks themselves."""
    B, Ho, Wo, C = 2, 5, 7, 4
    g = (ctypes.c_float * (B * 3 * Ho * Wo))()
    loss = (ctypes.c_double * B)()
    out = (ctypes.c_float * (B * C * Ho * Wo))()
    stats = (ctypes.c_double * ((B + 1) * 4))()
    ptr = lambda a: ctypes.cast(a, ctypes.c_void_p)
    strides = (3 * Ho * Wo, Ho * Wo, Wo, 1)

    def call(g_=g, loss_=loss, out_=out, stats_=stats, B_=B, Ho_=Ho, Wo_=Wo, C_=C):
        return op(ptr(g_) if g_ is not None else None, *strides, ptr(loss_) if loss_ is not None else None, B_, Ho_, Wo_, C_,
                  1.0, 0.0, 0.0, ptr(out_) if out_ is not None else None, ptr(stats_) if stats_ is not None else None, None)
    assert call(g_=None) == -1
    assert call(loss_=None) == -1
    assert call(out_=None) == -1
    assert call(stats_=None) == -1
    assert call(B_=0) == -1 and call(B_=-3) == -1
    assert call(C_=2) == -1 and call(C_=0) == -1
    assert call(Ho_=0) == -1 and call(Wo_=0) == -1 and call(Ho_=-1) == -1 and call(Wo_=-5) == -1
    assert call(Ho_=1 << 16, Wo_=1 << 15) == -2                  # the cell index is an int: XL_ERR_GRID
    assert all(v == 0 for v in out) and all(v == 0 for v in stats)


def _opt(*extra):
    from crossloc_amd import train_e2e
    return train_e2e._config_parser(["naturescape", "--network_in", "model.net", *extra])


def test_parser_carries_the_solver_options_with_their_defaults():
    from crossloc_amd import dsacstar
    o = _opt()
    assert o.task == "coord" and o.mode == "rgb" and o.network_in == "model.net"
    assert (o.hypotheses, o.threshold, o.inlieralpha, o.maxpixelerror) == (64, 10, 100, 100)
    assert (o.weightrot, o.weighttrans, o.softclamp, o.learningrate) == (1.0, 100.0, 100, 1e-6)
    assert (o.clip_norm, o.init_weight, o.seed) == (0.0, 0.0, dsacstar.RANSAC_SEED)
    assert o.batch_size == 4 and o.max_steps is None and not o.auto_resume            # training.common_parser's own
    o = _opt("--mode", "rgbd", "--hypotheses", "16", "--threshold", "5", "--inlieralpha", "50", "--maxpixelerror", "80",
             "--weightrot", "2", "--weighttrans", "50", "--softclamp", "10", "--learningrate", "1e-5", "--clip_norm", "3",
             "--init_weight", "0.5", "--seed", "7", "--auto_resume", "--max_steps", "5", "--uncertainty", "MLE")
    assert (o.mode, o.hypotheses, o.threshold, o.inlieralpha, o.maxpixelerror) == ("rgbd", 16, 5, 50, 80)
    assert (o.weightrot, o.weighttrans, o.softclamp, o.learningrate) == (2, 50, 10, 1e-5)
    assert (o.clip_norm, o.init_weight, o.seed, o.auto_resume, o.max_steps, o.uncertainty) == (3, 0.5, 7, True, 5, "MLE")


def test_parser_refusals():
    from crossloc_amd import train_e2e
    for argv in (["naturescape"],                                                    # no --network_in
                 ["naturescape", "--network_in", "m.net", "--mode", "depth"],
                 ["naturescape", "--network_in", "m.net", "--task", "depth"],
                 ["naturescape", "--network_in", "m.net", "--fullsize"]):
        with pytest.raises(SystemExit):
            train_e2e._config_parser(argv)


def test_the_existing_entry_points_still_require_a_task():
    from crossloc_amd import train_single_task
    with pytest.raises(SystemExit):
        train_single_task._config_parser(["naturescape"])


@pytest.mark.parametrize("mode", ["rgb", "rgbd"])
def test_augmentation_no_rotation_and_a_fixed_scale_for_rgbd(mode, tmp_path):
    from crossloc_amd import dataset, train_e2e
    kw = train_e2e.dataset_options(_opt("--mode", mode))
    assert kw["aug_rotation"] == 0 and kw["coord"] is True and kw["depth"] is (mode == "rgbd")
    (tmp_path / "rgb").mkdir()
    ds = dataset.CamLocDataset(str(tmp_path), augment=True, **kw)
    assert ds.aug_rotation == 0
    if mode == "rgbd":
        assert ds.aug_scale_min == ds.aug_scale_max == 1 and ds.depth
    else:
        assert (ds.aug_scale_min, ds.aug_scale_max) == (2 / 3, 3 / 2) and not ds.depth     # the per-batch scale stays


def test_step_keys_depend_on_the_batch_and_the_step_index_only():
    from crossloc_amd import training
    n, batch = 23, 4
    for world in (1, 2):
        for rank in range(world):
            batches = training.epoch_batches(n, 1, batch, rank, world)
            for k, b in enumerate(batches):
                seed, image0 = training.e2e_keys(1305, b, 10 + k)
                assert (seed, image0) == (1305 + 10 + k, b[0])
                assert training.e2e_keys(1305, list(b), 10 + k) == (seed, image0)          # nothing else enters
    assert training.e2e_keys(7, [5, 9], 0) != training.e2e_keys(7, [5, 9], 1)
    assert training.e2e_keys(7, [5, 9], 0) != training.e2e_keys(7, [6, 9], 0)


def test_image_keys_must_be_an_arithmetic_sequence():
    from crossloc_amd import loss
    assert loss.e2e_image_keys([4, 5, 6], 3) == (4, 1)
    assert loss.e2e_image_keys([10, 13, 16], 3) == (10, 3)
    assert loss.e2e_image_keys([9], 1) == (9, 1)
    for bad in ([4, 5, 7], [3, 2, 1], [1, 2]):
        with pytest.raises(ValueError):
            loss.e2e_image_keys(bad, 3)
    assert loss.E2E_MAX_TRIES == 4096
