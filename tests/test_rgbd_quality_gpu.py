"""GPU parity of the RGB-D pose-quality pass: xl_dsac_pose_quality_rgbd_batch (through dsacstar.pose_quality_rgbd_batch) against
the serial C restatement tests/rgbd_quality_ref.c.  Every row comparison is bitwise on all 64 doubles (NaNs by position): the two
sides compile the same header, so this checks the kernel's orchestration - the two cell walks, the strides, the butterfly and
wave order, the centroid between the walks - and that gcc and hipcc agree.  The formulas: tests/test_rgbd_quality_cpu.py."""
import numpy as np
import pytest

import rgbd_quality_cases as qc
import rgbd_quality_ref
from crossloc_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PAR = (qc.NOISY_THR, qc.ALPHA, qc.NOISY_MAX_DIST)


@pytest.fixture(scope="module")
def qref(tmp_path_factory):
    return rgbd_quality_ref.load(tmp_path_factory.mktemp("rgbd_quality_ref"))


def _dev(a, dtype=np.float32):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _rows(coords, poses, par=PAR, cam=None, depth=None, **kw):
    """coords / cam / depth: numpy (uploaded contiguous) or torch CUDA tensors (used as they are); poses [B,4,4] -> numpy [B,64]"""
    import dsacstar
    coords = _dev(coords)
    out = dsacstar.pose_quality_rgbd_batch(coords, None if cam is None else _dev(cam), _dev(poses), *par,
                                           depth=None if depth is None else _dev(depth), **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.float64 and tuple(out.shape) == (coords.shape[0], 64)
    return out.cpu().numpy()


def _depth_kw(bt):
    return dict(focalLength=bt["focal"], ppointX=bt["ppx"], ppointY=bt["ppy"], subSampling=qc.SUB)


def _assert_rows(qref, got, bt, poses, frames, what, par=PAR):
    for b in frames:
        want = qref.row(bt["coords"][b], poses[b], *par, cam=bt["cam"][b])
        assert qc.same_bits(got[b], want), (what, b, np.flatnonzero(got[b] != want))


@pytest.mark.parametrize("Ho,Wo", [(60, 90), (37, 53), (7, 9), (129, 128)])
def test_rows_bit_exact_at_grid_sizes(qref, Ho, Wo):
    """5400 cells; 1961 (no multiple of 64); 63 (less than a wave, most threads idle); 16512 (above the solver's cell limit: ground
    truth poses only).  Frames 0, 2 and 5 of a batch of 6 (0.5 m noise, 1 % depth noise, 20 % holes, 30 % outliers), at ground
    truth and at the pose forward_rgbd_batch wrote."""
    import dsacstar
    B, frames = 6, (0, 2, 5)
    bt = qc.batch(4021, B, Ho, Wo, **qc.NOISY)
    N = Ho * Wo
    got = _rows(bt["coords"], bt["pose"], cam=bt["cam"])
    _assert_rows(qref, got, bt, bt["pose"], frames, "ground truth")
    n_valid = (bt["depth"].reshape(B, -1) != 0).sum(1)
    assert (got[:, 0] == N).all() and np.array_equal(got[:, 58], n_valid) and (n_valid < N).all()
    assert (got[:, 1] <= got[:, 58]).all()
    if N >= 1000:
        # 80 % valid, 70 % of them no outliers, and 1 % depth noise at 150 to 350 m puts part of the rest beyond 3 m
        assert (got[:, 6] == 0).all() and (got[:, 1] > 0.2 * N).all() and (got[:, 1] < 0.6 * N).all()
    if N > dsacstar.RGBD_MAX_CELLS:
        return
    co, cam = _dev(bt["coords"]), _dev(bt["cam"])
    est = torch.zeros((B, 4, 4), dtype=torch.float32, device="cuda")
    dbg = dsacstar.forward_rgbd_batch(co, cam, est, 64, *PAR, debug=True)["dbg"]
    got = _rows(co, est, cam=cam)
    dbg = dbg.cpu().numpy()
    _assert_rows(qref, got, bt, est.cpu().numpy(), frames, "solver pose")
    assert np.array_equal(got[:, 58], dbg[:, 1])
    if N >= 1000:
        # the refinement's last inlier count belongs to the pose before its last fit, and the row re-reads the pose from float32
        assert np.abs(got[:, 1] - dbg[:, 3]).max() <= 0.01 * N
        assert (got[:, 6] == 0).all() and (got[:, 8] < 1.0).all() and (got[:, 9] < 0.5).all()


@pytest.fixture(scope="module")
def one_batch():
    bt = qc.batch(4100, 6, 37, 53, **qc.NOISY)
    return bt, _rows(bt["coords"], bt["pose"], cam=bt["cam"])


def test_depth_form_and_per_image_focals(qref, one_batch):
    """the depth form is bitwise the camera-coordinate form given camera_coordinates(depth); per-image focals give, frame by
    frame, the bits of the scalar form"""
    import dsacstar
    bt, base = one_batch
    _assert_rows(qref, base, bt, bt["pose"], range(6), "contiguous")
    kw = _depth_kw(bt)
    got = _rows(bt["coords"], bt["pose"], depth=bt["depth"], **kw)
    cam = dsacstar.camera_coordinates(_dev(bt["depth"]), bt["focal"], 37 * qc.SUB, 53 * qc.SUB, qc.SUB)
    assert qc.same_bits(got, _rows(bt["coords"], bt["pose"], cam=cam))
    assert qc.same_bits(got, base)                                       # (the scenes' camera tensor is the same formula in numpy)
    focals = [480.0, 455.5, 512.25, 480.0, 470.0, 500.0]
    per = _rows(bt["coords"], bt["pose"], depth=bt["depth"], focals=torch.tensor(focals), ppointX=kw["ppointX"], ppointY=kw["ppointY"],
                subSampling=qc.SUB)
    for b, f in enumerate(focals):
        one = _rows(bt["coords"][b:b + 1], bt["pose"][b:b + 1], depth=bt["depth"][b:b + 1], **dict(kw, focalLength=f))
        assert qc.same_bits(per[b], one[0]), b
        want = qref.row(bt["coords"][b], bt["pose"][b], *PAR, depth=bt["depth"][b], focal=f, ppx=bt["ppx"], ppy=bt["ppy"], sub=qc.SUB)
        assert qc.same_bits(per[b], want), b
    assert qc.same_bits(per[0], base[0]) and not qc.same_bits(per[1], base[1])


def _strided_forms(t):
    """a contiguous [B,C,Ho,Wo] CUDA tensor as: the channel slice of a wider tensor, channels-last, a padded row pitch"""
    B, C, Ho, Wo = t.shape
    wide_c = torch.randn((B, C + 1, Ho, Wo), device="cuda")
    wide_c[:, :C] = t
    sl = wide_c[:, :C]
    cl = t.contiguous(memory_format=torch.channels_last)
    wide = torch.full((B, C, Ho + 3, Wo + 11), float("nan"), device="cuda")
    wide[:, :, 2:2 + Ho, 5:5 + Wo] = t
    pitched = wide[:, :, 2:2 + Ho, 5:5 + Wo]
    assert not sl.is_contiguous() and cl.stride(1) == 1 and pitched.stride(2) == Wo + 11
    return dict(channel_slice=sl, channels_last=cl, pitched=pitched)


def test_strided_inputs_give_the_bits_of_the_contiguous_copy(one_batch):
    bt, base = one_batch
    co, cam, depth = _dev(bt["coords"]), _dev(bt["cam"]), _dev(bt["depth"])
    for name, view in _strided_forms(co).items():
        assert qc.same_bits(_rows(view, bt["pose"], cam=cam), base), ("coords", name)
    for name, view in _strided_forms(cam).items():
        assert qc.same_bits(_rows(co, bt["pose"], cam=view), base), ("cam", name)
    kw = _depth_kw(bt)
    pred = torch.randn((6, 4, 37, 53), device="cuda")
    pred[:, 3] = depth
    inter = torch.randn((6, 37, 53, 2), device="cuda")
    inter[..., 0] = depth
    wide = torch.full((6, 40, 64), float("nan"), device="cuda")
    wide[:, 2:39, 5:58] = depth
    for name, view in (("channel_slice", pred[:, 3]), ("interleaved", inter[..., 0]), ("pitched", wide[:, 2:39, 5:58])):
        assert not view.is_contiguous()
        assert qc.same_bits(_rows(co, bt["pose"], depth=view, **kw), base), ("depth", name)
    both = _strided_forms(co)["pitched"], _strided_forms(cam)["channels_last"]
    assert qc.same_bits(_rows(both[0], bt["pose"], cam=both[1]), base)


def test_slot_independence(one_batch):
    bt, base = one_batch
    co, cam, poses = bt["coords"], bt["cam"], bt["pose"]
    alone = _rows(co[3:4], poses[3:4], cam=cam[3:4])
    assert qc.same_bits(alone[0], base[3])
    first = [3, 0, 1, 2, 4, 5]
    got = _rows(co[first], poses[first], cam=cam[first])
    assert qc.same_bits(got[0], base[3]) and qc.same_bits(got[1], base[0])
    last = [0, 1, 2, 4, 5, 3]
    got = _rows(co[last], poses[last], cam=cam[last])
    assert qc.same_bits(got[5], base[3]) and qc.same_bits(got[4], base[5])


@pytest.mark.parametrize("Ho,Wo", [(12, 16), (200, 4)])
def test_status_cases(qref, Ho, Wo):
    par = (qc.THR, qc.ALPHA, qc.MAX_DIST)
    for name, co, cam, pose, status, n_inl, n_valid in qc.status_cases(Ho, Wo):
        got = _rows(co[None], pose[None], par=par, cam=cam[None])[0]
        qc.assert_status_row(got, status, n_inl, n_valid, Ho, Wo)
        assert qc.same_bits(got, qref.row(co, pose, *par, cam=cam)), name


class _PlantNet(torch.nn.Module):
    """Stand-in for the network in the wiring test: the solver's input is given by the caller (`scene_coords`)."""
    num_task_channel = 3
    OUTPUT_SUBSAMPLE = qc.SUB

    def forward(self, images, plan_slot=0):
        return torch.zeros((images.shape[0], 4, 60, 90), device=images.device)


def test_localize_batch_and_pipelined_localizer_wiring():
    """quality="rgbd": the poses of the plain call, the rows of a separate pose_quality_rgbd_batch call; quality=True with depth:
    still the reprojection pass's rows; quality="rgbd" without depth raises"""
    import dsacstar
    from crossloc_amd import evaluation
    bt = qc.batch(5200, 4, 60, 90, **qc.NOISY)
    co, depth, cam = _dev(bt["coords"]), _dev(bt["depth"]), _dev(bt["cam"])
    images = torch.zeros((4, 3, 480, 720), device="cuda")
    net = _PlantNet()
    kw = dict(image0=3, scene_coords=co, rgbd_threshold=PAR[0], max_dist_error=PAR[2])
    loc_args = (net, images, 64, synth.FOCAL, 480, 720)
    plain = evaluation.localize_batch(*loc_args, depth=depth, **kw)
    out = evaluation.localize_batch(*loc_args, depth=depth, quality="rgbd", **kw)
    out_cam = evaluation.localize_batch(*loc_args, cam_coords=cam, quality="rgbd", **kw)
    rgb = evaluation.localize_batch(*loc_args, depth=depth, quality=True, **kw)
    torch.cuda.synchronize()
    assert len(plain) == 2 and len(out) == 3 and len(out_cam) == 3 and len(rgb) == 3
    assert torch.equal(out[0], plain[0]) and torch.equal(out_cam[0], plain[0]) and torch.equal(rgb[0], plain[0])
    sep = dsacstar.pose_quality_rgbd_batch(co, None, plain[0], *PAR, depth=depth, focalLength=synth.FOCAL, ppointX=360.0, ppointY=240.0,
                                           subSampling=qc.SUB)
    sep_rgb = dsacstar.pose_quality_batch(co, plain[0], 10.0, synth.FOCAL, 360.0, 240.0, 100.0, 100.0, qc.SUB)
    torch.cuda.synchronize()
    sep, sep_rgb = sep.cpu().numpy(), sep_rgb.cpu().numpy()
    assert qc.same_bits(out[2].cpu().numpy(), sep) and qc.same_bits(out_cam[2].cpu().numpy(), sep) and (sep[:, 6] == 0).all()
    assert qc.same_bits(rgb[2].cpu().numpy(), sep_rgb) and not qc.same_bits(sep, sep_rgb)
    assert (sep[:, 58] == (bt["depth"].reshape(4, -1) != 0).sum(1)).all() and (sep_rgb[:, 58] == 0).all()
    table = evaluation.selective_accuracy(np.arange(4.0), np.ones(4), sep[:, dsacstar.RGBD_QUALITY_FIELDS["sigma_pos_m"]], keep=(0.5,))
    assert table[0][1] == 2                                              # column 8 as in the RGB row: the table takes it unchanged

    loc = evaluation.PipelinedLocalizer(net, 64, synth.FOCAL, 480, 720)
    p_plain = loc.submit(images, depth=depth, **kw)
    p_out = loc.submit(images, depth=depth, quality="rgbd", **kw)
    p_rgb = loc.submit(images, depth=depth, quality=True, **kw)
    loc.finish()
    torch.cuda.synchronize()
    assert len(p_plain) == 2 and len(p_out) == 3 and len(p_rgb) == 3
    assert torch.equal(p_plain[0], plain[0]) and torch.equal(p_out[0], plain[0]) and torch.equal(p_rgb[0], plain[0])
    assert qc.same_bits(p_out[2].cpu().numpy(), sep) and qc.same_bits(p_rgb[2].cpu().numpy(), sep_rgb)
    with pytest.raises(RuntimeError, match="needs depth or cam_coords"):
        loc.submit(images, image0=3, scene_coords=co, quality="rgbd")
    with pytest.raises(RuntimeError, match="needs depth or cam_coords"):
        evaluation.localize_batch(*loc_args, image0=3, scene_coords=co, quality="rgbd")
