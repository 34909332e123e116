"""GPU parity of the RGB-D DSAC* solver: xl_dsac_forward_rgbd_batch (through dsacstar.forward_rgbd_batch) against the serial C
restatement tests/dsac_rgbd_ref.c, bit for bit: sampled cells, tries, scores, winner, nValid, refinement rounds, inlier count,
the refined R and t as doubles and the float32 pose.  The two sides compile the same header, so this checks the kernel's
orchestration - the x-major valid list, strides, ballots, butterflies, wave order, selection, the refinement loop - and that
gcc and hipcc agree.  The formulas themselves: tests/test_dsac_rgbd_cpu.py."""
import numpy as np
import pytest

import dsac_rgbd_cases as rc
import dsac_rgbd_ref
from crossloc_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

THR, ALPHA, MAX_DIST = 50.0, 100.0, 1000.0


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return dsac_rgbd_ref.load(tmp_path_factory.mktemp("dsac_rgbd_ref"))


def _gpu(coords, n_hyp, cam=None, depth=None, thr=THR, max_dist=MAX_DIST, **kw):
    """coords / cam / depth: numpy (uploaded contiguous) or torch CUDA tensors (used as they are) -> dict of numpy arrays"""
    import dsacstar
    up = lambda a: a if a is None or isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    coords, cam, depth = up(coords), up(cam), up(depth)
    poses = torch.full((coords.shape[0], 4, 4), float("nan"), dtype=torch.float32, device="cuda")
    out = dsacstar.forward_rgbd_batch(coords, cam, poses, n_hyp, thr, ALPHA, max_dist, debug=True, depth=depth, **kw)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["pose"] = poses.cpu().numpy()
    return res


def _assert_same(got, b, want, what):
    for k in ("cells", "tries", "scores", "dbg", "pose"):
        g, w = np.ascontiguousarray(got[k][b]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, k, np.flatnonzero(g.reshape(-1) != w.reshape(-1))[:8])


GRIDS = [(5, 7, 0.4), (8, 12, 0.0), (33, 17, 0.2), (60, 90, 0.0)]


@pytest.fixture(scope="module")
def scenes():
    """one scene per (grid, outlier ratio), 0.1 m coordinate noise; holes where the grid asks for them"""
    return {(Ho, Wo, ratio): rc.rgbd_scene(7, Ho, Wo, noise=0.1, outlier_ratio=ratio, holes=holes)
            for Ho, Wo, holes in GRIDS for ratio in (0.3, 0.6)}


@pytest.mark.parametrize("ratio", [0.3, 0.6])
@pytest.mark.parametrize("Ho,Wo,holes", GRIDS)
def test_bit_exact_at_grids_and_hypothesis_counts(ref, scenes, Ho, Wo, holes, ratio):
    """5 x 7 with holes (nValid = 21 < 64: a partial wave), 8 x 12, 33 x 17 (odd width, nValid = 449: no multiple of 64 or 256),
    60 x 90 (LDS nearly full); 1, 3 (fewer than the four waves) and 32 hypotheses."""
    sc = scenes[(Ho, Wo, ratio)]
    for n_hyp in (1, 3, 32):
        got = _gpu(sc["coords"][None], n_hyp, cam=sc["cam"][None], image0=3)
        want = ref.forward(sc["coords"], n_hyp, THR, ALPHA, MAX_DIST, cam=sc["cam"], image=3)
        _assert_same(got, 0, want, (Ho, Wo, ratio, n_hyp))
        assert got["dbg"][0, 1] == Ho * Wo - round(holes * Ho * Wo)
    if Ho * Wo >= 96 and ratio == 0.3:
        t_err, r_err = synth.pose_error(sc["pose"], got["pose"][0].astype(np.float64))
        assert t_err < 1.0 and r_err < 0.5, (t_err, r_err)


def test_stride_forms(ref):
    """contiguous; a channels-last view; the [:, :3] slice of a [B,4,Ho,Wo] prediction; a camera tensor that is every second
    column of a wider buffer - all give the bits of the contiguous call"""
    sc = rc.rgbd_scene(8, 33, 17, noise=0.1, outlier_ratio=0.3, holes=0.2)
    want = ref.forward(sc["coords"], 8, THR, ALPHA, MAX_DIST, cam=sc["cam"], image=0)
    co = torch.from_numpy(sc["coords"][None]).cuda()
    cm = torch.from_numpy(sc["cam"][None]).cuda()
    _assert_same(_gpu(co, 8, cam=cm), 0, want, "contiguous")
    co_cl = co.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    cm_cl = cm.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert co_cl.stride() != co.stride()
    _assert_same(_gpu(co_cl, 8, cam=cm_cl), 0, want, "channels last")
    pred = torch.randn(1, 4, 33, 17, device="cuda")
    pred[:, :3] = co
    _assert_same(_gpu(pred[:, :3], 8, cam=cm), 0, want, "slice of a prediction")
    wide = torch.randn(1, 3, 33, 34, device="cuda")
    wide[..., ::2] = cm
    assert wide[..., ::2].stride(3) == 2
    _assert_same(_gpu(co, 8, cam=wide[..., ::2]), 0, want, "every second column")
    dwide = torch.randn(1, 33, 34, device="cuda")
    dwide[..., ::2] = torch.from_numpy(sc["depth"][None]).cuda()
    got = _gpu(pred[:, :3], 8, depth=dwide[..., ::2], focalLength=sc["focal"], ppointX=sc["ppx"], ppointY=sc["ppy"], subSampling=8)
    _assert_same(got, 0, want, "strided depth")


def test_batch_keys_and_per_image_focals(ref):
    """batch 5 with image0 = 11, image_stride = 3: row b equals the single-image call keyed 11 + 3 b (GPU and restatement);
    depth form with one focal length per image"""
    B, Ho, Wo = 5, 8, 12
    scs = [rc.rgbd_scene(40 + b, Ho, Wo, noise=0.1, outlier_ratio=0.3, holes=0.1) for b in range(B)]
    coords = np.stack([s["coords"] for s in scs])
    cam = np.stack([s["cam"] for s in scs])
    got = _gpu(coords, 16, cam=cam, image0=11, image_stride=3)
    for b in range(B):
        _assert_same(got, b, ref.forward(coords[b], 16, THR, ALPHA, MAX_DIST, cam=cam[b], image=11 + 3 * b), ("batch", b))
        one = _gpu(coords[b:b + 1], 16, cam=cam[b:b + 1], image0=11 + 3 * b)
        for k in got:
            assert got[k][b].tobytes() == one[k][0].tobytes(), (k, b)
    focals = np.array([480.0, 455.5, 512.25, 470.0, 499.0], np.float32)
    depth = np.stack([s["depth"] for s in scs])
    kw = dict(ppointX=scs[0]["ppx"], ppointY=scs[0]["ppy"], subSampling=8)
    got = _gpu(coords, 16, depth=depth, focals=torch.from_numpy(focals), image0=11, image_stride=3, **kw)
    for b in range(B):
        want = ref.forward(coords[b], 16, THR, ALPHA, MAX_DIST, depth=depth[b], focal=focals[b], ppx=scs[0]["ppx"], ppy=scs[0]["ppy"],
                           sub=8, image=11 + 3 * b)
        _assert_same(got, b, want, ("focals", b))
    assert got["dbg"][0].tobytes() != got["dbg"][1].tobytes()


def test_depth_form_equals_camera_tensor_form(ref):
    """a depth map and the tensor dsacstar.camera_coordinates makes of it give identical bits (odd width: the centre column
    has x_cam == 0 and stays valid)"""
    import dsacstar
    scs = [rc.rgbd_scene(50 + b, 33, 17, noise=0.1, outlier_ratio=0.3, holes=0.2) for b in range(2)]
    coords = np.stack([s["coords"] for s in scs])
    depth = torch.from_numpy(np.stack([s["depth"] for s in scs])).cuda()
    focals = torch.tensor([480.0, 517.25])
    cam = dsacstar.camera_coordinates(depth, focals, 33 * 8, 17 * 8, 8)
    assert cam.is_cuda and tuple(cam.shape) == (2, 3, 33, 17)
    assert bool((cam[:, 0, :, 8] == 0).all()) and bool((cam[:, 2, :, 8] != 0).any())
    a = _gpu(coords, 16, cam=cam)
    b = _gpu(coords, 16, depth=depth, focals=focals, ppointX=17 * 4.0, ppointY=33 * 4.0, subSampling=8)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    want = ref.forward(coords[1], 16, THR, ALPHA, MAX_DIST, cam=cam[1].cpu().numpy(), image=1)
    _assert_same(a, 1, want, "camera_coordinates tensor")
    assert a["dbg"][1, 1] == int((depth[1] != 0).sum())


def test_edge_cases(ref):
    sc = rc.rgbd_scene(4, 8, 12, noise=0.0, outlier_ratio=0.3)
    co = sc["coords"][None]
    kw = dict(focalLength=sc["focal"], ppointX=sc["ppx"], ppointY=sc["ppy"], subSampling=8)
    # depth all zero: identity pose, no NaN, nValid = 0
    zero = np.zeros((1, 8, 12), np.float32)
    got = _gpu(co, 8, depth=zero, thr=10.0, max_dist=100.0, **kw)
    assert np.array_equal(got["pose"][0], np.eye(4, dtype=np.float32)) and got["dbg"][0, 1] == 0
    assert all(np.isfinite(got[k]).all() for k in ("pose", "scores", "dbg"))
    _assert_same(got, 0, ref.forward(sc["coords"], 8, 10.0, ALPHA, 100.0, depth=zero[0]), "no valid cell")
    # exactly two valid cells
    two = zero.copy()
    two[0, 2, 3], two[0, 6, 9] = sc["depth"][2, 3], sc["depth"][6, 9]
    got = _gpu(co, 8, depth=two, thr=10.0, max_dist=100.0, **kw)
    assert got["dbg"][0, 1] == 2 and np.isfinite(got["pose"]).all() and np.isfinite(got["scores"]).all()
    _assert_same(got, 0, ref.forward(sc["coords"], 8, 10.0, ALPHA, 100.0, depth=two[0]), "two valid cells")
    # max_tries = 2 at 90 % outliers: tries exhausted, the hypothesis is still scored
    hard = rc.rgbd_scene(6, 8, 12, noise=0.0, outlier_ratio=0.9)
    got = _gpu(hard["coords"][None], 16, cam=hard["cam"][None], thr=10.0, max_dist=100.0, max_tries=2)
    assert (got["tries"] == -2).any() and np.isfinite(got["scores"]).all()
    _assert_same(got, 0, ref.forward(hard["coords"], 16, 10.0, ALPHA, 100.0, cam=hard["cam"], max_tries=2), "tries exhausted")
    # a threshold so small that no refinement round is accepted
    noisy = rc.rgbd_scene(9, 8, 12, noise=0.5, outlier_ratio=0.3)
    got = _gpu(noisy["coords"][None], 16, cam=noisy["cam"][None], thr=1e-3, max_dist=100.0, max_tries=128)
    assert got["dbg"][0, 2] == 0 and got["dbg"][0, 3] == 0
    _assert_same(got, 0, ref.forward(noisy["coords"], 16, 1e-3, ALPHA, 100.0, cam=noisy["cam"], max_tries=128), "no round")


def test_wiring_and_untouched_names():
    """localize_batch(..., depth=...) and PipelinedLocalizer.submit(..., depth=...) return the poses of the direct call; without
    the new keywords both run the RGB solver exactly as before (the poses of forward_rgb_batch); forward_rgbd still raises"""
    import dsacstar
    from crossloc_amd import evaluation, networks
    from crossloc_amd.weights import seeded_state_dict
    B, Ho, Wo = 3, 16, 24
    H, W = Ho * 8, Wo * 8
    scs = [rc.rgbd_scene(60 + b, Ho, Wo, noise=0.5, outlier_ratio=0.3, holes=0.1) for b in range(B)]
    coords = torch.from_numpy(np.stack([s["coords"] for s in scs])).cuda()
    depth = torch.from_numpy(np.stack([s["depth"] for s in scs])).cuda()
    cam = torch.from_numpy(np.stack([s["cam"] for s in scs])).cuda()
    net = networks.TransPoseNet(torch.tensor(synth.SCENE_MEAN, dtype=torch.float32), True, False, 0, 0, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=3))
    net = net.cuda().eval()
    images = torch.rand(B, 3, H, W, device="cuda")
    direct = torch.zeros(B, 4, 4, device="cuda")
    dsacstar.forward_rgbd_batch(coords, cam, direct, 16, 300.0, 100.0, 3000.0, image0=5, image_stride=2)
    rgb = torch.zeros(B, 4, 4, device="cuda")
    dsacstar.forward_rgb_batch(coords, rgb, 16, 10.0, synth.FOCAL, W / 2.0, H / 2.0, 100.0, 100.0, 8, image0=5, image_stride=2)
    kw = dict(image0=5, image_stride=2, scene_coords=coords)
    rk = dict(rgbd_threshold=300.0, max_dist_error=3000.0)
    a, _ = evaluation.localize_batch(net, images, 16, synth.FOCAL, H, W, depth=depth, **kw, **rk)
    b, _ = evaluation.localize_batch(net, images, 16, synth.FOCAL, H, W, cam_coords=cam, **kw, **rk)
    c, _ = evaluation.localize_batch(net, images, 16, synth.FOCAL, H, W, **kw)
    loc = evaluation.PipelinedLocalizer(net, 16, synth.FOCAL, H, W)
    d, _ = loc.submit(images, depth=depth, **kw, **rk)
    e, _ = loc.submit(images, **kw)
    loc.finish()
    torch.cuda.synchronize()
    assert torch.equal(a, direct) and torch.equal(b, direct) and torch.equal(d, direct)
    assert torch.equal(c, rgb) and torch.equal(e, rgb)
    assert not torch.equal(direct, rgb)
    for s, p in zip(scs, direct.cpu().numpy()):
        t_err, r_err = synth.pose_error(s["pose"], p.astype(np.float64))
        assert t_err < 2.0 and r_err < 0.5
    with pytest.raises(RuntimeError):
        evaluation.localize_batch(net, images, 16, synth.FOCAL, H, W, depth=depth, cam_coords=cam, **kw)
    with pytest.raises(NotImplementedError):
        dsacstar.forward_rgbd()
    with pytest.raises(RuntimeError):
        dsacstar.forward_rgbd_batch(torch.zeros(1, 3, 80, 80, device="cuda"), torch.zeros(1, 3, 80, 80, device="cuda"),
                                    torch.zeros(1, 4, 4, device="cuda"), 8, 10.0, 100.0, 100.0)         # 6400 cells: XL_ERR_GRID
