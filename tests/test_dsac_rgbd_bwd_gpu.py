"""GPU parity of the RGB-D DSAC* backward pass: xl_dsac_backward_rgbd_batch (through dsacstar.backward_rgbd_batch) against the
serial C restatement tests/dsac_rgbd_bwd_ref.c, bit for bit: the expected loss, columns 0-57 of every hypothesis record and the
float32 gradient.  The two sides compile the same header, so this checks the kernels' orchestration - K0's split over
workgroups, staging, the refinement loop, the block reductions, the per-cell assembly, strides, accumulation - and that gcc and
hipcc agree.  The formulas themselves: tests/test_dsac_rgbd_bwd_cpu.py."""
import numpy as np
import pytest

import dsac_rgbd_bwd_ref as bref
import dsac_rgbd_cases as rc
from crossloc_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

THR, ALPHA, MAX_DIST = 10.0, 100.0, 100.0
SEED = 1305


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return bref.load(tmp_path_factory.mktemp("dsac_rgbd_bwd_ref"))


def moved_pose(pose):
    out = pose.copy()
    out[:3, :3] = out[:3, :3] @ synth._rot_xyz(0.01, -0.015, 0.02)
    out[:3, 3] += [0.3, -0.2, 0.4]
    return out


def scenes_of(B, Ho, Wo, seed0, noise=0.05):
    scs = [rc.rgbd_scene(seed0 + b, Ho, Wo, noise=noise, outlier_ratio=0.3, holes=0.2) for b in range(B)]
    for s in scs:
        s["gt"] = moved_pose(s["pose"])
    return scs


def stack(scs, key):
    return np.stack([np.asarray(s[key], np.float32) for s in scs])


def _gpu(coords, gt, n_hyp, cam=None, depth=None, grad=None, w=(1.0, 100.0, 1e6), thr=THR, max_dist=MAX_DIST, **kw):
    """numpy arrays are uploaded contiguous, torch CUDA tensors are used as they are -> (loss [B], rec [B,nHyp,64], grad) numpy"""
    import dsacstar
    up = lambda a: a if a is None or isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    coords, cam, depth, gt = up(coords), up(cam), up(depth), up(gt)
    if grad is None:
        grad = torch.zeros(tuple(coords.shape), dtype=torch.float32, device="cuda")
    loss, rec = dsacstar.backward_rgbd_batch(coords, cam, grad, gt, n_hyp, thr, w[0], w[1], w[2], ALPHA, max_dist, SEED, debug=True,
                                             depth=depth, **kw)
    torch.cuda.synchronize()
    return loss.cpu().numpy(), rec.cpu().numpy(), grad.cpu().numpy()


def _assert_same(got, b, want, what):
    loss, rec, grad = got
    assert loss.dtype == np.float64 and loss[b] == want["loss"], (what, loss[b], want["loss"])
    g, w = np.ascontiguousarray(rec[b][:, :58]), np.ascontiguousarray(want["rec"][:, :58])
    assert g.tobytes() == w.tobytes(), (what, "record", np.argwhere(g != w)[:8])
    assert not rec[b][:, 58:].any(), what
    g, w = np.ascontiguousarray(grad[b]), np.ascontiguousarray(want["grad"])
    assert g.dtype == np.float32 and g.tobytes() == w.tobytes(), (what, "gradient", np.argwhere(g != w)[:8])


@pytest.mark.parametrize("Ho,Wo,n_hyp,B", [(8, 12, 16, 3), (8, 12, 64, 3), (17, 23, 64, 3), (60, 90, 16, 1)])
def test_bit_exact_against_the_restatement(ref, Ho, Wo, n_hyp, B):
    """B = 3 at 8 x 12 (16 and 64 hypotheses: K0 runs as 2 and as 16 workgroups per image) and 17 x 23 (391 cells, no multiple of
    256), one image at 60 x 90 (the largest LDS footprint); 0.05 m noise, 30 % outliers, 20 % holes; image0 = 5, stride 2"""
    scs = scenes_of(B, Ho, Wo, 90)
    got = _gpu(stack(scs, "coords"), stack(scs, "gt"), n_hyp, cam=stack(scs, "cam"), image0=5, image_stride=2)
    for b, s in enumerate(scs):
        want = ref.backward(s["coords"], s["gt"], n_hyp, THR, ALPHA, MAX_DIST, cam=s["cam"], image=5 + 2 * b)
        _assert_same(got, b, want, (Ho, Wo, n_hyp, b))
        assert (got[1][b][:, bref.ACTIVE] > 0).any()
        assert np.isfinite(got[2][b]).all() and got[2][b].any()
        assert np.isfinite(got[1][b]).all()


def test_interface_variants(ref):
    """a strided gradient view inside a larger tensor (the neighbouring channels untouched), accumulation into 0.125, per-image
    focals in depth form, and the depth form against the camera form"""
    import dsacstar
    B, Ho, Wo = 2, 8, 12
    scs = scenes_of(B, Ho, Wo, 120)
    coords, cam, depth, gt = stack(scs, "coords"), stack(scs, "cam"), stack(scs, "depth"), stack(scs, "gt")
    plain = _gpu(coords, gt, 16, cam=cam)
    big = torch.full((B, 5, Ho, 2 * Wo), 0.125, dtype=torch.float32, device="cuda")
    view = big[:, 1:4, :, ::2]
    assert view.stride(3) == 2 and not view.is_contiguous()
    got = _gpu(coords, gt, 16, cam=cam, grad=view)
    for b, s in enumerate(scs):
        want = ref.backward(s["coords"], s["gt"], 16, THR, ALPHA, MAX_DIST, cam=s["cam"], image=b, grad=np.full((3, Ho, Wo), 0.125, np.float32))
        _assert_same((got[0], got[1], view.cpu().numpy()), b, want, ("strided accumulate", b))
    bigc = big.cpu().numpy()
    assert (bigc[:, 0] == 0.125).all() and (bigc[:, 4] == 0.125).all() and (bigc[:, 1:4, :, 1::2] == 0.125).all()
    assert np.array_equal(got[0], plain[0])
    valid = cam[:, 2] != 0
    assert (view.cpu().numpy().transpose(1, 0, 2, 3)[:, ~valid] == 0.125).all()         # holes get nothing
    # depth form == camera form (one focal for both images)
    kw = dict(ppointX=scs[0]["ppx"], ppointY=scs[0]["ppy"], subSampling=8)
    dep = _gpu(coords, gt, 16, depth=depth, focalLength=scs[0]["focal"], **kw)
    for a, d in zip(plain, dep):
        assert a.tobytes() == d.tobytes()
    # per-image focals in depth form == the camera tensor camera_coordinates makes with them
    focals = torch.tensor([480.0, 517.25])
    cam_f = dsacstar.camera_coordinates(torch.from_numpy(depth).cuda(), focals, Ho * 8, Wo * 8, 8)
    a = _gpu(coords, gt, 16, cam=cam_f)
    d = _gpu(coords, gt, 16, depth=depth, focals=focals, **kw)
    for x, y in zip(a, d):
        assert x.tobytes() == y.tobytes()
    want = ref.backward(coords[1], gt[1], 16, THR, ALPHA, MAX_DIST, depth=depth[1], focal=517.25, ppx=scs[0]["ppx"], ppy=scs[0]["ppy"],
                        sub=8, image=1)
    _assert_same(d, 1, want, "per-image focal")
    assert a[0][0] != plain[0][0] or a[0][1] != plain[0][1]


@pytest.mark.parametrize("w", [(3.0, 100.0, 1e6), (1.0, 25.0, 1e6), (1.0, 100.0, 20.0)])
def test_weights_and_soft_clamp(ref, w):
    """w_rot, w_trans, and a soft clamp below every loss (the sqrt branch of dloss)"""
    s = scenes_of(1, 17, 23, 130)[0]
    got = _gpu(s["coords"][None], s["gt"][None], 16, cam=s["cam"][None], w=w)
    want = ref.backward(s["coords"], s["gt"], 16, THR, ALPHA, MAX_DIST, *w, cam=s["cam"])
    _assert_same(got, 0, want, w)
    if w[2] < 1e6:
        assert (got[1][0][:, bref.LOSS] > w[2]).all()


def test_edge_launches(ref):
    """no valid cell, a single hypothesis, an exhausted sampling budget: bit-exact, no NaN; max_tries <= 128 throughout"""
    s = scenes_of(1, 8, 12, 140, noise=0.0)[0]
    kw = dict(focalLength=s["focal"], ppointX=s["ppx"], ppointY=s["ppy"], subSampling=8)
    zero = np.zeros((1, 8, 12), np.float32)
    got = _gpu(s["coords"][None], s["gt"][None], 8, depth=zero, max_tries=128, **kw)
    want = ref.backward(s["coords"], s["gt"], 8, THR, ALPHA, MAX_DIST, depth=zero[0], max_tries=128)
    _assert_same(got, 0, want, "no valid cell")
    assert not got[2].any() and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    got = _gpu(s["coords"][None], s["gt"][None], 1, cam=s["cam"][None], max_tries=128)
    want = ref.backward(s["coords"], s["gt"], 1, THR, ALPHA, MAX_DIST, cam=s["cam"], max_tries=128)
    _assert_same(got, 0, want, "one hypothesis")
    assert got[1][0, 0, bref.PROB] == 1.0 and got[1][0, 0, bref.SOG] == 0.0 and np.isfinite(got[2]).all()
    hard = rc.rgbd_scene(6, 8, 12, noise=0.5, outlier_ratio=0.9)
    gt = moved_pose(hard["pose"]).astype(np.float32)
    got = _gpu(hard["coords"][None], gt[None], 16, cam=hard["cam"][None], thr=0.1, max_tries=128)
    want = ref.backward(hard["coords"], gt, 16, 0.1, ALPHA, MAX_DIST, cam=hard["cam"], max_tries=128)
    _assert_same(got, 0, want, "tries exhausted")
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()


def test_consistent_with_the_forward_pass(ref):
    """the hypotheses are the forward pass's: for the same seed and image keys the soft-max of forward_rgbd_batch's debug scores
    (the header's soft-max, through the restatement) equals the backward records' probabilities bit for bit, and the winner of
    the forward pass is the most probable hypothesis"""
    import dsacstar
    scs = scenes_of(2, 17, 23, 150)
    coords, cam, gt = (torch.from_numpy(stack(scs, k)).cuda() for k in ("coords", "cam", "gt"))
    poses = torch.zeros(2, 4, 4, device="cuda")
    fwd = dsacstar.forward_rgbd_batch(coords, cam, poses, 32, THR, ALPHA, MAX_DIST, image0=9, image_stride=4, seed=SEED, debug=True)
    _, rec, _ = _gpu(coords, gt, 32, cam=cam, image0=9, image_stride=4)
    scores = fwd["scores"].cpu().numpy()
    for b in range(2):
        want = ref.backward(scs[b]["coords"], scs[b]["gt"], 32, THR, ALPHA, MAX_DIST, cam=scs[b]["cam"], image=9 + 4 * b)
        assert want["scores"].tobytes() == scores[b].tobytes()
        assert ref.softmax(scores[b]).tobytes() == np.ascontiguousarray(rec[b][:, bref.PROB]).tobytes()
        assert int(fwd["dbg"][b, 0].item()) == int(np.argmax(rec[b][:, bref.PROB]))


def test_descent_end_to_end():
    """a small step against the returned gradient (the largest coordinate moves by a millimetre) lowers the returned expected
    loss, by at least half of what the gradient predicts to first order.  The expected loss is piecewise smooth: the scenes are
    two on which, both keyed as image 0 (image_stride = 0), such a step changes no inlier count and no active flag (checked here
    through the records)"""
    scs = scenes_of(2, 17, 23, 167)
    coords, cam, gt = (torch.from_numpy(stack(scs, k)).cuda() for k in ("coords", "cam", "gt"))
    l0, r0, g = _gpu(coords, gt, 16, cam=cam, image_stride=0)
    g = torch.from_numpy(g).cuda()
    step = 1e-3 / g.abs().amax(dim=(1, 2, 3), keepdim=True)
    l1, r1, _ = _gpu(coords - step * g, gt, 16, cam=cam, image_stride=0)
    assert np.array_equal(r0[:, :, bref.ACTIVE], r1[:, :, bref.ACTIVE]) and np.array_equal(r0[:, :, bref.INLIERS], r1[:, :, bref.INLIERS])
    predicted = (step.reshape(-1).double() * (g.double() ** 2).sum(dim=(1, 2, 3))).cpu().numpy()
    assert (l1 < l0).all() and (l0 - l1 >= 0.5 * predicted).all(), (l0, l1, predicted)


def test_backward_leaves_no_state_behind():
    """forward_rgbd_batch before and after a backward call on another batch returns identical poses"""
    import dsacstar
    a, b = scenes_of(2, 17, 23, 170), scenes_of(3, 8, 12, 180)
    co, cm = (torch.from_numpy(stack(a, k)).cuda() for k in ("coords", "cam"))
    first, second = torch.zeros(2, 4, 4, device="cuda"), torch.zeros(2, 4, 4, device="cuda")
    dsacstar.forward_rgbd_batch(co, cm, first, 16, THR, ALPHA, MAX_DIST)
    _gpu(stack(b, "coords"), stack(b, "gt"), 16, cam=stack(b, "cam"))
    dsacstar.forward_rgbd_batch(co, cm, second, 16, THR, ALPHA, MAX_DIST)
    torch.cuda.synchronize()
    assert torch.equal(first, second) and bool(torch.isfinite(first).all())
