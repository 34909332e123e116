"""GPU parity of the ray-aware pose refinement behind the RGB-D solver: xl_dsac_refine_pose_rgbd_batch (through
dsacstar.refine_pose_rgbd_batch) against the serial C restatement tests/rgbd_refine_ref.c.  Every comparison is bitwise on the 16
floats of the pose, all 64 doubles of the row and the 12 doubles of the world->camera pose (NaNs by position): the two sides
compile the same header, so this checks the kernel's orchestration - strides, the cell walks, the rounds, the butterfly and wave
order - and that gcc and hipcc agree.  The model itself: tests/test_rgbd_refine_cpu.py."""
import numpy as np
import pytest

import guarded
import rgbd_refine_cases as rc
import rgbd_refine_ref
from crossloc_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALPHA = 100.0
PAR = (rc.THR, rc.MAX_DIST)
K = 0.01                                   # the relative depth noise of the scenes


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return rgbd_refine_ref.load(tmp_path_factory.mktemp("rgbd_refine_ref"))


def _dev(a, dtype=None):
    if isinstance(a, torch.Tensor) or a is None:
        return a
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _run(coords, cam, sigma, poses, depth=None, depth_sigma=None, depth_rel=0.0, par=PAR, **kw):
    """tensors: torch CUDA (any strides) or numpy -> (poses [B,4,4] f32, rows [B,64], w2c [B,12]) numpy"""
    import dsacstar
    coords, cam, sigma, depth, depth_sigma = (_dev(a) for a in (coords, cam, sigma, depth, depth_sigma))
    poses = _dev(poses, np.float32)
    B = coords.shape[0]
    w2c = torch.full((B, 12), -7.0, dtype=torch.float64, device="cuda")
    if depth is not None:
        kw = dict(dict(focalLength=synth.FOCAL, ppointX=coords.shape[3] * rc.SUB / 2.0, ppointY=coords.shape[2] * rc.SUB / 2.0,
                       subSampling=rc.SUB), **kw)
    out, rows = dsacstar.refine_pose_rgbd_batch(coords, cam, sigma, poses, *par, depthSigma=depth_sigma, depthRel=depth_rel,
                                                depth=depth, w2c=w2c, **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 4, 4)
    assert rows.dtype == torch.float64 and tuple(rows.shape) == (B, 64)
    return out.cpu().numpy(), rows.cpu().numpy(), w2c.cpu().numpy()


def _same(got, want):
    return (np.array_equal(np.isnan(got[0]), np.isnan(want[0]))
            and np.array_equal(np.asarray(got[0]).view(np.int32)[~np.isnan(got[0])], np.asarray(want[0]).view(np.int32)[~np.isnan(want[0])])
            and rc.same_bits(got[1], want[1]) and rc.same_bits(got[2], want[2]))


def _frame(got, b):
    return got[0][b], got[1][b], got[2][b]


def _all_same(got, base, B):
    return all(_same(_frame(got, b), _frame(base, b)) for b in range(B))


def _batch(seed0, B, Ho, Wo, holes=0.1):
    """B scenes stacked: dict(coords, cam, depth, sigma, depth_sigma, pose [B,4,4] f64)"""
    scs = [rc.scene(seed0 + i, Ho, Wo, holes=holes) for i in range(B)]
    return {k: np.stack([s[k] for s in scs]) for k in ("coords", "cam", "depth", "sigma", "depth_sigma", "pose")}


def _forms(bt):
    """(name, sigma, depth_sigma, depth_rel): sigma + sigma_z map + depthRel, sigma only, plain"""
    return [("full", bt["sigma"], bt["depth_sigma"], K), ("sigma", bt["sigma"], None, 0.0), ("plain", None, None, 0.0)]


def _want(ref, bt, b, pose, sigma, depth_sigma, k, **kw):
    return ref.refine(bt["coords"][b], pose, *PAR, cam=bt["cam"][b], sigma=None if sigma is None else sigma[b],
                      depth_sigma=None if depth_sigma is None else depth_sigma[b], depth_rel=k, **kw)[:3]


@pytest.mark.parametrize("Ho,Wo,B", [(7, 9, 6), (24, 36, 6), (37, 53, 6), (60, 90, 3)])
def test_bit_exact_at_grid_sizes(ref, Ho, Wo, B):
    """63 cells (fewer than one wave); 864 (a ragged 3.4 cells per thread); 1961 (no multiple of 64); 5400 (the workload grid).
    First, middle and last frame of the batch, from the pose forward_rgbd_batch wrote (64 hypotheses) and from a perturbed
    ground truth; sigma + sigma_z map + depthRel, sigma only and the plain form; the depth form gives the camera-tensor form's
    bits."""
    import dsacstar
    frames = sorted({0, B // 2, B - 1})
    bt = _batch(2021, B, Ho, Wo)
    co, cam = _dev(bt["coords"]), _dev(bt["cam"])
    est = torch.zeros((B, 4, 4), dtype=torch.float32, device="cuda")
    dsacstar.forward_rgbd_batch(co, cam, est, 64, rc.THR, ALPHA, rc.MAX_DIST)
    starts = {"solver pose": est.cpu().numpy(),
              "perturbed ground truth": np.stack([rc.perturbed(bt["pose"][b], b) for b in range(B)]).astype(np.float32)}
    for what, poses in starts.items():
        for form, sg, sz, k in _forms(bt):
            got = _run(co, cam, sg, poses, depth_sigma=sz, depth_rel=k)
            for b in frames:
                want = _want(ref, bt, b, poses[b], sg, sz, k)
                g = _frame(got, b)
                assert _same(g, want), (what, form, b, np.flatnonzero(~((g[1] == want[1]) | (np.isnan(g[1]) & np.isnan(want[1])))))
            assert _all_same(_run(co, None, sg, poses, depth=bt["depth"], depth_sigma=sz, depth_rel=k), got, B), (what, form)
            if Ho * Wo >= 800 and what == "perturbed ground truth":
                assert (got[1][:, 6] == 0).all() and (got[1][:, 58] >= 1).all() and (got[1][:, 63] > 0.85 * Ho * Wo).all()


@pytest.fixture(scope="module")
def one_batch():
    bt = _batch(3100, 6, 37, 53)
    poses = np.stack([rc.perturbed(bt["pose"][b], b) for b in range(6)]).astype(np.float32)
    return bt, poses, _run(bt["coords"], bt["cam"], bt["sigma"], poses, depth_sigma=bt["depth_sigma"], depth_rel=K)


def _padded(t, top, left, bottom, right):
    """`t` [..., Ho, Wo] as the interior of a NaN-filled tensor with a padded row pitch"""
    Ho, Wo = t.shape[-2:]
    wide = torch.full(tuple(t.shape[:-2]) + (Ho + top + bottom, Wo + left + right), float("nan"), device="cuda")
    wide[..., top:top + Ho, left:left + Wo] = t
    return wide[..., top:top + Ho, left:left + Wo]


def test_strided_inputs_give_the_bits_of_the_contiguous_copies(ref, one_batch):
    bt, poses, base = one_batch
    for b in range(6):
        assert _same(_frame(base, b), _want(ref, bt, b, poses[b], bt["sigma"], bt["depth_sigma"], K)), b
    co, cam, sg, sz, depth = (_dev(bt[k]) for k in ("coords", "cam", "sigma", "depth_sigma", "depth"))
    B, _, Ho, Wo = co.shape
    kw = dict(depth_rel=K)
    # the channel views of [B,4,Ho,Wo] tensors: the coordinate network's output, and a depth network's (depth, sigma_z, ...)
    pred = torch.randn((B, 4, Ho, Wo), device="cuda")
    pred[:, :3], pred[:, 3] = co, sg
    camt = torch.randn((B, 4, Ho, Wo), device="cuda")
    camt[:, :3], camt[:, 3] = cam, sz
    dnet = torch.randn((B, 4, Ho, Wo), device="cuda")
    dnet[:, 0], dnet[:, 3] = depth, sz
    assert not pred[:, :3].is_contiguous() and not pred[:, 3].is_contiguous()
    assert _all_same(_run(pred[:, :3], camt[:, :3], pred[:, 3], poses, depth_sigma=camt[:, 3], **kw), base, B)
    assert _all_same(_run(pred[:, :3], None, pred[:, 3], poses, depth=dnet[:, 0], depth_sigma=dnet[:, 3], **kw), base, B)
    cl, ccl, dcl = (t.contiguous(memory_format=torch.channels_last) for t in (pred, camt, dnet))
    assert cl.stride(1) == 1 and cl[:, 3].stride(2) == 4
    assert _all_same(_run(cl[:, :3], ccl[:, :3], cl[:, 3], poses, depth_sigma=ccl[:, 3], **kw), base, B)
    assert _all_same(_run(cl[:, :3], None, cl[:, 3], poses, depth=dcl[:, 0], depth_sigma=dcl[:, 3], **kw), base, B)
    # padded row pitches with NaN borders
    pco, pcam, psg, psz, pd = _padded(co, 2, 5, 1, 6), _padded(cam, 1, 3, 3, 2), _padded(sg, 1, 3, 4, 4), _padded(sz, 0, 7, 2, 1), \
        _padded(depth, 3, 1, 1, 9)
    assert pco.stride(2) == Wo + 11 and psg.stride(1) == Wo + 7 and pd.stride(1) == Wo + 10
    got = _run(pco, pcam, psg, poses, depth_sigma=psz, **kw)
    assert _all_same(got, base, B) and (got[1][:, 5] == 0).all()
    assert _all_same(_run(pco, None, psg, poses, depth=pd, depth_sigma=psz, **kw), base, B)


def test_slot_independence_in_place_and_focals(ref, one_batch):
    bt, poses, base = one_batch
    pick = lambda order: (bt["coords"][order], bt["cam"][order], bt["sigma"][order], poses[order])
    kw = lambda order: dict(depth_sigma=bt["depth_sigma"][order], depth_rel=K)
    alone = _run(*pick([3]), **kw([3]))
    assert _same(_frame(alone, 0), _frame(base, 3))
    order = [3, 0, 1, 2, 4, 5]
    got = _run(*pick(order), **kw(order))
    assert _same(_frame(got, 0), _frame(base, 3)) and _same(_frame(got, 1), _frame(base, 0))
    order = [0, 1, 2, 4, 5, 3]
    got = _run(*pick(order), **kw(order))
    assert _same(_frame(got, 5), _frame(base, 3)) and _same(_frame(got, 4), _frame(base, 5))
    # in place
    po = _dev(poses, np.float32).clone()
    got = _run(bt["coords"], bt["cam"], bt["sigma"], po, outPoses=po, **kw(slice(None)))
    assert _all_same(got, base, 6) and np.array_equal(po.cpu().numpy().view(np.int32), base[0].view(np.int32))
    # per-frame focals equal a scalar focal length (the depth form reads the focal length)
    scs = [synth.make_hetero_rgbd_scene(40 + i, Ho=20, Wo=30, holes=0.1, focal=f) for i, f in enumerate((480.0, 455.5, 512.25))]
    st = {k: np.stack([s[k] for s in scs]) for k in ("coords", "depth", "sigma", "depth_sigma")}
    starts = np.stack([rc.perturbed(s["pose"], i) for i, s in enumerate(scs)]).astype(np.float32)
    focals = torch.tensor([s["focal"] for s in scs])
    geo = dict(ppointX=120.0, ppointY=80.0, subSampling=rc.SUB)
    got = _run(st["coords"], None, st["sigma"], starts, depth=st["depth"], depth_sigma=st["depth_sigma"], depth_rel=K,
               focalLength=1.0, focals=focals, **geo)                       # the scalar is ignored
    for b, s in enumerate(scs):
        one = _run(st["coords"][b:b + 1], None, st["sigma"][b:b + 1], starts[b:b + 1], depth=st["depth"][b:b + 1],
                   depth_sigma=st["depth_sigma"][b:b + 1], depth_rel=K, focalLength=s["focal"], **geo)
        assert _same(_frame(got, b), _frame(one, 0))
        want = ref.refine(s["coords"], starts[b], *PAR, depth=s["depth"], sigma=s["sigma"], depth_sigma=s["depth_sigma"], depth_rel=K,
                          focal=s["focal"])[:3]
        assert _same(_frame(got, b), want)
    assert (got[1][:, 6] == 0).all()


def test_no_writes_outside_the_outputs(monkeypatch, one_batch):
    """outPoses, w2c and the rows the wrapper allocates lie between guard bands (tests/guarded.py)"""
    from crossloc_amd import dsacstar as shim
    bt, poses, base = one_batch
    co, cam, sg, sz = (_dev(bt[k]) for k in ("coords", "cam", "sigma", "depth_sigma"))
    po = _dev(poses, np.float32)
    guarded.guard_modules(monkeypatch, shim)
    try:
        out = guarded.REGISTRY.empty((6, 4, 4), dtype=torch.float32, device="cuda")
        w2c = guarded.REGISTRY.empty((6, 12), dtype=torch.float64, device="cuda")
        n = guarded.handed_out()
        got_p, rows = shim.refine_pose_rgbd_batch(co, cam, sg, po, *PAR, depthSigma=sz, depthRel=K, outPoses=out, w2c=w2c)
        assert guarded.handed_out() == n + 1 and got_p is out                # the rows
        guarded.assert_intact()
        got = (out.cpu().numpy(), rows.cpu().numpy(), w2c.cpu().numpy())
    finally:
        guarded.stop()
    assert _all_same(got, base, 6)


def test_status_and_edge_cases_on_the_device(ref):
    """12x16: every status code, the NaN patterns and the input pose left in place bit for bit; unusable sigma and sigma_z are
    left out and counted; one round against the default; zero maps with s0 = 1 against the plain form."""
    half = np.full((12, 16), 0.5, np.float32)
    for name, coords, cam, pose, status, n_inl, n_valid in rc.status_cases(12, 16):
        for sigma, k in ((None, 0.0), (half, K)):
            got = _frame(_run(coords[None], cam[None], None if sigma is None else sigma[None], pose[None], depth_rel=k,
                              par=(10.0, 100.0)), 0)
            rc.assert_status_row(name, got[1], got[0], got[2], pose, status, n_inl, n_valid)
            assert _same(got, ref.refine(coords, pose, 10.0, 100.0, cam=cam, sigma=sigma, depth_rel=k)[:3]), name
    zero_depth = np.zeros((1, 12, 16), np.float32)                           # all depth zero, the depth form
    sc = rc.scene(77, 12, 16, outlier_ratio=0.0)
    pose = sc["pose"].astype(np.float32)
    got = _frame(_run(sc["coords"][None], None, None, pose[None], depth=zero_depth), 0)
    rc.assert_status_row("all depth zero", got[1], got[0], got[2], pose, 1, 0, 0)

    sig, sig_z, n_bad = rc.sigma_status_maps()
    got = _frame(_run(sc["coords"][None], sc["cam"][None], sig[None], pose[None], depth_sigma=sig_z[None], par=(3000.0, 1e5)), 0)
    assert got[1][6] == 0 and got[1][5] == n_bad and got[1][63] == 12 * 16 and got[1][1] == 12 * 16 - n_bad
    assert _same(got, ref.refine(sc["coords"], pose, 3000.0, 1e5, cam=sc["cam"], sigma=sig, depth_sigma=sig_z)[:3])

    hs = rc.scene(78, 12, 16)
    far = rc.perturbed(hs["pose"], 3, 1.0, 0.2).astype(np.float32)
    args = (hs["coords"][None], hs["cam"][None], hs["sigma"][None], far[None])
    one = _frame(_run(*args, depth_rel=K, maxRounds=1), 0)
    full = _frame(_run(*args, depth_rel=K), 0)
    assert one[1][58] == 1 and one[1][60] == 0 and full[1][60] == 1 and 1 <= full[1][58] <= 8
    assert _same(one, ref.refine(hs["coords"], far, *PAR, cam=hs["cam"], sigma=hs["sigma"], depth_rel=K, max_rounds=1)[:3])
    assert _same(full, ref.refine(hs["coords"], far, *PAR, cam=hs["cam"], sigma=hs["sigma"], depth_rel=K)[:3])

    plain = _frame(_run(hs["coords"][None], hs["cam"][None], None, far[None]), 0)
    zeros = np.zeros((1, 12, 16), np.float32)
    zero = _frame(_run(hs["coords"][None], hs["cam"][None], zeros, far[None], depth_sigma=zeros, sigmaFloorM=1.0), 0)
    assert _same(plain, zero) and plain[1][6] == 0


class _PlantNet(torch.nn.Module):
    """Stand-in for the network in the wiring tests: the solver's input is given by the caller (`scene_coords`); `channels`
    4: an uncertainty channel that predicts 0.1 m everywhere, 3: none."""
    num_task_channel = 3
    OUTPUT_SUBSAMPLE = rc.SUB

    def __init__(self, channels=4):
        super().__init__()
        self.channels = channels

    def forward(self, images, plan_slot=0):
        return torch.full((images.shape[0], self.channels, 60, 90), 0.1, device=images.device)


def _sym6(ut):
    M = np.zeros((6, 6))
    M[np.triu_indices(6)] = ut
    return M + np.triu(M, 1).T


def test_chained_path_and_the_quality_row_at_the_output_pose():
    import dsacstar
    from crossloc_amd import evaluation
    bt = _batch(5200, 4, 60, 90)
    co, sg, depth, sz = (_dev(bt[k]) for k in ("coords", "sigma", "depth", "depth_sigma"))
    images = torch.zeros((4, 3, 480, 720), device="cuda")
    net = _PlantNet()
    geo = dict(depth=depth, focalLength=synth.FOCAL, ppointX=360.0, ppointY=240.0, subSampling=rc.SUB)
    kw = dict(image0=3, scene_coords=co, depth=depth, rgbd_threshold=rc.THR, max_dist_error=rc.MAX_DIST)
    plain = evaluation.localize_batch(net, images, 64, synth.FOCAL, 480, 720, **kw)
    want_p, want_r = dsacstar.refine_pose_rgbd_batch(co, None, sg, plain[0], *PAR, depthSigma=sz, depthRel=K, **geo)
    want_q = dsacstar.pose_quality_rgbd_batch(co, None, want_p, rc.THR, ALPHA, rc.MAX_DIST, **geo)
    ref_kw = dict(refine="rgbd_sigma", sigma=sg, depth_sigma=sz, depth_rel=K, quality="rgbd")
    out = evaluation.localize_batch(net, images, 64, synth.FOCAL, 480, 720, **ref_kw, **kw)
    torch.cuda.synchronize()
    assert len(out) == 4 and torch.equal(out[0], want_p) and not torch.equal(want_p, plain[0]) and (want_r[:, 6] == 0).all()
    assert rc.same_bits(out[3].cpu().numpy(), want_r.cpu().numpy()) and rc.same_bits(out[2].cpu().numpy(), want_q.cpu().numpy())
    # without a side input: the prediction's own uncertainty channel
    own_p, own_r = dsacstar.refine_pose_rgbd_batch(co, None, torch.full((4, 60, 90), 0.1, device="cuda"), plain[0], *PAR, depthRel=K,
                                                   **geo)
    out = evaluation.localize_batch(net, images, 64, synth.FOCAL, 480, 720, refine="rgbd_sigma", depth_rel=K, **kw)
    torch.cuda.synchronize()
    assert len(out) == 3 and torch.equal(out[0], own_p) and rc.same_bits(out[2].cpu().numpy(), own_r.cpu().numpy())
    nodepth = dict(image0=3, scene_coords=co)
    with pytest.raises(RuntimeError):
        evaluation.localize_batch(net, images, 64, synth.FOCAL, 480, 720, refine="rgbd_sigma", sigma=sg, **nodepth)
    with pytest.raises(RuntimeError):
        evaluation.localize_batch(_PlantNet(3), images, 64, synth.FOCAL, 480, 720, refine="rgbd_sigma", **kw)

    loc = evaluation.PipelinedLocalizer(net, 64, synth.FOCAL, 480, 720)
    p_sig = loc.submit(images, **ref_kw, **kw)
    loc.finish()
    torch.cuda.synchronize()
    assert len(p_sig) == 4 and torch.equal(p_sig[0], want_p)
    assert rc.same_bits(p_sig[3].cpu().numpy(), want_r.cpu().numpy()) and rc.same_bits(p_sig[2].cpu().numpy(), want_q.cpu().numpy())
    with pytest.raises(RuntimeError):
        loc.submit(images, refine="rgbd_inliers", **nodepth)

    # the plain form on converged frames: the inlier set of the last round is the set at the output pose, which the RGB-D
    # quality row rates - equal counts, and JtJ to 1e-9 of its largest entry (double sums of <= 5400 terms in different orders)
    out = evaluation.localize_batch(net, images, 64, synth.FOCAL, 480, 720, refine="rgbd_inliers", quality="rgbd", **kw)
    torch.cuda.synchronize()
    q, r = out[2].cpu().numpy(), out[3].cpu().numpy()
    conv = r[:, 60] == 1
    assert conv.any() and (r[:, 6] == 0).all()
    for b in np.flatnonzero(conv):
        assert q[b, 1] == r[b, 1] and q[b, 58] == r[b, 63]
        Jq, Jr = _sym6(q[b, 10:31]), _sym6(r[b, 10:31])
        assert np.abs(Jq - Jr).max() <= 1e-9 * np.abs(Jq).max()
        assert abs(q[b, 7] - r[b, 7]) <= 1e-9 * q[b, 7]                     # chi of the plain form is the quality row's sigma_m
