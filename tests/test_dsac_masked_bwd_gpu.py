"""GPU checks of the masked RGB backward pass (dsacstar.backward_rgb_masked_batch): loss, the 53 record fields, gradient and status
bitwise against the serial restatement tests/dsac_masked_bwd_ref.c in both launch forms, the three identities (all-ones mask ==
backward_rgb_batch; the values at masked-out cells influence nothing; their gradient keeps its incoming value), a dead image
between live ones, hypotheses exhausted on a mask-rejected try, and the plumbing through
loss.expected_pose_loss_and_output_gradient and training.make_e2e_step."""
import numpy as np
import pytest
import torch

import dsac_masked_bwd_ref
from crossloc_amd import synth

pytestmark = pytest.mark.gpu

GRIDS = [(8, 12), (9, 13), (24, 36)]
UNSPLIT, SPLIT = 6, 16                     # hypotheses: the sample + score launch with one / with four workgroups per image at B = 3
THR, ALPHA, MAX_REPROJ, SUB = 10.0, 100.0, 100.0, 8
W_ROT, W_TRANS, SOFT_CLAMP = 1.0, 100.0, 100.0
FIELDS = dsac_masked_bwd_ref.FIELDS
EXHAUSTED = dsac_masked_bwd_ref.EXHAUSTED
G0 = 0.125                                 # the incoming gradient, everywhere
OUT = ("loss", "rec", "grad", "status")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return dsac_masked_bwd_ref.load(tmp_path_factory.mktemp("dsac_masked_bwd_ref"))


def _sub_blocks(B, n_hyp):
    from crossloc_amd import _lib
    return int(_lib.lib().xl_dsac_backward_sub_blocks(B, n_hyp))


def _seeded_mask(seed, Ho, Wo, usable):
    return (np.random.default_rng([seed, 0x4d41]).random((Ho, Wo)) < usable).astype(np.uint8)


_BATCHES = {}


def _batch(Ho, Wo):
    """three images with a mask each: all ones, a seeded random 50 %, the decoy band -> coords [3,3,Ho,Wo], masks [3,Ho,Wo],
    ground-truth poses [3,4,4] float32"""
    if (Ho, Wo) not in _BATCHES:
        a, b = synth.make_scene(11, Ho=Ho, Wo=Wo), synth.make_scene(12, Ho=Ho, Wo=Wo)
        c = synth.make_decoy_scene(13, decoy=0.6, Ho=Ho, Wo=Wo)
        coords = np.stack([a["coords"], b["coords"], c["coords"]])
        masks = np.stack([np.ones((Ho, Wo), np.uint8), _seeded_mask(12, Ho, Wo, 0.5), c["mask"]])
        poses = np.stack([a["pose"], b["pose"], c["pose"]]).astype(np.float32)
        _BATCHES[(Ho, Wo)] = (coords, masks, poses)
    return _BATCHES[(Ho, Wo)]


def _args(Ho, Wo, alpha=ALPHA):
    return (THR, synth.FOCAL, Wo * SUB / 2.0, Ho * SUB / 2.0, W_ROT, W_TRANS, SOFT_CLAMP, alpha, MAX_REPROJ, SUB)


def _result(losses, rec, g, status):
    torch.cuda.synchronize()
    res = dict(loss=losses.cpu().numpy(), rec=np.ascontiguousarray(rec.cpu().numpy()[:, :, :FIELDS]),
               grad=np.ascontiguousarray(g.cpu().numpy()), rec_tail=rec.cpu().numpy()[:, :, FIELDS:])
    res["status"] = status.cpu().numpy() if status is not None else np.zeros(len(res["loss"]), np.int32)
    return res


def _gpu(coords, masks, poses, n_hyp, Ho, Wo, g=None, alpha=ALPHA, seed=1305, **kw):
    """backward_rgb_masked_batch with the records -> dict of numpy arrays (coords / masks / poses: tensors on the device; g: the
    gradient tensor to accumulate into, G0 everywhere when None)"""
    import dsacstar
    if g is None:
        g = torch.full(tuple(coords.shape), G0, dtype=torch.float32, device="cuda")
    losses, rec, status = dsacstar.backward_rgb_masked_batch(coords, masks, g, poses, n_hyp, *_args(Ho, Wo, alpha), seed, debug=True, **kw)
    assert status.dtype == torch.int32 and losses.dtype == torch.float64
    return _result(losses, rec, g, status)


def _plain(coords, poses, n_hyp, Ho, Wo, seed=1305, **kw):
    import dsacstar
    g = torch.full(tuple(coords.shape), G0, dtype=torch.float32, device="cuda")
    losses, rec = dsacstar.backward_rgb_batch(coords, g, poses, n_hyp, *_args(Ho, Wo), seed, debug=True, **kw)
    return _result(losses, rec, g, None)


_REFS = {}


def _ref_image(ref, key, coords, mask, pose, n_hyp, Ho, Wo, alpha=ALPHA, **kw):
    """the restatement of one image (incoming gradient G0), computed once per key"""
    if key not in _REFS:
        _REFS[key] = ref.backward(coords, mask, pose, n_hyp, *_args(Ho, Wo, alpha), grad=np.full((3, Ho, Wo), G0, np.float32), **kw)
    return _REFS[key]


def _assert_image(got, b, want, what):
    assert int(got["status"][b]) == want["status"], what
    assert got["loss"][b].tobytes() == np.float64(want["loss"]).tobytes(), (what, got["loss"][b], want["loss"])
    for k in ("rec", "grad"):
        x, y = np.ascontiguousarray(got[k][b]), np.ascontiguousarray(want[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        if x.tobytes() != y.tobytes():
            bits = np.uint64 if x.dtype == np.float64 else np.uint32
            bad = np.argwhere(x.view(bits) != y.view(bits))
            raise AssertionError((what, k, len(bad), bad[:8].tolist(), x[tuple(bad[0])], y[tuple(bad[0])]))


def _assert_same(a, b, what, keys=OUT):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


def _cuda(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("n_hyp", [UNSPLIT, SPLIT])
@pytest.mark.parametrize("Ho,Wo", GRIDS)
def test_bitwise_against_the_restatement(ref, Ho, Wo, n_hyp, strided):
    # the backward pass spreads sample + score over S = 1 workgroup per image at 6 hypotheses and S = 4 at 16 (B = 3)
    assert _sub_blocks(3, n_hyp) == (1 if n_hyp == UNSPLIT else 4)
    coords, masks, poses = _batch(Ho, Wo)
    m, gt = _cuda(masks, poses)
    g = None
    if strided:
        pred = torch.zeros((3, 4, Ho, Wo), device="cuda")
        pred[:, :3] = torch.from_numpy(coords).cuda()
        co = pred[:, :3]
        buf = torch.full((3, 4, Ho, Wo), G0, device="cuda")
        g = buf[:, :3]
        assert not co.is_contiguous() and not g.is_contiguous()
    else:
        co, = _cuda(coords)
    got = _gpu(co, m, gt, n_hyp, Ho, Wo, g=g, image0=20)
    for b in range(3):
        want = _ref_image(ref, (Ho, Wo, n_hyp, b), coords[b], masks[b], poses[b], n_hyp, Ho, Wo, image=20 + b)
        _assert_image(got, b, want, (Ho, Wo, n_hyp, strided, b))
        assert (want["rec"][:, 2] == 1).any() and (want["grad"] != np.float32(G0)).any()        # the case differentiates something
    assert (got["status"] == 0).all()
    if strided:
        assert (buf[:, 3] == G0).all()


@pytest.mark.parametrize("Ho,Wo,n_hyp,B", [(24, 36, UNSPLIT, 3), (24, 36, SPLIT, 3), (60, 90, 64, 2)])
def test_all_ones_mask_equals_the_unmasked_backward_pass(Ho, Wo, n_hyp, B):
    """identity A"""
    scenes = [synth.make_scene(30 + b, Ho=Ho, Wo=Wo) for b in range(B)]
    co, gt = _cuda(np.stack([s["coords"] for s in scenes]), np.stack([s["pose"] for s in scenes]).astype(np.float32))
    ones = torch.ones((B, Ho, Wo), dtype=torch.uint8, device="cuda")
    got = _gpu(co, ones, gt, n_hyp, Ho, Wo, image0=4)
    want = _plain(co, gt, n_hyp, Ho, Wo, image0=4)
    _assert_same(got, want, (Ho, Wo, n_hyp), ("loss", "rec", "grad"))
    assert (got["status"] == 0).all() and (got["rec"][:, :, 2] == 1).any()
    as_bool = _gpu(co, ones.to(torch.bool), gt, n_hyp, Ho, Wo, image0=4)          # a bool mask is viewed as uint8
    _assert_same(as_bool, got, "bool mask")


@pytest.mark.parametrize("n_hyp", [UNSPLIT, SPLIT])
@pytest.mark.parametrize("Ho,Wo", [(9, 13), (24, 36)])
def test_masked_cells_influence_nothing_and_keep_their_gradient(Ho, Wo, n_hyp):
    """identities B and C: NaN, +Inf, -Inf and 1e30 at the masked-out cells, an incoming gradient of 0.125 everywhere"""
    coords, masks, poses = _batch(Ho, Wo)
    m, gt = _cuda(masks, poses)
    want = _gpu(_cuda(coords)[0], m, gt, n_hyp, Ho, Wo, image0=20)
    out = np.broadcast_to((masks == 0)[:, None], want["grad"].shape)
    assert out.any() and (want["grad"][out] == np.float32(G0)).all()                            # C
    assert (want["grad"][~out] != np.float32(G0)).any()
    for poison in (np.nan, np.inf, -np.inf, 1e30):
        co = coords.copy()
        co[:, 0][masks == 0] = poison
        co[:, 1][masks == 0] = poison
        co[:, 2][masks == 0] = poison
        _assert_same(_gpu(_cuda(co)[0], m, gt, n_hyp, Ho, Wo, image0=20), want, (Ho, Wo, n_hyp, poison))    # B


@pytest.mark.parametrize("n_hyp", [UNSPLIT, SPLIT])
def test_a_dead_image_between_two_live_ones(ref, n_hyp):
    Ho, Wo = 9, 13
    coords, masks, poses = _batch(Ho, Wo)
    masks = masks.copy()
    masks[1] = 0
    masks[1].reshape(-1)[[5, 40, 116]] = 1                                      # three usable cells
    co, m, gt = _cuda(coords, masks, poses)
    got = _gpu(co, m, gt, n_hyp, Ho, Wo, image0=20)
    assert got["status"].tolist() == [0, 1, 0]
    assert got["loss"][1] == 0.0 and not np.signbit(got["loss"][1])
    assert (got["grad"][1] == np.float32(G0)).all() and not got["rec"][1].any() and not got["rec_tail"][1].any()
    for b in (0, 2):
        _assert_image(got, b, _ref_image(ref, (Ho, Wo, n_hyp, b), coords[b], masks[b], poses[b], n_hyp, Ho, Wo, image=20 + b), b)
        single = _gpu(co[b:b + 1], m[b:b + 1], gt[b:b + 1], n_hyp, Ho, Wo, image0=20 + b)
        for k in OUT:
            assert got[k][b].tobytes() == single[k][0].tobytes(), (b, k)
    none = _gpu(co, torch.zeros_like(m), gt, n_hyp, Ho, Wo, image0=20)         # no usable cell at all
    assert none["status"].tolist() == [1, 1, 1] and not none["loss"].any() and (none["grad"] == np.float32(G0)).all()
    assert not none["rec"].any()


def test_hypotheses_exhausted_on_a_mask_rejected_try(ref):
    """the case of tests/test_dsac_masked_bwd_cpu.py, bitwise: exhausted hypotheses above the probability threshold reach K3 with
    masked-out cells among their four and get the zero dPNP without those cells being read (NaN there changes nothing)"""
    c = EXHAUSTED
    Ho, Wo, n_hyp = c["Ho"], c["Wo"], c["n_hyp"]
    sc, mask = synth.make_scene(c["scene"], Ho=Ho, Wo=Wo), _seeded_mask(c["scene"], Ho, Wo, c["usable"])
    kw = dict(max_tries=c["max_tries"], alpha=c["alpha"])
    want = _ref_image(ref, "exhausted", sc["coords"], mask, sc["pose"], n_hyp, Ho, Wo, image=c["image"], **kw)
    flat = mask.reshape(-1)
    rejected = [h for h in range(n_hyp) if want["tries"][h] < 0 and not flat[want["cells"][h]].all()]
    assert rejected and any(want["rec"][h, 0] >= 1e-3 for h in rejected) and (want["tries"] > 0).any()
    m, gt = _cuda(mask[None], sc["pose"].astype(np.float32)[None])
    got = _gpu(_cuda(sc["coords"][None])[0], m, gt, n_hyp, Ho, Wo, image0=c["image"], **kw)
    _assert_image(got, 0, want, "exhausted")
    co = sc["coords"].copy()
    co[:, mask == 0] = np.nan
    _assert_same(_gpu(_cuda(co[None])[0], m, gt, n_hyp, Ho, Wo, image0=c["image"], **kw), got, "NaN at the masked cells")


def test_front_end_refuses_mismatched_masks():
    import dsacstar
    Ho, Wo = 8, 12
    co = torch.zeros((2, 3, Ho, Wo), device="cuda")
    g = torch.zeros_like(co)
    gt = torch.eye(4, device="cuda").repeat(2, 1, 1)
    ok = torch.ones((2, Ho, Wo), dtype=torch.uint8, device="cuda")
    bad = [ok[:1], ok.to(torch.float32), ok.to(torch.int32), ok.cpu(), torch.ones((2, Wo, Ho), dtype=torch.uint8, device="cuda"),
           torch.ones((2, Ho, 2 * Wo), dtype=torch.uint8, device="cuda")[:, :, ::2], None]
    for m in bad:
        with pytest.raises(RuntimeError):
            dsacstar.backward_rgb_masked_batch(co, m, g, gt, 6, *_args(Ho, Wo), 1305)
    with pytest.raises(RuntimeError):
        dsacstar.backward_rgb_masked_batch(co, ok, g.cpu(), gt, 6, *_args(Ho, Wo), 1305)
    with pytest.raises(RuntimeError):
        dsacstar.backward_rgb_masked_batch(co, ok, g[:1], gt, 6, *_args(Ho, Wo), 1305)
    assert not g.any()


def test_expected_pose_loss_form_with_a_mask():
    """loss.expected_pose_loss_and_output_gradient(mask=...) at 24x36, B = 3, the middle frame dead"""
    from crossloc_amd import loss as xl_loss
    Ho, Wo, B = 24, 36, 3
    coords, masks, poses = _batch(Ho, Wo)
    masks = masks.copy()
    masks[0] = _seeded_mask(11, Ho, Wo, 0.7)
    masks[1] = 0
    masks[1].reshape(-1)[[5, 40, 116]] = 1
    pred = torch.zeros((B, 4, Ho, Wo), device="cuda")
    pred[:, :3] = torch.from_numpy(coords).cuda()
    pred[:, 3] = 1.0
    m, gt = _cuda(masks, poses)
    args = (gt, [synth.FOCAL] * B, Ho * SUB, Wo * SUB, SPLIT, THR, ALPHA, MAX_REPROJ, W_ROT, W_TRANS, SOFT_CLAMP, 1305)
    mean_loss, stats, grad = xl_loss.expected_pose_loss_and_output_gradient(pred, *args, image0=20, mask=m)
    torch.cuda.synchronize()
    acc = xl_loss.E2E_FRAME_FIELDS["accepted"]
    assert float(stats[B, xl_loss.E2E_SUMMARY_FIELDS["accepted"]]) == 2
    assert stats[:B, acc].tolist() == [1.0, 0.0, 1.0]
    assert grad.shape == pred.shape and not grad[1].any() and not grad[:, 3].any()
    for b in (0, 2):
        assert not grad[b, :3][:, m[b] == 0].any() and grad[b, :3][:, m[b] != 0].any(), b
    live = stats[[0, 2], xl_loss.E2E_FRAME_FIELDS["loss"]]
    assert torch.isfinite(live).all() and float(mean_loss) == float((live[0] + live[1]) / 2)

    ones = torch.ones((B, Ho, Wo), dtype=torch.uint8, device="cuda")
    _, stats_ones, grad_ones = xl_loss.expected_pose_loss_and_output_gradient(pred, *args, image0=20, mask=ones)
    _, stats_free, grad_free = xl_loss.expected_pose_loss_and_output_gradient(pred, *args, image0=20)
    assert torch.equal(grad_ones, grad_free) and torch.equal(stats_ones, stats_free)
    assert float(stats_free[B, 1]) == B and not torch.equal(grad_free, grad)
    for kw in (dict(depth=torch.ones((B, Ho, Wo), device="cuda")), dict(cam_coords=torch.ones((B, 3, Ho, Wo), device="cuda"))):
        with pytest.raises(RuntimeError):
            xl_loss.expected_pose_loss_and_output_gradient(pred, *args, image0=20, mask=m, **kw)


def test_one_e2e_step_with_the_label_mask(monkeypatch):
    """make_e2e_step with opt.mask = 'labels' on a tiny network: the top two label rows are nodata; the step runs, every frame is
    accepted, the pose gradient is exact zeros on those rows and not zero elsewhere"""
    from crossloc_amd import loss as xl_loss, networks, optim, train_e2e, training
    from crossloc_amd.weights import seeded_state_dict
    B, H, W, HYP, FOCAL = 2, 64, 96, 16, 60.0
    Ho, Wo = H // SUB, W // SUB
    _, gt, poses = synth.make_batch(10, B, noise=0.5, outlier_ratio=0.0, Ho=Ho, Wo=Wo, focal=FOCAL)
    opt = train_e2e._config_parser(["naturescape", "--network_in", "unused", "--uncertainty", "MLE", "--hypotheses", str(HYP),
                                    "--seed", "5", "--mask", "labels"])
    nodata = training.get_nodata_value(opt.scene)
    gt = gt.copy()
    gt[:, :, :2] = nodata
    net = networks.TransPoseNet(torch.tensor(synth.SCENE_MEAN, dtype=torch.float32), True, False, 0, 0, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=11))
    net = net.cuda().train()
    before = [p.detach().clone() for p in net.parameters()]
    seen = {}
    inner = xl_loss.expected_pose_loss_and_output_gradient

    def spy(*a, **kw):
        out = inner(*a, **kw)
        seen.update(mask=kw.get("mask"), grad=out[2].clone(), stats=out[1].clone())
        return out

    monkeypatch.setattr(training.xl_loss, "expected_pose_loss_and_output_gradient", spy)
    step = training.make_e2e_step(net, optim.Adam(net.parameters(), lr=1e-4), opt)
    images = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(2)).cuda()
    loss, summary = step(images, torch.from_numpy(poses.astype(np.float32)).cuda(), torch.from_numpy(gt).cuda(),
                         torch.tensor([FOCAL, FOCAL * 1.01]), 4, image0=3)
    torch.cuda.synchronize()
    want_mask = torch.ones((B, Ho, Wo), dtype=torch.uint8, device="cuda")
    want_mask[:, :2] = 0
    assert seen["mask"] is not None and torch.equal(seen["mask"], want_mask)
    assert float(summary[xl_loss.E2E_SUMMARY_FIELDS["accepted"]]) == B and bool(torch.isfinite(loss))
    pose_grad = seen["grad"][:, :3]
    assert not pose_grad[:, :, :2].any()
    for b in range(B):
        assert pose_grad[b, :, 2:].any(), b
    assert any(not torch.equal(a, b) for a, b in zip(net.parameters(), before))
