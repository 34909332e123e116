"""GPU checks of the masked RGB backward pass under the compact sampler (dsacstar.backward_rgb_masked_batch(sampler="compact")):
loss, status, the 53 record fields and the gradient bitwise against the serial restatement tests/dsac_compact_ref.c with one and
with four sample + score workgroups per image, the hypotheses being the compact forward's, masked-out cells keeping their
incoming gradient, exhausted hypotheses, and the plumbing through loss.expected_pose_loss_and_output_gradient."""
import numpy as np
import pytest
import torch

import dsac_compact_ref
from crossloc_amd import synth

pytestmark = pytest.mark.gpu

GRIDS = [(9, 13), (24, 36)]
UNSPLIT, SPLIT = 6, 16                     # hypotheses: the sample + score launch with one / with four workgroups per image at B = 3
THR, ALPHA, MAX_REPROJ, SUB = 10.0, 100.0, 100.0, 8
W_ROT, W_TRANS, SOFT_CLAMP = 1.0, 100.0, 100.0
MAX_TRIES = 4096
FIELDS = dsac_compact_ref.FIELDS
G0 = 0.125                                 # the incoming gradient, everywhere
OUT = ("loss", "rec", "grad", "status")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return dsac_compact_ref.load(tmp_path_factory.mktemp("dsac_compact_ref"))


def _sub_blocks(B, n_hyp):
    from crossloc_amd import _lib
    return int(_lib.lib().xl_dsac_backward_sub_blocks(B, n_hyp))


def _seeded_mask(seed, Ho, Wo, usable):
    return (np.random.default_rng([seed, 0x4d41]).random((Ho, Wo)) < usable).astype(np.uint8)


_BATCHES = {}


def _batch(Ho, Wo):
    """three images with a mask each: a seeded random 50 %, a seeded 10 %, the decoy band -> coords [3,3,Ho,Wo], masks [3,Ho,Wo],
    ground-truth poses [3,4,4] float32"""
    if (Ho, Wo) not in _BATCHES:
        a, b = synth.make_scene(11, Ho=Ho, Wo=Wo), synth.make_scene(12, Ho=Ho, Wo=Wo)
        c = synth.make_decoy_scene(13, decoy=0.6, Ho=Ho, Wo=Wo)
        coords = np.stack([a["coords"], b["coords"], c["coords"]])
        masks = np.stack([_seeded_mask(11, Ho, Wo, 0.5), _seeded_mask(12, Ho, Wo, 0.1), c["mask"]])
        assert (masks.reshape(3, -1).sum(1) >= 4).all()
        poses = np.stack([a["pose"], b["pose"], c["pose"]]).astype(np.float32)
        _BATCHES[(Ho, Wo)] = (coords, masks, poses)
    return _BATCHES[(Ho, Wo)]


def _args(Ho, Wo, alpha=ALPHA):
    return (THR, synth.FOCAL, Wo * SUB / 2.0, Ho * SUB / 2.0, W_ROT, W_TRANS, SOFT_CLAMP, alpha, MAX_REPROJ, SUB)


def _gpu(coords, masks, poses, n_hyp, Ho, Wo, g=None, alpha=ALPHA, seed=1305, sampler="compact", max_tries=MAX_TRIES, **kw):
    """backward_rgb_masked_batch with the records -> dict of numpy arrays (coords / masks / poses: tensors on the device; g: the
    gradient tensor to accumulate into, G0 everywhere when None)"""
    import dsacstar
    if g is None:
        g = torch.full(tuple(coords.shape), G0, dtype=torch.float32, device="cuda")
    losses, rec, status = dsacstar.backward_rgb_masked_batch(coords, masks, g, poses, n_hyp, *_args(Ho, Wo, alpha), seed, debug=True,
                                                             sampler=sampler, max_tries=max_tries, **kw)
    torch.cuda.synchronize()
    assert status.dtype == torch.int32 and losses.dtype == torch.float64
    return dict(loss=losses.cpu().numpy(), rec=np.ascontiguousarray(rec.cpu().numpy()[:, :, :FIELDS]),
                grad=np.ascontiguousarray(g.cpu().numpy()), status=status.cpu().numpy())


def _forward_cells(coords, masks, n_hyp, Ho, Wo, max_tries=MAX_TRIES, **kw):
    import dsacstar
    poses = torch.zeros((coords.shape[0], 4, 4), dtype=torch.float32, device="cuda")
    out = dsacstar.forward_rgb_masked_batch(coords, masks, poses, n_hyp, THR, synth.FOCAL, Wo * SUB / 2.0, Ho * SUB / 2.0, ALPHA,
                                            MAX_REPROJ, SUB, debug=True, sampler="compact", max_tries=max_tries, **kw)
    torch.cuda.synchronize()
    return out["cells"].cpu().numpy(), out["tries"].cpu().numpy()


_REFS = {}


def _ref_image(ref, key, coords, mask, pose, n_hyp, Ho, Wo, alpha=ALPHA, max_tries=MAX_TRIES, **kw):
    """the restatement of one image (incoming gradient G0), computed once per key"""
    if key not in _REFS:
        _REFS[key] = ref.backward(coords, mask, pose, n_hyp, *_args(Ho, Wo, alpha), grad=np.full((3, Ho, Wo), G0, np.float32),
                                  max_tries=max_tries, **kw)
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
    cells, tries = _forward_cells(co, m, n_hyp, Ho, Wo, image0=20)
    for b in range(3):
        want = _ref_image(ref, (Ho, Wo, n_hyp, b), coords[b], masks[b], poses[b], n_hyp, Ho, Wo, image=20 + b)
        _assert_image(got, b, want, (Ho, Wo, n_hyp, strided, b))
        assert (want["rec"][:, 2] == 1).any() and (want["grad"] != np.float32(G0)).any()        # the case differentiates something
        # the hypotheses differentiated are the compact forward's for the same keys
        assert np.array_equal(want["cells"], cells[b]) and np.array_equal(want["tries"], tries[b]), b
        out = np.broadcast_to((masks[b] == 0)[None], got["grad"][b].shape)
        assert out.any() and (got["grad"][b][out] == np.float32(G0)).all()                      # masked-out cells keep theirs
    assert (got["status"] == 0).all()
    if strided:
        assert (buf[:, 3] == G0).all()


@pytest.mark.parametrize("n_hyp", [UNSPLIT, SPLIT])
def test_masked_cells_influence_nothing(n_hyp):
    """NaN, +Inf, -Inf and 1e30 at the masked-out cells"""
    Ho, Wo = 9, 13
    coords, masks, poses = _batch(Ho, Wo)
    m, gt = _cuda(masks, poses)
    want = _gpu(_cuda(coords)[0], m, gt, n_hyp, Ho, Wo, image0=20)
    for poison in (np.nan, np.inf, -np.inf, 1e30):
        co = coords.copy()
        for c in range(3):
            co[:, c][masks == 0] = poison
        got = _gpu(_cuda(co)[0], m, gt, n_hyp, Ho, Wo, image0=20)
        for k in OUT:
            assert got[k].tobytes() == want[k].tobytes(), (n_hyp, poison, k)


def test_exhausted_hypotheses_are_differentiated_like_the_unmasked_ones(ref):
    """two tries per hypothesis on a noisy frame with a soft inlier count (alpha 0.1 keeps every hypothesis above the probability
    threshold): hypotheses that ran out carry four usable cells and their last P3P result, and K3 solves for them"""
    Ho, Wo, n_hyp = 24, 36, SPLIT
    sc = synth.make_scene(7, Ho=Ho, Wo=Wo, noise=2.0, outlier_ratio=0.5)
    mask = _seeded_mask(7, Ho, Wo, 0.4)
    kw = dict(max_tries=2, alpha=0.1)
    want = _ref_image(ref, "exhausted", sc["coords"], mask, sc["pose"], n_hyp, Ho, Wo, image=7, **kw)
    out_of_tries = np.flatnonzero(want["tries"] < 0)
    assert out_of_tries.size > 0 and (want["rec"][out_of_tries, 0] >= 1e-3).any()
    assert mask.reshape(-1)[want["cells"]].all()
    m, gt = _cuda(mask[None], sc["pose"].astype(np.float32)[None])
    got = _gpu(_cuda(sc["coords"][None])[0], m, gt, n_hyp, Ho, Wo, image0=7, **kw)
    _assert_image(got, 0, want, "exhausted")


def test_a_dead_image_between_two_live_ones(ref):
    Ho, Wo, n_hyp = 9, 13, SPLIT
    coords, masks, poses = _batch(Ho, Wo)
    masks = masks.copy()
    masks[1] = 0
    masks[1].reshape(-1)[[5, 40, 116]] = 1                                      # three usable cells
    co, m, gt = _cuda(coords, masks, poses)
    got = _gpu(co, m, gt, n_hyp, Ho, Wo, image0=20)
    assert got["status"].tolist() == [0, 1, 0]
    assert got["loss"][1] == 0.0 and (got["grad"][1] == np.float32(G0)).all() and not got["rec"][1].any()
    for b in (0, 2):
        _assert_image(got, b, _ref_image(ref, (Ho, Wo, n_hyp, b), coords[b], masks[b], poses[b], n_hyp, Ho, Wo, image=20 + b), b)


def test_expected_pose_loss_form_with_the_compact_sampler():
    """loss.expected_pose_loss_and_output_gradient(mask=..., mask_sampler="compact") returns backward_rgb_masked_batch's numbers"""
    import dsacstar
    from crossloc_amd import loss as xl_loss
    Ho, Wo, B = 24, 36, 3
    coords, masks, poses = _batch(Ho, Wo)
    pred = torch.zeros((B, 4, Ho, Wo), device="cuda")
    pred[:, :3] = torch.from_numpy(coords).cuda()
    pred[:, 3] = 1.0
    m, gt = _cuda(masks, poses)
    args = (gt, [synth.FOCAL] * B, Ho * SUB, Wo * SUB, SPLIT, THR, ALPHA, MAX_REPROJ, W_ROT, W_TRANS, SOFT_CLAMP, 1305)
    mean_loss, stats, grad = xl_loss.expected_pose_loss_and_output_gradient(pred, *args, image0=20, mask=m, mask_sampler="compact")
    g = torch.zeros((B, 3, Ho, Wo), device="cuda")
    focals = torch.full((B,), synth.FOCAL, device="cuda")
    losses, status = dsacstar.backward_rgb_masked_batch(pred[:, :3], m, g, gt, SPLIT, THR, 0.0, Wo * SUB / 2, Ho * SUB / 2, W_ROT,
                                                        W_TRANS, SOFT_CLAMP, ALPHA, MAX_REPROJ, SUB, 1305, image0=20, focals=focals,
                                                        max_tries=xl_loss.E2E_MAX_TRIES, sampler="compact")
    want_grad, want_stats = xl_loss.finish_pose_gradient(g, losses, 4, 1.0, 0.0, None, 0.0)
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0, 0]
    assert torch.equal(grad, want_grad) and torch.equal(stats, want_stats) and float(mean_loss) == float(want_stats[B, 0])
    # under the default sampler the 10 % frame exhausts its hypotheses: other numbers
    _, stats_reject, _ = xl_loss.expected_pose_loss_and_output_gradient(pred, *args, image0=20, mask=m)
    assert not torch.equal(stats_reject, stats)
    with pytest.raises(RuntimeError, match="needs mask"):
        xl_loss.expected_pose_loss_and_output_gradient(pred, *args, image0=20, mask_sampler="compact")
