"""GPU checks of the masked RGB DSAC* solver (dsacstar.forward_rgb_masked_batch): every output bitwise against the serial
restatement tests/dsac_masked_ref.c in both launch forms, the two identities (all-ones mask == forward_rgb_batch; the values at
masked-out cells influence nothing), dead images, a sparse mask with exhausted hypotheses, and the plumbing through
evaluation.localize_batch / PipelinedLocalizer."""
import numpy as np
import pytest
import torch

import dsac_masked_ref
from crossloc_amd import synth

pytestmark = pytest.mark.gpu

GRIDS = [(8, 12), (9, 13), (24, 36)]
FUSED, SPLIT = 6, 16                       # hypotheses: one fused launch / four sub-blocks per image at B = 3
THR, ALPHA, MAX_REPROJ, SUB = 10.0, 100.0, 100.0, 8
OUT = ("pose", "cells", "tries", "scores", "dbg")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return dsac_masked_ref.load(tmp_path_factory.mktemp("dsac_masked_ref"))


def _sub_blocks(B, n_hyp):
    from crossloc_amd import _lib
    return int(_lib.lib().xl_dsac_forward_sub_blocks(B, n_hyp))


def _seeded_mask(seed, Ho, Wo, usable):
    return (np.random.default_rng([seed, 0x4d41]).random((Ho, Wo)) < usable).astype(np.uint8)


_BATCHES = {}


def _batch(Ho, Wo):
    """three images with a mask each: all ones, a seeded random 50 %, the decoy band -> coords [3,3,Ho,Wo], masks [3,Ho,Wo]"""
    if (Ho, Wo) not in _BATCHES:
        a, b = synth.make_scene(11, Ho=Ho, Wo=Wo), synth.make_scene(12, Ho=Ho, Wo=Wo)
        c = synth.make_decoy_scene(13, decoy=0.6, Ho=Ho, Wo=Wo)
        coords = np.stack([a["coords"], b["coords"], c["coords"]])
        masks = np.stack([np.ones((Ho, Wo), np.uint8), _seeded_mask(12, Ho, Wo, 0.5), c["mask"]])
        _BATCHES[(Ho, Wo)] = (coords, masks)
    return _BATCHES[(Ho, Wo)]


def _intr(Ho, Wo):
    return (THR, synth.FOCAL, Wo * SUB / 2.0, Ho * SUB / 2.0, ALPHA, MAX_REPROJ, SUB)


def _gpu(coords, masks, n_hyp, Ho, Wo, **kw):
    """forward_rgb_masked_batch with debug outputs -> dict of numpy arrays (coords / masks: tensors on the device)"""
    import dsacstar
    poses = torch.full((coords.shape[0], 4, 4), 7.0, dtype=torch.float32, device="cuda")
    out = dsacstar.forward_rgb_masked_batch(coords, masks, poses, n_hyp, *_intr(Ho, Wo), debug=True, **kw)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["pose"] = poses.cpu().numpy()
    return res


def _plain(coords, n_hyp, Ho, Wo, **kw):
    import dsacstar
    poses = torch.full((coords.shape[0], 4, 4), 7.0, dtype=torch.float32, device="cuda")
    out = dsacstar.forward_rgb_batch(coords, poses, n_hyp, *_intr(Ho, Wo), debug=True, **kw)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["pose"] = poses.cpu().numpy()
    return res


_REFS = {}


def _ref_image(ref, key, coords, mask, n_hyp, Ho, Wo, **kw):
    """the restatement of one image, computed once per key"""
    if key not in _REFS:
        _REFS[key] = ref.forward(coords, mask, n_hyp, *_intr(Ho, Wo), **kw)
    return _REFS[key]


def _assert_image(got, b, want, what):
    assert int(got["status"][b]) == want["status"], what
    for k in OUT:
        x, y = np.ascontiguousarray(got[k][b]), np.ascontiguousarray(want[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        assert x.tobytes() == y.tobytes(), (what, k)


def _assert_same(a, b, what, keys=OUT + ("status",)):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("n_hyp", [FUSED, SPLIT])
@pytest.mark.parametrize("Ho,Wo", GRIDS)
def test_bitwise_against_the_restatement(ref, Ho, Wo, n_hyp, strided):
    assert _sub_blocks(3, n_hyp) == (1 if n_hyp == FUSED else 4)
    coords, masks = _batch(Ho, Wo)
    if strided:
        pred = torch.zeros((3, 4, Ho, Wo), device="cuda")
        pred[:, :3] = torch.from_numpy(coords).cuda()
        co = pred[:, :3]
        assert not co.is_contiguous()
    else:
        co = torch.from_numpy(coords).cuda()
    got = _gpu(co, torch.from_numpy(masks).cuda(), n_hyp, Ho, Wo, image0=20)
    for b in range(3):
        want = _ref_image(ref, (Ho, Wo, n_hyp, b), coords[b], masks[b], n_hyp, Ho, Wo, image=20 + b)
        _assert_image(got, b, want, (Ho, Wo, n_hyp, strided, b))
    assert (got["status"] == 0).all()


def test_fused_form_with_several_hypotheses_per_wave(ref):
    """B = 260 at 8x12 with 12 hypotheses: one workgroup per image, three hypotheses per wavefront"""
    Ho, Wo, n_hyp, B = 8, 12, 12, 260
    assert _sub_blocks(B, n_hyp) == 1
    coords3, masks3 = _batch(Ho, Wo)
    idx = np.arange(B) % 3
    coords, masks = coords3[idx], masks3[idx]
    got = _gpu(torch.from_numpy(coords).cuda(), torch.from_numpy(masks).cuda(), n_hyp, Ho, Wo, image0=5, image_stride=3)
    for b in (0, 1, 2, 130, 259):
        want = ref.forward(coords[b], masks[b], n_hyp, *_intr(Ho, Wo), image=5 + 3 * b)
        _assert_image(got, b, want, b)
    assert (got["status"] == 0).all()


@pytest.mark.parametrize("Ho,Wo,n_hyp,B", [(24, 36, FUSED, 3), (24, 36, SPLIT, 3), (60, 90, 64, 2)])
def test_all_ones_mask_equals_the_unmasked_solver(Ho, Wo, n_hyp, B):
    """identity A"""
    coords = np.stack([synth.make_scene(30 + b, Ho=Ho, Wo=Wo)["coords"] for b in range(B)])
    co = torch.from_numpy(coords).cuda()
    ones = torch.ones((B, Ho, Wo), dtype=torch.uint8, device="cuda")
    got = _gpu(co, ones, n_hyp, Ho, Wo, image0=4)
    want = _plain(co, n_hyp, Ho, Wo, image0=4)
    _assert_same(got, want, (Ho, Wo, n_hyp), OUT)
    assert (got["status"] == 0).all()
    as_bool = _gpu(co, ones.to(torch.bool), n_hyp, Ho, Wo, image0=4)           # a bool mask is viewed as uint8
    _assert_same(as_bool, got, "bool mask")


@pytest.mark.parametrize("n_hyp", [FUSED, SPLIT])
@pytest.mark.parametrize("Ho,Wo", [(9, 13), (24, 36)])
def test_masked_cell_values_influence_no_output_bit(Ho, Wo, n_hyp):
    """identity B: NaN, +Inf, -Inf and 1e30 at the masked-out cells"""
    coords, masks = _batch(Ho, Wo)
    m = torch.from_numpy(masks).cuda()
    want = _gpu(torch.from_numpy(coords).cuda(), m, n_hyp, Ho, Wo, image0=20)
    for poison in (np.nan, np.inf, -np.inf, 1e30):
        co = coords.copy()
        co[:, 0][masks == 0] = poison
        co[:, 1][masks == 0] = poison
        co[:, 2][masks == 0] = poison
        _assert_same(_gpu(torch.from_numpy(co).cuda(), m, n_hyp, Ho, Wo, image0=20), want, (Ho, Wo, n_hyp, poison))


@pytest.mark.parametrize("n_hyp", [FUSED, SPLIT])
def test_a_dead_image_between_two_live_ones(ref, n_hyp):
    Ho, Wo = 9, 13
    coords, masks = _batch(Ho, Wo)
    masks = masks.copy()
    masks[1] = 0
    masks[1].reshape(-1)[[5, 40, 116]] = 1                                      # three usable cells; max_tries at its default
    co, m = torch.from_numpy(coords).cuda(), torch.from_numpy(masks).cuda()
    got = _gpu(co, m, n_hyp, Ho, Wo, image0=20)
    assert got["status"].tolist() == [0, 1, 0]
    assert (got["tries"][1] == 0).all() and (got["scores"][1] == 0).all() and (got["cells"][1] == -1).all()
    assert got["dbg"][1][0] == -1 and np.array_equal(got["pose"][1], np.eye(4, dtype=np.float32))
    _assert_image(got, 1, ref.forward(coords[1], masks[1], n_hyp, *_intr(Ho, Wo), image=21), "dead")
    for b in (0, 2):
        single = _gpu(co[b:b + 1], m[b:b + 1], n_hyp, Ho, Wo, image0=20 + b)
        for k in OUT + ("status",):
            assert got[k][b].tobytes() == single[k][0].tobytes(), (b, k)
    none = _gpu(co, torch.zeros_like(m), n_hyp, Ho, Wo, image0=20)             # no usable cell at all
    assert none["status"].tolist() == [1, 1, 1] and (none["tries"] == 0).all()


def test_sparse_mask_with_exhausted_hypotheses(ref):
    """10 % usable at 24x36, 4096 tries: hypotheses that find no usable quadruple are the last try's result"""
    Ho, Wo, n_hyp, max_tries = 24, 36, SPLIT, 4096
    coords, _ = _batch(Ho, Wo)
    masks = np.stack([_seeded_mask(40 + b, Ho, Wo, 0.1) for b in range(3)])
    got = _gpu(torch.from_numpy(coords).cuda(), torch.from_numpy(masks).cuda(), n_hyp, Ho, Wo, image0=20, max_tries=max_tries)
    for b in range(3):
        _assert_image(got, b, ref.forward(coords[b], masks[b], n_hyp, *_intr(Ho, Wo), image=20 + b, max_tries=max_tries), b)
    assert (got["tries"] == -max_tries).any() and (got["tries"] > 0).any()
    fused = _gpu(torch.from_numpy(coords[:1]).cuda(), torch.from_numpy(masks[:1]).cuda(), FUSED, Ho, Wo, image0=20, max_tries=100)
    _assert_image(fused, 0, ref.forward(coords[0], masks[0], FUSED, *_intr(Ho, Wo), image=20, max_tries=100), "fused, 100 tries")


class _PlantNet(torch.nn.Module):
    """Stand-in for the network in the wiring tests: the solver's input is given by the caller (`scene_coords`); the fourth
    channel of the output, if any, is the given sigma map."""
    num_task_channel = 3
    OUTPUT_SUBSAMPLE = SUB

    def __init__(self, sigma=None):
        super().__init__()
        self.sigma = sigma

    def forward(self, images, plan_slot=0):
        B, _, H, W = images.shape
        out = torch.zeros((B, 3 if self.sigma is None else 4, H // SUB, W // SUB), device=images.device)
        if self.sigma is not None:
            out[:, 3] = self.sigma
        return out


def test_localize_batch_and_pipelined_localizer_plumbing():
    import dsacstar
    from crossloc_amd import evaluation
    Ho, Wo, n_hyp = 24, 36, SPLIT
    H, W = Ho * SUB, Wo * SUB
    coords, masks = _batch(Ho, Wo)
    co, m = torch.from_numpy(coords).cuda(), torch.from_numpy(masks).cuda()
    images = torch.zeros((3, 3, H, W), device="cuda")
    direct = torch.zeros((3, 4, 4), device="cuda")
    status = dsacstar.forward_rgb_masked_batch(co, m, direct, n_hyp, *_intr(Ho, Wo), image0=3)
    assert status.dtype == torch.int32 and tuple(status.shape) == (3,)
    sigma = torch.from_numpy(np.random.default_rng(9).uniform(0.1, 2.0, size=(3, Ho, Wo)).astype(np.float32)).cuda()
    by_hand = torch.zeros((3, 4, 4), device="cuda")
    dsacstar.forward_rgb_masked_batch(co, evaluation.cell_mask(sigma=sigma, max_sigma=1.0), by_hand, n_hyp, *_intr(Ho, Wo), image0=3)
    net, net_sigma = _PlantNet(), _PlantNet(sigma)

    plain = evaluation.localize_batch(net, images, n_hyp, synth.FOCAL, H, W, image0=3, scene_coords=co)
    assert len(plain) == 2                                                     # without a mask: the old tuple
    out = evaluation.localize_batch(net, images, n_hyp, synth.FOCAL, H, W, image0=3, scene_coords=co, mask=m)
    sg = evaluation.localize_batch(net_sigma, images, n_hyp, synth.FOCAL, H, W, image0=3, scene_coords=co, mask_max_sigma=1.0)
    loc = evaluation.PipelinedLocalizer(net, n_hyp, synth.FOCAL, H, W)
    p_plain = loc.submit(images, image0=3, scene_coords=co)
    p_out = loc.submit(images, image0=3, scene_coords=co, mask=m)
    p_sg = evaluation.PipelinedLocalizer(net_sigma, n_hyp, synth.FOCAL, H, W)
    p_sg_out = p_sg.submit(images, image0=3, scene_coords=co, mask_max_sigma=1.0)
    loc.finish()
    p_sg.finish()
    torch.cuda.synchronize()
    assert len(out) == 3 and len(sg) == 3 and len(p_plain) == 2 and len(p_out) == 3 and len(p_sg_out) == 3
    assert torch.equal(p_plain[0], plain[0]) and not torch.equal(plain[0], direct)
    for got in (out, p_out):
        assert torch.equal(got[0], direct) and torch.equal(got[2], status)
    for got in (sg, p_sg_out):
        assert torch.equal(got[0], by_hand) and not torch.equal(got[0], direct)
        assert got[2].dtype == torch.int32 and got[2].tolist() == [0, 0, 0]

    depth = torch.ones((3, Ho, Wo), device="cuda")
    refused = [dict(mask=m, depth=depth), dict(mask=m, cam_coords=torch.ones((3, 3, Ho, Wo), device="cuda")),
               dict(mask=m, quality=True), dict(mask=m, refine="inliers"), dict(mask=m, refine="sigma"),
               dict(mask_max_sigma=1.0, quality=True), dict(mask=m, mask_max_sigma=1.0)]
    for kw in refused:
        with pytest.raises(RuntimeError):
            evaluation.localize_batch(net_sigma, images, n_hyp, synth.FOCAL, H, W, scene_coords=co, **kw)
        with pytest.raises(RuntimeError):
            p_sg.submit(images, scene_coords=co, **kw)
    with pytest.raises(RuntimeError, match="uncertainty channel"):
        evaluation.localize_batch(net, images, n_hyp, synth.FOCAL, H, W, scene_coords=co, mask_max_sigma=1.0)
    p_sg.finish()
    torch.cuda.synchronize()


def test_front_end_refuses_mismatched_masks():
    import dsacstar
    Ho, Wo = 8, 12
    co = torch.zeros((2, 3, Ho, Wo), device="cuda")
    poses = torch.zeros((2, 4, 4), device="cuda")
    ok = torch.ones((2, Ho, Wo), dtype=torch.uint8, device="cuda")
    bad = [ok[:1], ok.to(torch.float32), ok.to(torch.int32), ok.cpu(), torch.ones((2, Wo, Ho), dtype=torch.uint8, device="cuda"),
           torch.ones((2, Ho, 2 * Wo), dtype=torch.uint8, device="cuda")[:, :, ::2], None]
    for m in bad:
        with pytest.raises(RuntimeError):
            dsacstar.forward_rgb_masked_batch(co, m, poses, 6, *_intr(Ho, Wo))
    with pytest.raises(RuntimeError):
        dsacstar.forward_rgb_masked_batch(co, ok, poses.cpu(), 6, *_intr(Ho, Wo))


def test_cell_mask_criteria():
    from crossloc_amd import evaluation
    Ho, Wo = 4, 6
    sigma = torch.full((1, Ho, Wo), 0.5, device="cuda")
    sigma[0, 0, 0], sigma[0, 1, 1] = 2.0, float("nan")
    full = torch.zeros((1, Ho * SUB, Wo * SUB), dtype=torch.int64, device="cuda")
    full[0, 2 * SUB + 4, 3 * SUB + 4] = 5                                       # the centre of cell (2, 3)
    full[0, 2 * SUB + 3, 4 * SUB + 4] = 5                                       # not a cell centre
    labels = torch.zeros((1, 3, Ho, Wo), device="cuda")
    labels[0, 1, 3, 5] = -1.0
    got = evaluation.cell_mask(sigma=sigma, max_sigma=1.0, class_map=full, exclude_classes=(5, 7), labels=labels)
    want = torch.ones((1, Ho, Wo), dtype=torch.uint8, device="cuda")
    for y, x in ((0, 0), (1, 1), (2, 3), (3, 5)):
        want[0, y, x] = 0
    assert got.dtype == torch.uint8 and got.is_contiguous() and got.is_cuda and torch.equal(got, want)
    per_cell = full[:, SUB // 2::SUB, SUB // 2::SUB].contiguous()
    assert torch.equal(evaluation.cell_mask(class_map=per_cell, exclude_classes=(5,)),
                       evaluation.cell_mask(sigma=sigma, max_sigma=9.0, class_map=full, exclude_classes=(5,)) | (sigma != sigma).to(torch.uint8))
    with pytest.raises(RuntimeError):
        evaluation.cell_mask()
    with pytest.raises(RuntimeError):
        evaluation.cell_mask(sigma=sigma)
