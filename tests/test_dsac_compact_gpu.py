"""GPU checks of the compact sampler of the masked RGB DSAC* solver (dsacstar.forward_rgb_masked_batch(sampler="compact")): every
output bitwise against the serial restatement tests/dsac_compact_ref.c in both launch forms, a grid with 317 mask words, several
hypotheses per wave, the default sampler untouched, poisoned masked cells, dead images, the 10 % mask that exhausts the reject
sampler, and the plumbing through evaluation.localize_batch / PipelinedLocalizer."""
import numpy as np
import pytest
import torch

import dsac_compact_ref
from crossloc_amd import synth

pytestmark = pytest.mark.gpu

GRIDS = [(8, 12), (9, 13), (24, 36)]
FUSED, SPLIT = 6, 16                       # hypotheses: one fused launch / four sub-blocks per image at B = 3 .. 5
THR, ALPHA, MAX_REPROJ, SUB = 10.0, 100.0, 100.0, 8
MAX_TRIES = 4096
OUT = ("pose", "cells", "tries", "scores", "dbg")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return dsac_compact_ref.load(tmp_path_factory.mktemp("dsac_compact_ref"))


def _sub_blocks(B, n_hyp):
    from crossloc_amd import _lib
    return int(_lib.lib().xl_dsac_forward_sub_blocks(B, n_hyp))


def _seeded_mask(seed, Ho, Wo, usable):
    return (np.random.default_rng([seed, 0x4d41]).random((Ho, Wo)) < usable).astype(np.uint8)


def _four_cells(Ho, Wo):
    """exactly four usable cells spread over the grid (no three of them on a line of the grid)"""
    m = np.zeros((Ho, Wo), np.uint8)
    for y, x in ((1, 2), (Ho // 2, Wo - 2), (Ho - 2, 1), (Ho - 1, Wo // 2 + 1)):
        m[y, x] = 1
    assert int(m.sum()) == 4
    return m


_BATCHES = {}


def _batch(Ho, Wo):
    """five images with a mask each: all ones, a seeded random 50 %, the decoy band, a seeded 10 %, four usable cells
    -> coords [5,3,Ho,Wo], masks [5,Ho,Wo]"""
    if (Ho, Wo) not in _BATCHES:
        a, b = synth.make_scene(11, Ho=Ho, Wo=Wo), synth.make_scene(12, Ho=Ho, Wo=Wo)
        c = synth.make_decoy_scene(13, decoy=0.6, Ho=Ho, Wo=Wo)
        d, e = synth.make_scene(14, Ho=Ho, Wo=Wo), synth.make_scene(15, Ho=Ho, Wo=Wo, noise=0.0, outlier_ratio=0.0)
        coords = np.stack([a["coords"], b["coords"], c["coords"], d["coords"], e["coords"]])
        masks = np.stack([np.ones((Ho, Wo), np.uint8), _seeded_mask(12, Ho, Wo, 0.5), c["mask"], _seeded_mask(14, Ho, Wo, 0.1),
                          _four_cells(Ho, Wo)])
        assert (masks.reshape(5, -1).sum(1) >= 4).all()
        _BATCHES[(Ho, Wo)] = (coords, masks)
    return _BATCHES[(Ho, Wo)]


def _intr(Ho, Wo):
    return (THR, synth.FOCAL, Wo * SUB / 2.0, Ho * SUB / 2.0, ALPHA, MAX_REPROJ, SUB)


def _gpu(coords, masks, n_hyp, Ho, Wo, sampler="compact", max_tries=MAX_TRIES, **kw):
    """forward_rgb_masked_batch with debug outputs -> dict of numpy arrays (coords / masks: tensors on the device)"""
    import dsacstar
    poses = torch.full((coords.shape[0], 4, 4), 7.0, dtype=torch.float32, device="cuda")
    if sampler is not None:
        kw["sampler"] = sampler
    out = dsacstar.forward_rgb_masked_batch(coords, masks, poses, n_hyp, *_intr(Ho, Wo), debug=True, max_tries=max_tries, **kw)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["pose"] = poses.cpu().numpy()
    return res


_REFS = {}


def _ref_image(ref, key, coords, mask, n_hyp, Ho, Wo, max_tries=MAX_TRIES, **kw):
    """the restatement of one image, computed once per key"""
    if key not in _REFS:
        _REFS[key] = ref.forward(coords, mask, n_hyp, *_intr(Ho, Wo), max_tries=max_tries, **kw)
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
    B = 5
    assert _sub_blocks(3, n_hyp) == _sub_blocks(B, n_hyp) == (1 if n_hyp == FUSED else 4)
    coords, masks = _batch(Ho, Wo)
    if strided:
        pred = torch.zeros((B, 4, Ho, Wo), device="cuda")
        pred[:, :3] = torch.from_numpy(coords).cuda()
        co = pred[:, :3]
        assert not co.is_contiguous()
    else:
        co = torch.from_numpy(coords).cuda()
    m = torch.from_numpy(masks).cuda()
    got = _gpu(co, m, n_hyp, Ho, Wo, image0=20)
    flat = masks.reshape(B, -1)
    for b in range(B):
        want = _ref_image(ref, (Ho, Wo, n_hyp, b), coords[b], masks[b], n_hyp, Ho, Wo, image=20 + b)
        _assert_image(got, b, want, (Ho, Wo, n_hyp, strided, b))
        assert flat[b][got["cells"][b]].all(), b                              # usable cells only, accepted or not
    assert (got["status"] == 0).all()
    # the image with exactly four usable cells once more with two tries per hypothesis (its hypotheses then run out unless one of
    # the first two tries drew the four cells in an order P3P accepts): bitwise again, accepted or exhausted
    few = _gpu(co[4:5], m[4:5], n_hyp, Ho, Wo, image0=24, max_tries=2)
    want = _ref_image(ref, (Ho, Wo, n_hyp, "four cells, two tries"), coords[4], masks[4], n_hyp, Ho, Wo, image=24, max_tries=2)
    _assert_image(few, 0, want, (Ho, Wo, n_hyp, strided, "four cells, two tries"))
    assert (few["tries"] == -2).any() and flat[4][few["cells"][0]].all()


def test_a_grid_of_317_mask_words(ref):
    """48 x 211 = 10128 cells: 317 mask words, the last one partial (16 cells); nine binary-search steps; 16 hypotheses"""
    Ho, Wo, n_hyp = 48, 211, SPLIT
    sc = synth.make_scene(16, Ho=Ho, Wo=Wo)
    mask = _seeded_mask(16, Ho, Wo, 0.1)
    mask[-1, -16:] = [1, 0] * 8                                                # usable cells in the partial word
    got = _gpu(torch.from_numpy(sc["coords"][None]).cuda(), torch.from_numpy(mask[None]).cuda(), n_hyp, Ho, Wo, image0=31)
    _assert_image(got, 0, ref.forward(sc["coords"], mask, n_hyp, *_intr(Ho, Wo), image=31, max_tries=MAX_TRIES), "48x211")
    assert (got["tries"] > 0).all()


def test_fused_form_with_several_hypotheses_per_wave(ref):
    """B = 260 at 8x12 with 12 hypotheses: one workgroup per image, three hypotheses per wavefront"""
    Ho, Wo, n_hyp, B = 8, 12, 12, 260
    assert _sub_blocks(B, n_hyp) == 1
    coords5, masks5 = _batch(Ho, Wo)
    idx = np.arange(B) % 5
    coords, masks = coords5[idx], masks5[idx]
    got = _gpu(torch.from_numpy(coords).cuda(), torch.from_numpy(masks).cuda(), n_hyp, Ho, Wo, image0=5, image_stride=3)
    for b in (0, 1, 2, 133, 259):
        want = ref.forward(coords[b], masks[b], n_hyp, *_intr(Ho, Wo), image=5 + 3 * b, max_tries=MAX_TRIES)
        _assert_image(got, b, want, b)
    assert (got["status"] == 0).all()


@pytest.mark.parametrize("n_hyp", [FUSED, SPLIT])
def test_the_reject_sampler_is_the_call_without_the_keyword(n_hyp):
    Ho, Wo = 24, 36
    coords, masks = _batch(Ho, Wo)
    co, m = torch.from_numpy(coords).cuda(), torch.from_numpy(masks).cuda()
    old = _gpu(co, m, n_hyp, Ho, Wo, sampler=None, image0=20)
    _assert_same(_gpu(co, m, n_hyp, Ho, Wo, sampler="reject", image0=20), old, n_hyp)
    new = _gpu(co, m, n_hyp, Ho, Wo, sampler="compact", image0=20)
    assert new["cells"].tobytes() != old["cells"].tobytes()                    # (the other sampler does run)


@pytest.mark.parametrize("n_hyp", [FUSED, SPLIT])
@pytest.mark.parametrize("Ho,Wo", [(9, 13), (24, 36)])
def test_masked_cell_values_influence_no_output_bit(Ho, Wo, n_hyp):
    """NaN, +Inf, -Inf and 1e30 at the masked-out cells"""
    coords, masks = _batch(Ho, Wo)
    m = torch.from_numpy(masks).cuda()
    want = _gpu(torch.from_numpy(coords).cuda(), m, n_hyp, Ho, Wo, image0=20)
    for poison in (np.nan, np.inf, -np.inf, 1e30):
        co = coords.copy()
        for c in range(3):
            co[:, c][masks == 0] = poison
        _assert_same(_gpu(torch.from_numpy(co).cuda(), m, n_hyp, Ho, Wo, image0=20), want, (Ho, Wo, n_hyp, poison))


@pytest.mark.parametrize("n_hyp", [FUSED, SPLIT])
def test_a_dead_image_between_two_live_ones(ref, n_hyp):
    Ho, Wo = 9, 13
    coords, masks = _batch(Ho, Wo)
    coords, masks = coords[:3], masks[:3].copy()
    masks[1] = 0
    masks[1].reshape(-1)[[5, 40, 116]] = 1                                      # three usable cells
    co, m = torch.from_numpy(coords).cuda(), torch.from_numpy(masks).cuda()
    got = _gpu(co, m, n_hyp, Ho, Wo, image0=20)
    assert got["status"].tolist() == [0, 1, 0]
    assert (got["tries"][1] == 0).all() and (got["scores"][1] == 0).all() and (got["cells"][1] == -1).all()
    assert got["dbg"][1][0] == -1 and np.array_equal(got["pose"][1], np.eye(4, dtype=np.float32))
    _assert_image(got, 1, ref.forward(coords[1], masks[1], n_hyp, *_intr(Ho, Wo), image=21, max_tries=MAX_TRIES), "dead")
    for b in (0, 2):
        single = _gpu(co[b:b + 1], m[b:b + 1], n_hyp, Ho, Wo, image0=20 + b)
        for k in OUT + ("status",):
            assert got[k][b].tobytes() == single[k][0].tobytes(), (b, k)
    none = _gpu(co, torch.zeros_like(m), n_hyp, Ho, Wo, image0=20)             # no usable cell at all
    assert none["status"].tolist() == [1, 1, 1] and (none["tries"] == 0).all()


def test_ten_percent_usable_exhausts_reject_but_not_compact(ref):
    """the input of test_dsac_masked_gpu.test_sparse_mask_with_exhausted_hypotheses: 24x36, 10 % usable, 4096 tries, 3 images"""
    Ho, Wo, n_hyp = 24, 36, SPLIT
    coords, _ = _batch(Ho, Wo)
    coords = coords[:3]
    masks = np.stack([_seeded_mask(40 + b, Ho, Wo, 0.1) for b in range(3)])
    co, m = torch.from_numpy(coords).cuda(), torch.from_numpy(masks).cuda()
    old = _gpu(co, m, n_hyp, Ho, Wo, sampler="reject", image0=20)
    assert (old["tries"] == -MAX_TRIES).any()
    new = _gpu(co, m, n_hyp, Ho, Wo, sampler="compact", image0=20)
    assert (new["tries"] > 0).all() and (new["status"] == 0).all()
    print("tries per hypothesis: reject %s exhausted of %d; compact mean %.1f max %d"
          % (int((old["tries"] < 0).sum()), old["tries"].size, new["tries"].mean(), new["tries"].max()))
    for b in range(3):
        _assert_image(new, b, ref.forward(coords[b], masks[b], n_hyp, *_intr(Ho, Wo), image=20 + b, max_tries=MAX_TRIES), b)


class _PlantNet(torch.nn.Module):
    """Stand-in for the network in the wiring tests: the solver's input is given by the caller (`scene_coords`); the fourth
    channel of the output is the given sigma map."""
    num_task_channel = 3
    OUTPUT_SUBSAMPLE = SUB

    def __init__(self, sigma):
        super().__init__()
        self.sigma = sigma

    def forward(self, images, plan_slot=0):
        B, _, H, W = images.shape
        out = torch.zeros((B, 4, H // SUB, W // SUB), device=images.device)
        out[:, 3] = self.sigma
        return out


def test_localize_batch_and_pipelined_localizer_plumbing():
    import dsacstar
    from crossloc_amd import evaluation
    Ho, Wo, n_hyp, B = 24, 36, SPLIT, 3
    H, W = Ho * SUB, Wo * SUB
    coords, masks = _batch(Ho, Wo)
    co, m = torch.from_numpy(coords[1:4]).cuda(), torch.from_numpy(masks[1:4]).cuda()      # 50 %, the decoy band, 10 %
    images = torch.zeros((B, 3, H, W), device="cuda")
    intr = _intr(Ho, Wo)
    direct = torch.zeros((B, 4, 4), device="cuda")
    status = dsacstar.forward_rgb_masked_batch(co, m, direct, n_hyp, *intr, image0=3, sampler="compact")
    rejected = torch.zeros((B, 4, 4), device="cuda")
    dsacstar.forward_rgb_masked_batch(co, m, rejected, n_hyp, *intr, image0=3)
    assert not torch.equal(direct, rejected)
    sigma = torch.from_numpy(np.random.default_rng(9).uniform(0.1, 2.0, size=(B, Ho, Wo)).astype(np.float32)).cuda()
    net = _PlantNet(sigma)
    loc = evaluation.PipelinedLocalizer(net, n_hyp, synth.FOCAL, H, W)
    args = (n_hyp, synth.FOCAL, H, W)
    kw = dict(image0=3, scene_coords=co, mask=m, mask_sampler="compact")

    out = evaluation.localize_batch(net, images, *args, **kw)
    p_out = loc.submit(images, **kw)
    loc.finish()
    for got in (out, p_out):
        assert len(got) == 3 and torch.equal(got[0], direct) and torch.equal(got[2], status)
    assert torch.equal(evaluation.localize_batch(net, images, *args, image0=3, scene_coords=co, mask=m, mask_sampler="reject")[0],
                       rejected)

    # the masked passes behind the compact solver: the direct calls on the pose it wrote
    for refine in ("masked_inliers", "masked_sigma"):
        want_poses, want_rows = dsacstar.refine_pose_masked_batch(co, m, sigma if refine == "masked_sigma" else None, direct,
                                                                  intr[0], *intr[1:4], intr[5], SUB)
        want_q = dsacstar.pose_quality_masked_batch(co, m, want_poses, *intr)
        out = evaluation.localize_batch(net, images, *args, refine=refine, quality="masked", **kw)
        p_out = loc.submit(images, refine=refine, quality="masked", **kw)
        loc.finish()
        torch.cuda.synchronize()
        for got in (out, p_out):
            assert len(got) == 5
            assert torch.equal(got[0], want_poses) and torch.equal(got[2], want_q) and torch.equal(got[3], want_rows), refine
            assert torch.equal(got[4], status)

    for call in (lambda **k: evaluation.localize_batch(net, images, *args, scene_coords=co, **k),
                 lambda **k: loc.submit(images, scene_coords=co, **k)):
        with pytest.raises(RuntimeError, match="needs mask"):
            call(mask_sampler="compact")
        with pytest.raises(RuntimeError, match="mask_sampler"):
            call(mask=m, mask_sampler="weighted")
    loc.finish()
    torch.cuda.synchronize()
