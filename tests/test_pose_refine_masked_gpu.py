"""GPU checks of the masked pose refinement (dsacstar.refine_pose_masked_batch): the 16 floats of every pose, all 64 doubles of
every row and the 12 doubles of w2c bitwise against the serial restatement tests/pose_refine_masked_ref.c, the all-ones identity
against refine_pose_batch, poison at masked-out cells (coordinates and sigma), the substitution identity against the UNMASKED
pass, dead and sparse images, the largest grid (bit 39 of the per-thread word) and the front end's refusals."""
import numpy as np
import pytest
import torch

import pose_masked_cases as mc
import pose_refine_masked_ref
import pose_refine_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_refine_masked_ref")
    return dict(r=pose_refine_ref.load(d), rm=pose_refine_masked_ref.load(d))


def _dev(a):
    return a if isinstance(a, torch.Tensor) or a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _call(fn, tensors, args, **kw):
    B = len(tensors[-1])
    w2c = torch.full((B, 12), -7.0, dtype=torch.float64, device="cuda")
    out, rows = fn(*[_dev(t) for t in tensors], *args, w2c=w2c, **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 4, 4) and tuple(rows.shape) == (B, 64)
    return out.cpu().numpy(), rows.cpu().numpy(), w2c.cpu().numpy()


def _masked(coords, mask, sigma, poses, args, **kw):
    import dsacstar
    return _call(dsacstar.refine_pose_masked_batch, (coords, mask, sigma, poses), args, **kw)


def _plain(coords, sigma, poses, args, **kw):
    import dsacstar
    return _call(dsacstar.refine_pose_batch, (coords, sigma, poses), args, **kw)


def _frame(got, b):
    return got[0][b], got[1][b], got[2][b]


def _same_batch(a, b):
    return all(mc.same_refine(_frame(a, i), _frame(b, i)) for i in range(len(a[0])))


_BATCHES = {}


def _batch(Ho, Wo):
    if (Ho, Wo) not in _BATCHES:
        _BATCHES[(Ho, Wo)] = mc.batch(40, Ho, Wo)
    return _BATCHES[(Ho, Wo)]


def _pred(bt):
    """A network output [B,4,Ho,Wo] holding the batch: the strided views pred[:, :3] and pred[:, 3]"""
    B, _, Ho, Wo = bt["coords"].shape
    pred = torch.randn((B, 4, Ho, Wo), device="cuda")
    pred[:, :3] = _dev(bt["coords"])
    pred[:, 3] = _dev(bt["sigma"])
    assert not pred[:, :3].is_contiguous() and not pred[:, 3].is_contiguous()
    return pred


@pytest.mark.parametrize("Ho,Wo", mc.GRIDS)
def test_bit_exact_against_the_restatement(refs, Ho, Wo):
    bt = _batch(Ho, Wo)
    pred = _pred(bt)
    for coords, sigma, s_np in ((bt["coords"], bt["sigma"], bt["sigma"]), (pred[:, :3], pred[:, 3], bt["sigma"]),
                                (bt["coords"], None, None)):
        got = _masked(coords, bt["mask"], sigma, bt["poses"], bt["rargs"])
        for b in range(3):
            want = refs["rm"].refine(bt["coords"][b], bt["mask"][b], None if s_np is None else s_np[b], bt["poses"][b], *bt["rargs"])
            assert mc.same_refine(_frame(got, b), want[:3]), (b, np.flatnonzero(got[1][b] != want[1]))
            assert got[1][b][63] == float((bt["mask"][b] == 0).sum()) and got[1][b][0] == Ho * Wo
        assert (got[1][:2, 6] == 0.0).all() and (got[1][:2, 58] >= 1.0).all()      # the hetero frames complete a round
    assert _same_batch(_masked(bt["coords"], _dev(bt["mask"]).bool(), None, bt["poses"], bt["rargs"]), got)


def test_bit_exact_at_the_largest_grid(refs):
    """One image of 48 x 211 = REFINE_MAX_CELLS cells: threads 0..143 own 40 cells, the per-thread word uses bit 39"""
    import dsacstar
    Ho, Wo = mc.MAX_GRID
    assert Ho * Wo == dsacstar.REFINE_MAX_CELLS and (Ho * Wo - 1) // 256 == 39
    fr = mc.hetero_frame(3, Ho, Wo)
    last = fr["mask"].reshape(-1)[39 * 256:]                                  # the cells of bit 39, in both states
    last[:] = np.arange(last.size) % 2
    args = mc.refine_args(fr)
    got = _masked(fr["coords"][None], fr["mask"][None], fr["sigma"][None], fr["start"][None], args)
    want = refs["rm"].refine(fr["coords"], fr["mask"], fr["sigma"], fr["start"], *args)
    assert mc.same_refine(_frame(got, 0), want[:3]) and want[1][6] == 0.0
    co, sg = mc.poisoned(fr["coords"], fr["sigma"], fr["mask"], np.nan)
    assert _same_batch(_masked(co[None], fr["mask"][None], sg[None], fr["start"][None], args), got)
    ones = np.ones_like(fr["mask"])[None]
    assert _same_batch(_masked(fr["coords"][None], ones, fr["sigma"][None], fr["start"][None], args),
                       _plain(fr["coords"][None], fr["sigma"][None], fr["start"][None], args))


@pytest.mark.parametrize("Ho,Wo", mc.GRIDS)
def test_all_ones_mask_is_the_unmasked_pass(Ho, Wo):
    bt = _batch(Ho, Wo)
    ones = np.ones_like(bt["mask"])
    for sigma in (bt["sigma"], None):
        assert _same_batch(_masked(bt["coords"], ones, sigma, bt["poses"], bt["rargs"]),
                           _plain(bt["coords"], sigma, bt["poses"], bt["rargs"]))


@pytest.mark.parametrize("Ho,Wo", mc.GRIDS)
def test_poison_at_masked_out_cells_changes_no_bit(Ho, Wo):
    bt = _batch(Ho, Wo)
    base = _masked(bt["coords"], bt["mask"], bt["sigma"], bt["poses"], bt["rargs"])
    for v in mc.POISON:
        co, sg = mc.poisoned(bt["coords"], bt["sigma"], bt["mask"], v)
        assert _same_batch(_masked(co, bt["mask"], sg, bt["poses"], bt["rargs"]), base), v
    assert (base[1][:, 5] == 0.0).all()                                      # n_bad_sigma counts usable cells only
    _, sg = mc.poisoned(bt["coords"], bt["sigma"], bt["mask"], np.nan)
    assert (_plain(bt["coords"], sg, bt["poses"], bt["rargs"])[1][1:, 5] > 0.0).all()   # the unmasked pass counts them


def test_substitution_identity(refs):
    """Masked pass on the original data == UNMASKED pass on data whose masked-out cells hold a point 10 km away, 45 degrees off
    axis (finite sigma there), in pose, w2c and every row column but [63].  The premise is asserted before the comparison: equal
    inlier counts, status 0, and no substituted cell in the restatement's final inlier set.  Seeds 1 and 4 run two rounds at
    24 x 36."""
    two_rounds = 0
    for Ho, Wo in mc.GRIDS:
        frames = [mc.hetero_frame(seed, Ho, Wo) for seed in (1, 4, 5)]
        coords, sigma = np.stack([f["coords"] for f in frames]), np.stack([f["sigma"] for f in frames])
        subst = [mc.substituted(f) for f in frames]
        sco, ssg = np.stack([s[0] for s in subst]), np.stack([s[1] for s in subst])
        mask, poses = np.stack([f["mask"] for f in frames]), np.stack([f["start"] for f in frames])
        args = mc.refine_args(frames[0])
        want = _plain(sco, ssg, poses, args)
        got = _masked(coords, mask, sigma, poses, args)
        for b, f in enumerate(frames):
            r = refs["r"].refine(sco[b], ssg[b], poses[b], *args)
            assert mc.same_refine(_frame(want, b), r[:3])
            assert r[1][6] == 0.0 and not r[3][f["mask"] == 0].any(), (Ho, Wo, b)                       # the premise
            assert got[1][b][1] == want[1][b][1] and got[1][b][2] == want[1][b][2] and got[1][b][1] >= 4.0
            assert mc.same_refine(_frame(got, b), _frame(want, b), skip=(63,)), (Ho, Wo, b)
            assert got[1][b][63] == float((f["mask"] == 0).sum()) and want[1][b][63] == 0.0
            two_rounds += got[1][b][58] >= 2.0
    assert two_rounds >= 1


def test_dead_and_sparse_images():
    """Images 1 and 3 of five have three usable cells and none: status 1 and the input pose bit for bit; the live images around
    them equal their single-image runs."""
    Ho, Wo = 9, 13
    bt = _batch(Ho, Wo)
    N = Ho * Wo
    order = [0, 1, 1, 2, 2]
    coords, sigma = bt["coords"][order], bt["sigma"][order]
    mask, poses = bt["mask"][order].copy(), bt["poses"][order].copy()
    sparse = np.zeros(N, np.uint8)
    sparse[[5, 60, 116]] = 1
    mask[1], mask[3] = sparse.reshape(Ho, Wo), 0
    poses[3] = np.eye(4, dtype=np.float32)                                    # what the masked solver writes for a dead image
    got = _masked(coords, mask, sigma, poses, bt["rargs"])
    for b, usable in ((1, 3), (3, 0)):
        row = got[1][b]
        assert row[6] == 1.0 and row[63] == N - usable and row[1] <= usable and row[58] == 0.0 and row[0] == N
        assert mc.same_pose_bits(got[0][b], poses[b])
    for b in (0, 2, 4):
        alone = _masked(coords[b:b + 1], mask[b:b + 1], sigma[b:b + 1], poses[b:b + 1], bt["rargs"])
        assert mc.same_refine(_frame(got, b), _frame(alone, 0)), b
    bad = poses.copy()
    bad[2, 0, 3] = np.nan
    row = _masked(coords, mask, sigma, bad, bt["rargs"])[1][2]
    assert row[6] == 3.0 and row[0] == N and np.isnan(np.delete(row, [0, 6])).all()                    # [63] NaN like its neighbours


def test_front_end_refusals():
    import dsacstar
    Ho, Wo = 8, 12
    bt = _batch(Ho, Wo)
    co, sg, ok, poses = _dev(bt["coords"]), _dev(bt["sigma"]), _dev(bt["mask"]), _dev(bt["poses"])
    bad = [ok[:1], ok.to(torch.float32), ok.to(torch.int32), ok.cpu(), torch.ones((3, Wo, Ho), dtype=torch.uint8, device="cuda"),
           torch.ones((3, Ho, 2 * Wo), dtype=torch.uint8, device="cuda")[:, :, ::2], None]
    for m in bad:
        with pytest.raises(RuntimeError):
            dsacstar.refine_pose_masked_batch(co, m, sg, poses, *bt["rargs"])
    with pytest.raises(RuntimeError):
        dsacstar.refine_pose_masked_batch(co, ok, sg, poses.cpu(), *bt["rargs"])
    assert dsacstar.REFINE_FIELDS["n_masked"] == 63 and "reserved" not in dsacstar.REFINE_FIELDS
    from crossloc_amd import _lib
    out, rows = torch.zeros_like(poses), torch.zeros((3, 64), dtype=torch.float64, device="cuda")
    a = bt["rargs"]
    null = _lib.lib().xl_dsac_refine_pose_masked_batch(co.data_ptr(), *co.stride(), sg.data_ptr(), *sg.stride(), 3, Ho, Wo, None,
                                                       poses.data_ptr(), out.data_ptr(), rows.data_ptr(), None,
                                                       *[float(v) for v in a[:5]], int(a[5]), None, 1.0, 8, None)
    assert null == -1                                                                                   # XL_ERR_ARG, nothing launched
