"""GPU checks of the masked pose-quality pass (dsacstar.pose_quality_masked_batch): all 64 doubles of every row bitwise against
the serial restatement tests/pose_quality_masked_ref.c, the all-ones identity against pose_quality_batch, poison at masked-out
cells, the substitution identity against the UNMASKED pass, dead and sparse images and the front end's refusals."""
import numpy as np
import pytest
import torch

import pose_masked_cases as mc
import pose_quality_masked_ref
import pose_quality_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_quality_masked_ref")
    return dict(q=pose_quality_ref.load(d), qm=pose_quality_masked_ref.load(d))


def _dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _masked(coords, mask, poses, args):
    import dsacstar
    rows = dsacstar.pose_quality_masked_batch(_dev(coords), _dev(mask), _dev(poses), *args)
    torch.cuda.synchronize()
    assert rows.dtype == torch.float64 and tuple(rows.shape) == (len(poses), 64)
    return rows.cpu().numpy()


def _plain(coords, poses, args):
    import dsacstar
    rows = dsacstar.pose_quality_batch(_dev(coords), _dev(poses), *args)
    torch.cuda.synchronize()
    return rows.cpu().numpy()


_BATCHES = {}


def _batch(Ho, Wo):
    if (Ho, Wo) not in _BATCHES:
        _BATCHES[(Ho, Wo)] = mc.batch(40, Ho, Wo)
    return _BATCHES[(Ho, Wo)]


def _strided(bt):
    """The network output's channel view pred[:, :3] holding the batch's coordinates"""
    B, _, Ho, Wo = bt["coords"].shape
    pred = torch.randn((B, 4, Ho, Wo), device="cuda")
    pred[:, :3] = _dev(bt["coords"])
    assert not pred[:, :3].is_contiguous()
    return pred[:, :3]


@pytest.mark.parametrize("Ho,Wo", mc.GRIDS)
def test_bit_exact_against_the_restatement(refs, Ho, Wo):
    bt = _batch(Ho, Wo)
    for coords in (bt["coords"], _strided(bt)):
        got = _masked(coords, bt["mask"], bt["poses"], bt["qargs"])
        for b in range(3):
            want = refs["qm"].row(bt["coords"][b], bt["mask"][b], bt["poses"][b], *bt["qargs"])
            assert mc.same_row(got[b], want), (b, np.flatnonzero(got[b] != want))
            assert got[b][58] == float((bt["mask"][b] == 0).sum()) and got[b][0] == Ho * Wo
    bool_mask = _dev(bt["mask"]).bool()
    assert mc.same_bits(_masked(bt["coords"], bool_mask, bt["poses"], bt["qargs"]), got)
    assert got[0][6] == 0.0 and got[1][6] == 0.0                       # the hetero frames are rated, not refused


@pytest.mark.parametrize("Ho,Wo", mc.GRIDS)
def test_all_ones_mask_is_the_unmasked_pass(Ho, Wo):
    bt = _batch(Ho, Wo)
    ones = np.ones_like(bt["mask"])
    assert mc.same_bits(_masked(bt["coords"], ones, bt["poses"], bt["qargs"]), _plain(bt["coords"], bt["poses"], bt["qargs"]))


@pytest.mark.parametrize("Ho,Wo", mc.GRIDS)
def test_poison_at_masked_out_cells_changes_no_bit(Ho, Wo):
    bt = _batch(Ho, Wo)
    base = _masked(bt["coords"], bt["mask"], bt["poses"], bt["qargs"])
    for v in mc.POISON:
        co, _ = mc.poisoned(bt["coords"], bt["sigma"], bt["mask"], v)
        assert mc.same_bits(_masked(co, bt["mask"], bt["poses"], bt["qargs"]), base), v
    co, _ = mc.poisoned(bt["coords"], bt["sigma"], bt["mask"], np.nan)
    assert np.isnan(_plain(co, bt["poses"], bt["qargs"])[1:, 2]).all()   # what the unmasked pass makes of the same data


def test_substitution_identity(refs):
    """Masked pass on the original data == UNMASKED pass on data whose masked-out cells hold a point 10 km away, 45 degrees off
    axis, in every column but [2] and [58].  The premise (equal inlier counts, status 0) is asserted before the comparison."""
    for Ho, Wo in mc.GRIDS:
        frames = [mc.hetero_frame(seed, Ho, Wo) for seed in (1, 4, 5)]
        coords = np.stack([f["coords"] for f in frames])
        subst = np.stack([mc.substituted(f)[0] for f in frames])
        mask, poses = np.stack([f["mask"] for f in frames]), np.stack([f["start"] for f in frames])
        args = mc.quality_args(frames[0])
        want = _plain(subst, poses, args)
        got = _masked(coords, mask, poses, args)
        for b, f in enumerate(frames):
            assert mc.same_row(want[b], refs["q"].row(subst[b], poses[b], *args))
            assert want[b][6] == 0.0 and got[b][1] == want[b][1] and got[b][1] >= 4.0, (Ho, Wo, b)    # the premise
            assert mc.same_row(got[b], want[b], skip=(2, 58)), (Ho, Wo, b)
            assert got[b][58] == float((f["mask"] == 0).sum()) and want[b][58] == 0.0


def test_dead_and_sparse_images():
    """Images 1 and 3 of five have three usable cells and none, at the identity pose the masked solver writes for them; the live
    images around them equal their single-image runs."""
    Ho, Wo = 9, 13
    bt = _batch(Ho, Wo)
    N = Ho * Wo
    order = [0, 1, 1, 2, 2]
    coords, mask, poses = bt["coords"][order], bt["mask"][order].copy(), bt["poses"][order].copy()
    sparse = np.zeros(N, np.uint8)
    sparse[[5, 60, 116]] = 1
    mask[1], mask[3] = sparse.reshape(Ho, Wo), 0
    poses[1] = poses[3] = np.eye(4, dtype=np.float32)
    got = _masked(coords, mask, poses, bt["qargs"])
    for b, usable in ((1, 3), (3, 0)):
        assert got[b][6] == 1.0 and got[b][1] == 0.0 and got[b][58] == N - usable and got[b][0] == N
        assert np.isnan(got[b][7:10]).all() and np.isnan(got[b][31:58]).all() and (got[b][59:] == 0.0).all()
    for b in (0, 2, 4):
        alone = _masked(coords[b:b + 1], mask[b:b + 1], poses[b:b + 1], bt["qargs"])
        assert mc.same_row(got[b], alone[0]), b
    bad = poses.copy()
    bad[2, 0, 3] = np.nan
    row = _masked(coords, mask, bad, bt["qargs"])[2]
    assert row[6] == 3.0 and row[0] == N and np.isnan(np.delete(row, [0, 6])).all()                # [58] NaN like its neighbours


def test_front_end_refusals():
    import dsacstar
    Ho, Wo = 8, 12
    bt = _batch(Ho, Wo)
    co, ok, poses = _dev(bt["coords"]), _dev(bt["mask"]), _dev(bt["poses"])
    bad = [ok[:1], ok.to(torch.float32), ok.to(torch.int32), ok.cpu(), torch.ones((3, Wo, Ho), dtype=torch.uint8, device="cuda"),
           torch.ones((3, Ho, 2 * Wo), dtype=torch.uint8, device="cuda")[:, :, ::2], None]
    for m in bad:
        with pytest.raises(RuntimeError):
            dsacstar.pose_quality_masked_batch(co, m, poses, *bt["qargs"])
    with pytest.raises(RuntimeError):
        dsacstar.pose_quality_masked_batch(co, ok, poses.cpu(), *bt["qargs"])
    assert dsacstar.QUALITY_FIELDS["n_masked"] == 58 and dsacstar.QUALITY_FIELDS["reserved"] == slice(59, 64)
    from crossloc_amd import _lib
    null = _lib.lib().xl_dsac_pose_quality_masked_batch(co.data_ptr(), *co.stride(), 3, Ho, Wo, None, poses.data_ptr(),
                                                        *[float(a) for a in bt["qargs"][:6]], 8, None, poses.data_ptr(), None)
    assert null == -1                                                                               # XL_ERR_ARG, nothing launched
