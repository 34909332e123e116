"""The masked pose-quality and pose-refinement passes on the CPU: the serial restatements tests/pose_quality_masked_ref.c and
tests/pose_refine_masked_ref.c (the orchestrations of the masked kernels over the product's shared headers) against the
unmasked restatements the GPU suites already hold the unmasked kernels to.

  * all-ones mask: the masked restatement is the unmasked one bit for bit (rows, poses, w2c, the final inlier set);
  * substitution identity: the masked pass on the original data is the unmasked pass on data whose masked-out cells hold a
    point no pose near the truth can admit (10 km away, 45 degrees off axis) - an independent check of "a masked-out cell is
    never an inlier and adds to no sum" that needs no code beyond the unmasked restatement;
  * the values stored at masked-out cells reach no output bit; dead and sparse images."""
import numpy as np
import pytest

import pose_masked_cases as mc
import pose_quality_masked_ref
import pose_quality_ref
import pose_refine_masked_ref
import pose_refine_ref


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_masked_ref")
    return dict(q=pose_quality_ref.load(d), qm=pose_quality_masked_ref.load(d), r=pose_refine_ref.load(d),
                rm=pose_refine_masked_ref.load(d))


FRAMES = [(seed, Ho, Wo) for Ho, Wo in mc.GRIDS for seed in mc.SUBST_SEEDS]


@pytest.fixture(scope="module")
def frames():
    return {key: mc.hetero_frame(*key) for key in FRAMES}


def test_all_ones_mask_is_the_unmasked_restatement(refs, frames):
    for (seed, Ho, Wo), fr in frames.items():
        if seed > 1:
            continue
        ones = np.ones((Ho, Wo), np.uint8)
        q = refs["q"].row(fr["coords"], fr["start"], *mc.quality_args(fr))
        qm = refs["qm"].row(fr["coords"], ones, fr["start"], *mc.quality_args(fr))
        assert mc.same_row(qm, q) and qm[58] == 0.0, (seed, Ho, Wo)
        for sigma in (fr["sigma"], None):
            r = refs["r"].refine(fr["coords"], sigma, fr["start"], *mc.refine_args(fr))
            rm = refs["rm"].refine(fr["coords"], ones, sigma, fr["start"], *mc.refine_args(fr))
            assert mc.same_refine(rm, r) and np.array_equal(rm[3], r[3]) and rm[1][63] == 0.0, (seed, Ho, Wo)
            assert r[1][6] == 0.0


def test_substitution_identity_refinement(refs, frames):
    """The masked pass on the original data == the unmasked pass on the substituted data, in pose, w2c and every row column but
    [63].  The premise is asserted first: status 0, at least 4 inliers, and no substituted cell in the unmasked pass's final
    inlier set, on every frame; at least one frame runs two rounds."""
    two_rounds = 0
    for (seed, Ho, Wo), fr in frames.items():
        co, sg = mc.substituted(fr)
        want = refs["r"].refine(co, sg, fr["start"], *mc.refine_args(fr))
        assert want[1][6] == 0.0 and want[1][1] >= 4.0, (seed, Ho, Wo, want[1][:7])
        assert not want[3][fr["mask"] == 0].any(), (seed, Ho, Wo)                                  # the premise
        got = refs["rm"].refine(fr["coords"], fr["mask"], fr["sigma"], fr["start"], *mc.refine_args(fr))
        assert got[1][1] == want[1][1] and got[1][2] == want[1][2], (seed, Ho, Wo)                 # n_inliers, both ends
        assert mc.same_refine(got, want, skip=(63,)) and np.array_equal(got[3], want[3]), (seed, Ho, Wo)
        assert got[1][63] == float((fr["mask"] == 0).sum()) and want[1][63] == 0.0
        two_rounds += got[1][58] >= 2.0
    assert two_rounds >= 1


def test_substitution_identity_quality(refs, frames):
    """The same for the quality row, in every column but [2] (the substituted cells still add their clamped soft term) and [58]"""
    for (seed, Ho, Wo), fr in frames.items():
        co, _ = mc.substituted(fr)
        want = refs["q"].row(co, fr["start"], *mc.quality_args(fr))
        got = refs["qm"].row(fr["coords"], fr["mask"], fr["start"], *mc.quality_args(fr))
        assert want[6] == 0.0 and got[1] == want[1] and got[1] >= 4.0, (seed, Ho, Wo)              # the premise
        assert mc.same_row(got, want, skip=(2, 58)), (seed, Ho, Wo)
        assert got[58] == float((fr["mask"] == 0).sum()) and got[0] == Ho * Wo
        assert 0.0 < got[2] <= want[2]                          # usable cells only; a far cell's soft term is ~e^-45


def test_masked_out_values_reach_no_bit(refs, frames):
    fr = frames[(1, 9, 13)]
    q0 = refs["qm"].row(fr["coords"], fr["mask"], fr["start"], *mc.quality_args(fr))
    r0 = refs["rm"].refine(fr["coords"], fr["mask"], fr["sigma"], fr["start"], *mc.refine_args(fr))
    for v in mc.POISON:
        co, sg = mc.poisoned(fr["coords"], fr["sigma"], fr["mask"], v)
        assert mc.same_row(refs["qm"].row(co, fr["mask"], fr["start"], *mc.quality_args(fr)), q0), v
        r = refs["rm"].refine(co, fr["mask"], sg, fr["start"], *mc.refine_args(fr))
        assert mc.same_refine(r, r0) and np.array_equal(r[3], r0[3]), v


def test_dead_and_sparse_images(refs, frames):
    fr = frames[(0, 8, 12)]
    N = 8 * 12
    for usable in (3, 0):
        mask = np.zeros(N, np.uint8)
        mask[np.random.default_rng(5).choice(N, usable, replace=False)] = 1
        mask = mask.reshape(8, 12)
        q = refs["qm"].row(fr["coords"], mask, fr["start"], *mc.quality_args(fr))
        assert q[6] == 1.0 and q[1] <= usable and q[58] == N - usable and q[0] == N
        pose, row, w2c, inl = refs["rm"].refine(fr["coords"], mask, fr["sigma"], fr["start"], *mc.refine_args(fr))
        assert row[6] == 1.0 and row[63] == N - usable and row[5] == 0.0 and not inl.any()
        assert mc.same_pose_bits(pose, fr["start"])


def test_bad_pose_leaves_n_masked_nan(refs, frames):
    fr = frames[(0, 8, 12)]
    bad = fr["start"].copy()
    bad[1, 2] = np.inf
    q = refs["qm"].row(fr["coords"], fr["mask"], bad, *mc.quality_args(fr))
    r = refs["rm"].refine(fr["coords"], fr["mask"], fr["sigma"], bad, *mc.refine_args(fr))
    for row in (q, r[1]):
        assert row[6] == 3.0 and row[0] == 96 and np.isnan(np.delete(row, [0, 6])).all()
