"""The RGB-D restatements against their own past (CPU).  tests/golden/rgbd_ref_pin.npz holds the bits tests/dsac_rgbd_ref.c,
tests/dsac_rgbd_bwd_ref.c and tests/rgbd_quality_ref.c produced before the family's block sum, pose helpers, input record
and refinement model were each written once.  Kernels and restatements compile the same xl_dsac_rgbd*_math.h and
xl_dsac_reduce.h, so a reordering there moves both at once and the GPU == restatement tests cannot see it.  This test can:
every recorded value must come out bit for bit (the arithmetic is + - * / sqrt floor without contraction; no recorded value
depends on the gcc optimisation level, so none is left out).  Recorder and inputs: tests/golden/make_rgbd_ref_pin.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_rgbd_ref_pin as pin                                    # noqa: E402

RUNS = [(g, f) for g in pin.GRIDS for f in pin.FORMS]


@pytest.fixture(scope="module")
def recorded():
    with np.load(pin.PATH) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def computed(tmp_path_factory):
    return pin.compute(tmp_path_factory.mktemp("rgbd_ref_pin"))


def _assert_same_bits(name, want, got):
    got = np.asarray(got)
    assert want.shape == got.shape and want.dtype == got.dtype, name
    if want.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(nan, np.isnan(got)), name + ": NaNs moved"
        ints = {4: np.int32, 8: np.int64}[want.dtype.itemsize]
        want, got = np.where(nan, 0, want).view(ints), np.where(nan, 0, got).view(ints)
    assert np.array_equal(want, got), name + ": bits differ from the recorded restatement"


def test_fixture_is_complete(recorded, computed):
    assert set(recorded) == set(computed)
    want = {"%s_%s_%s_%s" % (g, f, p, k) for g, f in RUNS for p, ks in (("f", pin.FORWARD), ("b", pin.BACKWARD), ("q", pin.QUALITY))
            for k in ks}
    assert want | {"status_q_row"} | {g + s for g in pin.GRIDS for s in ("_in_coords", "_in_depth")} == set(recorded)


def test_scene_inputs_are_the_recorded_ones(recorded, computed):
    """The scenes come from dsac_rgbd_cases.rgbd_scene; if these move, the generator changed, not the restatements."""
    for g in pin.GRIDS:
        for s in ("_in_coords", "_in_depth"):
            _assert_same_bits(g + s, recorded[g + s], computed[g + s])


def test_recorded_runs_cover_the_paths(recorded):
    """What the grids were chosen for is in the record: accepted hypotheses, fitted refinement rounds, active hypotheses with
    both gradient paths open, and holes in the larger grid."""
    for g, f in RUNS:
        tag = "%s_%s_" % (g, f)
        assert (recorded[tag + "f_tries"] > 0).all() and recorded[tag + "f_dbg"][2] >= 1
        assert len(recorded[tag + "f_round_poses"]) == recorded[tag + "f_dbg"][2]
        rec = recorded[tag + "b_rec"]
        assert ((rec[:, 2] > 0) & (rec[:, 4] == 0) & (rec[:, 43] == 0)).any() and recorded[tag + "b_grad"].any()
        assert recorded[tag + "q_row"][6] == 0
    assert recorded["17x23_cam_f_dbg"][1] < 17 * 23 and (recorded["17x23_in_depth"] == 0).any()


@pytest.mark.parametrize("grid,form", RUNS)
@pytest.mark.parametrize("what", pin.FORWARD)
def test_forward(recorded, computed, grid, form, what):
    """16 hypotheses: pose, sampled cells, try counts, fp64 scores, the debug record, every hypothesis' pose, and the inlier
    count and pose of every refinement round."""
    k = "%s_%s_f_%s" % (grid, form, what)
    _assert_same_bits(k, recorded[k], computed[k])


@pytest.mark.parametrize("grid,form", RUNS)
@pytest.mark.parametrize("what", pin.BACKWARD)
def test_backward(recorded, computed, grid, form, what):
    """The same scenes against the moved ground truth: expected loss, all 64 columns of every record, the whole gradient."""
    k = "%s_%s_b_%s" % (grid, form, what)
    _assert_same_bits(k, recorded[k], computed[k])


@pytest.mark.parametrize("grid,form", RUNS)
@pytest.mark.parametrize("what", pin.QUALITY)
def test_quality(recorded, computed, grid, form, what):
    """The row and the reduced sums at the forward restatement's refined pose."""
    k = "%s_%s_q_%s" % (grid, form, what)
    _assert_same_bits(k, recorded[k], computed[k])


def test_quality_status_case(recorded, computed):
    _assert_same_bits("status_q_row", recorded["status_q_row"], computed["status_q_row"])
