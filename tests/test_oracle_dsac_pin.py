"""The oracle against its own past (CPU).  tests/golden/dsac_oracle_pin.npz holds the bits oracle/libxl_oracle.so produced
when it still carried its own copy of every solver formula; since then the kernels and the oracle compile the same
crossloc_amd/csrc/xl_dsac_math.h, so a reordering in that header moves both at once and the GPU==oracle tests cannot see it.
This test can: every recorded value must come out bit for bit (the arithmetic is + - * / sqrt floor without contraction, so the
bits do not depend on the compiler).  Recorder and inputs: tests/golden/make_dsac_oracle_pin.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_dsac_oracle_pin as pin                                 # noqa: E402

UNIT = ["exp", "sincos", "atan2", "quartic", "draws", "p3p", "dpnp", "log_so3", "rodrigues_jac", "pinv6", "resid_row",
        "dproject_dobj", "pose_loss", "dloss", "score"]
FORWARD = ["pose", "cells", "tries", "scores", "counts", "pose01"]       # counts: winner, rounds, inliers, LM evaluations
BACKWARD = ["loss", "grad_sha", "grad_sample"]


@pytest.fixture(scope="module")
def recorded():
    with np.load(pin.PATH) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def units(recorded):
    return pin.unit_results({k: v for k, v in recorded.items() if k.startswith("in_")})


@pytest.fixture(scope="module")
def scenes():
    return pin.scene_results()


def _assert_same_bits(name, want, got):
    got = np.asarray(got)
    assert want.shape == got.shape and want.dtype == got.dtype, name
    if want.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(nan, np.isnan(got)), name + ": NaNs moved"
        ints = {4: np.int32, 8: np.int64}[want.dtype.itemsize]
        want, got = np.where(nan, 0, want).view(ints), np.where(nan, 0, got).view(ints)
    assert np.array_equal(want, got), name + ": bits differ from the recorded oracle"


def test_fixture_is_complete(recorded, units, scenes):
    assert set(UNIT) <= set(units) and set(recorded) == {k for k in recorded if k.startswith("in_")} | set(units) | set(scenes)


@pytest.mark.parametrize("name", UNIT)
def test_unit_entry_points(recorded, units, name):
    _assert_same_bits(name, recorded[name], units[name])


def test_quartic_and_p3p_cases_cover_the_branches(recorded):
    """What the unit inputs were chosen for is in them: quartics with 0, 2 and 4 real roots and non-finite ones, P3P
    problems that are solved and ones that are not."""
    n = recorded["quartic"][:, 0]
    assert {0.0, 2.0, 4.0} <= set(n.tolist()) and not np.isfinite(recorded["in_quartic"]).all()
    assert 0 < recorded["p3p"][:, 0].sum() < len(recorded["p3p"])


def test_scene_inputs_are_the_recorded_ones(recorded, scenes):
    """The frames come from synth.make_scene; if these digests move, the generator changed, not the solver."""
    for k in ("frames_in_sha", "ragged_in_sha"):
        assert np.array_equal(recorded[k], scenes[k]), k


@pytest.mark.parametrize("what", FORWARD)
def test_forward_frames(recorded, scenes, what):
    """16 frames at 60x90, 64 hypotheses: pose, sampled cells, try counts, fp64 scores, winner and refinement counts."""
    want, got = recorded["frames_f_" + what], scenes["frames_f_" + what]
    assert len(want) == pin.FRAMES
    _assert_same_bits(what, want, got)


@pytest.mark.parametrize("what", BACKWARD)
def test_backward_frames(recorded, scenes, what):
    """The same frames, 16 hypotheses: expected loss, digest of the gradient bytes and a strided sample of it."""
    _assert_same_bits(what, recorded["frames_b_" + what], scenes["frames_b_" + what])


@pytest.mark.parametrize("scene", ["nodata", "ragged"])
def test_degenerate_scenes(recorded, scenes, scene):
    """An all-nodata 60x90 scene (no try is ever accepted) and a ragged 7x5 one (fewer cells than threads)."""
    for what in FORWARD:
        _assert_same_bits(what, recorded["%s_f_%s" % (scene, what)], scenes["%s_f_%s" % (scene, what)])
    for what in BACKWARD:
        _assert_same_bits(what, recorded["%s_b_%s" % (scene, what)], scenes["%s_b_%s" % (scene, what)])
    if scene == "nodata":
        assert (recorded["nodata_f_tries"] == -100).all()
