"""CPU: the branch scenes of loss_branch_cases.py and everything the GPU test (test_loss_branches_gpu.py) relies on -
the census (every branch populated, every deciding quantity off its threshold), the oracle against the reference fixture
in float64 and fp32, the yardstick table, and the comparator's power to reject what it is there to reject."""
import numpy as np
import pytest
import torch

import loss_branch_cases as bc
import loss_branch_oracle as bo

F = bo.FIXTURE
REG = ("coord", "depth", "normal")
CASES = [pytest.param(l, s, m, c, id="%s-%s-%s" % (l, bc.tag(s), bc.run_tag(l, m, c))) for l in REG for s in bc.SHAPES
         for m, c in bc.runs(l)]


@pytest.fixture(autouse=True)
def _one_thread():
    """fp32 sums in a fixed order on every host (test_loss_oracle.py)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _fx(loss, shape, mode, clamp, dt, what):
    return bc.stored(F, loss, shape, mode, clamp, dt, what)


@pytest.mark.parametrize("shape", bc.SHAPES, ids=bc.tag)
@pytest.mark.parametrize("loss", REG)
def test_census(loss, shape):
    inp = bc.load_inputs(F, loss, shape)
    bc.CHECK[loss](inp, bc.classes(loss, shape))
    built = bc.BUILD[loss](shape)                               # the fixture holds what the builders make (up to host libm)
    for k, v in inp.items():
        assert v.dtype == np.float32 and np.allclose(built[k], v, rtol=1e-5, atol=1e-6), k


@pytest.mark.parametrize("shape", bc.SHAPES, ids=bc.tag)
@pytest.mark.parametrize("C", bc.SEM_CHANNELS)
def test_semantics_census(C, shape):
    inp = bc.load_inputs(F, "sem%d" % C, shape)
    c = bc.check_sem_census(inp, bc.classes("sem", shape))
    assert np.array_equal(bc.build_sem(shape, C)["labels"], inp["labels"])
    for dt in ("f32", "f64"):                                   # ties count as first-maximum arg-max counts them
        assert float(F[bc.key("sem%d" % C, shape, dt, "rate")]) == c["count"] / c["lab"].size


def _census_count(loss, shape, clamp):
    inp = bc.load_inputs(F, loss, shape)
    if loss == "coord":
        return bc.coord_census(inp, *bc.COORD_CLAMPS[clamp])["count"]
    return (bc.depth_census if loss == "depth" else bc.normal_census)(inp)["count"]


@pytest.mark.parametrize("loss,shape,mode,clamp", CASES)
def test_classification_is_the_same_in_fp32_and_float64(loss, shape, mode, clamp):
    B, Ho, Wo = shape
    rate = _census_count(loss, shape, clamp) / (B * Ho * Wo)
    assert float(_fx(loss, shape, mode, clamp, "f64", "rate")) == rate
    assert float(_fx(loss, shape, mode, clamp, "f32", "rate")) == rate
    inp = bc.load_inputs(F, loss, shape)
    for dt in (torch.float32, torch.float64):
        assert bo.evaluate(loss, inp, mode, clamp, dt, 'mean')[1] == rate


@pytest.mark.parametrize("loss,shape,mode,clamp", CASES)
def test_oracle_float64_reproduces_reference(loss, shape, mode, clamp):
    got = bo.weighted_gradients(loss, bc.load_inputs(F, loss, shape), mode, clamp, torch.float64)
    assert np.allclose(got["loss_none"], _fx(loss, shape, mode, clamp, "f64", "loss_none"), rtol=1e-12, atol=0)
    mean = bo.evaluate(loss, bc.load_inputs(F, loss, shape), mode, clamp, torch.float64, 'mean')[0].item()
    assert mean == pytest.approx(float(_fx(loss, shape, mode, clamp, "f64", "loss_mean")), rel=1e-12)
    for o in ("dpred", "dunc") if mode else ("dpred",):
        ok, worst = bc.compare(got[o], _fx(loss, shape, mode, clamp, "f64", o), 1e-12, bc.classes(loss, shape), bc.CLASSES[loss])
        assert ok, bc.report(o, 1e-12, worst)
    assert mode or "dunc" not in got


@pytest.fixture
def _fixture_host_blas(monkeypatch):
    """The fp32 oracle's two MKL calls as the fixture's host rounds them, as in test_loss_oracle.py: torch.linalg.inv returns
    the recorded inverse (checked against this host's), torch.bmm accumulates each dot product in the fixture host's order.
    Elementwise operations round the same everywhere."""
    inv = torch.linalg.inv
    recorded = {s: (F[bc.key("coord", s, "poses")], F[bc.key("coord", s, "poses_inv")]) for s in bc.SHAPES}

    def recorded_inv(a):
        poses, rec = next((p, r) for p, r in recorded.values() if p.shape == tuple(a.shape))
        assert np.array_equal(a.numpy(), poses)
        assert torch.allclose(inv(a), torch.tensor(rec), rtol=1e-5, atol=1e-5)
        return torch.tensor(rec)

    def ordered_bmm(a, b):
        a64, b64 = a.double(), b.double()
        acc = (a64[:, :, :1] * b64[:, None, 0]).float()
        for k in range(1, a.shape[2]):
            acc = (a64[:, :, k:k + 1] * b64[:, None, k] + acc.double()).float()
        return acc
    monkeypatch.setattr(torch.linalg, "inv", recorded_inv)
    monkeypatch.setattr(torch, "bmm", ordered_bmm)


@pytest.mark.parametrize("loss,shape,mode,clamp", CASES)
def test_oracle_fp32_reproduces_reference(loss, shape, mode, clamp, _fixture_host_blas):
    """The host tolerance of test_loss_oracle.py, with the oracle's MKL calls pinned as there (bit for bit on the fixture's
    host without the pin)."""
    got = bo.weighted_gradients(loss, bc.load_inputs(F, loss, shape), mode, clamp, torch.float32)
    assert np.allclose(got["loss_none"], _fx(loss, shape, mode, clamp, "f32", "loss_none"), rtol=2e-6, atol=0)
    for o in ("dpred", "dunc") if mode else ("dpred",):
        ref = _fx(loss, shape, mode, clamp, "f32", o)
        assert ref.dtype == np.float32 and np.allclose(got[o], ref, rtol=1e-4, atol=1e-7), o


@pytest.mark.parametrize("shape", bc.SHAPES, ids=bc.tag)
@pytest.mark.parametrize("C", bc.SEM_CHANNELS)
def test_semantics_oracle_reproduces_reference(C, shape):
    loss = "sem%d" % C
    inp = bc.load_inputs(F, loss, shape)
    for dt, dn, rv, rg in ((torch.float64, "f64", 1e-12, 1e-12), (torch.float32, "f32", 2e-6, 1e-5)):
        got = bo.weighted_gradients(loss, inp, None, 0, dt)
        assert np.allclose(got["loss_none"], F[bc.key(loss, shape, dn, "loss_none")], rtol=rv, atol=0)
        assert np.allclose(got["dpred"], F[bc.key(loss, shape, dn, "dpred")], rtol=rg, atol=1e-9 if dn == "f32" else 1e-300)
        assert got["rate"] == float(F[bc.key(loss, shape, dn, "rate")])


def test_yardstick_table_is_what_the_fixture_gives():
    measured = bc.measured_yardstick(F)
    assert set(measured) == set(bc.YARDSTICK)
    for k, v in measured.items():
        print(k, "measured %.3e table %.1e" % (v, bc.YARDSTICK[k]))
        assert 0.5 * bc.YARDSTICK[k] <= v <= bc.YARDSTICK[k], k
    # orders of magnitude inside what the whole-tensor tolerances of test_loss_gpu.py admit at a median element
    assert max(v for k, v in bc.YARDSTICK.items()) < 2e-4


def _self_test_cases():
    return [pytest.param(l, s, o, id="%s-%s-%s" % (l, bc.tag(s), o)) for l in REG for s in bc.SHAPES for o in ("dpred", "dunc")]


# classes whose float64 gradient is exactly zero in every cell, per (loss, output): zeroing one of their cells changes nothing
ALL_ZERO = {("coord", "dpred"): set(),
            ("coord", "dunc"): {"nodata_all", "nodata_one", "far_on_nodata", "sigma_clamped"},
            ("depth", "dpred"): {"nodata", "exact_hit", "err_sq_clamped", "below_min_depth_on_nodata"},
            ("depth", "dunc"): {"nodata", "below_min_depth_on_nodata", "sigma_clamped"},
            ("normal", "dpred"): {"label_down", "nodata"},
            ("normal", "dunc"): {"label_down", "nodata", "sigma_clamped"}}


@pytest.mark.parametrize("loss,shape,output", _self_test_cases())
def test_comparator_rejects_what_it_must(loss, shape, output):
    """Fed the float64 truth at the bound the GPU test uses, the comparator accepts the truth and the reference's own fp32
    gradients, and rejects: one zeroed cell (tried for a cell of every class), one class scaled by 1 + 1e-3, and d loss / d
    sigma of the sigma^2-clamped class without the kernels' guard."""
    cls, names = bc.classes(loss, shape), bc.CLASSES[loss]
    bound = bc.gradient_bound(loss, "MLE", output)
    truth = _fx(loss, shape, "MLE", 0, "f64", output)
    ok = lambda g: bc.compare(g, truth, bound, cls, names)[0]
    assert ok(truth) and ok(_fx(loss, shape, "MLE", 0, "f32", output))
    live = set()
    for c, name in enumerate(names):
        cells = np.argwhere(cls == c)
        nonzero = [tuple(i) for i in cells if np.abs(truth[i[0], :, i[1], i[2]]).max() > 0]
        assert (name in ALL_ZERO[loss, output]) == (not nonzero), name
        if not nonzero:
            assert not truth.transpose(0, 2, 3, 1)[cls == c].any()
            continue
        live.add(name)
        b, y, x = nonzero[len(nonzero) // 2]
        zeroed = truth.copy()
        zeroed[b, :, y, x] = 0.0
        assert not ok(zeroed), name
        scaled = truth.copy()
        scaled.transpose(0, 2, 3, 1)[cls == c] *= 1.0 + 1e-3
        assert not ok(scaled), name
        one_wrong = truth.copy()                                 # a single cell off by twice the bound
        one_wrong[b, :, y, x] *= 1.0 + 2.0 * bound
        assert not ok(one_wrong), name
    assert live == set(names) - ALL_ZERO[loss, output]
    if output == "dunc":
        inp = bc.load_inputs(F, loss, shape)
        census = bc.coord_census(inp, *bc.COORD_CLAMPS[0]) if loss == "coord" else \
            (bc.depth_census if loss == "depth" else bc.normal_census)(inp)
        B, Ho, Wo = shape
        mid = cls == names.index("sigma_sq_clamped")
        w = (bc.weights(B) / (Ho * Wo))[:, None, None] + np.zeros(cls.shape)
        guarded = w * bc.MLE_K[loss] / census["sigma"]            # the clamp of sigma^2 has derivative 0
        assert np.allclose(truth[:, 0][mid], guarded[mid], rtol=1e-12)
        bad = truth.copy()
        bad[:, 0][mid] = bc.unguarded_dunc(loss, census["err2"], census["sigma"], w)[mid]
        assert np.abs(bad[:, 0][mid] / truth[:, 0][mid]).min() > 100.0
        assert not ok(bad)


def test_zero_rule_of_the_comparator():
    truth = np.zeros((1, 2, 1, 3))
    truth[0, :, 0, 1] = (1.0, 0.0)
    got = truth.copy()
    assert bc.cell_errors(got, truth).max() == 0
    got[0, 1, 0, 1] = 1e-30                                      # a zero element of a live cell
    got[0, 0, 0, 2] = np.nan
    e = bc.cell_errors(got, truth)
    assert e[0, 0, 0] == 0 and np.isinf(e[0, 0, 1]) and np.isinf(e[0, 0, 2])
