"""GPU: the fused loss kernels (csrc/xl_loss.hip, through crossloc_amd.loss) cell by cell, on every branch, against the
imported reference evaluated in float64 (tests/golden/loss_branches.npz).  Scenes, classes, error measure and bounds:
loss_branch_cases.py; test_loss_branches_cpu.py proves on the CPU that every class is populated and off its thresholds and
that the comparator rejects a zeroed cell, a class scaled by 1 + 1e-3 and a missing sigma^2 guard.  No cell is excluded.

    gradients    per-cell scaled error <= max(4 x YARDSTICK, 2e-6); exact zeros where float64 is exactly zero
    loss values  |value - float64| <= max(4 x YARDSTICK_value x |float64|, 1e-6 x mean |per-cell term|)
    valid rate   == float32(count / (B N)) with the float64 census's count
    training form (task_loss_and_output_gradient, prediction and sigma in one tensor): the bits of the autograd form
    semantics    the elementwise tolerances of test_semantics_gpu.py, against float64

A failure names the worst per-cell error of every class, so a red run points at the branch."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import loss_branch_cases as bc                        # noqa: E402
import loss_branch_oracle as bo                       # noqa: E402
from crossloc_amd import loss as xl_loss              # noqa: E402

pytestmark = pytest.mark.gpu
F = bo.FIXTURE
REG = ("coord", "depth", "normal")
CASES = [pytest.param(l, s, m, c, id="%s-%s-%s" % (l, bc.tag(s), bc.run_tag(l, m, c))) for l in REG for s in bc.SHAPES
         for m, c in bc.runs(l)]


def _dev(a, grad=False):
    return torch.tensor(a, device="cuda", requires_grad=grad)


def _fx(loss, shape, mode, clamp, what):
    return bc.stored(F, loss, shape, mode, clamp, "f64", what)


def _pred_name(loss):
    return "logits" if loss == "normal" else "pred"


def _autograd_form(loss, inp, mode, clamp, reduction):
    """(loss, rate, prediction leaf, sigma leaf) of the reference-signature function."""
    p, u = _dev(inp[_pred_name(loss)], True), _dev(inp["unc"], True)
    gt = _dev(inp["gt"])
    if loss == "coord":
        B, _, Ho, Wo = p.shape
        f, cx, cy = bc.coord_intrinsics((B, Ho, Wo))
        soft, hard = bc.COORD_CLAMPS[clamp]
        val, rate = xl_loss.scene_coords_regression_loss(bc.MIN_DEPTH, soft, hard, bc.TOL, mode, xl_loss.get_pixel_grid(int(bc.SUB)),
                                                         bc.NODATA, xl_loss.get_cam_mat(2 * cx, 2 * cy, f), p, u,
                                                         _dev(inp["poses"]), gt, reduction=reduction)
    elif loss == "depth":
        val, rate = xl_loss.depth_regression_loss(bc.MIN_DEPTH, bc.DEPTH_HARD, mode, bc.NODATA, p, u, gt, reduction=reduction)
    else:
        val, rate = xl_loss.normal_regression_loss(bc.NORMAL_HARD, mode, bc.NODATA, p, u, gt, reduction=reduction)
    return val, rate, p, u


def _check_values(got, want, loss, shape, mode, clamp, reduction):
    """Per-image values (reduction None) or the mean against float64, with the budget of the module docstring."""
    scale = bo.mean_abs_cell_term(loss, tuple(shape), mode, clamp)
    scale = scale if reduction is None else scale.mean()
    got, want = np.atleast_1d(got.detach().cpu().numpy().astype(np.float64)), np.atleast_1d(want)
    lim = np.maximum(bc.value_bound(loss, mode) * np.abs(want), 1e-6 * scale)
    print("values", got, "float64", want, "allowed", lim)
    assert got.shape == want.shape and (np.abs(got - want) <= lim).all(), (got - want, lim)


@pytest.mark.parametrize("reduction", ["mean", None])
@pytest.mark.parametrize("loss,shape,mode,clamp", CASES)
def test_every_branch_cell_by_cell(loss, shape, mode, clamp, reduction):
    inp = bc.load_inputs(F, loss, shape)
    B, Ho, Wo = shape
    cls, names = bc.classes(loss, shape), bc.CLASSES[loss]
    census = bc.CHECK[loss](inp, cls)                          # the scene is what the bounds were derived for
    count = (census[clamp] if loss == "coord" else census)["count"]
    val, rate, p, u = _autograd_form(loss, inp, mode, clamp, reduction)
    (val * _dev(bc.weights(B).astype(np.float32))).sum().backward() if reduction is None else val.backward()
    assert tuple(val.shape) == (() if reduction is not None else (B,))
    assert rate.dtype == torch.float32 and float(rate) == float(np.float32(count / (B * Ho * Wo)))
    _check_values(val, _fx(loss, shape, mode, clamp, "loss_none" if reduction is None else "loss_mean"), loss, shape, mode,
                  clamp, reduction)
    failures = []
    for o, leaf in (("dpred", p), ("dunc", u)):
        if o == "dunc" and mode is None:
            assert u.grad is None
            continue
        truth = _fx(loss, shape, mode, clamp, o)
        if reduction is not None:
            truth = bc.mean_gradient(truth, B)
        bound = bc.gradient_bound(loss, mode, o)
        ok, worst = bc.compare(leaf.grad.cpu().numpy(), truth, bound, cls, names)
        print(bc.report(o, bound, worst))
        if not ok:
            failures.append(bc.report(o, bound, worst))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("loss,shape,mode,clamp", CASES)
def test_training_form_gives_the_bits_of_the_autograd_form(loss, shape, mode, clamp):
    """task_loss_and_output_gradient reads prediction and sigma from ONE [B, C (+1), H, W] tensor (other per-image strides,
    in-place gradient): same loss, rate and gradients, bit for bit, as the autograd form with reduction 'mean'."""
    inp = bc.load_inputs(F, loss, shape)
    val, rate, p, u = _autograd_form(loss, inp, mode, clamp, "mean")
    val.backward()
    nt = inp[_pred_name(loss)].shape[1]
    stacked = np.concatenate([inp[_pred_name(loss)], inp["unc"]], 1) if mode else inp[_pred_name(loss)]
    kw = {}
    if loss == "coord":
        f, cx, cy = bc.coord_intrinsics(shape)
        soft, hard = bc.COORD_CLAMPS[clamp]
        kw = dict(gt_poses=_dev(inp["poses"]), pixel_grid=xl_loss.get_pixel_grid(int(bc.SUB)),
                  cam_mat=xl_loss.get_cam_mat(2 * cx, 2 * cy, f), soft_clamp=soft, hard_clamp=hard, init_tolerance=bc.TOL)
    else:
        kw = dict(hard_clamp=bc.DEPTH_HARD if loss == "depth" else bc.NORMAL_HARD)
    l2, r2, grad = xl_loss.task_loss_and_output_gradient(loss, mode, _dev(stacked), nt, _dev(inp["gt"]), nodata_value=bc.NODATA,
                                                         min_depth=bc.MIN_DEPTH, **kw)
    assert torch.equal(l2, val.detach()) and torch.equal(r2, rate)
    assert torch.equal(grad[:, :nt], p.grad)
    if mode:
        assert torch.equal(grad[:, nt:], u.grad)
    else:
        assert grad.shape[1] == nt and u.grad is None


SEM_CASES = [pytest.param(C, s, id="C%d-%s" % (C, bc.tag(s))) for C in bc.SEM_CHANNELS for s in bc.SHAPES]


@pytest.mark.parametrize("reduction", ["mean", None])
@pytest.mark.parametrize("C,shape", SEM_CASES)
def test_semantics_planted_classes(C, shape, reduction):
    """Ties (label on the first / on the second maximum), logits of +-80, a dominant class and the ignore label -100, at 6 and
    3 classes: tolerances of test_semantics_gpu.py (already per element), held against float64; the rate counts a tie exactly
    as first-maximum arg-max does; an ignored cell has loss and gradient exactly 0 and stays in the denominator."""
    loss = "sem%d" % C
    inp = bc.load_inputs(F, loss, shape)
    B, Ho, Wo = shape
    cls = bc.classes("sem", shape)
    census = bc.check_sem_census(inp, cls)
    p = _dev(inp["logits"], True)
    val, rate = xl_loss.semantics_classification_loss(None, p, None, _dev(inp["labels"]), xl_loss.CrossEntropyLoss2d(), reduction)
    (val * _dev(bc.weights(B).astype(np.float32))).sum().backward() if reduction is None else val.backward()
    assert float(rate) == float(np.float32(census["count"] / (B * Ho * Wo)))
    want = F[bc.key(loss, shape, "f64", "loss_none" if reduction is None else "loss_mean")]
    assert np.allclose(np.atleast_1d(val.detach().cpu().numpy()), np.atleast_1d(want), rtol=2e-6, atol=0)
    truth = F[bc.key(loss, shape, "f64", "dpred")]
    truth = truth if reduction is None else bc.mean_gradient(truth, B)
    got = p.grad.cpu().numpy()
    assert np.isfinite(got).all()
    bad = ~np.isclose(got, truth, rtol=2e-4, atol=1e-11)
    worst = {n: float((np.abs(got - truth) / np.maximum(np.abs(truth), 1e-11)).transpose(0, 2, 3, 1)[cls == c].max())
             for c, n in enumerate(bc.SEM_CLASSES)}
    assert not bad.any(), "elements out of tolerance by class: %s; worst relative error by class: %s" % (
        {n: int(bad.any(1)[cls == c].sum()) for c, n in enumerate(bc.SEM_CLASSES)}, worst)
    assert not got.transpose(0, 2, 3, 1)[cls == bc.SEM_CLASSES.index("ignore_label")].any()
    if reduction is not None:                                   # the training form: the bits of the autograd form
        l3, r3, g3 = xl_loss.task_loss_and_output_gradient("semantics", None, _dev(inp["logits"]), C, _dev(inp["labels"]))
        assert torch.equal(l3, val.detach()) and torch.equal(r3, rate) and torch.equal(g3, p.grad)
