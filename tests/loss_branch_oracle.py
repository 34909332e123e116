"""oracle/loss_oracle.py on the scenes of loss_branch_cases.py, in fp32 or float64 - shared by
test_loss_branches_cpu.py (the oracle against the reference fixture) and test_loss_branches_gpu.py (per-cell terms for the
error budget of the loss values)."""
import functools
import os

import numpy as np
import torch

import loss_branch_cases as bc
from oracle import loss_oracle

FIXTURE = np.load(os.path.join(os.path.dirname(__file__), "golden", "loss_branches.npz"))


def evaluate(loss, inp, mode, clamp=0, dtype=torch.float64, reduction=None):
    """(value, rate, prediction leaf, uncertainty leaf or None) of the oracle on one scene; reduction None, 'mean' or
    'cell' (the unreduced per-cell terms [B,N])."""
    torch.set_default_dtype(dtype)
    try:
        def T(k, grad=False):
            return torch.tensor(inp[k], dtype=dtype, requires_grad=grad)
        mle = mode == "MLE"
        if loss.startswith("sem"):
            p, u = T("logits", True), None
            val, rate = loss_oracle.semantics_loss(p, T("labels"), reduction)
        elif loss == "coord":
            p, u = T("pred", True), T("unc", True)
            f, cx, cy = bc.coord_intrinsics((p.shape[0], p.shape[2], p.shape[3]))
            soft, hard = bc.COORD_CLAMPS[clamp]
            val, rate = loss_oracle.coord_loss(p, u, T("poses"), T("gt"), f, cx, cy, bc.SUB, bc.MIN_DEPTH, soft, hard, bc.TOL,
                                               bc.NODATA, mle, reduction)
        elif loss == "depth":
            p, u = T("pred", True), T("unc", True)
            val, rate = loss_oracle.depth_loss(p, u, T("gt"), bc.MIN_DEPTH, bc.DEPTH_HARD, bc.NODATA, mle, reduction)
        else:
            p, u = T("logits", True), T("unc", True)
            val, rate = loss_oracle.normal_loss(p, u, T("gt"), bc.NORMAL_HARD, bc.NODATA, mle, reduction)
    finally:
        torch.set_default_dtype(torch.float32)
    return val, rate, p, u


def weighted_gradients(loss, inp, mode, clamp=0, dtype=torch.float64):
    """dict(loss_none, rate, dpred[, dunc]) as make_golden.py lossbranches records them from the reference."""
    val, rate, p, u = evaluate(loss, inp, mode, clamp, dtype, None)
    (val * torch.linspace(0.5, 1.5, val.shape[0], dtype=dtype)).sum().backward()
    out = dict(loss_none=val.detach().double().numpy(), rate=rate, dpred=p.grad.numpy())
    if u is not None and u.grad is not None:
        out["dunc"] = u.grad.numpy()
    return out


@functools.lru_cache(maxsize=None)
def mean_abs_cell_term(loss, shape, mode, clamp=0):
    """Per image, the mean |per-cell loss term| of the float64 oracle: the scale of the rounding a sum of those terms can
    carry (the terms change sign where log(sigma) < 0, so the loss itself can be much smaller).  [B] float64."""
    with torch.no_grad():
        cell, _, _, _ = evaluate(loss, bc.load_inputs(FIXTURE, loss, shape), mode, clamp, torch.float64, 'cell')
    return cell.abs().mean(dim=1).numpy()
