"""Float64 references of the two head ops and of conv1's weight gradient, shared by the per-op GPU tests
(tests/test_head_ops_gpu.py, tests/test_conv1_wgrad_gpu.py) and pinned on the CPU against oracle/cnn_oracle.py by
tests/test_head_refs.py.  Plain torch; autograd supplies the gradients.  Every tensor is taken in the dtype it arrives in."""
import math

import torch
import torch.nn.functional as F

CLAMP_LO, CLAMP_HI = -16.10, 13.82


def head_reference(x, w, b, mean, n_task, n_pos, lo=CLAMP_LO, hi=CLAMP_HI):
    """XL_OP_HEAD: x [B,Cin,H,W], w [Cout,Cin] or [Cout,Cin,1,1], b [Cout], mean [n_task] -> ([B,Cout,H,W], raw fc3 output):
    fc3, the mean on the task channels, exp(hardtanh) on the positive channels."""
    sc = F.conv2d(x, w.reshape(w.shape[0], w.shape[1], 1, 1), b)
    out = sc[:, :n_task] + mean[None, :, None, None]
    if n_pos:
        out = torch.cat([out, torch.exp(F.hardtanh(sc[:, n_task:], min_val=lo, max_val=hi))], dim=1)
    return out, sc


def duc_head_reference(x, w, b, mean, n_task, n_pos, hw, lo=CLAMP_LO, hi=CLAMP_HI):
    """XL_OP_DUC_HEAD: x [B,C*64,Hs,Ws] (the DUC activation) -> x8 pixel shuffle -> bilinear resize to hw -> the head."""
    v = F.pixel_shuffle(x, 8)
    v = F.interpolate(v, tuple(hw), mode="bilinear", align_corners=False)
    return head_reference(v, w, b, mean, n_task, n_pos, lo, hi)


def clamp_census(sc_pos, lo=CLAMP_LO, hi=CLAMP_HI):
    """Shares of positive-channel cells (at the lower bound, at the upper bound, strictly inside) of the raw fc3 output."""
    n = float(sc_pos.numel())
    return ((sc_pos <= lo).sum().item() / n, (sc_pos >= hi).sum().item() / n, ((sc_pos > lo) & (sc_pos < hi)).sum().item() / n)


def map_positive_row(w, b, z, row):
    """Scale fc3's positive row so that ceil(12 %) of the raw values z (float64, that row's output) lie half a unit or more
    below CLAMP_LO and as many above CLAMP_HI; the rest spreads in between."""
    z = z.flatten().sort().values
    n = z.numel()
    k = max(1, math.ceil(0.12 * n))
    a = ((CLAMP_HI + 0.5) - (CLAMP_LO - 0.5)) / (z[n - k] - z[k - 1]).item()
    c = (CLAMP_LO - 0.5) - a * z[k - 1].item()
    w[row] = (w[row].double() * a).float()
    b[row] = float(a * b[row].double().item() + c)


def conv1_wgrad_reference(img, dy):
    """XL_OP_CONV1_WGRAD, plain form: img [B,Cin,H,W], dy [B,32,H,W] -> (dW [32,Cin,3,3], db [32]) of a 3x3 s1 p1 conv."""
    dw = torch.nn.grad.conv2d_weight(img, (dy.shape[1], img.shape[1], 3, 3), dy, stride=1, padding=1)
    return dw, dy.sum((0, 2, 3))


def conv1_gn_relu(img, w, b, gamma, beta, relu=True, eps=1e-5):
    """conv1 -> GroupNorm(32, 32) -> ReLU, the layer whose backward the folded form of XL_OP_CONV1_WGRAD evaluates."""
    raw = F.conv2d(img, w, b, stride=1, padding=1)
    o = F.group_norm(raw, 32, gamma, beta, eps)
    return (F.relu(o) if relu else o), raw
