"""Float64 numpy restatement of the depth, normal and semantics evaluation metrics and of the frame grouping - our own,
like tests/head_refs.py - shared by tests/test_eval_metrics_cpu.py (which pins it to the values recorded from the reference's
functions, tests/golden/eval_metrics.npz) and tests/test_eval_metrics_gpu.py (which holds the HIP kernels to it).

Formulas: utils/evaluation.py:247-267 (depth), :294-316 with utils/learning.py:417-440 (normal), :339-414 (semantics).
Rows are the per-image sums of include/crossloc_metrics.h; every figure the reference reports is a ratio of row sums."""
import numpy as np

NUM_CLASS = 6


def depth_rows(depth, gt, nodata=-1.0):
    """depth [B,1,H,W], gt [B,1,H,W] float32 -> float64 [B,3] = {sum |d-g|*m/g, sum (|d-g|*m)^2, sum m}"""
    B = depth.shape[0]
    m = (gt.reshape(B, -1) != np.float32(nodata)).astype(np.float64)
    d, g = depth.reshape(B, -1).astype(np.float64), gt.reshape(B, -1).astype(np.float64)
    em = np.abs(d - g) * m
    return np.stack([(em / g).sum(1), (em * em).sum(1), m.sum(1)], 1)


def normal_angles(logits, gt):
    """logits [B,2,N] float32, gt [B,3,N] float32 -> angular error in degrees, float64 [B,N] (mask not applied)"""
    r = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
    r = (np.clip(r, 1.e-7, 1 - 1.e-7) * 2 - 1.0) * np.pi
    xy = np.cos(r[:, 1])
    v = np.stack([np.cos(r[:, 0]) * xy, np.sin(r[:, 0]) * xy, np.sin(r[:, 1])], 1)
    v = v / np.maximum(np.sqrt((v * v).sum(1, keepdims=True)), 1.e-12)          # F.normalize
    g = gt.astype(np.float64)
    vn = v / np.maximum(np.sqrt((v * v).sum(1, keepdims=True)), 1.e-8)          # cosine_similarity: clamped norms first
    gn = g / np.maximum(np.sqrt((g * g).sum(1, keepdims=True)), 1.e-8)
    c = np.clip((vn * gn).sum(1), -1 + 1.e-7, 1 - 1.e-7)
    return np.arccos(c) / np.pi * 180.0


def normal_rows(logits, gt, nodata=-1.0):
    """logits [B,2,H,W], gt [B,3,H,W] float32 -> float64 [B,2] = {sum angle_deg*m, sum m}"""
    B = logits.shape[0]
    g = gt.reshape(B, 3, -1)
    m = ((g == np.float32(nodata)).sum(1) == 0).astype(np.float64)
    a = normal_angles(logits.reshape(B, 2, -1), g)
    return np.stack([(a * m).sum(1), m.sum(1)], 1)


def class_map(logits):
    """first arg-max over the class channel: [B,6,H,W] -> int64 [B,H,W]"""
    return np.argmax(logits, axis=1)


def semantics_rows(logits, labels):
    """logits [B,6,H,W], labels [B,1,H,W] float32 -> int64 [B,36] confusion counts, rows = ground truth"""
    B = logits.shape[0]
    cls = class_map(logits).reshape(B, -1)
    lab = labels.reshape(B, -1)
    rows = np.zeros((B, NUM_CLASS * NUM_CLASS), np.int64)
    for b in range(B):
        m = (lab[b] >= 0) & (lab[b] < NUM_CLASS)                                # on the float label, before truncation
        rows[b] = np.bincount(NUM_CLASS * lab[b][m].astype(np.int64) + cls[b][m], minlength=NUM_CLASS * NUM_CLASS)
    return rows


def segmentation_metrics(cm):
    """(pixel accuracy, mean IoU, frequency-weighted IoU) of one 6x6 confusion matrix; NaN where the reference has 0/0"""
    cm = np.asarray(cm, np.float64).reshape(NUM_CLASS, NUM_CLASS)
    d = np.diag(cm)
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = d.sum() / cm.sum()
        iu = d / (cm.sum(1) + cm.sum(0) - d)
        fr = cm.sum(1) / cm.sum()
    miou = np.nan if np.all(np.isnan(iu)) else np.nanmean(iu)
    return acc, miou, (fr[fr > 0] * iu[fr > 0]).sum()


def group(task, rows, size=4):
    """rows [K,D] in dataset order -> depth (abs_rel[G], rms[G]); normal err[G]; semantics (acc[K], miou[K], fwiou[K]).
    G = groups of `size` consecutive frames, the last one shorter; a group without a valid cell is NaN."""
    rows = np.asarray(rows, np.float64)
    if task == "semantics":
        m = np.array([segmentation_metrics(r) for r in rows], np.float64).reshape(-1, 3)
        return m[:, 0], m[:, 1], m[:, 2]
    s = np.array([rows[i:i + size].sum(0) for i in range(0, len(rows), size)], np.float64).reshape(-1, rows.shape[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        if task == "depth":
            return s[:, 0] / s[:, 2], np.sqrt(s[:, 1] / s[:, 2])
        return s[:, 0] / s[:, 1]
