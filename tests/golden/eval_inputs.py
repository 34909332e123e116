"""Seeded inputs of the evaluation-metric fixtures (tests/golden/eval_metrics.npz holds the reference's OUTPUTS only; both
the fixture generator, make_eval_golden.py, and the tests regenerate the inputs from here, like golden_inputs.py).

Cases are (B, H, W): the smallest shapes at which the kernels of csrc/xl_metrics.hip can go wrong (4096 cells per chunk).
  b4_60x90     the product map (5400 cells: two chunks, the second ragged)
  b3_37x53     1961 cells: odd, so planes and image bases are not 16-byte aligned from channel / image 1 on
  b5_120x180   21600 cells: six chunks, the last one ragged (1120 cells)
  b1_480x720   semantics only: the full-size map (85 chunks)
Every tensor that stands for a network output carries one channel more than the task has ([B, nt+1, H, W]); the tests
hand the kernels the strided `[:, :nt]` view of it.

Planted in every case: ~20 % nodata cells; image 1 without any valid cell (not in the one-image case, which would be left
empty); depth labels of valid cells >= 1; logits of +-40 (both sigmoid clamps bind); normal cells exactly parallel and
antiparallel to the label (both cosine clamps bind) and cells with a single nodata channel; semantics labels -1, 6, 255
and 4.5; exact two-way and six-way logit ties.
"""
import numpy as np

NODATA = -1.0
CASES = {"b4_60x90": (4, 60, 90), "b3_37x53": (3, 37, 53), "b5_120x180": (5, 120, 180)}
SEM_CASES = dict(CASES, b1_480x720=(1, 480, 720))
EMPTY_IMAGE = 1                       # the image without a valid cell (cases with more than one image)
_SEED = {"b4_60x90": 401, "b3_37x53": 402, "b5_120x180": 403, "b1_480x720": 404}


def _rng(tag, task):
    return np.random.default_rng(_SEED[tag] * 10 + {"depth": 1, "normal": 2, "semantics": 3}[task])


def _planted_cells(rng, B, n, count):
    """`count` distinct (image, cell) pairs outside the empty image, the very first and the very last cell among them."""
    imgs = [b for b in range(B) if b != EMPTY_IMAGE or B == 1]
    flat = rng.choice(len(imgs) * n, size=count, replace=False)
    flat[0], flat[1] = 0, len(imgs) * n - 1
    assert len(set(flat.tolist())) == count
    return np.array([imgs[i] for i in flat // n]), flat % n


def depth_inputs(tag):
    """-> (output [B,2,H,W] float32: depth + sigma, gt_depth [B,1,H,W] float32)"""
    B, H, W = CASES[tag]
    rng = _rng(tag, "depth")
    gt = rng.uniform(1.0, 300.0, size=(B, 1, H, W)).astype(np.float32)
    out = np.empty((B, 2, H, W), np.float32)
    out[:, 0] = gt[:, 0] + rng.normal(0.0, 5.0, size=(B, H, W)).astype(np.float32)
    out[:, 1] = np.exp(rng.uniform(-2, 3, size=(B, H, W))).astype(np.float32)
    gt[rng.random(size=gt.shape) < 0.2] = NODATA
    gt[EMPTY_IMAGE] = NODATA
    b, c = _planted_cells(rng, B, H * W, 4)
    g = gt.reshape(B, -1)
    g[b, c] = np.array([1.0, 1.0, 250.0, 299.5], np.float32)                     # valid cells at the ends; the smallest label
    out.reshape(B, 2, -1)[b[2], 0, c[2]] = 250.0                                 # an exact hit
    return out, gt


def logits_to_xyz(logits):
    """float64 direction of a pair of angle logits [..., 2] (utils/learning.py:417-440), used to plant the (anti)parallel cells."""
    r = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
    r = (np.clip(r, 1.e-7, 1 - 1.e-7) * 2 - 1.0) * np.pi
    xy = np.cos(r[..., 1])
    return np.stack([np.cos(r[..., 0]) * xy, np.sin(r[..., 0]) * xy, np.sin(r[..., 1])], -1)


def normal_inputs(tag):
    """-> (output [B,3,H,W] float32: azimuth and elevation logits + sigma, gt_normals [B,3,H,W] float32)"""
    B, H, W = CASES[tag]
    n = H * W
    rng = _rng(tag, "normal")
    out = rng.normal(0.0, 2.0, size=(B, 3, H, W)).astype(np.float32)
    out[:, 2] = np.exp(out[:, 2])
    gt = rng.normal(size=(B, 3, H, W))
    gt = (gt / np.linalg.norm(gt, axis=1, keepdims=True)).astype(np.float32)
    nod = rng.random(size=(B, 1, H, W)) < 0.2
    gt[np.broadcast_to(nod, gt.shape)] = NODATA
    gt[EMPTY_IMAGE] = NODATA
    b, c = _planted_cells(rng, B, n, 16)
    o, g = out.reshape(B, 3, n), gt.reshape(B, 3, n)
    # saturated sigmoids, both signs, on either angle
    o[b[0], 0, c[0]] = 40.0; o[b[1], 1, c[1]] = -40.0; o[b[2], 0, c[2]] = -40.0; o[b[3], 1, c[3]] = 40.0
    for k in range(16):
        g[b[k], :, c[k]] = np.array([0.6, -0.48, 0.64], np.float32)              # valid labels on every planted cell
    for k in range(4, 12):                                                       # parallel (even k) / antiparallel (odd k)
        v = logits_to_xyz(o[b[k], :2, c[k]])
        g[b[k], :, c[k]] = (v if k % 2 == 0 else -v).astype(np.float32)
    for k, ch in ((12, 0), (13, 1), (14, 2)):                                    # ONE nodata channel invalidates the cell
        g[b[k], ch, c[k]] = NODATA
    return out, gt


def semantics_case(tag):
    """-> (output [B,7,H,W] float32: 6 class logits + one spare channel, labels [B,1,H,W] float32,
    ties = (image, cell, expected class) of the planted exact ties)"""
    B, H, W = SEM_CASES[tag]
    n = H * W
    rng = _rng(tag, "semantics")
    out = rng.normal(0.0, 2.0, size=(B, 7, H, W)).astype(np.float32)
    lab = rng.integers(0, 6, size=(B, 1, H, W)).astype(np.float32)
    # the prediction follows the label on about half of the cells
    hit = rng.random(size=(B, H, W)) < 0.5
    bi, yi, xi = np.nonzero(hit)
    out[bi, lab[bi, 0, yi, xi].astype(np.int64), yi, xi] += 6.0
    odd = rng.random(size=lab.shape)
    for k, v in enumerate((-1.0, 6.0, 255.0, 4.5)):
        lab[(odd >= 0.05 * k) & (odd < 0.05 * (k + 1))] = v
    if B > 1:
        lab[EMPTY_IMAGE] = np.where(rng.random(size=lab[EMPTY_IMAGE].shape) < 0.5, -1.0, 255.0)
    b, c = _planted_cells(rng, B, n, 12)
    o, g = out.reshape(B, 7, n), lab.reshape(B, 1, n)
    for k in range(12):
        g[b[k], 0, c[k]] = float(k % 6) if k != 5 else 4.5
    for k in range(0, 4):                                                        # six-way ties -> class 0
        o[b[k], :6, c[k]] = np.float32(0.75 * k - 1.0)
    pairs = ((2, 5), (0, 1), (4, 5), (1, 3), (3, 4), (0, 5), (2, 3), (1, 5))
    for k, (i, j) in zip(range(4, 12), pairs):
        o[b[k], :6, c[k]] = np.linspace(-3.0, -1.0, 6, dtype=np.float32)        # two-way ties -> the lower index i
        o[b[k], i, c[k]] = o[b[k], j, c[k]] = np.float32(1.25)
    return out, lab, (b, c, np.array([0, 0, 0, 0] + [i for i, _ in pairs]))


def semantics_inputs(tag):
    return semantics_case(tag)[:2]


def checksum(*arrays):
    return float(sum(np.asarray(a, np.float64).sum() for a in arrays))
