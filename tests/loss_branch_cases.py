"""Well-conditioned scenes that put every branch of the fused loss kernels (csrc/xl_loss.hip) into every workgroup, the
float64 census that proves each branch is populated, and the per-cell comparator of tests/test_loss_branches_{cpu,gpu}.py.
numpy only.

Scenes.  Camera-frame depths of 8 - 30 m, poses within a few metres of the origin, f = 200, 8-pixel cells: fp32 rounding
of the geometry stays near 1e-6 of a gradient, where the O(500 m) scenes of test_loss_gpu.py need 1e-3.  Shapes
(B, Ho, Wo) = (3, 19, 29) - 551 cells per image, three workgroups, the last with 39 live lanes - and (2, 3, 131) - 393
cells, rows of odd width wider than half a workgroup.  Twelve slots are dealt out by (5 i + 3 b) mod 12 over the flat
cell index i and the image b, so every class occurs in every image and every workgroup; the three sigma classes live in
the last image only (their err^2 / 2e-7 terms would swamp the per-image values of the others) and are regular cells
elsewhere.  A class that is invalid is so for its own reason alone: a coord cell behind the camera or under min_depth
still reprojects 2 - 15 px from its pixel (with the depth on its clamp) and lies within the tolerance, so only the depth test
removes it (check_coord_census asserts that under both clamp pairs).  Regular uncertainties keep err^2 / (k sigma^2) outside (0.64, 1.56): k / sigma - err^2 / sigma^3 does not
cancel, so d loss / d sigma is as well conditioned as its two terms.

Error measure.  A gradient cell (all channels of one pixel) is compared with the imported reference evaluated in float64
(tests/golden/loss_branches.npz, written by tests/golden/make_golden.py lossbranches) and the largest channel difference
is scaled by the largest |float64 gradient| over that cell's own channels: the "per-cell scaled" error.  An element that
is exactly 0 in float64 (invalid, saturated, exact hit, ignore label) must be exactly 0.  No cell is left out.

Yardstick.  YARDSTICK[loss, mode, output] is the largest per-cell scaled distance of the reference's own fp32 gradients
from its float64 gradients over both shapes (and both clamp pairs for coord); output "value" is the largest relative
distance of its fp32 per-image and mean loss values.  Measured on the fixture (test_loss_branches_cpu.py recomputes them
and holds the table to within [0.5, 1] of what it finds):

    loss    mode   dpred     dunc      value
    coord   MLE    1.2e-4    2.6e-5    2.1e-7
    coord   plain  1.2e-4    -         1.4e-7
    depth   MLE    2.0e-7    7.3e-7    1.8e-7
    depth   plain  4.0e-8    -         1.2e-7
    normal  MLE    1.3e-5    4.4e-5    7.3e-7
    normal  plain  1.2e-6    -         1.9e-7

The kernels are held to max(4 x YARDSTICK, 2e-6) per cell (gradient_bound): the same fp32 formulas in another operation
order, a pose inverse computed in double and device logf / expf / atan2f / acosf within 1 - 2 ulp of the host's; the floor
is about 16 fp32 ulp for the dozen operations of the longest chain.  Nothing here comes from GPU output.
"""
import numpy as np

SHAPES = [(3, 19, 29), (2, 3, 131)]
SUB, FOCAL, MIN_DEPTH, TOL, NODATA = 8.0, 200.0, 0.1, 50.0, -1.0
COORD_CLAMPS = [(100.0, 1000.0), (20.0, 60.0)]          # (soft, hard): the reference's, and one that reaches both branches
DEPTH_HARD = NORMAL_HARD = 10.0
MODES = ["MLE", None]
MARGIN = 0.01                                            # every deciding quantity is this far (relative) from its threshold
MIN_CELLS = 20                                           # cells per class and image it lives in
SIG_CLAMP = 1e-7                                         # clamp of sigma, of sigma^2 and of err^2 in all three MLE terms

COORD_CLASSES = ("regular", "nodata_all", "nodata_one", "far_on_nodata", "far_on_valid", "behind_camera", "below_min_depth",
                 "between_clamps", "above_hard", "sigma_clamped", "sigma_sq_clamped", "sigma_small")
DEPTH_CLASSES = ("regular", "nodata", "pred_below_min_depth", "pred_negative", "above_hard", "exact_hit", "err_sq_clamped",
                 "below_min_depth_on_nodata", "sigma_clamped", "sigma_sq_clamped", "sigma_small")
NORMAL_CLASSES = ("regular", "azimuth_far", "azimuth_wrap", "azimuth_logit_25", "elevation_logit_m40", "label_up",
                  "label_down", "nodata", "sigma_clamped", "sigma_sq_clamped", "sigma_small")
SEM_CLASSES = ("regular", "tie_label_first", "tie_label_second", "saturated_on_max", "saturated_off_max", "dominant",
               "ignore_label")
CLASSES = {"coord": COORD_CLASSES, "depth": DEPTH_CLASSES, "normal": NORMAL_CLASSES, "sem": SEM_CLASSES}
MLE_K = {"coord": 3.0, "depth": 1.0, "normal": 2.0}      # k log(sigma) + err^2 / (2 sigma^2)

# largest per-cell scaled distance fp32 reference -> float64 reference (module docstring)
YARDSTICK = {
    ("coord", "MLE", "dpred"): 1.2e-4, ("coord", "MLE", "dunc"): 2.6e-5, ("coord", "MLE", "value"): 2.1e-7,
    ("coord", "plain", "dpred"): 1.2e-4, ("coord", "plain", "value"): 1.4e-7,
    ("depth", "MLE", "dpred"): 2.0e-7, ("depth", "MLE", "dunc"): 7.3e-7, ("depth", "MLE", "value"): 1.8e-7,
    ("depth", "plain", "dpred"): 4.0e-8, ("depth", "plain", "value"): 1.2e-7,
    ("normal", "MLE", "dpred"): 1.3e-5, ("normal", "MLE", "dunc"): 4.4e-5, ("normal", "MLE", "value"): 7.3e-7,
    ("normal", "plain", "dpred"): 1.2e-6, ("normal", "plain", "value"): 1.9e-7,
}


def gradient_bound(loss, mode, output):
    return max(4.0 * YARDSTICK[loss, mode or "plain", output], 2e-6)


def value_bound(loss, mode):
    return 4.0 * YARDSTICK[loss, mode or "plain", "value"]


def tag(shape):
    return "%dx%dx%d" % tuple(shape)


def key(loss, shape, *parts):
    """Name of a fixture array: loss, shape, then input name or mode / clamp pair / dtype / output."""
    return "_".join([loss, tag(shape)] + [str(p) for p in parts])


def weights(B):
    """The per-image weighting of the reduction=None gradients (as the ragged tests of test_loss_gpu.py)."""
    return np.linspace(0.5, 1.5, B)


def mean_gradient(g_none, B):
    """d mean-loss / d input from the weighted reduction=None gradient: both are the per-cell gradient over N, times
    weights(B)[b] there and 1 / B here."""
    w = weights(B).reshape((B,) + (1,) * (g_none.ndim - 1))
    return np.asarray(g_none, np.float64) / (w * B)


def _slots(shape):
    B, Ho, Wo = shape
    i = np.arange(Ho * Wo)[None, :]
    b = np.arange(B)[:, None]
    return ((5 * i + 3 * b) % 12).reshape(B, Ho, Wo)


def classes(loss, shape):
    """Integer class map [B,Ho,Wo] (index into CLASSES[loss]); pure integer arithmetic."""
    s = _slots(shape)
    if loss == "sem":
        return s % len(SEM_CLASSES)
    n = len(CLASSES[loss])
    c = np.where(s < n, s, 0)
    c[:-1][c[:-1] >= n - 3] = 0                          # sigma classes: last image only
    return c


def _two_sided(rng, lo, hi, size):
    return rng.uniform(lo, hi, size) * np.where(rng.uniform(size=size) < 0.5, -1.0, 1.0)


def _sigma(rng, cls, loss, err):
    """Uncertainties: regular ones a factor 0.4 - 0.8 or 1.25 - 2.5 off err / sqrt(k); then the three clamp classes."""
    n = len(CLASSES[loss])
    base = np.where(err > 0.05, err, 1.0) / np.sqrt(MLE_K[loss])
    r = np.where(rng.uniform(size=err.shape) < 0.5, rng.uniform(0.4, 0.8, err.shape), rng.uniform(1.25, 2.5, err.shape))
    s = base * r
    s = np.where(cls == n - 3, rng.uniform(1e-9, 5e-8, err.shape), s)
    s = np.where(cls == n - 2, np.exp(rng.uniform(np.log(2e-7), np.log(3e-4), err.shape)), s)
    s = np.where(cls == n - 1, rng.uniform(1e-3, 1e-2, err.shape), s)
    return s[:, None].astype(np.float32)


def _rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


# ------------------------------------------------------------------------------------------------------------- coord

def coord_intrinsics(shape):
    """(focal, cx, cy): the principal point is the centre of the SUB * Wo x SUB * Ho frame."""
    _, Ho, Wo = shape
    return FOCAL, SUB * Wo / 2.0, SUB * Ho / 2.0


def build_coord(shape, seed=11):
    B, Ho, Wo = shape
    rng = np.random.default_rng(seed + Wo)
    cls = classes("coord", shape)
    f, cx, cy = coord_intrinsics(shape)
    u = (np.arange(Wo) * SUB + SUB / 2)[None, None, :] + np.zeros((B, Ho, 1))
    v = (np.arange(Ho) * SUB + SUB / 2)[None, :, None] + np.zeros((B, 1, Wo))
    zg = rng.uniform(8.0, 30.0, (B, Ho, Wo))
    zg = np.where((cls == 5) | (cls == 6), rng.uniform(8.0, 12.0, zg.shape), zg)        # keeps their d under the tolerance
    Gc = np.stack([zg * (u - cx) / f, zg * (v - cy) / f, zg], 1)
    e = rng.uniform(2.0, 15.0, zg.shape)
    e = np.where(cls == 7, rng.uniform(25.0, 50.0, zg.shape), e)
    e = np.where(cls == 8, rng.uniform(150.0, np.minimum(600.0, 40.0 * f / zg)), e)      # lateral offset stays under 40 m
    th = rng.uniform(0, 2 * np.pi, zg.shape)
    zp = zg + _two_sided(rng, 0.1, 0.5, zg.shape)
    zp = np.where(cls == 4, zg + rng.uniform(52.0, 60.0, zg.shape), zp)                    # d > tol along the ray
    # a nodata label sits within a few metres of the camera: 60 - 70 m out is beyond the tolerance from it; the reprojection
    # gradient of a point that far is the worst conditioned of the scene, so its error is kept at 8 px or more
    zp = np.where(cls == 3, rng.uniform(60.0, 70.0, zg.shape), zp)
    e = np.where(cls == 3, rng.uniform(8.0, 15.0, zg.shape), e)
    Xc = np.stack([zp * (u + e * np.cos(th) - cx) / f, zp * (v + e * np.sin(th) - cy) / f, zp], 1)
    # behind the camera / under min_depth, and nothing else wrong: with the depth clamped to min_depth the projection still
    # lands e = 2 - 15 px from the cell centre, so only `z_cam < min_depth` makes the cell invalid
    zbad = np.where(cls == 5, -rng.uniform(0.5, 2.0, zg.shape), rng.uniform(0.02, 0.08, zg.shape))
    off = ((cls == 5) | (cls == 6))[:, None]
    Xc = np.where(off, np.stack([(MIN_DEPTH * (u + e * np.cos(th)) - cx * zbad) / f,
                                 (MIN_DEPTH * (v + e * np.sin(th)) - cy * zbad) / f, zbad], 1), Xc)
    d = np.linalg.norm(Xc - Gc, axis=1)
    poses = np.zeros((B, 4, 4))
    for b in range(B):
        poses[b, :3, :3] = _rodrigues(rng.uniform(-0.2, 0.2, 3))
        poses[b, :3, 3] = rng.uniform(-3.0, 3.0, 3)
        poses[b, 3, 3] = 1.0
    X = np.einsum("bij,bjhw->bihw", poses[:, :3, :3], Xc) + poses[:, :3, 3, None, None]
    G = np.einsum("bij,bjhw->bihw", poses[:, :3, :3], Gc) + poses[:, :3, 3, None, None]
    G = np.where(((cls == 1) | (cls == 3))[:, None], NODATA, G)
    one = (np.arange(Ho * Wo).reshape(1, 1, Ho, Wo) % 3 == np.arange(3).reshape(1, 3, 1, 1)) & (cls == 2)[:, None]
    G = np.where(one, NODATA, G)
    return dict(pred=X.astype(np.float32), unc=_sigma(rng, cls, "coord", d), gt=G.astype(np.float32),
                poses=poses.astype(np.float32))


def coord_census(inp, soft, hard):
    """float64 evaluation of every deciding quantity of loss/coord.py:87-188 on the fp32 inputs."""
    X, G, S = (inp[k].astype(np.float64) for k in ("pred", "gt", "unc"))
    B, _, Ho, Wo = X.shape
    f, cx, cy = coord_intrinsics((B, Ho, Wo))
    P = np.linalg.inv(inp["poses"].astype(np.float64))[:, :3]
    Xc = np.einsum("bij,bjhw->bihw", P[:, :, :3], X) + P[:, :, 3, None, None]
    Gc = np.einsum("bij,bjhw->bihw", P[:, :, :3], G) + P[:, :, 3, None, None]
    d = np.linalg.norm(Xc - Gc, axis=1)
    zt = np.maximum(Xc[:, 2], MIN_DEPTH)
    ru = (f * Xc[:, 0] + cx * Xc[:, 2]) / zt - (np.arange(Wo) * SUB + SUB / 2)[None, None, :]
    rv = (f * Xc[:, 1] + cy * Xc[:, 2]) / zt - (np.arange(Ho) * SUB + SUB / 2)[None, :, None]
    e = np.maximum(np.sqrt(ru * ru + rv * rv), 1e-7)
    g = (inp["gt"] != NODATA).all(1)
    valid = ~(Xc[:, 2] < MIN_DEPTH) & ~(e > hard) & ~((d > TOL) & g)
    return dict(zc=Xc[:, 2], d=d, e=e, g=g, nodata_channels=(inp["gt"] == NODATA).sum(1), valid=valid, sigma=S[:, 0],
                err2=d * d, count=int(valid.sum()))


def _away(x, thr, where=None):
    """x is at least MARGIN (relative) away from thr wherever it decides."""
    ok = np.abs(x - thr) >= MARGIN * abs(thr)
    return bool(ok.all() if where is None else ok[where].all())


def _populated(cls, names):
    """Every class has MIN_CELLS cells in every image it lives in, and a cell in each of that image's 256-cell workgroups."""
    B = cls.shape[0]
    flat = cls.reshape(B, -1)
    for c, name in enumerate(names):
        sig = name.startswith("sigma_")
        if sig:
            assert not (cls[:-1] == c).any(), name
        for b in ([B - 1] if sig else range(B)):
            assert (flat[b] == c).sum() >= MIN_CELLS, (name, b, int((flat[b] == c).sum()))
            for k in range(0, flat.shape[1], 256):
                assert (flat[b, k:k + 256] == c).any(), (name, b, k)


def _check_sigma(s, cls, n):
    assert _away(s, SIG_CLAMP) and _away(s * s, SIG_CLAMP)
    assert (s[cls == n - 3] < SIG_CLAMP).all()
    mid = s[cls == n - 2]
    assert ((mid > SIG_CLAMP) & (mid * mid < SIG_CLAMP)).all()
    small = s[cls == n - 1]
    assert ((small > 1e-3) & (small < 1e-2)).all()
    assert (s[cls < n - 3] ** 2 > SIG_CLAMP).all()


def check_coord_census(inp, cls):
    """The conditions of the scene, asserted in float64 before any result is compared.  Returns the census per clamp pair."""
    _populated(cls, COORD_CLASSES)
    out = []
    for soft, hard in COORD_CLAMPS:
        c = coord_census(inp, soft, hard)
        front = c["zc"] >= MIN_DEPTH
        assert _away(c["zc"], MIN_DEPTH) and _away(c["d"], TOL, c["g"])
        assert _away(c["e"], soft) and _away(c["e"], hard)
        alone = (cls == 5) | (cls == 6)                          # the depth test alone makes these cells invalid
        assert (~front & ~(c["e"] > hard) & ~((c["d"] > TOL) & c["g"]) & c["g"] & ~c["valid"])[alone].all()
        assert front[~alone].all()
        out.append(c)
    c, t = out                                               # reference clamps (100, 1000), tight clamps (20, 60)
    _check_sigma(c["sigma"], cls, len(COORD_CLASSES))
    is_ = lambda k: cls == k
    reg = is_(0) | (cls >= 9)
    assert ((c["e"][reg] >= 2) & (c["e"][reg] <= 15) & (c["d"][reg] >= 0.05) & c["g"][reg] & t["valid"][reg]).all()
    assert (c["nodata_channels"][is_(1)] == 3).all() and t["valid"][is_(1)].all()
    assert (c["nodata_channels"][is_(2)] == 1).all() and t["valid"][is_(2)].all()
    assert (c["nodata_channels"][~(is_(1) | is_(2) | is_(3))] == 0).all()
    assert (~c["g"][is_(3)] & (c["d"][is_(3)] > TOL) & t["valid"][is_(3)]).all()
    assert (c["g"][is_(4)] & (c["d"][is_(4)] > TOL) & ~c["valid"][is_(4)] & (t["e"][is_(4)] < 20)).all()
    assert (c["zc"][is_(5)] < 0).all() and not c["valid"][is_(5)].any()
    assert ((c["zc"][is_(6)] > 0) & (c["zc"][is_(6)] < MIN_DEPTH)).all() and not c["valid"][is_(6)].any()
    assert ((t["e"][is_(7)] > 20) & (t["e"][is_(7)] < 60) & t["valid"][is_(7)] & (c["e"][is_(7)] < 100)).all()
    assert ((t["e"][is_(8)] > 60) & ~t["valid"][is_(8)]).all()
    assert ((c["e"][is_(8)] > 100) & (c["e"][is_(8)] < 1000) & c["valid"][is_(8)]).all()
    return out


# ------------------------------------------------------------------------------------------------------------- depth

def build_depth(shape, seed=23):
    B, Ho, Wo = shape
    rng = np.random.default_rng(seed + Wo)
    cls = classes("depth", shape)
    gd = rng.uniform(8.0, 30.0, cls.shape).astype(np.float32)
    gd = np.where((cls == 2) | (cls == 3), rng.uniform(2.0, 6.0, cls.shape).astype(np.float32), gd)    # err stays under hard
    pd = (gd + _two_sided(rng, 0.05, 2.0, cls.shape)).astype(np.float32)
    pd = np.where((cls == 2) | (cls == 7), np.float32(0.05), pd)
    pd = np.where(cls == 3, -rng.uniform(0.5, 3.0, cls.shape), pd).astype(np.float32)
    pd = np.where(cls == 4, gd + rng.uniform(12.0, 20.0, cls.shape), pd).astype(np.float32)
    pd = np.where(cls == 5, gd, pd)
    pd = np.where(cls == 6, gd + np.float32(1e-5), pd).astype(np.float32)
    err = np.abs(pd.astype(np.float64) - gd)
    gd = np.where((cls == 1) | (cls == 7), np.float32(NODATA), gd)
    return dict(pred=pd[:, None], unc=_sigma(rng, cls, "depth", err), gt=gd[:, None].astype(np.float32))


def depth_census(inp):
    D, G, S = (inp[k].astype(np.float64)[:, 0] for k in ("pred", "gt", "unc"))
    err = np.abs(D - G)
    g = inp["gt"][:, 0] != NODATA
    valid = ~(D < MIN_DEPTH) & ~(err > DEPTH_HARD) & g
    return dict(pred=D, err=err, g=g, valid=valid, sigma=S, err2=err * err, count=int(valid.sum()),
                equal=inp["pred"][:, 0] == inp["gt"][:, 0])


def check_depth_census(inp, cls):
    _populated(cls, DEPTH_CLASSES)
    c = depth_census(inp)
    assert _away(c["pred"], MIN_DEPTH) and _away(c["err"], DEPTH_HARD, c["g"])
    _check_sigma(c["sigma"], cls, len(DEPTH_CLASSES))
    is_ = lambda k: cls == k
    reg = is_(0) | (cls >= 8)
    assert (c["valid"][reg] & (c["err"][reg] >= 0.04) & (c["err2"][reg] > SIG_CLAMP)).all()
    assert (~c["g"][is_(1)] & (c["pred"][is_(1)] > MIN_DEPTH)).all()
    for k in (2, 3):
        assert (c["g"][is_(k)] & (c["pred"][is_(k)] < MIN_DEPTH) & (c["err"][is_(k)] < DEPTH_HARD) & ~c["valid"][is_(k)]).all()
    assert (c["pred"][is_(3)] < 0).all()
    assert (c["g"][is_(4)] & (c["err"][is_(4)] > DEPTH_HARD) & (c["pred"][is_(4)] > MIN_DEPTH)).all()
    assert c["equal"][is_(5)].all() and c["valid"][is_(5)].all() and not c["equal"][~is_(5)].any()
    assert ((c["err"][is_(6)] > 0) & (c["err2"][is_(6)] < (1 - MARGIN) * SIG_CLAMP) & c["valid"][is_(6)]).all()
    assert (~c["g"][is_(7)] & (c["pred"][is_(7)] < MIN_DEPTH)).all()
    assert _away(c["err2"], SIG_CLAMP, ~c["equal"])
    return c


# ------------------------------------------------------------------------------------------------------------ normal

def _to_logit(angle):
    p = (angle / np.pi + 1.0) / 2.0
    return np.log(p / (1.0 - p))


def build_normal(shape, seed=37):
    B, Ho, Wo = shape
    rng = np.random.default_rng(seed + Wo)
    cls = classes("normal", shape)
    azg = _two_sided(rng, 0.2, 2.9, cls.shape)
    elg = rng.uniform(-1.2, 1.2, cls.shape)
    az = azg + _two_sided(rng, 0.03, 0.06, cls.shape)
    el = elg + _two_sided(rng, 0.036, 0.06, cls.shape)          # 2.06 degrees by elevation alone, 4.9 with the azimuth's
    az = np.where(cls == 1, azg - np.sign(azg) * rng.uniform(1.0, 2.5, cls.shape), az)
    azw = _two_sided(rng, 2.0, 2.7, cls.shape)
    azg = np.where(cls == 2, azw, azg)
    az = np.where(cls == 2, -np.sign(azw) * rng.uniform(2.0, 2.7, cls.shape), az)
    up = cls == 5
    az = np.where(up, _two_sided(rng, 0.03, 0.06, cls.shape), az)
    el = np.where(up, np.pi / 2 - rng.uniform(0.036, 0.06, cls.shape), el)
    gn = np.stack([np.cos(azg) * np.cos(elg), np.sin(azg) * np.cos(elg), np.sin(elg)], 1)
    gn = np.where(up[:, None], np.array([0.0, 0.0, 1.0]).reshape(1, 3, 1, 1), gn)
    gn = np.where((cls == 6)[:, None], np.array([0.0, 0.0, -1.0]).reshape(1, 3, 1, 1), gn)
    gn = np.where((cls == 7)[:, None], NODATA, gn)
    logits = np.stack([_to_logit(az), _to_logit(el)], 1)
    i = np.arange(Ho * Wo).reshape(1, Ho, Wo)
    logits[:, 0] = np.where(cls == 3, np.where(i % 2 == 0, 25.0, -25.0), logits[:, 0])
    logits[:, 1] = np.where(cls == 4, -40.0, logits[:, 1])
    inp = dict(logits=logits.astype(np.float32), gt=gn.astype(np.float32))
    inp["unc"] = np.ones((B, 1, Ho, Wo), np.float32)
    inp["unc"] = _sigma(rng, cls, "normal", normal_census(inp)["E"])
    return inp


def normal_census(inp):
    L, G, S = (inp[k].astype(np.float64) for k in ("logits", "gt", "unc"))
    sg = 1.0 / (1.0 + np.exp(-L))
    inside = (sg >= 1e-7) & (sg <= 1 - 1e-7)
    ae = (np.clip(sg, 1e-7, 1 - 1e-7) * 2 - 1.0) * np.pi
    az, el = ae[:, 0], ae[:, 1]
    azg = np.arctan2(G[:, 1], G[:, 0])
    elg = np.arctan2(G[:, 2], np.sqrt(G[:, 0] ** 2 + G[:, 1] ** 2))
    dlt = np.abs(azg - az)
    E = np.maximum(2.0 * np.abs(np.minimum(dlt, 2 * np.pi - dlt)) + np.abs(el - elg), 1e-7)
    n = np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], 1)
    cs = (n * G).sum(1) / (np.maximum(np.linalg.norm(n, axis=1), 1e-8) * np.maximum(np.linalg.norm(G, axis=1), 1e-8))
    ang = np.degrees(np.arccos(np.clip(cs, -1 + 1e-7, 1 - 1e-7)))
    g = (inp["gt"] != NODATA).all(1)
    valid = ~(ang > NORMAL_HARD) & g
    return dict(az=az, el=el, azg=azg, elg=elg, dlt=dlt, E=E, angle=ang, g=g, valid=valid, inside=inside, sigma=S[:, 0],
                err2=E * E, count=int(valid.sum()), logits=L)


def check_normal_census(inp, cls):
    _populated(cls, NORMAL_CLASSES)
    c = normal_census(inp)
    g = c["g"]
    assert _away(c["angle"], NORMAL_HARD, g) and _away(c["dlt"], np.pi, g)
    assert _away(np.abs(c["logits"]), 16.0)                    # sigmoid leaves [1e-7, 1 - 1e-7] at |logit| = 16.1
    assert (np.abs(c["azg"] - c["az"])[g] >= 0.02).all() and (np.abs(c["el"] - c["elg"])[g] >= 0.02).all()    # off the |x| kinks
    assert (c["err2"][g] > SIG_CLAMP).all()
    _check_sigma(c["sigma"], cls, len(NORMAL_CLASSES))
    is_ = lambda k: cls == k
    reg = is_(0) | (cls >= 8)
    assert (c["valid"][reg] & (c["angle"][reg] > 2.0) & (c["angle"][reg] < 5.0) & c["inside"].all(1)[reg]).all()
    assert (g[is_(1)] & (c["dlt"][is_(1)] > 0.99) & (c["dlt"][is_(1)] < np.pi) & ~c["valid"][is_(1)]).all()
    assert (g[is_(2)] & (c["dlt"][is_(2)] > np.pi) & ~c["valid"][is_(2)]).all()
    assert (g[is_(3)] & ~c["inside"][:, 0][is_(3)] & c["inside"][:, 1][is_(3)]).all()
    assert (g[is_(4)] & c["inside"][:, 0][is_(4)] & ~c["inside"][:, 1][is_(4)]).all()
    assert c["inside"][:, 0][~is_(3)].all() and c["inside"][:, 1][~is_(4)].all()
    assert (inp["gt"].transpose(0, 2, 3, 1)[is_(5)] == np.array([0, 0, 1], np.float32)).all() and c["valid"][is_(5)].all()
    assert (inp["gt"].transpose(0, 2, 3, 1)[is_(6)] == np.array([0, 0, -1], np.float32)).all() and not g[is_(6)].any()
    assert (inp["gt"].transpose(0, 2, 3, 1)[is_(7)] == NODATA).all() and not g[is_(7)].any()
    assert g[~(is_(6) | is_(7))].all()
    return c


# --------------------------------------------------------------------------------------------------------- semantics

SEM_CHANNELS = [6, 3]


def build_sem(shape, C, seed=53):
    B, Ho, Wo = shape
    rng = np.random.default_rng(seed + Wo + C)
    cls = classes("sem", shape)
    lg = rng.normal(0, 2.0, (B, C, Ho, Wo))
    lab = rng.integers(0, C, cls.shape)
    ch = np.arange(C).reshape(1, C, 1, 1)
    first = rng.integers(0, C - 1, cls.shape)                  # two equal maxima at first < second
    second = first + 1 + rng.integers(0, C, cls.shape) % (C - 1 - first)
    tie = ((cls == 1) | (cls == 2))[:, None]
    low = rng.uniform(-3.0, 0.0, lg.shape)
    lg = np.where(tie, np.where((ch == first[:, None]) | (ch == second[:, None]), 1.5, low), lg)
    lab = np.where(cls == 1, first, np.where(cls == 2, second, lab))
    top = rng.integers(0, C, cls.shape)
    sat = ((cls == 3) | (cls == 4))[:, None]
    lg = np.where(sat, np.where(ch == top[:, None], 80.0, -80.0), lg)
    lab = np.where(cls == 3, top, np.where(cls == 4, (top + 1 + rng.integers(0, C - 1, cls.shape)) % C, lab))
    dom = (cls == 5)[:, None]
    low_max = np.where(ch == top[:, None], -np.inf, low).max(1)
    lg = np.where(dom, np.where(ch == top[:, None], (low_max + rng.uniform(2.0, 4.99, cls.shape))[:, None], low), lg)
    lab = np.where(cls == 6, -100, lab)
    return dict(logits=lg.astype(np.float32), labels=lab[:, None].astype(np.float32))


def sem_census(inp):
    L = inp["logits"].astype(np.float64)
    lab = inp["labels"][:, 0].astype(np.int64)
    top = L.max(1)
    arg = L.argmax(1)                                          # first maximum
    n_top = (L == top[:, None]).sum(1)
    srt = np.sort(L, 1)
    return dict(lab=lab, arg=arg, n_top=n_top, margin=srt[:, -1] - srt[:, -2], count=int((arg == lab).sum()),
                top=top, low=srt[:, 0])


def check_sem_census(inp, cls):
    B = cls.shape[0]
    for c, name in enumerate(SEM_CLASSES):
        for b in range(B):
            assert (cls[b] == c).sum() >= MIN_CELLS, (name, b)
    c = sem_census(inp)
    C = inp["logits"].shape[1]
    is_ = lambda k: cls == k
    assert ((c["lab"] >= 0) & (c["lab"] < C))[~is_(6)].all() and (c["lab"][is_(6)] == -100).all()
    for k in (1, 2):
        assert ((c["n_top"][is_(k)] == 2) & (c["margin"][is_(k)] == 0)).all()
    assert (c["arg"][is_(1)] == c["lab"][is_(1)]).all()
    assert (c["arg"][is_(2)] < c["lab"][is_(2)]).all()
    assert (inp["logits"].transpose(0, 2, 3, 1)[is_(2)][np.arange(is_(2).sum()), c["lab"][is_(2)]] == c["top"][is_(2)]).all()
    assert (c["n_top"][~(is_(1) | is_(2))] == 1).all()
    assert (c["margin"][~(is_(1) | is_(2))] > 1e-4).all()       # no accidental near-tie: arg-max is the same in fp32
    for k in (3, 4):
        assert ((c["top"][is_(k)] == 80) & (c["low"][is_(k)] == -80)).all()
    assert (c["arg"][is_(3)] == c["lab"][is_(3)]).all() and (c["arg"][is_(4)] != c["lab"][is_(4)]).all()
    assert ((c["margin"][is_(5)] >= 1.99) & (c["margin"][is_(5)] <= 5.0)).all()
    return c


BUILD = {"coord": build_coord, "depth": build_depth, "normal": build_normal}
INPUTS = {"coord": ("pred", "unc", "gt", "poses"), "depth": ("pred", "unc", "gt"), "normal": ("logits", "unc", "gt"),
          "sem6": ("logits", "labels"), "sem3": ("logits", "labels")}
CHECK = {"coord": check_coord_census, "depth": check_depth_census, "normal": check_normal_census}


def load_inputs(fixture, loss, shape):
    return {k: fixture[key(loss, shape, k)] for k in INPUTS[loss]}


def run_tag(loss, mode, clamp=0):
    """Fixture name part of one run of the reference: mode, and for coord the clamp pair."""
    m = mode or "plain"
    return "%s_c%d" % (m, clamp) if loss == "coord" else m


def pack_clamp_runs(arrays):
    """Gradients of the coord runs under the second clamp pair differ from the first pair's only where the clamps decide
    (the uncertainty gradient nowhere): the fixture keeps the cells that differ (<name>_cells: flat indices over [B,Ho,Wo],
    <name>_values: [n,C]) in place of the whole array.  In place, on the dict make_golden.py is about to save."""
    for k in [k for k in arrays if "_c1_" in k and k.endswith(("_dpred", "_dunc"))]:
        g1, g0 = arrays.pop(k), arrays[k.replace("_c1_", "_c0_")]
        C = g1.shape[1]
        cells = np.flatnonzero((g1 != g0).any(1))
        arrays[k + "_cells"] = cells.astype(np.int32)
        arrays[k + "_values"] = g1.transpose(0, 2, 3, 1).reshape(-1, C)[cells]


def stored(fixture, loss, shape, mode, clamp, dtype, what):
    """One recorded array of a run (dtype "f32" / "f64"; what: loss_none, loss_mean, rate, dpred, dunc), unpacked."""
    k = key(loss, shape, run_tag(loss, mode, clamp), dtype, what)
    if k in fixture.files:
        return fixture[k]
    base = fixture[key(loss, shape, run_tag(loss, mode, 0), dtype, what)]
    B, C, Ho, Wo = base.shape
    flat = np.ascontiguousarray(base.transpose(0, 2, 3, 1)).reshape(-1, C)
    flat[fixture[k + "_cells"]] = fixture[k + "_values"]
    return flat.reshape(B, Ho, Wo, C).transpose(0, 3, 1, 2)


# -------------------------------------------------------------------------------------------------------- comparator

def cell_errors(got, truth):
    """Per-cell scaled error [B,Ho,Wo] of a gradient [B,C,Ho,Wo] against the float64 truth: largest channel difference over
    the largest |truth| of the cell's channels; inf where an exactly-zero element of the truth is not exactly zero, or where
    the result is not finite."""
    got, truth = np.asarray(got, np.float64), np.asarray(truth, np.float64)
    assert got.shape == truth.shape and got.ndim == 4
    scale = np.abs(truth).max(1)
    with np.errstate(invalid="ignore"):
        diff = np.abs(got - truth).max(1)
    err = np.zeros(scale.shape)
    nz = scale > 0
    err[nz] = diff[nz] / scale[nz]
    err[((truth == 0) & (got != 0)).any(1) | ~np.isfinite(got).all(1)] = np.inf
    return err


def compare(got, truth, bound, cls, names, class_bounds=None):
    """(ok, worst): ok iff every cell's scaled error is within `bound` (class_bounds: {class name: its own bound});
    worst: {class name: largest error of its cells}, for the failure message."""
    err = cell_errors(got, truth)
    lim = np.full(err.shape, float(bound))
    for name, b in (class_bounds or {}).items():
        lim[cls == names.index(name)] = b
    worst = {names[c]: float(err[cls == c].max()) for c in np.unique(cls)}
    return bool((err <= lim).all()), worst


def report(what, bound, worst):
    return "%s: bound %.2e; worst per-cell scaled error by class: %s" % (
        what, bound, ", ".join("%s %.2e%s" % (n, e, " <--" if e > bound else "") for n, e in worst.items()))


def unguarded_dunc(loss, err2, sigma, weight_over_n):
    """d loss / d sigma WITHOUT the `sigma^2 >= 1e-7` guard of the kernels (what a kernel that forgot the zero derivative of
    the clamp would write), for the comparator's self-test.  Valid where sigma >= 1e-7 and the label is valid."""
    s2c = np.maximum(sigma * sigma, SIG_CLAMP)
    return weight_over_n * (MLE_K[loss] / sigma - np.maximum(err2, SIG_CLAMP) / (s2c * sigma))


# --------------------------------------------------------------------------------------------------------- yardstick

def runs(loss):
    """(mode, clamp pair index) of every run of the reference on a scene of `loss`."""
    return [(m, c) for m in MODES for c in range(len(COORD_CLAMPS) if loss == "coord" else 1)]


def measured_yardstick(fixture):
    """The table of the module docstring, recomputed from the fixture's fp32 and float64 arrays."""
    out = {}
    for loss in ("coord", "depth", "normal"):
        for mode, clamp in runs(loss):
            m = mode or "plain"
            for shape in SHAPES:
                for output in ("dpred", "dunc") if mode else ("dpred",):
                    e = cell_errors(stored(fixture, loss, shape, mode, clamp, "f32", output),
                                    stored(fixture, loss, shape, mode, clamp, "f64", output)).max()
                    out[loss, m, output] = max(out.get((loss, m, output), 0.0), float(e))
                for v in ("loss_none", "loss_mean"):
                    a, b = (np.atleast_1d(stored(fixture, loss, shape, mode, clamp, dt, v)) for dt in ("f32", "f64"))
                    out[loss, m, "value"] = max(out.get((loss, m, "value"), 0.0), float((np.abs(a - b) / np.abs(b)).max()))
    return out
