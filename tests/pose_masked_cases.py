"""Inputs shared by tests/test_pose_masked_cpu.py, tests/test_pose_quality_masked_gpu.py and tests/test_pose_refine_masked_gpu.py:
the grids, the three masks of a batch, the frames of the substitution identity and the bitwise comparisons."""
import numpy as np

from pose_quality_cases import same_bits                                   # noqa: F401  (shared helper)
from crossloc_amd import synth

THR, MAX_REPROJ, SUB, ALPHA = 10.0, 100.0, 8, 100.0
GRIDS = ((8, 12), (9, 13), (24, 36))         # 96 cells; 117, odd with a ragged last stride; 864: threads own up to four cells
MAX_GRID = (48, 211)                         # 10128 cells = REFINE_MAX_CELLS: the per-thread word uses bit 39
SUBST_SEEDS = tuple(range(6))
POISON = (np.nan, np.inf, -np.inf, 1e30)


def quality_args(sc):
    """(thr, focal, ppx, ppy, alpha, max_reproj, sub): the positional tail of pose_quality_batch and of its restatements"""
    return (THR, sc["focal"], sc["ppx"], sc["ppy"], ALPHA, MAX_REPROJ, SUB)


def refine_args(sc):
    """(thr, focal, ppx, ppy, max_reproj, sub): the positional tail of refine_pose_batch and of its restatements"""
    return (THR, sc["focal"], sc["ppx"], sc["ppy"], MAX_REPROJ, SUB)


def half_mask(seed, Ho, Wo):
    """The seeded 50 % mask: every cell usable with probability 1/2"""
    return (np.random.default_rng([seed, 0x4d41]).random((Ho, Wo)) < 0.5).astype(np.uint8)


def moved(pose_c2w, seed, sd=0.3):
    """`pose_c2w` with its translation moved by N(0, sd metres) per axis (float32 4x4, what the passes read)"""
    T = np.array(pose_c2w, np.float64)
    T[:3, 3] += np.random.default_rng([seed, 0x4d50]).normal(0.0, sd, size=3)
    return T.astype(np.float32)


def hetero_frame(seed, Ho, Wo):
    """A heteroscedastic frame with its seeded 50 % mask and its start pose"""
    sc = synth.make_hetero_scene(seed, Ho=Ho, Wo=Wo)
    return dict(sc, mask=half_mask(seed, Ho, Wo), start=moved(sc["pose"], seed))


def batch(seed0, Ho, Wo):
    """The batch of three of the GPU tests: an all-ones mask and a seeded 50 % mask on heteroscedastic frames, and a
    synth.make_decoy_scene band (its own mask; sigma 0.5 m everywhere).  -> dict of stacked numpy arrays + `args` per pass"""
    a, b = hetero_frame(seed0, Ho, Wo), hetero_frame(seed0 + 1, Ho, Wo)
    a["mask"] = np.ones((Ho, Wo), np.uint8)
    d = synth.make_decoy_scene(seed0 + 2, decoy=0.6, Ho=Ho, Wo=Wo)
    d = dict(d, sigma=np.full((Ho, Wo), 0.5, np.float32), start=moved(d["pose"], seed0 + 2))
    frames = [a, b, d]
    return dict(coords=np.stack([f["coords"] for f in frames]), sigma=np.stack([f["sigma"] for f in frames]),
                mask=np.stack([f["mask"] for f in frames]), poses=np.stack([f["start"] for f in frames]),
                qargs=quality_args(a), rargs=refine_args(a))


def substituted(fr):
    """The frame of the substitution identity: the coordinates of every masked-out cell replaced by the point 10 km from the
    camera centre, 45 degrees off the optical axis of the ground-truth pose, C + R (1e4, 0, 1e4); sigma finite (1 m) there.
    -> (coords, sigma)"""
    P = np.asarray(fr["pose"], np.float64)
    far = P[:3, 3] + P[:3, :3] @ np.array([1e4, 0.0, 1e4])
    out = fr["mask"] == 0
    coords, sigma = fr["coords"].copy(), fr["sigma"].copy()
    coords[:, out] = far.astype(np.float32)[:, None]
    sigma[out] = 1.0
    return coords, sigma


def poisoned(coords, sigma, mask, value):
    """Copies of coords [..,3,Ho,Wo] and sigma [..,Ho,Wo] with `value` stored at every masked-out cell"""
    out = np.asarray(mask) == 0
    c, s = coords.copy(), sigma.copy()
    np.moveaxis(c, -3, 0)[:, out] = value
    s[out] = value
    return c, s


def same_pose_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def same_refine(got, want, skip=()):
    """(pose, row, w2c) against (pose, row, w2c), bit for bit; `skip`: row columns left out"""
    keep = np.ones(64, bool)
    keep[list(skip)] = False
    return (same_pose_bits(got[0], want[0]) and same_bits(np.asarray(got[1])[keep], np.asarray(want[1])[keep])
            and same_bits(got[2], want[2]))


def same_row(got, want, skip=()):
    keep = np.ones(64, bool)
    keep[list(skip)] = False
    return same_bits(np.asarray(got)[keep], np.asarray(want)[keep])
