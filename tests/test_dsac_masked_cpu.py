"""CPU checks of the masked RGB DSAC* solver through its serial restatement tests/dsac_masked_ref.c (which the GPU kernel must
match bit for bit, tests/test_dsac_masked_gpu.py): the restatement against the pinned oracle under an all-ones mask (identity
A), poisoned masked cells (identity B), decoy frames with and without the mask, dead images, exhausted hypotheses, a sanitizer
run of the restatement as a program of its own, and the argument validation of the C entry point.  No GPU."""
import ctypes
import subprocess

import numpy as np
import pytest

import dsac_masked_ref
from crossloc_amd import synth

GRIDS = [(8, 12), (9, 13), (24, 36)]
THR, ALPHA, MAX_REPROJ, SUB = 10.0, 100.0, 100.0, 8
FIELDS = ("cells", "tries", "scores", "winner", "rounds", "inliers", "lm_evals", "pose0", "pose1", "pose")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return dsac_masked_ref.load(tmp_path_factory.mktemp("dsac_masked_ref"))


def _scene(seed, Ho, Wo, **kw):
    return synth.make_scene(seed, Ho=Ho, Wo=Wo, **kw)


def _run(ref, sc, mask, n_hyp, coords=None, **kw):
    return ref.forward(sc["coords"] if coords is None else coords, mask, n_hyp, THR, sc["focal"], sc["ppx"], sc["ppy"], ALPHA,
                       MAX_REPROJ, SUB, **kw)


def _same(a, b, fields=FIELDS, what=""):
    for k in fields:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert x.tobytes() == y.tobytes(), (what, k)


def _seeded_mask(seed, Ho, Wo, usable):
    return (np.random.default_rng([seed, 0x4d41]).random((Ho, Wo)) < usable).astype(np.uint8)


@pytest.mark.parametrize("Ho,Wo", GRIDS)
def test_all_ones_mask_equals_the_pinned_oracle(ref, oracle, Ho, Wo):
    """identity A on the CPU: ties the new restatement to oracle/dsac_oracle.c"""
    for seed, n_hyp in ((3, 6), (4, 16)):
        sc = _scene(seed, Ho, Wo)
        pose, dbg = oracle.forward_rgb(sc["coords"], n_hyp, THR, sc["focal"], sc["ppx"], sc["ppy"], ALPHA, MAX_REPROJ, SUB,
                                       image=seed, debug=True)
        dbg["pose"] = pose
        got = _run(ref, sc, np.ones((Ho, Wo), np.uint8), n_hyp, image=seed)
        assert got["status"] == 0
        for k in ("winner", "rounds", "inliers", "lm_evals"):
            assert got[k] == dbg[k], k
        _same(got, dbg, ("cells", "tries", "scores", "pose0", "pose1", "pose"), (Ho, Wo, seed))


@pytest.mark.parametrize("Ho,Wo", GRIDS)
def test_masked_cell_values_influence_no_output_bit(ref, Ho, Wo):
    """identity B: NaN, +Inf and 1e30 at the masked-out cells"""
    sc = _scene(5, Ho, Wo)
    mask = _seeded_mask(5, Ho, Wo, 0.5)
    want = _run(ref, sc, mask, 8, image=5)
    assert want["status"] == 0
    for poison in (np.nan, np.inf, 1e30):
        co = sc["coords"].copy()
        co[:, mask == 0] = poison
        _same(_run(ref, sc, mask, 8, coords=co, image=5), want, what=poison)


def _t_err(pose_a, pose_b):
    return float(np.linalg.norm(np.asarray(pose_a, np.float64)[:3, 3] - np.asarray(pose_b, np.float64)[:3, 3]))


@pytest.mark.parametrize("Ho,Wo", [(24, 36), (12, 16)])
def test_decoy_frames_need_the_mask(ref, oracle, Ho, Wo):
    """60 % of the rows hold the exact view of a second camera: the unmasked solver returns that camera's pose, the masked one
    the true pose.  Observed at the time of writing (translation error against the true pose, 12 seeds): see README.md."""
    for seed in range(12):
        sc = synth.make_decoy_scene(seed, decoy=0.6, Ho=Ho, Wo=Wo)
        plain = oracle.forward_rgb(sc["coords"], 64, THR, sc["focal"], sc["ppx"], sc["ppy"], ALPHA, MAX_REPROJ, SUB, image=seed)
        got = _run(ref, sc, sc["mask"], 64, image=seed)
        e_plain, e_masked = _t_err(plain, sc["pose"]), _t_err(got["pose"], sc["pose"])
        print("decoy %dx%d seed %d: unmasked %.2f m from the truth, %.3f m from the decoy; masked %.3f m from the truth"
              % (Ho, Wo, seed, e_plain, _t_err(plain, sc["decoy_pose"]), e_masked))
        assert _t_err(plain, sc["decoy_pose"]) < 1.0, seed
        assert e_masked < 0.1 * e_plain, seed


@pytest.mark.parametrize("n_usable", [3, 0])
def test_fewer_than_four_usable_cells(ref, n_usable):
    Ho, Wo, n_hyp = 9, 13, 6
    sc = _scene(6, Ho, Wo)
    mask = np.zeros((Ho, Wo), np.uint8)
    mask.reshape(-1)[[5, 40, 116][:n_usable]] = 1
    got = _run(ref, sc, mask, n_hyp, image=6)
    assert got["status"] == 1
    assert np.array_equal(got["pose"], np.eye(4, dtype=np.float32))
    assert (got["tries"] == 0).all() and (got["scores"] == 0).all() and (got["cells"] == -1).all() and got["winner"] == -1
    ident = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    assert np.array_equal(got["pose0"], ident) and np.array_equal(got["pose1"], ident)
    assert (got["rounds"], got["inliers"], got["lm_evals"]) == (0, 0, 0)


def test_exhausted_hypotheses_follow_the_rule(ref, oracle):
    """10 % usable, 64 tries: a hypothesis without an accepted try is its last try's result - the identity pose where the mask
    rejected that try - and scores like any other."""
    Ho, Wo, n_hyp, max_tries = 24, 36, 16, 64
    sc = _scene(7, Ho, Wo)
    mask = _seeded_mask(7, Ho, Wo, 0.1)
    got = _run(ref, sc, mask, n_hyp, image=7, max_tries=max_tries)
    assert got["status"] == 0
    exhausted = np.flatnonzero(got["tries"] < 0)
    assert exhausted.size > 0, "the case must exhaust at least one hypothesis"
    assert (got["tries"][exhausted] == -max_tries).all()
    flat = mask.reshape(-1)
    ident = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    n_rejected = 0
    for h in exhausted:
        draws = oracle.draws(1305, 7, int(h), max_tries - 1, Wo, Ho)                  # the last try's (x, y) pairs
        cells = draws[:, 1] * Wo + draws[:, 0]
        assert np.array_equal(got["cells"][h], cells.astype(np.int32))
        if not flat[cells].all():
            # rejected by the mask: the identity pose, whose score over the usable cells the oracle's score restates
            n_rejected += 1
            assert got["scores"][h] == _score_usable(oracle, sc["coords"], mask, ident, sc)
    assert n_rejected > 0
    for h in np.flatnonzero(got["tries"] > 0):
        assert flat[got["cells"][h]].all()                                             # an accepted try drew usable cells only
    if got["winner"] in exhausted and not flat[got["cells"][got["winner"]]].all():
        assert np.array_equal(got["pose0"], ident)


def _score_usable(oracle, coords, mask, pose12, sc):
    """the soft-inlier score of `pose12` over the usable cells, restated in numpy with the types of xl_dsac_math.h (float32 pixel,
    clamp and sigmoid argument, float64 elsewhere, the oracle's deterministic exp): lane l sums cells l, l + 64, ..., then the
    xor butterfly and the factor alpha / Wo / Ho in float32"""
    Ho, Wo = mask.shape
    flat = mask.reshape(-1)
    f32 = np.float32
    fac = f32(ALPHA) / f32(Wo) / f32(Ho)
    beta = f32(5.0) / f32(THR)
    co = coords.reshape(3, -1).astype(np.float64)
    R, t = pose12[:9], pose12[9:]
    part = np.zeros(64)
    for i in np.flatnonzero(flat):
        y, x = divmod(int(i), Wo)
        X, Y, Z = co[:, i]
        xc = R[0] * X + R[1] * Y + R[2] * Z + t[0]
        yc = R[3] * X + R[4] * Y + R[5] * Z + t[1]
        zc = R[6] * X + R[7] * Y + R[8] * Z + t[2]
        z = 1.0 / zc if zc != 0.0 else 1.0
        u, v = f32(xc * z * sc["focal"] + sc["ppx"]), f32(yc * z * sc["focal"] + sc["ppy"])
        dx, dy = f32(x * SUB + SUB // 2) - u, f32(y * SUB + SUB // 2) - v
        a = f32(np.sqrt(np.float64(dx) * np.float64(dx) + np.float64(dy) * np.float64(dy)))
        a = f32(MAX_REPROJ) if f32(MAX_REPROJ) < a else a
        stf = beta * (a - f32(THR))
        part[i % 64] += 1.0 - 1.0 / (1.0 + oracle.exp(-float(stf)))
    off = 32
    while off >= 1:
        part = part + part[np.arange(64) ^ off]
        off >>= 1
    return float(part[0] * np.float64(fac))


def test_sanitizer_program_runs_clean(tmp_path):
    """the restatement as a program of its own under AddressSanitizer and UBSan, on a masked 9x13 case"""
    Ho, Wo = 9, 13
    prog = dsac_masked_ref.build_program(tmp_path, sanitize=True)
    sc = _scene(8, Ho, Wo)
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(sc["coords"]).tobytes())
        f.write(_seeded_mask(8, Ho, Wo, 0.5).tobytes())
    p = subprocess.run([prog, str(path), str(Ho), str(Wo), "8", str(THR), "4096"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr


def test_abi_refuses_null_mask_and_empty_batch():
    """argument validation runs before any HIP call, so it is testable without a GPU"""
    from crossloc_amd import build
    lib = ctypes.CDLL(build.build())
    fn = lib.xl_dsac_forward_rgb_masked_batch
    vp, i64, ci, cf, u64, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint32
    fn.restype = ci
    fn.argtypes = [vp, i64, i64, i64, i64, ci, ci, ci, vp, vp, vp, ci, cf, cf, cf, cf, cf, cf, ci, vp, u64, u64, u64, u32,
                   vp, vp, vp, vp, vp]
    some = ctypes.c_void_p(4096)                                   # never dereferenced: the call returns before any HIP call

    def call(coords, mask, poses, B, Ho=8, Wo=12):
        return fn(coords, 3 * Ho * Wo, Ho * Wo, Wo, 1, B, Ho, Wo, mask, poses, None, 6, 10.0, 480.0, 48.0, 32.0, 100.0, 100.0, 8,
                  None, 1305, 0, 1, 1000000, None, None, None, None, None)

    assert call(some, None, some, 1) == -1
    assert call(some, some, some, 0) == -1
    assert call(None, some, some, 1) == -1
    assert call(some, some, None, 1) == -1
    # 96 x 140: 2384 B of reduction scratch + 161280 B of coordinate planes fit in the 163840 B of LDS, the 1680 B of the bit plane
    # on top of them do not: refused before any launch
    assert call(some, some, some, 1, 96, 140) == -2
