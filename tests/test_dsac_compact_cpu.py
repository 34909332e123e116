"""CPU checks of the compact sampler of the masked RGB DSAC* solver through its serial restatement tests/dsac_compact_ref.c
(which the GPU kernels must match bit for bit, tests/test_dsac_compact_gpu.py and test_dsac_compact_bwd_gpu.py): mask_select
against numpy, the drawn cells against the generator restated in Python integers, usable cells only (exhausted hypotheses
included), poisoned masked cells forward and backward, dead images against the reject restatement, the case the sampler was
built for (10 % usable, 4096 tries: the reject sampler exhausts every hypothesis, the compact one none), accuracy against the
reject sampler with a million tries, a sanitizer run of the restatement as a program of its own, and the argument validation
of the C entry points and the front ends.  No GPU."""
import ctypes
import subprocess

import numpy as np
import pytest

import dsac_compact_ref
import dsac_masked_bwd_ref
import dsac_masked_ref
from crossloc_amd import synth

THR, ALPHA, MAX_REPROJ, SUB = 10.0, 100.0, 100.0, 8
W_ROT, W_TRANS, SOFT_CLAMP = 1.0, 100.0, 100.0
FWD_FIELDS = ("cells", "tries", "scores", "winner", "rounds", "inliers", "lm_evals", "pose0", "pose1", "pose", "dbg")
E2E_MAX_TRIES = 4096                       # training's bound (loss.E2E_MAX_TRIES; asserted below)
# the frame of the motivating case: 24 x 36, make_scene(11), image key 20, 32 hypotheses, mask seed 40
FRAME = dict(Ho=24, Wo=36, scene=11, image=20, n_hyp=32, mask_seed=40)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return dsac_compact_ref.load(tmp_path_factory.mktemp("dsac_compact_ref"))


@pytest.fixture(scope="module")
def reject(tmp_path_factory):
    return dsac_masked_ref.load(tmp_path_factory.mktemp("dsac_masked_ref"))


@pytest.fixture(scope="module")
def reject_bwd(tmp_path_factory):
    return dsac_masked_bwd_ref.load(tmp_path_factory.mktemp("dsac_masked_bwd_ref"))


def _seeded_mask(seed, Ho, Wo, usable):
    return (np.random.default_rng([seed, 0x4d41]).random((Ho, Wo)) < usable).astype(np.uint8)


def _fwd(r, sc, mask, n_hyp, coords=None, **kw):
    return r.forward(sc["coords"] if coords is None else coords, mask, n_hyp, THR, sc["focal"], sc["ppx"], sc["ppy"], ALPHA,
                     MAX_REPROJ, SUB, **kw)


def _bwd(r, sc, mask, n_hyp, coords=None, **kw):
    return r.backward(sc["coords"] if coords is None else coords, mask, sc["pose"], n_hyp, THR, sc["focal"], sc["ppx"], sc["ppy"],
                      W_ROT, W_TRANS, SOFT_CLAMP, ALPHA, MAX_REPROJ, SUB, **kw)


def _same(a, b, fields, what=""):
    for k in fields:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert x.tobytes() == y.tobytes(), (what, k)


# ---------------------------------------------------------------------------------------------- 1. mask_select

SELECT_SIZES = [1, 31, 32, 33, 64, 96, 117, 864, 10128]


def _select_masks(N):
    """(name, mask [N]) for every family that exists at N cells"""
    words = (N + 31) // 32
    out = [("all ones", np.ones(N, np.uint8))]
    for name, idx in (("first cell", [0]), ("last cell", [N - 1]), ("word boundaries", [i for i in (31, 32, 63, 64) if i < N])):
        if idx:
            m = np.zeros(N, np.uint8)
            m[idx] = 1
            out.append((name, m))
    m = np.zeros(N, np.uint8)
    m[32 * (words - 1):] = 1                                   # the last word only (partial unless N is a multiple of 32)
    out.append(("last word", m))
    if words >= 4:
        m = np.zeros(N, np.uint8)                              # every third word usable (wholly or in part), the others empty
        for w in range(0, words, 3):
            m[32 * w:32 * w + 32:1 + w % 5] = 1
        out.append(("runs of empty words", m))
    for frac in (0.5, 0.1, 0.01):
        out.append(("seeded %g" % frac, (np.random.default_rng([N, int(frac * 100), 0x4d41]).random(N) < frac).astype(np.uint8)))
    return out


@pytest.mark.parametrize("N", SELECT_SIZES)
def test_mask_select_equals_flatnonzero(ref, N):
    """every rank k of every mask family: the selected cell is np.flatnonzero(mask)[k]; one past the last rank is refused"""
    for name, mask in _select_masks(N):
        want = np.flatnonzero(mask)
        got = np.array([ref.mask_select(mask, k) for k in range(want.size)], dtype=want.dtype)
        assert np.array_equal(got, want), (N, name)
        assert ref.mask_select(mask, want.size) == -1, (N, name)


# ---------------------------------------------------------------------------------------------- 2. the sampler, in Python integers

M64 = (1 << 64) - 1
GOLDEN = 0x9e3779b97f4a7c15


def _mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def _image_key(seed, image):
    return _mix64(seed + GOLDEN * (image + 1))


def _try_state(key, hyp, t):
    return _mix64(key ^ ((hyp << 32) | t))


def _draw(state, j, n):
    return ((_mix64(state + GOLDEN * (j + 1)) >> 32) * n) >> 32


def _expected_cells(mask, seed, image, hyp, t):
    usable = np.flatnonzero(np.asarray(mask).reshape(-1))
    st = _try_state(_image_key(seed, image), hyp, t)
    return [int(usable[_draw(st, j, usable.size)]) for j in range(4)]


@pytest.mark.parametrize("Ho,Wo", [(9, 13), (24, 36)])
@pytest.mark.parametrize("usable", [0.5, 0.1])
def test_cells_are_rank_draws_of_the_accepted_try(ref, Ho, Wo, usable):
    """independent of the C file: cell j of an accepted hypothesis is flatnonzero(mask)[draw(try_state(key, h, tries - 1), j, n)]"""
    sc = synth.make_scene(3, Ho=Ho, Wo=Wo)
    mask = _seeded_mask(3, Ho, Wo, usable)
    got = _fwd(ref, sc, mask, 16, image=9, max_tries=E2E_MAX_TRIES)
    accepted = np.flatnonzero(got["tries"] > 0)
    assert got["status"] == 0 and accepted.size > 0
    for h in accepted:
        assert got["cells"][h].tolist() == _expected_cells(mask, 1305, 9, int(h), int(got["tries"][h]) - 1), (Ho, Wo, usable, h)


# ---------------------------------------------------------------------------------------------- 3. usable cells only

def test_every_drawn_cell_is_usable_also_when_tries_run_out(ref):
    """a noisy frame and one try per hypothesis: most hypotheses run out, and their cells are still four usable ones - the last
    try's rank draws"""
    Ho, Wo, n_hyp = 24, 36, 32
    sc = synth.make_scene(7, Ho=Ho, Wo=Wo, noise=5.0, outlier_ratio=0.6)
    mask = _seeded_mask(7, Ho, Wo, 0.1)
    flat = mask.reshape(-1)
    got = _fwd(ref, sc, mask, n_hyp, image=7, max_tries=1)
    exhausted = np.flatnonzero(got["tries"] < 0)
    assert exhausted.size > 0, "the case must exhaust at least one hypothesis"
    assert (got["tries"][exhausted] == -1).all()
    assert flat[got["cells"]].all()
    for h in exhausted:
        assert got["cells"][h].tolist() == _expected_cells(mask, 1305, 7, int(h), 0), h
    back = _bwd(ref, sc, mask, n_hyp, image=7, max_tries=1)
    assert np.array_equal(back["cells"], got["cells"]) and np.array_equal(back["tries"], got["tries"])
    more = _fwd(ref, sc, mask, n_hyp, image=7, max_tries=E2E_MAX_TRIES)
    assert flat[more["cells"]].all()


# ---------------------------------------------------------------------------------------------- 4. poison

@pytest.mark.parametrize("Ho,Wo", [(9, 13), (24, 36)])
def test_masked_cell_values_influence_no_output_bit(ref, Ho, Wo):
    """NaN, +Inf, -Inf and 1e30 at the masked-out cells, forward and backward; an incoming gradient of 0.125 stays there"""
    sc = synth.make_scene(5, Ho=Ho, Wo=Wo)
    mask = _seeded_mask(5, Ho, Wo, 0.5)
    g0 = np.full((3, Ho, Wo), 0.125, np.float32)
    want = _fwd(ref, sc, mask, 8, image=5, max_tries=E2E_MAX_TRIES)
    want_b = _bwd(ref, sc, mask, 8, image=5, max_tries=E2E_MAX_TRIES, grad=g0)
    assert want["status"] == 0 and want_b["status"] == 0 and (want_b["rec"][:, 2] == 1).any()
    assert (want_b["grad"][:, mask == 0] == np.float32(0.125)).all()
    assert (want_b["grad"][:, mask != 0] != np.float32(0.125)).any()
    for poison in (np.nan, np.inf, -np.inf, 1e30):
        co = sc["coords"].copy()
        co[:, mask == 0] = poison
        _same(_fwd(ref, sc, mask, 8, coords=co, image=5, max_tries=E2E_MAX_TRIES), want, FWD_FIELDS, poison)
        got_b = _bwd(ref, sc, mask, 8, coords=co, image=5, max_tries=E2E_MAX_TRIES, grad=g0)
        assert got_b["status"] == 0 and np.float64(got_b["loss"]).tobytes() == np.float64(want_b["loss"]).tobytes(), poison
        _same(got_b, want_b, ("rec", "grad", "cells", "tries"), poison)


# ---------------------------------------------------------------------------------------------- 5. dead images

@pytest.mark.parametrize("n_usable", [0, 1, 2, 3])
def test_fewer_than_four_usable_cells_equal_the_reject_restatement(ref, reject, reject_bwd, n_usable):
    Ho, Wo, n_hyp = 9, 13, 6
    sc = synth.make_scene(6, Ho=Ho, Wo=Wo)
    mask = np.zeros((Ho, Wo), np.uint8)
    mask.reshape(-1)[[5, 40, 116][:n_usable]] = 1
    got, want = _fwd(ref, sc, mask, n_hyp, image=6), _fwd(reject, sc, mask, n_hyp, image=6)
    assert got["status"] == want["status"] == 1
    _same(got, want, FWD_FIELDS, n_usable)
    g0 = np.full((3, Ho, Wo), 0.125, np.float32)
    got_b, want_b = _bwd(ref, sc, mask, n_hyp, image=6, grad=g0), _bwd(reject_bwd, sc, mask, n_hyp, image=6, grad=g0)
    assert got_b["status"] == want_b["status"] == 1 and got_b["loss"] == want_b["loss"] == 0.0
    _same(got_b, want_b, ("rec", "grad", "cells", "tries"), n_usable)
    assert got_b["grad"].tobytes() == g0.tobytes()


# ---------------------------------------------------------------------------------------------- 6. the motivating case

def _frame():
    return synth.make_scene(FRAME["scene"], Ho=FRAME["Ho"], Wo=FRAME["Wo"])


def test_ten_percent_usable_exhausts_reject_but_not_compact(ref, reject, oracle):
    """10 % usable at training's 4096 tries: the reject sampler finds no hypothesis at all (a try draws four usable cells with
    probability 1e-4), the compact sampler finds every one, within the number of tries the unmasked solver needs on the frame"""
    from crossloc_amd import loss
    assert loss.E2E_MAX_TRIES == E2E_MAX_TRIES
    sc, n_hyp, image = _frame(), FRAME["n_hyp"], FRAME["image"]
    mask = _seeded_mask(FRAME["mask_seed"], FRAME["Ho"], FRAME["Wo"], 0.1)
    old = _fwd(reject, sc, mask, n_hyp, image=image, max_tries=E2E_MAX_TRIES)
    assert (old["tries"] == -E2E_MAX_TRIES).all(), "the input must exhaust every hypothesis of the reject sampler"
    new = _fwd(ref, sc, mask, n_hyp, image=image, max_tries=E2E_MAX_TRIES)
    assert new["status"] == 0 and (new["tries"] > 0).all()
    _, dbg = oracle.forward_rgb(sc["coords"], n_hyp, THR, sc["focal"], sc["ppx"], sc["ppy"], ALPHA, MAX_REPROJ, SUB, image=image,
                                debug=True)
    assert (dbg["tries"] > 0).all()
    print("tries: unmasked median %.1f max %d; compact at 10 %% median %.1f max %d"
          % (np.median(dbg["tries"]), dbg["tries"].max(), np.median(new["tries"]), new["tries"].max()))
    assert np.median(new["tries"]) <= dbg["tries"].max()


# ---------------------------------------------------------------------------------------------- 7. same distribution, same accuracy

def test_accuracy_is_the_reject_samplers(ref, reject):
    """12 seeds of the 10 % mask on the frame above, 32 hypotheses.  The yardstick is the reject restatement with a million tries
    (it then finds every hypothesis): the compact solver's median translation and rotation error against the true pose may not
    exceed the reject solver's worst seed.  Both sets of medians are printed (README.md quotes them)."""
    sc, n_hyp, image = _frame(), FRAME["n_hyp"], FRAME["image"]
    errs = {"reject": [], "compact": []}
    for s in range(12):
        mask = _seeded_mask(FRAME["mask_seed"] + s, FRAME["Ho"], FRAME["Wo"], 0.1)
        old = _fwd(reject, sc, mask, n_hyp, image=image, max_tries=1000000)
        new = _fwd(ref, sc, mask, n_hyp, image=image, max_tries=E2E_MAX_TRIES)
        assert old["status"] == new["status"] == 0
        errs["reject"].append(synth.pose_error(sc["pose"], old["pose"]))
        errs["compact"].append(synth.pose_error(sc["pose"], new["pose"]))
    old, new = np.array(errs["reject"]), np.array(errs["compact"])
    print("reject : median %.3f m %.3f deg, worst %.3f m %.3f deg" % (*np.median(old, 0), *old.max(0)))
    print("compact: median %.3f m %.3f deg, worst %.3f m %.3f deg" % (*np.median(new, 0), *new.max(0)))
    assert np.median(new[:, 0]) <= old[:, 0].max()
    assert np.median(new[:, 1]) <= old[:, 1].max()


# ---------------------------------------------------------------------------------------------- 8. sanitizers

def test_sanitizer_program_runs_clean(tmp_path):
    """the restatement as a program of its own under AddressSanitizer and UBSan: every rank selected, forward and backward, on a
    9x13 case whose last mask word is partial, and on the 48x211 grid with a 10 % mask (317 words)"""
    prog = dsac_compact_ref.build_program(tmp_path, sanitize=True)
    for Ho, Wo, usable, n_hyp in ((9, 13, 0.5, 8), (48, 211, 0.1, 2)):
        sc = synth.make_scene(8, Ho=Ho, Wo=Wo)
        path = tmp_path / ("case_%d.bin" % Ho)
        with open(path, "wb") as f:
            f.write(np.ascontiguousarray(sc["coords"]).tobytes())
            f.write(_seeded_mask(8, Ho, Wo, usable).tobytes())
        p = subprocess.run([prog, str(path), str(Ho), str(Wo), str(n_hyp), str(THR), "4096"], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr


# ---------------------------------------------------------------------------------------------- 9. ABI and front ends

def test_abi_refuses_null_mask_empty_batch_and_unknown_sampler():
    """argument validation runs before any HIP call, so it is testable without a GPU"""
    from crossloc_amd import build
    lib = ctypes.CDLL(build.build())
    vp, i64, ci, cf, u64, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint32
    fwd, bwd = lib.xl_dsac_forward_rgb_masked_sampled_batch, lib.xl_dsac_backward_rgb_masked_sampled_batch
    fwd.restype = bwd.restype = ci
    fwd.argtypes = [vp, i64, i64, i64, i64, ci, ci, ci, vp, ci, vp, vp, ci, cf, cf, cf, cf, cf, cf, ci, vp, u64, u64, u64, u32,
                    vp, vp, vp, vp, vp]
    bwd.argtypes = [vp, i64, i64, i64, i64, ci, ci, ci, vp, ci, vp, i64, i64, i64, i64, vp, vp, vp, ci, cf, cf, cf, cf, cf, cf, cf,
                    cf, cf, ci, vp, u64, u64, u64, u32, vp, vp]
    some = ctypes.c_void_p(4096)                                   # never dereferenced: the calls return before any HIP call

    def forward(coords, mask, sampler, poses, B, Ho=8, Wo=12):
        return fwd(coords, 3 * Ho * Wo, Ho * Wo, Wo, 1, B, Ho, Wo, mask, sampler, poses, None, 6, 10.0, 480.0, 48.0, 32.0, 100.0,
                   100.0, 8, None, 1305, 0, 1, 4096, None, None, None, None, None)

    def backward(coords, mask, sampler, grad, B, Ho=8, Wo=12, gt=some, loss=some):
        N = Ho * Wo
        return bwd(coords, 3 * N, N, Wo, 1, B, Ho, Wo, mask, sampler, grad, 3 * N, N, Wo, 1, gt, loss, None, 6, 10.0, 480.0, 48.0,
                   32.0, 1.0, 100.0, 100.0, 100.0, 100.0, 8, None, 1305, 0, 1, 4096, None, None)

    for sampler in (0, 1):
        assert forward(some, None, sampler, some, 1) == -1 and backward(some, None, sampler, some, 1) == -1
        assert forward(some, some, sampler, some, 0) == -1 and backward(some, some, sampler, some, 0) == -1
        assert forward(None, some, sampler, some, 1) == -1 and backward(None, some, sampler, some, 1) == -1
        assert forward(some, some, sampler, None, 1) == -1 and backward(some, some, sampler, None, 1) == -1
        # 96 x 140: refused for its LDS before any launch (tests/test_dsac_masked_cpu.py), with the rank plane all the more
        assert forward(some, some, sampler, some, 1, 96, 140) == -2 and backward(some, some, sampler, some, 1, 96, 140) == -2
    for sampler in (2, -1, 7):
        assert forward(some, some, sampler, some, 1) == -1 and backward(some, some, sampler, some, 1) == -1


def test_python_front_ends_refuse_an_unknown_sampler_and_a_sampler_without_a_mask():
    """checked before the tensors are looked at, so no device is needed"""
    import torch
    import dsacstar
    from crossloc_amd import evaluation, loss
    assert dsacstar.MASK_SAMPLERS == ("reject", "compact")
    coords, mask, poses = torch.zeros((1, 3, 8, 12)), torch.ones((1, 8, 12), dtype=torch.uint8), torch.zeros((1, 4, 4))
    with pytest.raises(RuntimeError, match="sampler"):
        dsacstar.forward_rgb_masked_batch(coords, mask, poses, 6, 10.0, 480.0, 48.0, 32.0, 100.0, 100.0, 8, sampler="weighted")
    with pytest.raises(RuntimeError, match="sampler"):
        dsacstar.backward_rgb_masked_batch(coords, mask, torch.zeros_like(coords), torch.eye(4)[None], 6, 10.0, 480.0, 48.0, 32.0,
                                           1.0, 100.0, 100.0, 100.0, 100.0, 8, 1305, sampler="weighted")
    args = (coords, torch.eye(4)[None], [480.0], 64, 96, 6, 10.0, 100.0, 100.0, 1.0, 100.0, 100.0, 1305)
    with pytest.raises(RuntimeError, match="mask_sampler"):
        loss.expected_pose_loss_and_output_gradient(*args, mask=mask, mask_sampler="weighted")
    with pytest.raises(RuntimeError, match="needs mask"):
        loss.expected_pose_loss_and_output_gradient(*args, mask_sampler="compact")
    images = torch.zeros((1, 3, 64, 96))
    for call in (lambda **kw: evaluation.localize_batch(None, images, 6, 480.0, 64, 96, **kw),
                 lambda **kw: evaluation.PipelinedLocalizer.submit(None, images, **kw)):
        with pytest.raises(RuntimeError, match="mask_sampler"):
            call(mask=mask, mask_sampler="weighted")
        with pytest.raises(RuntimeError, match="needs mask"):
            call(mask_sampler="compact")


def _e2e(*extra):
    from crossloc_amd import train_e2e
    return train_e2e._config_parser(["urbanscape", "--network_in", "model.net"] + list(extra))


def test_train_e2e_mask_sampler_option(capsys):
    from crossloc_amd import train_e2e
    off = _e2e("--mask", "labels")
    assert off.mask_sampler == "reject"
    on = _e2e("--mask", "labels", "--mask_sampler", "compact")
    assert on.mask_sampler == "compact" and on.mask == "labels"
    assert train_e2e.get_output_path(on) == train_e2e.get_output_path(off).replace("-masklabels", "-masklabels-compact")
    with pytest.raises(SystemExit):
        _e2e("--mask_sampler", "compact")
    assert "--mask labels" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _e2e("--mask", "labels", "--mask_sampler", "weighted")
