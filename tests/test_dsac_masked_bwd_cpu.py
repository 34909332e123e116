"""CPU checks of the masked RGB backward pass through its serial restatement tests/dsac_masked_bwd_ref.c (which the GPU kernels
must match bit for bit, tests/test_dsac_masked_bwd_gpu.py): the restatement against the pinned oracle under an all-ones mask
(identity A), poisoned masked cells and the untouched gradient there (identities B and C), dead images, hypotheses exhausted on
a mask-rejected try, decoy frames with and without the mask, a descent step, a sanitizer run of the restatement as a program
of its own, the argument validation of the C entry point and the option checks of the front ends.  No GPU."""
import ctypes
import subprocess

import numpy as np
import pytest

import dsac_masked_bwd_ref
from crossloc_amd import synth

GRIDS = [(8, 12), (9, 13), (24, 36)]
THR, ALPHA, MAX_REPROJ, SUB = 10.0, 100.0, 100.0, 8
W_ROT, W_TRANS, SOFT_CLAMP = 1.0, 100.0, 100.0
FIELDS = dsac_masked_bwd_ref.FIELDS
EXHAUSTED = dsac_masked_bwd_ref.EXHAUSTED


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return dsac_masked_bwd_ref.load(tmp_path_factory.mktemp("dsac_masked_bwd_ref"))


def _args(sc, alpha=ALPHA):
    return (THR, sc["focal"], sc["ppx"], sc["ppy"], W_ROT, W_TRANS, SOFT_CLAMP, alpha, MAX_REPROJ, SUB)


def _run(ref, sc, mask, n_hyp, coords=None, gt=None, alpha=ALPHA, **kw):
    return ref.backward(sc["coords"] if coords is None else coords, mask, sc["pose"] if gt is None else gt, n_hyp,
                        *_args(sc, alpha), **kw)


def _seeded_mask(seed, Ho, Wo, usable):
    return (np.random.default_rng([seed, 0x4d41]).random((Ho, Wo)) < usable).astype(np.uint8)


def _same(a, b, what=""):
    assert a["status"] == b["status"], what
    assert np.float64(a["loss"]).tobytes() == np.float64(b["loss"]).tobytes(), (what, a["loss"], b["loss"])
    for k in ("rec", "grad"):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("Ho,Wo", GRIDS)
def test_all_ones_mask_equals_the_pinned_oracle(ref, oracle, Ho, Wo):
    """identity A on the CPU: ties the new restatement to oracle/dsac_bwd_oracle.c - loss, 53 record fields, gradient"""
    for seed, n_hyp in ((3, 6), (4, 16)):
        sc = synth.make_scene(seed, Ho=Ho, Wo=Wo)
        g = np.full((3, Ho, Wo), 0.125, np.float32)
        loss, rec = oracle.backward_rgb(sc["coords"], g, sc["pose"], n_hyp, *_args(sc), 1305, image=seed, debug=True)
        got = _run(ref, sc, np.ones((Ho, Wo), np.uint8), n_hyp, image=seed, grad=np.full((3, Ho, Wo), 0.125, np.float32))
        assert got["status"] == 0
        assert np.float64(got["loss"]).tobytes() == np.float64(loss).tobytes(), (Ho, Wo, seed, got["loss"], loss)
        assert got["rec"].tobytes() == np.ascontiguousarray(rec[:, :FIELDS]).tobytes(), (Ho, Wo, seed)
        assert got["grad"].tobytes() == g.tobytes(), (Ho, Wo, seed)
        assert (got["rec"][:, 2] == 1).any() and np.abs(got["grad"] - 0.125).max() > 0        # something was differentiated


@pytest.mark.parametrize("Ho,Wo", GRIDS)
def test_masked_cells_influence_nothing_and_keep_their_gradient(ref, Ho, Wo):
    """identities B and C: NaN, +Inf and 1e30 at the masked-out cells; an incoming gradient of 0.125 everywhere"""
    sc = synth.make_scene(5, Ho=Ho, Wo=Wo)
    mask = _seeded_mask(5, Ho, Wo, 0.5)
    g0 = np.full((3, Ho, Wo), 0.125, np.float32)
    want = _run(ref, sc, mask, 8, image=5, grad=g0)
    assert want["status"] == 0 and (want["rec"][:, 2] == 1).any()
    assert (want["grad"][:, mask == 0] == np.float32(0.125)).all()                              # C
    assert (want["grad"][:, mask != 0] != np.float32(0.125)).any()
    for poison in (np.nan, np.inf, 1e30):
        co = sc["coords"].copy()
        co[:, mask == 0] = poison
        _same(_run(ref, sc, mask, 8, coords=co, image=5, grad=g0), want, poison)                # B


@pytest.mark.parametrize("n_usable", [3, 0])
def test_fewer_than_four_usable_cells(ref, n_usable):
    Ho, Wo, n_hyp = 9, 13, 6
    sc = synth.make_scene(6, Ho=Ho, Wo=Wo)
    mask = np.zeros((Ho, Wo), np.uint8)
    mask.reshape(-1)[[5, 40, 116][:n_usable]] = 1
    g0 = np.full((3, Ho, Wo), 0.125, np.float32)
    got = _run(ref, sc, mask, n_hyp, image=6, grad=g0)
    assert got["status"] == 1 and got["loss"] == 0.0 and not np.signbit(got["loss"])
    assert got["grad"].tobytes() == g0.tobytes()
    assert not got["rec"].any()


def test_hypotheses_exhausted_on_a_mask_rejected_try(ref):
    c = EXHAUSTED
    sc, mask = synth.make_scene(c["scene"], Ho=c["Ho"], Wo=c["Wo"]), _seeded_mask(c["scene"], c["Ho"], c["Wo"], c["usable"])
    n_hyp, kw = c["n_hyp"], dict(image=c["image"], max_tries=c["max_tries"], alpha=c["alpha"])
    got = _run(ref, sc, mask, n_hyp, **kw)
    assert got["status"] == 0
    flat = mask.reshape(-1)
    rejected = [h for h in range(n_hyp) if got["tries"][h] < 0 and not flat[got["cells"][h]].all()]
    accepted = [h for h in range(n_hyp) if got["tries"][h] > 0]
    print("exhausted on a mask-rejected try: %d, accepted: %d of %d" % (len(rejected), len(accepted), n_hyp))
    assert len(rejected) >= 1 and len(accepted) >= 1
    assert (got["tries"][rejected] == -c["max_tries"]).all()
    for h in accepted:
        assert flat[got["cells"][h]].all()
    rec = got["rec"]
    for h in rejected:
        assert not rec[h, 30:42].any() and rec[h, 43] == 0.0, h                 # zero support-point gradient, zero dPNP
    assert any(rec[h, 0] >= 1e-3 for h in rejected), "a rejected hypothesis must reach the score path for the case to bite"
    co = sc["coords"].copy()
    co[:, mask == 0] = np.nan
    _same(_run(ref, sc, mask, n_hyp, coords=co, **kw), got, "NaN at the masked cells")


def test_decoy_frames_need_the_mask(ref):
    """60 % of the rows hold the exact view of a second camera.  The expected loss against the true pose is lower with the
    decoy mask than with an all-ones mask, on every seed; the medians are printed (no ratio is fixed)."""
    Ho, Wo, n_hyp = 24, 36, 64
    plain, masked = [], []
    for seed in range(12):
        sc = synth.make_decoy_scene(seed, decoy=0.6, Ho=Ho, Wo=Wo)
        e_plain = _run(ref, sc, np.ones((Ho, Wo), np.uint8), n_hyp, image=seed)["loss"]
        e_masked = _run(ref, sc, sc["mask"], n_hyp, image=seed)["loss"]
        print("decoy seed %d: expected loss %.4f with an all-ones mask, %.4f with the decoy mask" % (seed, e_plain, e_masked))
        plain.append(e_plain)
        masked.append(e_masked)
    print("medians over 12 seeds: all-ones %.4f, decoy mask %.4f" % (np.median(plain), np.median(masked)))
    for seed in range(12):
        assert masked[seed] < plain[seed], (seed, masked[seed], plain[seed])


def test_gradient_descends_expected_loss(ref):
    """a step of 0.05 / max|g| against the gradient gives a lower expected loss than the same step along it"""
    Ho, Wo, n_hyp = 24, 36, 64
    sc = synth.make_decoy_scene(3, decoy=0.6, noise=1.0, Ho=Ho, Wo=Wo)
    co = sc["coords"]
    base = _run(ref, sc, sc["mask"], n_hyp, coords=co, image=3)
    g = base["grad"]
    assert np.abs(g).max() > 0 and not g[:, sc["mask"] == 0].any()
    eps = np.float32(0.05 / np.abs(g).max())
    lm = _run(ref, sc, sc["mask"], n_hyp, coords=(co - eps * g).astype(np.float32), image=3)["loss"]
    lp = _run(ref, sc, sc["mask"], n_hyp, coords=(co + eps * g).astype(np.float32), image=3)["loss"]
    print("expected loss: %.6f against the gradient, %.6f at the point, %.6f along it" % (lm, base["loss"], lp))
    assert lm < lp, (lm, base["loss"], lp)


def test_sanitizer_program_runs_clean(tmp_path):
    """the restatement as a program of its own under AddressSanitizer and UBSan, on a masked 9x13 case"""
    Ho, Wo = 9, 13
    prog = dsac_masked_bwd_ref.build_program(tmp_path, sanitize=True)
    sc = synth.make_scene(8, Ho=Ho, Wo=Wo)
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
    fn = lib.xl_dsac_backward_rgb_masked_batch
    vp, i64, ci, cf, u64, u32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint32
    fn.restype = ci
    fn.argtypes = [vp, i64, i64, i64, i64, ci, ci, ci, vp, vp, i64, i64, i64, i64, vp, vp, vp, ci, cf, cf, cf, cf, cf, cf, cf, cf,
                   cf, ci, vp, u64, u64, u64, u32, vp, vp]
    some = ctypes.c_void_p(4096)                                   # never dereferenced: the call returns before any HIP call

    def call(coords, mask, grad, B, Ho=8, Wo=12, gt=some, loss=some):
        N = Ho * Wo
        return fn(coords, 3 * N, N, Wo, 1, B, Ho, Wo, mask, grad, 3 * N, N, Wo, 1, gt, loss, None, 6, 10.0, 480.0, 48.0, 32.0,
                  1.0, 100.0, 100.0, 100.0, 100.0, 8, None, 1305, 0, 1, 4096, None, None)

    assert call(some, None, some, 1) == -1
    assert call(some, some, some, 0) == -1
    assert call(None, some, some, 1) == -1
    assert call(some, some, None, 1) == -1
    assert call(some, some, some, 1, gt=None) == -1 and call(some, some, some, 1, loss=None) == -1
    # 96 x 140: the reduction scratch and the 161280 B of coordinate planes fit in the 163840 B of LDS, the 1680 B of the bit plane
    # on top of them do not: refused before any allocation or launch
    assert call(some, some, some, 1, 96, 140) == -2
    sub = lib.xl_dsac_backward_sub_blocks
    sub.restype, sub.argtypes = ci, [ci, ci]
    assert (sub(3, 6), sub(0, 6), sub(3, 0)) == (1, 0, 0) and sub(3, 16) > 1


def test_loss_front_end_refuses_a_mask_beside_depth():
    """checked before the tensors are looked at, so no device is needed"""
    import torch
    from crossloc_amd import loss
    pred = torch.zeros((1, 3, 8, 12))
    mask = torch.ones((1, 8, 12), dtype=torch.uint8)
    args = (pred, torch.eye(4)[None], [480.0], 64, 96, 6, 10.0, 100.0, 100.0, 1.0, 100.0, 100.0, 1305)
    with pytest.raises(RuntimeError, match="mask"):
        loss.expected_pose_loss_and_output_gradient(*args, mask=mask, depth=torch.ones((1, 8, 12)))
    with pytest.raises(RuntimeError, match="mask"):
        loss.expected_pose_loss_and_output_gradient(*args, mask=mask, cam_coords=torch.ones((1, 3, 8, 12)))


def _e2e(*extra):
    from crossloc_amd import train_e2e
    return train_e2e._config_parser(["urbanscape", "--network_in", "model.net"] + list(extra))


def test_train_e2e_mask_option(capsys):
    from crossloc_amd import train_e2e
    off = _e2e()
    assert off.mask == "none" and "-mask" not in train_e2e.get_output_path(off)
    on = _e2e("--mask", "labels")
    assert on.mask == "labels" and on.mode == "rgb"
    path = train_e2e.get_output_path(on)
    assert "-masklabels" in path and path.replace("-masklabels", "") == train_e2e.get_output_path(off)
    assert "-canvas-masklabels-tiny" in train_e2e.get_output_path(_e2e("--mask", "labels", "--aug_canvas", "--tiny"))
    with pytest.raises(SystemExit):
        _e2e("--mask", "labels", "--mode", "rgbd")
    assert "--mask labels" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        _e2e("--mask", "sigma")
    assert _e2e("--mask", "none", "--mode", "rgbd").mask == "none"
