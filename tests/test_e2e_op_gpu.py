"""GPU: the finishing op of the end-to-end step (csrc/xl_e2e.hip) against tests/e2e_ref.py on planted values, with its
outputs and statistics between the guard bands of tests/guarded.py.  The solver is not involved."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import e2e_ref                                            # noqa: E402
import guarded                                            # noqa: E402
from crossloc_amd import loss as xl_loss                  # noqa: E402

pytestmark = pytest.mark.gpu
B = 3
SMALL = [(5, 7), (8, 12), (13, 17)]                       # fewer cells than a wave; one trip; a ragged tail
ALL = SMALL + [(60, 90)]                                  # ... and the training grid: several trips per thread


@pytest.fixture(autouse=True)
def _guards(monkeypatch):
    """Everything the wrapper allocates (out, stats) and the `out` buffers of the tests lie between guard bands."""
    guarded.guard_modules(monkeypatch, xl_loss)
    try:
        yield
        assert guarded.handed_out() > 0
        guarded.assert_intact()
    finally:
        guarded.stop()


def _inputs(Ho, Wo, seed=0, scale=1.0):
    rng = np.random.default_rng([seed, Ho, Wo])
    g = (rng.standard_normal((B, 3, Ho, Wo)) * scale).astype(np.float32)
    loss = rng.uniform(0.5, 40.0, size=B)
    return g, loss


def _run(g, loss, C, **kw):
    g = g if isinstance(g, torch.Tensor) else torch.from_numpy(g).cuda()
    grad, stats = xl_loss.finish_pose_gradient(g, torch.from_numpy(np.asarray(loss, np.float64)).cuda(), C, **kw)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), stats.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_stats(stats, ref, norm_rtol=1e-12):
    assert stats.shape == ref.shape
    for col in (0, 2, 3):
        assert np.array_equal(stats[:-1, col], ref[:-1, col], equal_nan=True), (col, stats, ref)
    ok = ref[:-1, 3] == 1.0
    assert np.allclose(stats[:-1, 1][ok], ref[:-1, 1][ok], rtol=norm_rtol, atol=0.0)
    assert not np.isfinite(stats[:-1, 1][~ok & ~np.isfinite(ref[:-1, 1])]).any()
    assert stats[-1, 0] == ref[-1, 0] and stats[-1, 1] == ref[-1, 1] and stats[-1, 3] == ref[-1, 3]
    assert np.isclose(stats[-1, 2], ref[-1, 2], rtol=norm_rtol, atol=0.0)


@pytest.mark.parametrize("Ho,Wo", ALL)
def test_unclipped_accepted_is_one_float32_multiply(Ho, Wo):
    g, loss = _inputs(Ho, Wo)
    out, stats = _run(g, loss, 4, weight=0.75)
    assert np.array_equal(_bits(out[:, :3]), _bits(g * np.float32(0.75 / B)))
    assert np.array_equal(_bits(out[:, 3:]), np.zeros((B, 1, Ho, Wo), np.uint32))            # exactly +0
    ref_out, ref_stats = e2e_ref.pose_gradient(g, loss, 4, weight=0.75)
    assert np.array_equal(_bits(out), _bits(ref_out))
    _assert_stats(stats, ref_stats)
    assert stats[-1, 1] == B and stats[-1, 3] == 0 and np.array_equal(stats[:-1, 2], np.full(B, np.float32(0.75 / B)))


@pytest.mark.parametrize("Ho,Wo", SMALL)
def test_strided_gradients_give_the_bits_of_the_contiguous_form(Ho, Wo):
    g, loss = _inputs(Ho, Wo, seed=1)
    base, stats0 = _run(g, loss, 3, clip_norm=1.0)
    wide = torch.full((B, 4, Ho, Wo), float("nan")).cuda()
    wide[:, :3] = torch.from_numpy(g).cuda()
    view = wide[:, :3]
    nhwc = torch.from_numpy(g).cuda().contiguous(memory_format=torch.channels_last)
    assert not view.is_contiguous() and not nhwc.is_contiguous() and nhwc.stride(1) == 1
    for form in (view, nhwc):
        out, stats = _run(form, loss, 3, clip_norm=1.0)
        assert np.array_equal(_bits(out), _bits(base))
        assert np.array_equal(stats, stats0)


@pytest.mark.parametrize("Ho,Wo", ALL)
def test_clipping_scales_the_frame_above_the_norm_only(Ho, Wo):
    g, loss = _inputs(Ho, Wo, seed=2)
    norms = np.sqrt((g.astype(np.float64) ** 2).reshape(B, -1).sum(1))
    clip = float(np.float32(0.5 * norms[0]))
    g[1] *= np.float32(0.25 * clip / norms[1])                          # frame 0 above, frame 1 below, frame 2 above
    out, stats = _run(g, loss, 4, clip_norm=clip)
    ref_out, ref_stats = e2e_ref.pose_gradient(g, loss, 4, clip_norm=clip)
    _assert_stats_clipped(stats, ref_stats)
    assert np.array_equal(_bits(out[1]), _bits(ref_out[1]))             # unclipped: bitwise
    assert np.array_equal(_bits(out[1, :3]), _bits(g[1] * np.float32(1.0 / B)))
    assert e2e_ref.ulp_distance(out, ref_out) <= 2                      # one rounding of s_b may differ
    assert np.array_equal(stats[:-1, 3], [1, 1, 1]) and stats[-1, 3] == 2
    got = np.sqrt((out[:, :3].astype(np.float64) ** 2).reshape(B, -1).sum(1)) * B
    assert np.allclose(got[[0, 2]], clip, rtol=1e-5) and got[1] < clip


def _assert_stats_clipped(stats, ref):
    """As _assert_stats, with the scale of a clipped frame within one float32 rounding of the reference's."""
    assert np.array_equal(stats[:-1, [0, 3]], ref[:-1, [0, 3]])
    assert np.allclose(stats[:, 1][:-1], ref[:-1, 1], rtol=1e-12, atol=0.0)
    assert e2e_ref.ulp_distance(stats[:-1, 2].astype(np.float32), ref[:-1, 2].astype(np.float32)) <= 1
    assert stats[-1, 0] == ref[-1, 0] and stats[-1, 1] == ref[-1, 1] and stats[-1, 3] == ref[-1, 3]
    assert np.isclose(stats[-1, 2], ref[-1, 2], rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("Ho,Wo", SMALL)
def test_rejected_frames_contribute_exact_zeros(Ho, Wo):
    """Planted values are data, not a fault: a NaN in frame 0's gradient, an infinite loss for frame 1."""
    g, loss = _inputs(Ho, Wo, seed=3)
    clean, stats_clean = _run(g, loss, 4, clip_norm=2.0)
    g2, loss2 = g.copy(), loss.copy()
    g2[0, 1, Ho // 2, Wo - 1] = np.nan
    loss2[1] = np.inf
    out, stats = _run(g2, loss2, 4, clip_norm=2.0)
    assert np.array_equal(_bits(out[:2]), np.zeros((2, 4, Ho, Wo), np.uint32))
    assert np.array_equal(_bits(out[2]), _bits(clean[2]))               # the remaining frame: as without the planted values
    assert np.array_equal(stats[2], stats_clean[2])
    assert np.array_equal(stats[:-1, 3], [0, 0, 1]) and np.array_equal(stats[:2, 2], [0, 0])
    assert np.isnan(stats[0, 1]) and stats[1, 0] == np.inf and stats[1, 1] == stats_clean[1, 1]
    assert stats[-1, 0] == loss[2] and stats[-1, 1] == 1 and stats[-1, 2] == stats[2, 1]
    assert stats[-1, 3] == (1 if stats[2, 1] > 2.0 else 0)
    ref_out, ref_stats = e2e_ref.pose_gradient(g2, loss2, 4, clip_norm=2.0)
    assert e2e_ref.ulp_distance(out, ref_out) <= 2
    # +inf in the gradient and every frame rejected: zeros everywhere, an all-zero summary
    g2[2, 0, 0, 0] = np.inf
    out, stats = _run(g2, loss2, 4)
    assert not out.any() and np.array_equal(stats[-1], [0, 0, 0, 0]) and not stats[:-1, 3].any()


@pytest.mark.parametrize("Ho,Wo", SMALL)
def test_beta_zero_does_not_read_out(Ho, Wo):
    g, loss = _inputs(Ho, Wo, seed=4)
    grad = torch.full((B, 5, Ho, Wo), float("nan"), dtype=torch.float32, device="cuda")
    base, _ = _run(g, loss, 5)
    out, _ = _run(g, loss, 5, grad=grad, beta=0.0)
    assert np.isfinite(out).all() and np.array_equal(_bits(out), _bits(base))
    assert np.array_equal(_bits(grad.cpu().numpy()), _bits(base))       # written in place


@pytest.mark.parametrize("Ho,Wo", ALL)
def test_beta_adds_onto_the_gradient_that_is_there(Ho, Wo):
    g, loss = _inputs(Ho, Wo, seed=5)
    g[1, 2, 0, 0] = np.nan                                              # a rejected frame still keeps beta * out
    prev = np.random.default_rng(9).standard_normal((B, 5, Ho, Wo)).astype(np.float32)
    grad = guarded.REGISTRY.empty((B, 5, Ho, Wo), dtype=torch.float32, device="cuda")
    grad.copy_(torch.from_numpy(prev))
    out, stats = _run(g, loss, 5, weight=2.0, grad=grad, beta=0.5)
    ref_out, ref_stats = e2e_ref.pose_gradient(g, loss, 5, weight=2.0, beta=0.5, out=prev)
    assert e2e_ref.ulp_distance(out, ref_out) <= 1
    assert np.array_equal(_bits(out[:, 3:]), _bits(np.float32(0.5) * prev[:, 3:]))
    assert np.array_equal(_bits(out[1, :3]), _bits(np.float32(0.5) * prev[1, :3] + np.float32(0)))
    assert np.array_equal(stats[:-1, 3], ref_stats[:-1, 3]) and np.array_equal(stats[-1, [1, 3]], ref_stats[-1, [1, 3]])


def test_summary_row_over_many_frames_in_back_to_back_calls():
    """More workgroups than the cases above (whichever finishes last writes the summary, from every frame's row) and calls
    queued behind each other without a synchronise (each finds the done-counter as the one before left it)."""
    n, Ho, Wo = 37, 5, 7
    rng = np.random.default_rng(6)
    cases, results = [], []
    for k in range(6):
        g = (rng.standard_normal((n, 3, Ho, Wo)) * rng.uniform(0.1, 3.0, size=(n, 1, 1, 1))).astype(np.float32)
        loss = rng.uniform(0.5, 40.0, size=n)
        g[rng.integers(0, n, size=k), 0, 0, 0] = np.nan
        loss[rng.integers(0, n, size=2)] = np.inf
        cases.append((g, loss))
        results.append(xl_loss.finish_pose_gradient(torch.from_numpy(g).cuda(), torch.from_numpy(loss).cuda(), 3, clip_norm=8.0))
    torch.cuda.synchronize()
    for (g, loss), (out, stats) in zip(cases, results):
        ref_out, ref_stats = e2e_ref.pose_gradient(g, loss, 3, clip_norm=8.0)
        stats = stats.cpu().numpy()
        assert np.array_equal(stats[:-1, 3], ref_stats[:-1, 3]) and 0 < ref_stats[-1, 1] < n
        assert np.array_equal(stats[-1, [1, 3]], ref_stats[-1, [1, 3]]) and 0 < ref_stats[-1, 3] < ref_stats[-1, 1]
        assert np.allclose(stats[-1, [0, 2]], ref_stats[-1, [0, 2]], rtol=1e-12, atol=0.0)
        assert e2e_ref.ulp_distance(out.cpu().numpy(), ref_out) <= 2


def test_wrapper_refusals():
    g = torch.zeros(B, 3, 5, 7, device="cuda")
    loss = torch.zeros(B, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError):
        xl_loss.finish_pose_gradient(g.cpu(), loss, 3)
    with pytest.raises(RuntimeError):
        xl_loss.finish_pose_gradient(g, loss.float(), 3)
    with pytest.raises(RuntimeError):
        xl_loss.finish_pose_gradient(g, loss, 2)
    with pytest.raises(RuntimeError):
        xl_loss.finish_pose_gradient(g, loss, 4, beta=0.5)                                   # nothing to add onto
    with pytest.raises(RuntimeError):
        xl_loss.finish_pose_gradient(g, loss, 4, grad=torch.zeros(B, 3, 5, 7, device="cuda"))
    xl_loss.finish_pose_gradient(g, loss, 3)                  # (the fixture expects one guarded allocation per test)
