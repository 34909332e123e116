"""Independent numpy implementation of the RGB-D DSAC* forward pass — TEST INFRASTRUCTURE ONLY.

Written from the description of the reference's dsacstar_rgbd_forward (valid cells x-major, three-point Kabsch hypotheses,
distance error map in centimetres, soft-inlier score, first-maximum selection, re-fit on the inliers while their number
grows).  It shares no code with crossloc_amd/csrc/xl_dsac_rgbd_math.h: Kabsch is numpy's SVD, the exponential is
numpy's, sums are numpy's, the sampler is numpy's PCG64 (or the caller's cells, for replays)."""
import numpy as np

MAX_REF_STEPS = 100


def kabsch_svd(p, X):
    """world->camera (R, t) minimising sum |p - (R X + t)|^2: R = U diag(1, 1, det(U V^T)) V^T of A = sum (p - cp)(X - cX)^T."""
    p, X = np.asarray(p, np.float64), np.asarray(X, np.float64)
    cp, cX = p.mean(0), X.mean(0)
    A = (p - cp).T @ (X - cX)
    U, W, Vt = np.linalg.svd(A)
    d = np.linalg.det(U @ Vt)
    R = U @ np.diag([1.0, 1.0, 1.0 if d >= 0 else -1.0]) @ Vt
    return R, cp - R @ cX, W


def objective(R, t, p, X):
    r = np.asarray(p, np.float64) - (np.asarray(X, np.float64) @ R.T + t)
    return float((r * r).sum())


def valid_list(cam):
    """cell indices y * Wo + x of the cells with cam z != 0, x outer, y inner"""
    _, Ho, Wo = cam.shape
    ok = (cam[2] != 0).T.reshape(-1)                    # index x * Ho + y
    j = np.nonzero(ok)[0]
    x, y = j // Ho, j % Ho
    return y * Wo + x


def error_map(R, t, co, cm, valid, max_dist):
    """float32 error of every cell [Ho*Wo]: min(float(|p - (R X + t)| * 100), maxDist) for valid cells, maxDist elsewhere"""
    err = np.full(co.shape[0], np.float32(max_dist), np.float32)
    d = cm[valid] - (co[valid] @ R.T + t)
    e = (np.sqrt((d * d).sum(1)) * 100.0).astype(np.float32)
    err[valid] = np.minimum(e, np.float32(max_dist))
    return err


def score_of(err, thr, alpha, Ho, Wo):
    thr = np.float32(thr)
    beta = np.float32(5.0) / thr
    st = (beta * (err - thr)).astype(np.float64)
    s = (1.0 - 1.0 / (1.0 + np.exp(-st))).sum()
    return s * float(np.float32(alpha) / np.float32(Wo) / np.float32(Ho))


def solve(coords, cam, n_hyp, thr, alpha, max_dist, cells=None, seed=0, max_tries=1000000):
    """coords, cam float32 [3,Ho,Wo].  `cells` [nHyp,3] (cell indices) replays a given sampling, otherwise hypotheses are drawn
    with numpy's generator.  Returns dict(pose cam->world [4,4] float64, R, t, scores, winner, round_counts, hyp (list of R, t))."""
    _, Ho, Wo = coords.shape
    co = np.asarray(coords, np.float64).reshape(3, -1).T
    cm = np.asarray(cam, np.float64).reshape(3, -1).T
    valid = valid_list(np.asarray(cam))
    if valid.size == 0:
        return dict(pose=np.eye(4), R=np.eye(3), t=np.zeros(3), scores=None, winner=0, round_counts=[], hyp=[])
    rng = np.random.default_rng(seed)
    hyp, scores = [], []
    for h in range(n_hyp):
        if cells is not None:
            idx = np.asarray(cells[h], np.int64)
            R, t, _ = kabsch_svd(cm[idx], co[idx])
        else:
            for _ in range(max_tries):
                idx = valid[rng.integers(0, valid.size, size=3)]
                R, t, _ = kabsch_svd(cm[idx], co[idx])
                res = np.linalg.norm(cm[idx] - (co[idx] @ R.T + t), axis=1) * 100.0
                if (res < thr).all():
                    break
        hyp.append((R, t))
        scores.append(score_of(error_map(R, t, co, cm, valid, max_dist), thr, alpha, Ho, Wo))
    scores = np.array(scores)
    winner = 0 if np.isnan(scores).any() else int(np.argmax(scores))      # argmax: first maximum
    R, t = hyp[winner]
    best, counts = 3, []
    is_valid = np.zeros(Ho * Wo, bool)
    is_valid[valid] = True
    for _ in range(MAX_REF_STEPS):
        inl = (error_map(R, t, co, cm, valid, max_dist) < np.float32(thr)) & is_valid
        counts.append(int(inl.sum()))
        if counts[-1] <= best:
            break
        best = counts[-1]
        R, t, _ = kabsch_svd(cm[inl], co[inl])
    pose = np.eye(4)
    pose[:3, :3] = R.T
    pose[:3, 3] = -R.T @ t
    return dict(pose=pose, R=R, t=t, scores=scores, winner=winner, round_counts=counts, hyp=hyp)
