"""Independent float64 numpy implementation of the uncertainty-weighted pose refinement — TEST INFRASTRUCTURE ONLY.

Written from the MODEL (include/crossloc_dsac.h), not from crossloc_amd/csrc/xl_dsac_refine_math.h: its own Rodrigues formula,
its own analytic Jacobian, np.linalg.solve and plain Gauss-Newton run to convergence where the product runs the solver's
Levenberg-Marquardt.  No float32 rounding anywhere, so a cell whose error sits on the threshold may fall on the other side
than in the product; callers compare poses only where the final inlier masks coincide.

Model.  A round starts at pose P_k = {R, t} (world -> camera).  Inliers: cells whose reprojection error at P_k is below thr and
whose sigma is finite and not negative.  Weights: w = 1 / (s0^2 + (f sigma / z)^2) with z the camera depth at P_k (all 1 when
sigma is None).  The round minimises sum w |r|^2 over the pose with set and weights fixed; rounds repeat until the set no longer
changes."""
import numpy as np


def rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / (th * th) * (K @ K)


def pixels(Ho, Wo, sub):
    ys, xs = np.divmod(np.arange(Ho * Wo), Wo)
    return np.stack([xs * sub + sub // 2, ys * sub + sub // 2], 1).astype(np.float64)


def residuals(R, t, X, px, f, cx, cy):
    """X [N,3] world, px [N,2] -> (r [N,2] pixels, q [N,3] camera points)"""
    q = X @ R.T + t
    uv = np.stack([f * q[:, 0] / q[:, 2] + cx, f * q[:, 1] / q[:, 2] + cy], 1)
    return uv - px, q


def jacobians(R, t, X, f):
    """d r / d (w, d) for R' = Exp(w) R, t' = t + d: [N,2,6]"""
    q = X @ R.T + t
    p = X @ R.T                                      # R X: the rotated point, which the rotation increment turns
    iz = 1.0 / q[:, 2]
    N = len(X)
    dq = np.zeros((N, 3, 6))
    # d q / d w = -[p]x, d q / d d = I
    dq[:, 0, 1], dq[:, 0, 2] = p[:, 2], -p[:, 1]
    dq[:, 1, 0], dq[:, 1, 2] = -p[:, 2], p[:, 0]
    dq[:, 2, 0], dq[:, 2, 1] = p[:, 1], -p[:, 0]
    dq[:, 0, 3] = dq[:, 1, 4] = dq[:, 2, 5] = 1.0
    du = np.zeros((N, 2, 3))
    du[:, 0, 0] = f * iz
    du[:, 0, 2] = -f * q[:, 0] * iz * iz
    du[:, 1, 1] = f * iz
    du[:, 1, 2] = -f * q[:, 1] * iz * iz
    return du @ dq


def refine(coords, sigma, R, t, thr, f, cx, cy, sub, s0=1.0, max_rounds=16, gn_iters=100):
    """coords [3,Ho,Wo], sigma [Ho,Wo] or None, world->camera start {R, t}.  Returns dict(R, t, mask [Ho,Wo] bool: the set of
    the last completed round, rounds, converged, status (0 ok, 1 fewer than 4 inliers at the start, 2 first round failed),
    chi2, cov [6,6] = chi2 (J^T W J)^-1 at the result, n)."""
    coords = np.asarray(coords, np.float64)
    _, Ho, Wo = coords.shape
    X = coords.reshape(3, -1).T
    px = pixels(Ho, Wo, sub)
    R, t = np.array(R, np.float64), np.array(t, np.float64)
    usable = np.ones(Ho * Wo, bool)
    sg = None
    if sigma is not None:
        sg = np.asarray(sigma, np.float64).reshape(-1)
        usable = np.isfinite(sg) & (sg >= 0)
    out = dict(R=R, t=t, mask=np.zeros((Ho, Wo), bool), rounds=0, converged=False, status=0, chi2=np.nan, cov=None, n=0)
    prev = None
    for k in range(max_rounds):
        r, q = residuals(R, t, X, px, f, cx, cy)
        inl = usable & (np.hypot(r[:, 0], r[:, 1]) < thr)
        if prev is not None and np.array_equal(inl, prev):
            out["converged"] = True
            break
        if inl.sum() < 4:
            if k == 0:
                out["status"] = 1
            break
        w = np.ones(inl.sum()) if sg is None else 1.0 / (s0 * s0 + np.square(f * sg[inl] / q[inl, 2]))
        Xi, pi = X[inl], px[inl]
        Rk, tk = R, t
        ok = True
        for _ in range(gn_iters):
            rr, _ = residuals(Rk, tk, Xi, pi, f, cx, cy)
            J = jacobians(Rk, tk, Xi, f)
            A = np.einsum("n,nai,naj->ij", w, J, J)
            g = np.einsum("n,nai,na->i", w, J, rr)
            try:
                d = np.linalg.solve(A, -g)
            except np.linalg.LinAlgError:
                ok = False
                break
            if not np.all(np.isfinite(d)):
                ok = False
                break
            Rk, tk = rodrigues(d[:3]) @ Rk, tk + d[3:]
            if np.linalg.norm(d) < 1e-13 * (1.0 + np.linalg.norm(tk)):
                break
        if not ok:
            if k == 0:
                out["status"] = 2
            break
        R, t, prev = Rk, tk, inl
        rr, _ = residuals(R, t, Xi, pi, f, cx, cy)
        J = jacobians(R, t, Xi, f)
        A = np.einsum("n,nai,naj->ij", w, J, J)
        n = int(inl.sum())
        chi2 = float(np.sum(w[:, None] * rr * rr)) / (2 * n - 6)
        out.update(R=R, t=t, mask=inl.reshape(Ho, Wo), rounds=k + 1, chi2=chi2, cov=chi2 * np.linalg.inv(A), n=n)
    return out


def c2w(R, t):
    T = np.eye(4)
    T[:3, :3] = R.T
    T[:3, 3] = -R.T @ t
    return T
