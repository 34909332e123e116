"""Independent float64 numpy implementation of the ray-aware pose refinement behind the RGB-D solver — TEST INFRASTRUCTURE ONLY.

Written from the MODEL (include/crossloc_dsac.h), not from crossloc_amd/csrc/xl_dsac_rgbd_refine_math.h: the information matrix
of a cell is np.linalg.inv of its covariance a I + b rho rho^T (no Sherman-Morrison), its own Rodrigues formula, np.linalg.solve
and plain Gauss-Newton about the inlier centroid run to convergence where the product runs the solver's Levenberg-Marquardt; the
covariance is formed from the UNCENTRED Jacobian [[R X]x, -I] and a numpy inverse.  For the plain form `kabsch` is the closed-form
least-squares fit by SVD.  No float32 rounding anywhere, so a cell whose error sits on the threshold may fall on the other side
than in the product; callers compare poses only where the final inlier masks coincide."""
import numpy as np


def rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / (th * th) * (K @ K)


def skew(q):
    """[q]x for q [n,3] -> [n,3,3]"""
    z = np.zeros(len(q))
    return np.stack([np.stack([z, -q[:, 2], q[:, 1]], 1), np.stack([q[:, 2], z, -q[:, 0]], 1), np.stack([-q[:, 1], q[:, 0], z], 1)], 1)


def information(p, sigma, sigma_z, s0, k):
    """W [n,3,3] of cells with camera coordinates p [n,3]: the inverse of a I + b rho rho^T"""
    pn = np.linalg.norm(p, axis=1)
    rho = p / pn[:, None]
    a = s0 * s0 + sigma * sigma
    b = (sigma_z * sigma_z + np.square(k * p[:, 2])) * np.square(pn / p[:, 2])
    cov = a[:, None, None] * np.eye(3) + b[:, None, None] * rho[:, :, None] * rho[:, None, :]
    return np.linalg.inv(cov)


def kabsch(X, p):
    """The rigid least-squares fit p ~ R X + t by SVD -> (R, t)"""
    cX, cp = X.mean(0), p.mean(0)
    U, _, Vt = np.linalg.svd((p - cp).T @ (X - cX))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, cp - R @ cX


def refine(coords, cam, R, t, thr_cm, max_dist_cm, sigma=None, depth_sigma=None, depth_rel=0.0, s0=0.01, max_rounds=16,
           gn_iters=100):
    """coords, cam [3,Ho,Wo]; sigma, depth_sigma [Ho,Wo] or None; world->camera start {R, t}.  Returns dict(R, t, mask [Ho,Wo]
    bool: the set of the last completed round, rounds, converged, status (0 ok, 1 fewer than 3 inliers at the start, 2 first
    round failed), chi2, JtJ, cov [6,6] in the row's parameters at the result, n, n_bad)."""
    _, Ho, Wo = np.shape(coords)
    X = np.asarray(coords, np.float64).reshape(3, -1).T
    p = np.asarray(cam, np.float64).reshape(3, -1).T
    N = Ho * Wo
    valid = p[:, 2] != 0
    sg = np.zeros(N) if sigma is None else np.asarray(sigma, np.float64).reshape(-1)
    sz = np.zeros(N) if depth_sigma is None else np.asarray(depth_sigma, np.float64).reshape(-1)
    usable = np.isfinite(sg) & (sg >= 0) & np.isfinite(sz) & (sz >= 0)
    cand = valid & usable
    plain = sigma is None and depth_sigma is None and depth_rel == 0
    W = np.zeros((N, 3, 3))
    W[cand] = np.eye(3) if plain else information(p[cand], sg[cand], sz[cand], s0, depth_rel)
    R, t = np.array(R, np.float64), np.array(t, np.float64)
    out = dict(R=R, t=t, mask=np.zeros((Ho, Wo), bool), rounds=0, converged=False, status=0, chi2=np.nan, cov=None, JtJ=None, n=0,
               n_bad=int((valid & ~usable).sum()))
    prev = None
    for k in range(max_rounds):
        r = p - (X @ R.T + t)
        inl = cand & (np.minimum(np.linalg.norm(r, axis=1) * 100.0, max_dist_cm) < thr_cm)
        if prev is not None and np.array_equal(inl, prev):
            out["converged"] = True
            break
        n = int(inl.sum())
        if n < 3:
            if k == 0:
                out["status"] = 1
            break
        Xi, pi, Wi = X[inl], p[inl], W[inl]
        Rk, tk = R, t
        c = (Xi @ Rk.T + tk).mean(0)
        ok = True
        for _ in range(gn_iters):
            m = Xi @ Rk.T + tk
            rr = pi - m
            J = np.concatenate([skew(m - c), -np.broadcast_to(np.eye(3), (n, 3, 3))], 2)         # d r / d (w, tau)
            A = np.einsum("nai,nab,nbj->ij", J, Wi, J)
            g = np.einsum("nai,nab,nb->i", J, Wi, rr)
            if not np.all(np.isfinite(A)) or np.linalg.cond(A) > 1e13:
                ok = False
                break
            d = np.linalg.solve(A, -g)
            E = rodrigues(d[:3])
            Rk, tk = E @ Rk, E @ (tk - c) + c + d[3:]
            if np.linalg.norm(d) < 1e-13 * (1.0 + np.linalg.norm(tk)):
                break
        if not ok:
            if k == 0:
                out["status"] = 2
            break
        R, t, prev = Rk, tk, inl
        rr = pi - (Xi @ R.T + t)
        J = np.concatenate([skew(Xi @ R.T), -np.broadcast_to(np.eye(3), (n, 3, 3))], 2)          # about R X, the row's parameters
        A = np.einsum("nai,nab,nbj->ij", J, Wi, J)
        chi2 = float(np.einsum("na,nab,nb->", rr, Wi, rr)) / (3 * n - 6)
        out.update(R=R, t=t, mask=inl.reshape(Ho, Wo), rounds=k + 1, chi2=chi2, JtJ=A, cov=chi2 * np.linalg.inv(A), n=n)
    return out


def c2w(R, t):
    T = np.eye(4)
    T[:3, :3] = R.T
    T[:3, 3] = -R.T @ t
    return T
