/*
 * xl_dsac_rgbd_bwd_math.h — the lane-local arithmetic of the RGB-D DSAC* backward pass, on top of xl_dsac_rgbd_math.h.
 *
 * The closed-form adjoint of the Horn (quaternion) Kabsch fit, the eigen-gap guard, the rotation Jacobian of a three-point
 * fit, dL/dR and dL/dt of the pose loss taken from dloss, and the per-cell derivative weight of the soft-inlier score.
 * Two consumers include it:
 *
 *   crossloc_amd/csrc/xl_dsac_rgbd_bwd.hip   the product: kernels K0-K4
 *   tests/dsac_rgbd_bwd_ref.c                test infrastructure: the same orchestration restated serially in C99 for gcc
 *
 * Contract as in xl_dsac_rgbd_math.h: lane-local code only, -ffp-contract=off, expression order is part of the interface.
 *
 * The adjoint.  The fit is R = R(q), t = c_p - R c_X with q the eigenvector of the largest eigenvalue of the symmetric 4x4
 * N(A), A = sum_k (p_k - c_p)(X_k - c_X)^T.  For a scalar L(R, t) with G_R = dL/dR and g_t = dL/dt:
 *     G' = G_R - g_t c_X^T                                   (t depends on R through -R c_X)
 *     g_q = (dR/dq)^T G'
 *     u = sum_{m != top} v_m (v_m . g_q) / (lambda_top - lambda_m)    (first-order perturbation of a simple eigenvector)
 *     H_ij = u^T N(E_ij) q = dL/dA_ij                        (N is linear in A)
 *     dL/dX_k = H^T (p_k - c_p) - R^T g_t / n                (the centring of X cancels: sum_k (p_k - c_p) = 0)
 * u is orthogonal to q, so the radial part of g_q (R(q) as written is not scale invariant) drops out, and the sign of q
 * cancels between u and q.
 */
#ifndef XL_DSAC_RGBD_BWD_MATH_H
#define XL_DSAC_RGBD_BWD_MATH_H

#include "xl_dsac_rgbd_math.h"

/* eigen-gap guard: the fit is treated as not unique (no derivative) when (lambda_top - lambda_second) / max_m |lambda_m| is
 * at or below this bound.  For three points the ratio is 2 s2 / (s1 + s2) of the singular values of A, about twice the
 * squared aspect ratio of the triangle: collinear or repeated points give 0 up to rounding (~1e-16).  The adjoint divides
 * by the gap, so its relative rounding error is about DBL_EPSILON / ratio: 2e-8 at the bound. */
#define XLR_GAP_REL 1.0e-8
/* path-II guard: largest entry of the 3x9 rotation Jacobian d omega / d X of the support points, rad / m */
#define XLR_MAX_DOMEGA 10.0
#define XLR_BWD_REC 64

/* relative eigen-gap of the fit; returns true when the guard fires (also for NaN) */
XL_MATH_FN bool rgbd_eig_gap(const HornEig *e, double *relGap)
{
    double top = e->lam[0];
    if (e->top == 1) top = e->lam[1];
    if (e->top == 2) top = e->lam[2];
    if (e->top == 3) top = e->lam[3];
    double second = 0.0, scale = 0.0;
    bool have = false;
    XL_MATH_UNROLL
    for (int m = 0; m < 4; ++m) {
        double a = fabs(e->lam[m]);
        if (a > scale) scale = a;
        if (m != e->top && (!have || e->lam[m] > second)) { second = e->lam[m]; have = true; }
    }
    double rel = (scale > 0.0) ? (top - second) / scale : 0.0;
    *relGap = rel;
    return !(rel > XLR_GAP_REL);
}

/* H[3 i + j] = dL/dA_ij of the fit with eigen-decomposition e and scene centroid cX, for G_R (row-major 3x3) and g_t */
XL_MATH_CALL_FN void rgbd_kabsch_adjoint(const HornEig *e, const double *cX, const double *GR, const double *gt, double *H)
{
    double G[9];
    XL_MATH_UNROLL
    for (int i = 0; i < 3; ++i)
        XL_MATH_UNROLL
        for (int j = 0; j < 3; ++j) G[3 * i + j] = GR[3 * i + j] - gt[i] * cX[j];
    const double q0 = e->q[0], qx = e->q[1], qy = e->q[2], qz = e->q[3];
    /* g_q[a] = sum_ij G_ij dR_ij / dq_a, R as rgbd_kabsch_fit_eig writes it */
    double gq[4];
    gq[0] = 2.0 * (q0 * G[0] - qz * G[1] + qy * G[2] + qz * G[3] + q0 * G[4] - qx * G[5] - qy * G[6] + qx * G[7] + q0 * G[8]);
    gq[1] = 2.0 * (qx * G[0] + qy * G[1] + qz * G[2] + qy * G[3] - qx * G[4] - q0 * G[5] + qz * G[6] + q0 * G[7] - qx * G[8]);
    gq[2] = 2.0 * (-(qy * G[0]) + qx * G[1] + q0 * G[2] + qx * G[3] + qy * G[4] + qz * G[5] - q0 * G[6] + qz * G[7] - qy * G[8]);
    gq[3] = 2.0 * (-(qz * G[0]) - q0 * G[1] + qx * G[2] + q0 * G[3] - qz * G[4] + qy * G[5] + qx * G[6] + qy * G[7] + qz * G[8]);
    double top = e->lam[0];
    if (e->top == 1) top = e->lam[1];
    if (e->top == 2) top = e->lam[2];
    if (e->top == 3) top = e->lam[3];
    double u[4] = { 0.0, 0.0, 0.0, 0.0 };
    XL_MATH_UNROLL
    for (int m = 0; m < 4; ++m) {
        double dot = e->V[m] * gq[0] + e->V[4 + m] * gq[1] + e->V[8 + m] * gq[2] + e->V[12 + m] * gq[3];
        double c = dot / (top - e->lam[m]);
        if (m != e->top) {
            u[0] += e->V[m] * c; u[1] += e->V[4 + m] * c; u[2] += e->V[8 + m] * c; u[3] += e->V[12 + m] * c;
        }
    }
    /* u^T N q split by the entries of N: diagonal products and symmetric off-diagonal pairs */
    double d0 = u[0] * q0, d1 = u[1] * qx, d2 = u[2] * qy, d3 = u[3] * qz;
    double s01 = u[0] * qx + u[1] * q0, s02 = u[0] * qy + u[2] * q0, s03 = u[0] * qz + u[3] * q0;
    double s12 = u[1] * qy + u[2] * qx, s13 = u[1] * qz + u[3] * qx, s23 = u[2] * qz + u[3] * qy;
    /* N00 = Sxx+Syy+Szz, N11 = Sxx-Syy-Szz, N22 = -Sxx+Syy-Szz, N33 = -Sxx-Syy+Szz, N01 = Syz-Szy, N02 = Szx-Sxz,
     * N03 = Sxy-Syx, N12 = Sxy+Syx, N13 = Szx+Sxz, N23 = Syz+Szy with S_ab = A[b][a] */
    H[0] = d0 + d1 - d2 - d3;          /* Sxx = A[0] */
    H[1] = s12 - s03;                  /* Syx = A[1] */
    H[2] = s02 + s13;                  /* Szx = A[2] */
    H[3] = s03 + s12;                  /* Sxy = A[3] */
    H[4] = d0 - d1 + d2 - d3;          /* Syy = A[4] */
    H[5] = s23 - s01;                  /* Szy = A[5] */
    H[6] = s13 - s02;                  /* Sxz = A[6] */
    H[7] = s01 + s23;                  /* Syz = A[7] */
    H[8] = d0 - d1 - d2 + d3;          /* Szz = A[8] */
}

/* out = H^T d */
XL_MATH_FN void rgbd_Ht_mul(const double *H, double d0, double d1, double d2, double *out)
{
    out[0] = H[0] * d0 + H[3] * d1 + H[6] * d2;
    out[1] = H[1] * d0 + H[4] * d1 + H[7] * d2;
    out[2] = H[2] * d0 + H[5] * d1 + H[8] * d2;
}

/* v = R^T g / n */
XL_MATH_FN void rgbd_Rt_mul_div(const double *R, const double *g, double n, double *v)
{
    v[0] = (R[0] * g[0] + R[3] * g[1] + R[6] * g[2]) / n;
    v[1] = (R[1] * g[0] + R[4] * g[1] + R[7] * g[2]) / n;
    v[2] = (R[2] * g[0] + R[5] * g[1] + R[8] * g[2]) / n;
}

/* G_R = dL/dR (row-major) and g_t = dL/dt of the pose loss at `est`, from dloss: it is linear in its dR argument, so three
 * calls with unit columns (call m: dR_{m c} / dr_c = 1) read off row m of dL/dR; every quirk of dloss is kept */
XL_MATH_CALL_FN void rgbd_loss_grad(const Pose *est, const Gt *g, double wRot, double wTrans, double cut, double *GR, double *gt)
{
    XL_MATH_NO_UNROLL
    for (int m = 0; m < 3; ++m) {
        double dR[27], jac[6];
        for (int i = 0; i < 27; ++i) dR[i] = 0.0;
        for (int c = 0; c < 3; ++c) dR[(3 * m + c) * 3 + c] = 1.0;
        dloss(est, dR, g, wRot, wTrans, cut, jac);
        for (int c = 0; c < 3; ++c) GR[3 * m + c] = jac[c];
        if (m == 0) { gt[0] = jac[3]; gt[1] = jac[4]; gt[2] = jac[5]; }
    }
}

/* the minimal fit of a hypothesis once more, with its eigen-decomposition and centroids (the sums of rgbd_try_fit) */
XL_MATH_FN void rgbd_fit3_eig(const double *pc, const double *Xw, Pose *out, HornEig *e, double *cp, double *cX)
{
    double s[XLR_SUMS_CENTROID], a[XLR_SUMS_COV];
    XL_MATH_UNROLL
    for (int k = 0; k < XLR_SUMS_CENTROID; ++k) s[k] = 0.0;
    XL_MATH_UNROLL
    for (int k = 0; k < XLR_SUMS_COV; ++k) a[k] = 0.0;
    XL_MATH_UNROLL
    for (int j = 0; j < 3; ++j)
        rgbd_acc_centroid(s, pc[3 * j], pc[3 * j + 1], pc[3 * j + 2], Xw[3 * j], Xw[3 * j + 1], Xw[3 * j + 2]);
    rgbd_centroids(s, cp, cX);
    XL_MATH_UNROLL
    for (int j = 0; j < 3; ++j)
        rgbd_acc_cov(a, cp, cX, pc[3 * j], pc[3 * j + 1], pc[3 * j + 2], Xw[3 * j], Xw[3 * j + 1], Xw[3 * j + 2]);
    rgbd_kabsch_fit_eig(cp, cX, a, out, e);
}

/* largest |d omega_c / d X_k| over the three support points of a minimal fit, delta R = [delta omega]x R:
 * omega_0 = (dR R^T)_21, omega_1 = (dR R^T)_02, omega_2 = (dR R^T)_10, i.e. G_R has row a = row b of R */
XL_MATH_CALL_FN double rgbd_max_domega(const HornEig *e, const Pose *p, const double *pc, const double *cp, const double *cX)
{
    double mx = 0.0;
    const double zero[3] = { 0.0, 0.0, 0.0 };
    XL_MATH_NO_UNROLL
    for (int c = 0; c < 3; ++c) {
        const int a = (c == 0) ? 2 : (c == 1) ? 0 : 1, b = (c == 0) ? 1 : (c == 1) ? 2 : 0;
        double GR[9], H[9];
        for (int i = 0; i < 9; ++i) GR[i] = 0.0;
        for (int j = 0; j < 3; ++j) GR[3 * a + j] = p->R[3 * b + j];
        rgbd_kabsch_adjoint(e, cX, GR, zero, H);
        for (int k = 0; k < 3; ++k) {
            double g[3];
            rgbd_Ht_mul(H, pc[3 * k] - cp[0], pc[3 * k + 1] - cp[1], pc[3 * k + 2] - cp[2], g);
            for (int j = 0; j < 3; ++j) { double v = fabs(g[j]); if (v > mx || v != v) mx = v; }
        }
    }
    return mx;
}

/* derivative weight of a valid cell under pose p: w = dE/d err_cm = -s (1 - s) beta softmaxGrad (alpha / W / H), s the sigmoid
 * of rgbd_soft_term's float argument, and dhat = d / (|d| + EPS) of the metre residual d of rgbd_dist_cm.  Returns false (the
 * cell contributes nothing) when its unclamped float error exceeds maxDist. */
XL_MATH_FN bool rgbd_cell_weight(const Pose *p, double X, double Y, double Z, double px, double py, double pz,
                                 float maxDist, float beta, float thr, double sog, float facf, double *w, double *dhat)
{
    double dx = px - (p->R[0] * X + p->R[1] * Y + p->R[2] * Z + p->t[0]);
    double dy = py - (p->R[3] * X + p->R[4] * Y + p->R[5] * Z + p->t[1]);
    double dz = pz - (p->R[6] * X + p->R[7] * Y + p->R[8] * Z + p->t[2]);
    double n = sqrt(dx * dx + dy * dy + dz * dz);
    float a = (float)(n * 100.0);
    if (!(a <= maxDist)) return false;
    float stf = beta * (a - thr);
    double st = 1.0 / (1.0 + det_exp(-(double)stf));
    double dRep = -st * (1.0 - st) * (double)beta * sog;
    dRep *= (double)facf;
    *w = dRep;
    double inv = 1.0 / (n + XLM_EPS);
    dhat[0] = dx * inv; dhat[1] = dy * inv; dhat[2] = dz * inv;
    return true;
}

/* direct term of a cell: w * (-100 R^T dhat) */
XL_MATH_FN void rgbd_cell_direct(const Pose *p, double w, const double *dhat, double *out)
{
    out[0] = w * (-100.0 * (p->R[0] * dhat[0] + p->R[3] * dhat[1] + p->R[6] * dhat[2]));
    out[1] = w * (-100.0 * (p->R[1] * dhat[0] + p->R[4] * dhat[1] + p->R[7] * dhat[2]));
    out[2] = w * (-100.0 * (p->R[2] * dhat[0] + p->R[5] * dhat[1] + p->R[8] * dhat[2]));
}

/* the twelve score sums of a cell: s[0..8] += w (-100 dhat X^T) row-major, s[9..11] += w (-100 dhat) */
XL_MATH_FN void rgbd_acc_score_sums(double *s, double w, const double *dhat, double X, double Y, double Z)
{
    XL_MATH_UNROLL
    for (int i = 0; i < 3; ++i) {
        double c = w * (-100.0 * dhat[i]);
        s[3 * i] += c * X; s[3 * i + 1] += c * Y; s[3 * i + 2] += c * Z;
        s[9 + i] += c;
    }
}

/* soft-max over the scores (dsacstar_util.h:684-704): probability of hypothesis h */
XL_MATH_FN double rgbd_softmax_prob(const double *sc, int nHyp, int h)
{
    double maxScore = 0.0, sum = 0.0;
    for (int i = 0; i < nHyp; ++i) if (i == 0 || sc[i] > maxScore) maxScore = sc[i];
    for (int i = 0; i < nHyp; ++i) sum += det_exp(sc[i] - maxScore);
    return det_exp(sc[h] - maxScore) / sum;
}

#endif  /* XL_DSAC_RGBD_BWD_MATH_H */
