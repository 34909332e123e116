/*
 * xl_dsac_rgbd_quality_math.h — the lane-local arithmetic of the per-frame RGB-D pose-quality pass, written once on top of
 * xl_dsac_rgbd_math.h (cell error, soft-inlier term, depth -> camera coordinate) and xl_dsac_quality_math.h (NaN, finiteness,
 * the pose of a float 4x4, the camera-centre tail of the row).
 *
 * The pass looks at ONE pose per image (usually the one the RGB-D solver returned) and rates it by its metric 3-D residuals
 * r = p - m, m = R X + t (p: camera coordinate of a cell, X: its scene coordinate, metres).  The covariance is that of the
 * unweighted rigid least-squares fit the refinement performs on the inliers, with isotropic noise of sigma metres per axis,
 * sigma^2 = SSE / (3 n - 6).  Everything is accumulated about the inlier centroid c of m in the camera frame: with u = m - c
 * and C = sum u u^T the fit decouples into a rotation about c with information M = tr(C) I - C and the centroid translation
 * tau with information n I.  The row reports JtJ and the covariance in the parameters of the RGB row, (w, d) with
 * R' = Exp(w) R, t' = t + d, through the linear map d = tau - [t - c]x w.  Two consumers:
 *
 *   crossloc_amd/csrc/xl_dsac_rgbd_quality.hip   the product: one 256-thread workgroup per image, two walks, canonical reductions
 *   tests/rgbd_quality_ref.c                     test infrastructure: the same orchestration restated serially in C99 for gcc
 *
 * Arithmetic contract as in xl_dsac_math.h: + - * / sqrt only, -ffp-contract=off on both sides, expression order is part of
 * the interface.
 */
#ifndef XL_DSAC_RGBD_QUALITY_MATH_H
#define XL_DSAC_RGBD_QUALITY_MATH_H

#include "xl_dsac_rgbd_math.h"
#include "xl_dsac_quality_math.h"

/* walk 1, reduced per image */
#define XLQR_SUMS1 9
#define XLQR_S_VALID 0                 /* number of valid cells (camera z != 0) */
#define XLQR_S_COUNT 1                 /* number of inliers */
#define XLQR_S_M 2                     /* sum of m over the inliers (3) */
#define XLQR_S_SOFT 5                  /* soft-inlier sum over the VALID cells */
#define XLQR_S_ERR 6                   /* sum of e over the inliers (e: the float cell error in cm, widened) */
#define XLQR_S_ERR2 7                  /* sum of e^2 over the inliers */
#define XLQR_S_SSE 8                   /* sum of |r|^2 over the inliers, m^2 */
/* walk 2, reduced per image */
#define XLQR_SUMS2 12
#define XLQR_S_C 0                     /* C = sum u u^T: xx xy xz yy yz zz */
#define XLQR_S_GW 6                    /* sum u x r (3): the gradient of the fit w.r.t. a rotation about c */
#define XLQR_S_GT 9                    /* sum r (3): the gradient w.r.t. the translation */

#define XLQR_PIVOT_REL 1e-12           /* a Cholesky pivot of M not above this times its diagonal entry: degenerate */

#define XLQR_COL_VALID 58              /* n_valid in the row */

typedef struct { float thr, alpha, maxDist; int Ho, Wo, N; } RgbdQ;

/* m = R X + t and r = p - m, the expressions of rgbd_dist_cm */
XL_MATH_FN void rgbdq_residual(const Pose *p, double X, double Y, double Z, double px, double py, double pz, double *m, double *r)
{
    m[0] = p->R[0] * X + p->R[1] * Y + p->R[2] * Z + p->t[0];
    m[1] = p->R[3] * X + p->R[4] * Y + p->R[5] * Z + p->t[1];
    m[2] = p->R[6] * X + p->R[7] * Y + p->R[8] * Z + p->t[2];
    r[0] = px - m[0];
    r[1] = py - m[1];
    r[2] = pz - m[2];
}

/* walk 1: everything one cell with scene coordinate (X, Y, Z) and camera coordinate (px, py, pz) adds to the 9 partials */
XL_MATH_FN void rgbdq_cell1(const Pose *p, double X, double Y, double Z, float px, float py, float pz, const RgbdQ *q, float beta,
                            double *a)
{
    if (!(pz != 0.0f)) return;                           /* invalid: enters the soft score in the final step */
    float e = rgbd_cell_err(p, X, Y, Z, (double)px, (double)py, (double)pz, q->maxDist);
    a[XLQR_S_VALID] += 1.0;
    a[XLQR_S_SOFT] += rgbd_soft_term(e, beta, q->thr);
    if (e < q->thr) {                                    /* the float comparison the refinement makes */
        double m[3], r[3];
        rgbdq_residual(p, X, Y, Z, (double)px, (double)py, (double)pz, m, r);
        a[XLQR_S_COUNT] += 1.0;
        a[XLQR_S_M] += m[0]; a[XLQR_S_M + 1] += m[1]; a[XLQR_S_M + 2] += m[2];
        a[XLQR_S_ERR] += (double)e;
        a[XLQR_S_ERR2] += (double)e * (double)e;
        a[XLQR_S_SSE] += r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    }
}

/* the inlier centroid of m from the reduced sums of walk 1 (no inliers: the origin) */
XL_MATH_FN void rgbdq_centroid(const double *s1, double *c)
{
    double n = s1[XLQR_S_COUNT];
    if (n > 0.0) { c[0] = s1[XLQR_S_M] / n; c[1] = s1[XLQR_S_M + 1] / n; c[2] = s1[XLQR_S_M + 2] / n; }
    else { c[0] = 0.0; c[1] = 0.0; c[2] = 0.0; }
}

/* walk 2: the inlier decision again, with the same bits, and the 12 centred partials */
XL_MATH_FN void rgbdq_cell2(const Pose *p, double X, double Y, double Z, float px, float py, float pz, const RgbdQ *q,
                            const double *c, double *a)
{
    if (!(pz != 0.0f)) return;
    float e = rgbd_cell_err(p, X, Y, Z, (double)px, (double)py, (double)pz, q->maxDist);
    if (e < q->thr) {
        double m[3], r[3];
        rgbdq_residual(p, X, Y, Z, (double)px, (double)py, (double)pz, m, r);
        double u0 = m[0] - c[0], u1 = m[1] - c[1], u2 = m[2] - c[2];
        a[XLQR_S_C] += u0 * u0;     a[XLQR_S_C + 1] += u0 * u1; a[XLQR_S_C + 2] += u0 * u2;
        a[XLQR_S_C + 3] += u1 * u1; a[XLQR_S_C + 4] += u1 * u2; a[XLQR_S_C + 5] += u2 * u2;
        a[XLQR_S_GW] += u1 * r[2] - u2 * r[1];
        a[XLQR_S_GW + 1] += u2 * r[0] - u0 * r[2];
        a[XLQR_S_GW + 2] += u0 * r[1] - u1 * r[0];
        a[XLQR_S_GT] += r[0]; a[XLQR_S_GT + 1] += r[1]; a[XLQR_S_GT + 2] += r[2];
    }
}

/* inverse of the symmetric 3x3 whose upper triangle (xx xy xz yy yz zz) is ut: Cholesky A = L L^T, N = L^-1, A^-1 = N^T N;
 * inv is the full matrix, row-major.  false on breakdown: a pivot that is not above XLQR_PIVOT_REL times its diagonal
 * entry, or a pivot or result that is not finite.  *minRatio: the smallest pivot / diagonal entry met (0 for a zero or
 * negative diagonal entry). */
XL_MATH_FN bool rgbdq_inv3(const double *ut, double *inv, double *minRatio)
{
    double A[3][3], L[3][3], N[3][3];
    A[0][0] = ut[0]; A[0][1] = ut[1]; A[0][2] = ut[2];
    A[1][0] = ut[1]; A[1][1] = ut[3]; A[1][2] = ut[4];
    A[2][0] = ut[2]; A[2][1] = ut[4]; A[2][2] = ut[5];
    XL_MATH_UNROLL
    for (int i = 0; i < 3; ++i)
        XL_MATH_UNROLL
        for (int j = 0; j < 3; ++j) { L[i][j] = 0.0; N[i][j] = 0.0; }
    bool ok = true;
    double worst = 1.0;
    XL_MATH_UNROLL
    for (int j = 0; j < 3; ++j) {
        double s = A[j][j];
        XL_MATH_UNROLL
        for (int m = 0; m < j; ++m) s -= L[j][m] * L[j][m];
        if (!(s > XLQR_PIVOT_REL * A[j][j]) || !quality_finite(s)) ok = false;
        double ratio = (A[j][j] > 0.0) ? s / A[j][j] : 0.0;
        if (!(ratio >= worst)) worst = ratio;
        double ljj = sqrt(s);
        L[j][j] = ljj;
        XL_MATH_UNROLL
        for (int i = j + 1; i < 3; ++i) {
            double v = A[i][j];
            XL_MATH_UNROLL
            for (int m = 0; m < j; ++m) v -= L[i][m] * L[j][m];
            L[i][j] = v / ljj;
        }
    }
    *minRatio = worst;
    if (!ok) return false;
    XL_MATH_UNROLL
    for (int c = 0; c < 3; ++c) {
        N[c][c] = 1.0 / L[c][c];
        XL_MATH_UNROLL
        for (int i = c + 1; i < 3; ++i) {
            double v = 0.0;
            XL_MATH_UNROLL
            for (int m = c; m < i; ++m) v -= L[i][m] * N[m][c];
            N[i][c] = v / L[i][i];
        }
    }
    XL_MATH_UNROLL
    for (int r = 0; r < 3; ++r)
        XL_MATH_UNROLL
        for (int c = r; c < 3; ++c) {
            double v = 0.0;
            XL_MATH_UNROLL
            for (int m = c; m < 3; ++m) v += N[m][r] * N[m][c];
            inv[3 * r + c] = v;
            inv[3 * c + r] = v;
            if (!quality_finite(v)) ok = false;
        }
    return ok;
}

/* the per-image step from the reduced sums of both walks to the output row (layout: include/crossloc_dsac.h).  pose: world ->
 * camera; c: the centroid walk 2 used; poseOk false: a pose entry was not finite and the sums were not formed.
 * minRatio (nullable): the smallest relative Cholesky pivot of M, NaN when M was not factored. */
XL_MATH_CALL_FN void rgbdq_row(const double *s1, const double *s2, const double *c, const Pose *pose, const RgbdQ *q, bool poseOk,
                               double *row, double *minRatio)
{
    const double qnan = quality_nan();
    if (minRatio) *minRatio = qnan;
    row[0] = (double)q->N;
    if (!poseOk) {
        for (int i = 1; i < XLQ_ROW; ++i) row[i] = qnan;
        row[6] = XLQ_STATUS_BAD_POSE;
        return;
    }
    const float beta = 5.0f / q->thr;
    const float fac = q->alpha / (float)q->Wo / (float)q->Ho;
    const double n = s1[XLQR_S_COUNT], nValid = s1[XLQR_S_VALID];
    /* the invalid cells all have the error maxDist and enter as one product, as in the solver's score */
    const double soft = s1[XLQR_S_SOFT] + ((double)q->N - nValid) * rgbd_soft_term(q->maxDist, beta, q->thr);
    row[1] = n;
    row[2] = soft * (double)fac;
    row[3] = s1[XLQR_S_ERR];
    row[4] = s1[XLQR_S_ERR2];
    row[5] = s1[XLQR_S_SSE];
    for (int i = 7; i < 10; ++i) row[i] = qnan;
    for (int i = 31; i < 58; ++i) row[i] = qnan;
    for (int i = 58; i < XLQ_ROW; ++i) row[i] = 0.0;
    row[XLQR_COL_VALID] = nValid;

    /* M = tr(C) I - C and K = [t - c]x */
    const double *C = s2 + XLQR_S_C;
    const double tr = C[0] + C[3] + C[5];
    const double Mu[6] = { tr - C[0], -C[1], -C[2], tr - C[3], -C[4], tr - C[5] };
    const double M[9] = { Mu[0], Mu[1], Mu[2], Mu[1], Mu[3], Mu[4], Mu[2], Mu[4], Mu[5] };
    const double k0 = pose->t[0] - c[0], k1 = pose->t[1] - c[1], k2 = pose->t[2] - c[2];
    const double K[9] = { 0.0, -k2, k1, k2, 0.0, -k0, -k1, k0, 0.0 };

    /* JtJ = G^-T diag(M, n I) G^-1 with G^-1 = [[I, 0], [K, I]]:  [[M + n K^T K, n K^T], [n K, n I]] */
    double J[36];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double ktk = K[i] * K[j] + K[3 + i] * K[3 + j] + K[6 + i] * K[6 + j];
            J[6 * i + j] = M[3 * i + j] + n * ktk;
            J[6 * i + 3 + j] = n * K[3 * j + i];
            J[6 * (3 + i) + j] = n * K[3 * i + j];
            J[6 * (3 + i) + 3 + j] = (i == j) ? n : 0.0;
        }
    {
        int k = 0;
        for (int r = 0; r < 6; ++r)
            for (int cc = r; cc < 6; ++cc) row[10 + k++] = J[6 * r + cc];
    }
    if (n < 3.0) { row[6] = XLQ_STATUS_FEW_INLIERS; return; }
    double P[9], ratio;
    const bool pd = rgbdq_inv3(Mu, P, &ratio);
    if (minRatio) *minRatio = ratio;
    if (!pd) { row[6] = XLQ_STATUS_NOT_PD; return; }
    row[6] = XLQ_STATUS_OK;

    const double var = s1[XLQR_S_SSE] / (3.0 * n - 6.0);  /* 3n residuals, 6 parameters */
    row[7] = sqrt(var);
    const double vt = var / n;
    for (int i = 0; i < 9; ++i) P[i] = var * P[i];
    /* cov = G diag(P, vt I) G^T with G = [[I, 0], [-K, I]]:  [[P, -P K^T], [-K P, K P K^T + vt I]] */
    double KP[9], S[36];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            KP[3 * i + j] = K[3 * i] * P[j] + K[3 * i + 1] * P[3 + j] + K[3 * i + 2] * P[6 + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            S[6 * i + j] = P[3 * i + j];
            S[6 * (3 + i) + j] = -KP[3 * i + j];
            S[6 * j + 3 + i] = -KP[3 * i + j];
        }
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            double v = KP[3 * i] * K[3 * j] + KP[3 * i + 1] * K[3 * j + 1] + KP[3 * i + 2] * K[3 * j + 2];
            if (i == j) v += vt;
            S[6 * (3 + i) + 3 + j] = v;
            S[6 * (3 + j) + 3 + i] = v;
        }
    {
        int k = 0;
        for (int r = 0; r < 6; ++r)
            for (int cc = r; cc < 6; ++cc) row[31 + k++] = S[6 * r + cc];
    }
    quality_center_tail(S, pose, row);
}

#endif  /* XL_DSAC_RGBD_QUALITY_MATH_H */
