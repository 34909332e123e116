/*
 * xl_dsac_rgbd_refine_math.h — the lane-local arithmetic of the ray-aware uncertainty-weighted pose refinement behind the RGB-D
 * solver, written once on top of xl_dsac_rgbd_quality_math.h (residual, centring, NaN and finiteness) and xl_dsac_refine_math.h
 * (the round / Levenberg-Marquardt constants, the step-size stop, the status codes, how far the pose moved).
 *
 * The pass takes ONE pose per image (usually the one the RGB-D solver returned) and re-fits it over its inliers with a full 3x3
 * information matrix per cell.  m = R X + t is the predicted camera point of a cell, r = p - m its residual in metres.  The
 * scene coordinate carries isotropic noise a = s0^2 + sigma^2; the depth carries noise along the unit viewing ray rho = p / |p|
 * with variance b = (sigma_z^2 + (k z)^2) |p|^2 / z^2.  The covariance of r is a I + b rho rho^T and its inverse, by
 * Sherman-Morrison, W = (I - b / (a + b) rho rho^T) / a.  rho, a and b belong to the measurement: they do not depend on the pose.
 * Everything is accumulated about the round's inlier centroid c of m, in the parameters (rotation w about c, centroid
 * translation tau): m' = Exp(w) (m - c) + c + tau, dr = [u]x w - tau with u = m - c.  Two consumers:
 *
 *   crossloc_amd/csrc/xl_dsac_rgbd_refine.hip   the product: one 256-thread workgroup per image, the canonical block reduction
 *   tests/rgbd_refine_ref.c                     test infrastructure: the same orchestration restated serially in C99 for gcc
 *
 * Arithmetic contract as in xl_dsac_math.h: + - * / sqrt only, -ffp-contract=off on both sides, expression order is part of the
 * interface.  Row layout and status codes: include/crossloc_dsac.h.
 */
#ifndef XL_DSAC_RGBD_REFINE_MATH_H
#define XL_DSAC_RGBD_REFINE_MATH_H

#include "xl_dsac_rgbd_quality_math.h"
#include "xl_dsac_refine_math.h"

/* the round-start walk, reduced per image */
#define XLRR_SUMS0 8
#define XLRR_S_COUNT 0                 /* inliers at the round's pose */
#define XLRR_S_BAD 1                   /* valid cells left out for an unusable sigma or sigma_z */
#define XLRR_S_VALID 2                 /* valid cells (camera z != 0) */
#define XLRR_S_DIFF 3                  /* cells whose inlier decision differs between the round's pose and the previous round's */
#define XLRR_S_M 4                     /* sum of m over the inliers (3); [7] unused */

#define XLRR_COL_VALID 63              /* n_valid in the row */

/* s0sq: the floor variance s0^2, 1.0 in the plain form; k: the relative depth noise */
typedef struct { float thr, maxDist; int Ho, Wo, N; double s0sq, k; } RgbdR;

/* the plain form: no sigma map, no sigma_z map, k == 0.  Every W is then the identity and s0 is not used */
XL_MATH_FN double rgbdr_s0sq(bool hasSigma, bool hasSigmaZ, float k, float s0)
{
    if (!hasSigma && !hasSigmaZ && k == 0.0f) return 1.0;
    return (double)s0 * (double)s0;
}

/* a cell the model cannot use: sigma or sigma_z not finite, or negative (a missing map is passed as 0) */
XL_MATH_FN bool rgbdr_unusable(double sigma, double sigmaZ) { return refine_sigma_bad(sigma) || refine_sigma_bad(sigmaZ); }

/* noise of the valid cell with camera coordinate p: the isotropic variance a, the along-ray variance b and the unit ray rho */
XL_MATH_FN void rgbdr_noise(double px, double py, double pz, double sigma, double sigmaZ, double s0sq, double k,
                            double *a, double *b, double *rho)
{
    double pn2 = px * px + py * py + pz * pz;
    double pn = sqrt(pn2);
    double kz = k * pz;
    rho[0] = px / pn; rho[1] = py / pn; rho[2] = pz / pn;
    *a = s0sq + sigma * sigma;
    *b = (sigmaZ * sigmaZ + kz * kz) * pn2 / (pz * pz);
}

/* out = W v,  W = (I - b / (a + b) rho rho^T) / a.  a == 1 and b == 0 return v itself */
XL_MATH_FN void rgbdr_apply_w(double a, double b, const double *rho, const double *v, double *out)
{
    double beta = b / (a + b);
    double dot = rho[0] * v[0] + rho[1] * v[1] + rho[2] * v[2];
    out[0] = (v[0] - beta * rho[0] * dot) / a;
    out[1] = (v[1] - beta * rho[1] * dot) / a;
    out[2] = (v[2] - beta * rho[2] * dot) / a;
}

/* contribution of one cell to the 28 normal-equation sums at pose p about the centre c, under the information matrix of
 * (a, b, rho):  acc[0..20] += upper triangle of J^T W J (row-major), acc[21..26] += J^T W r, acc[27] += r^T W r, with
 * J = dr / d(w, tau) = [[u]x, -I], u = m - c. */
XL_MATH_FN void rgbdr_cell_normal_eq(const Pose *p, double X, double Y, double Z, double px, double py, double pz, const double *c,
                                     double a, double b, const double *rho, double *acc)
{
    double m[3], r[3];
    rgbdq_residual(p, X, Y, Z, px, py, pz, m, r);
    double u0 = m[0] - c[0], u1 = m[1] - c[1], u2 = m[2] - c[2];
    double J[6][3], WJ[6][3], Wr[3];
    J[0][0] = 0.0;  J[0][1] = u2;   J[0][2] = -u1;
    J[1][0] = -u2;  J[1][1] = 0.0;  J[1][2] = u0;
    J[2][0] = u1;   J[2][1] = -u0;  J[2][2] = 0.0;
    J[3][0] = -1.0; J[3][1] = 0.0;  J[3][2] = 0.0;
    J[4][0] = 0.0;  J[4][1] = -1.0; J[4][2] = 0.0;
    J[5][0] = 0.0;  J[5][1] = 0.0;  J[5][2] = -1.0;
    XL_MATH_UNROLL
    for (int i = 0; i < 6; ++i) rgbdr_apply_w(a, b, rho, J[i], WJ[i]);
    rgbdr_apply_w(a, b, rho, r, Wr);
    int k = 0;
    XL_MATH_UNROLL
    for (int i = 0; i < 6; ++i)
        XL_MATH_UNROLL
        for (int j = i; j < 6; ++j) { acc[k] += J[i][0] * WJ[j][0] + J[i][1] * WJ[j][1] + J[i][2] * WJ[j][2]; ++k; }
    XL_MATH_UNROLL
    for (int i = 0; i < 6; ++i) acc[21 + i] += J[i][0] * Wr[0] + J[i][1] * Wr[1] + J[i][2] * Wr[2];
    acc[27] += r[0] * Wr[0] + r[1] * Wr[1] + r[2] * Wr[2];
}

/* the inlier decision of a usable valid cell at `pose`: the solver's clamp and float comparison */
XL_MATH_FN bool rgbdr_inlier(const Pose *pose, double X, double Y, double Z, float px, float py, float pz, const RgbdR *q)
{
    return rgbd_cell_err(pose, X, Y, Z, (double)px, (double)py, (double)pz, q->maxDist) < q->thr;
}

/* round-start walk: everything one cell adds to the XLRR_SUMS0 partials.  pose: the round's pose; prev: the previous round's
 * pose when hasPrev (the decision under both, their mismatches counted: zero mismatches <=> equal sets) */
XL_MATH_FN void rgbdr_cell_start(const Pose *pose, const Pose *prev, bool hasPrev, double X, double Y, double Z,
                                 float px, float py, float pz, double sigma, double sigmaZ, const RgbdR *q, double *a)
{
    if (!(pz != 0.0f)) return;
    a[XLRR_S_VALID] += 1.0;
    if (rgbdr_unusable(sigma, sigmaZ)) { a[XLRR_S_BAD] += 1.0; return; }
    bool in = rgbdr_inlier(pose, X, Y, Z, px, py, pz, q);
    if (hasPrev && in != rgbdr_inlier(prev, X, Y, Z, px, py, pz, q)) a[XLRR_S_DIFF] += 1.0;
    if (in) {
        double m[3], r[3];
        rgbdq_residual(pose, X, Y, Z, (double)px, (double)py, (double)pz, m, r);
        a[XLRR_S_COUNT] += 1.0;
        a[XLRR_S_M] += m[0]; a[XLRR_S_M + 1] += m[1]; a[XLRR_S_M + 2] += m[2];
    }
}

/* the round's centre from the reduced sums of its start walk (no inliers: the origin) */
XL_MATH_FN void rgbdr_centroid(const double *s0, double *c)
{
    double n = s0[XLRR_S_COUNT];
    if (n > 0.0) { c[0] = s0[XLRR_S_M] / n; c[1] = s0[XLRR_S_M + 1] / n; c[2] = s0[XLRR_S_M + 2] / n; }
    else { c[0] = 0.0; c[1] = 0.0; c[2] = 0.0; }
}

/* evaluation walk: everything one cell adds to a thread's 28 partials: the inlier decision at the round's pose pk, with the same
 * bits as the start walk, the noise of the measurement, the normal equations at the moving pose p about c */
XL_MATH_FN void rgbdr_cell_eval(const Pose *pk, const Pose *p, double X, double Y, double Z, float px, float py, float pz,
                                double sigma, double sigmaZ, const RgbdR *q, const double *c, double *acc)
{
    if (!(pz != 0.0f)) return;
    if (rgbdr_unusable(sigma, sigmaZ)) return;
    if (!rgbdr_inlier(pk, X, Y, Z, px, py, pz, q)) return;
    double a, b, rho[3];
    rgbdr_noise((double)px, (double)py, (double)pz, sigma, sigmaZ, q->s0sq, q->k, &a, &b, rho);
    rgbdr_cell_normal_eq(p, X, Y, Z, (double)px, (double)py, (double)pz, c, a, b, rho, acc);
}

/* param = prev (-) d in (rotation about c, centroid translation): R = E R_prev with E = Exp(-d_w) as apply_step forms it,
 * t = c + E (t_prev - c) - d_t; E (t_prev - c) is formed as R (R_prev^T (t_prev - c)) */
XL_MATH_FN void rgbdr_apply_step(const Pose *prev, const double *c, const double *d, Pose *out)
{
    apply_step(prev, d, out);
    double k0 = prev->t[0] - c[0], k1 = prev->t[1] - c[1], k2 = prev->t[2] - c[2];
    double v0 = prev->R[0] * k0 + prev->R[3] * k1 + prev->R[6] * k2;
    double v1 = prev->R[1] * k0 + prev->R[4] * k1 + prev->R[7] * k2;
    double v2 = prev->R[2] * k0 + prev->R[5] * k1 + prev->R[8] * k2;
    out->t[0] = (c[0] + (out->R[0] * v0 + out->R[1] * v1 + out->R[2] * v2)) - d[3];
    out->t[1] = (c[1] + (out->R[3] * v0 + out->R[4] * v1 + out->R[5] * v2)) - d[4];
    out->t[2] = (c[2] + (out->R[6] * v0 + out->R[7] * v1 + out->R[8] * v2)) - d[5];
}

/* the normal matrix of a round (upper triangle ut) has a Cholesky factor whose pivots all stay above XLQR_PIVOT_REL times
 * their diagonal entry: the relative test of the RGB-D quality row (inliers on one line leave a rotation unobserved, and
 * rounding alone would leave a tiny positive pivot) */
XL_MATH_FN bool rgbdr_well_posed(const double *ut)
{
    double A[6][6], L[6][6];
    {
        int k = 0;
        XL_MATH_UNROLL
        for (int r = 0; r < 6; ++r)
            XL_MATH_UNROLL
            for (int c = r; c < 6; ++c) { A[r][c] = ut[k]; A[c][r] = ut[k]; ++k; }
    }
    XL_MATH_UNROLL
    for (int i = 0; i < 6; ++i)
        XL_MATH_UNROLL
        for (int j = 0; j < 6; ++j) L[i][j] = 0.0;
    bool ok = true;
    XL_MATH_UNROLL
    for (int j = 0; j < 6; ++j) {
        double s = A[j][j];
        XL_MATH_UNROLL
        for (int m = 0; m < j; ++m) s -= L[j][m] * L[j][m];
        if (!(s > XLQR_PIVOT_REL * A[j][j]) || !quality_finite(s)) ok = false;
        double ljj = sqrt(s);
        L[j][j] = ljj;
        XL_MATH_UNROLL
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
            XL_MATH_UNROLL
            for (int m = 0; m < j; ++m) v -= L[i][m] * L[j][m];
            L[i][j] = v / ljj;
        }
    }
    return ok;
}

/* out = T^T S T for full 6x6 row-major matrices */
XL_MATH_CALL_FN void rgbdr_congruence(const double *T, const double *S, double *out)
{
    double ST[36];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double v = 0.0;
            for (int m = 0; m < 6; ++m) v += S[6 * i + m] * T[6 * m + j];
            ST[6 * i + j] = v;
        }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double v = 0.0;
            for (int m = 0; m < 6; ++m) v += T[6 * m + i] * ST[6 * m + j];
            out[6 * i + j] = v;
        }
}

/* the maps between the centred parameters (w, tau) and the row's (w, d), R' = Exp(w) R, t' = t + d: d = tau - K w with
 * K = [t - c]x, i.e. (w, d) = G (w, tau), G = [[I, 0], [-K, I]], the G of the RGB-D quality row.
 * Gi = G^-1 = [[I, 0], [K, I]] and Gt = G^T, both full 6x6 row-major */
XL_MATH_CALL_FN void rgbdr_g_maps(const Pose *pose, const double *c, double *Gi, double *Gt)
{
    const double k0 = pose->t[0] - c[0], k1 = pose->t[1] - c[1], k2 = pose->t[2] - c[2];
    const double K[9] = { 0.0, -k2, k1, k2, 0.0, -k0, -k1, k0, 0.0 };
    for (int i = 0; i < 36; ++i) { Gi[i] = 0.0; Gt[i] = 0.0; }
    for (int i = 0; i < 6; ++i) { Gi[6 * i + i] = 1.0; Gt[6 * i + i] = 1.0; }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            Gi[6 * (3 + i) + j] = K[3 * i + j];
            Gt[6 * j + 3 + i] = -K[3 * i + j];
        }
}

/* the per-image step from what the rounds left to the output row (layout: include/crossloc_dsac.h).
 *   status        XLR_STATUS_* (FEW_INLIERS here: fewer than 3);  with BAD_POSE nothing else is read
 *   n0, bad, nValid   inliers at the input pose, valid cells with an unusable sigma or sigma_z, valid cells
 *   cost0         cost r^T W r of the first evaluation (input pose)
 *   nLast, ne, c  inliers of the last completed round, the 28 sums of the closing evaluation at `out` over that round's set,
 *                 and the centre they were formed about; when no round completed (status 1, 2): n0 and the first evaluation
 *   in, out       world -> camera poses as read from the float matrices the caller gave and receives; out == in when no round
 *                 completed
 * JtJ = G^-T (J^T W J) G^-1 and Sigma = G (chi^2 (J^T W J)^-1) G^T in the row's parameters.  NaN pattern as in the sibling:
 * status 1, 2 leave [7..9] and [31..57] NaN, status 3 everything but [0] and [6]. */
XL_MATH_CALL_FN void rgbdr_row(double status, const RgbdR *q, double n0, double bad, double nValid, double cost0, double nLast,
                               const double *ne, const double *c, int rounds, int evals, int converged, const Pose *in,
                               const Pose *out, double *row)
{
    const double qnan = quality_nan();
    row[0] = (double)q->N;
    if (status == XLR_STATUS_BAD_POSE) {
        for (int i = 1; i < XLR_ROW; ++i) row[i] = qnan;
        row[6] = status;
        return;
    }
    row[1] = nLast;
    row[2] = n0;
    row[3] = cost0;
    row[4] = ne[27];
    row[5] = bad;
    row[6] = status;
    for (int i = 7; i < 10; ++i) row[i] = qnan;
    for (int i = 31; i < 58; ++i) row[i] = qnan;
    row[58] = (double)rounds;
    row[59] = (double)evals;
    row[60] = (double)converged;
    row[61] = 0.0; row[62] = 0.0;
    row[XLRR_COL_VALID] = nValid;

    double H[36], Gi[36], Gt[36], T[36];
    {
        int k = 0;
        for (int r = 0; r < 6; ++r)
            for (int cc = r; cc < 6; ++cc) { H[6 * r + cc] = ne[k]; H[6 * cc + r] = ne[k]; ++k; }
    }
    rgbdr_g_maps(out, c, Gi, Gt);
    rgbdr_congruence(Gi, H, T);
    {
        int k = 0;
        for (int r = 0; r < 6; ++r)
            for (int cc = r; cc < 6; ++cc) row[10 + k++] = T[6 * r + cc];
    }
    if (status != XLR_STATUS_OK) return;
    refine_moved(in, out, &row[61], &row[62]);

    const double chi2 = ne[27] / (3.0 * nLast - 6.0);    /* 3n residuals, 6 parameters; n >= 3 */
    row[7] = sqrt(chi2);
    double inv[36];
    if (!quality_inv6(ne, inv)) return;                  /* J^T W J at the output pose not positive definite: no covariance */
    for (int i = 0; i < 36; ++i) inv[i] = chi2 * inv[i];
    double S[36];
    rgbdr_congruence(Gt, inv, S);
    {
        int k = 0;
        for (int r = 0; r < 6; ++r)
            for (int cc = r; cc < 6; ++cc) row[31 + k++] = S[6 * r + cc];
    }
    quality_center_tail(S, out, row);
}

#endif  /* XL_DSAC_RGBD_REFINE_MATH_H */
