/*
 * xl_dsac_refine_math.h — the lane-local arithmetic of the uncertainty-weighted pose refinement, written once.
 *
 * The pass takes ONE pose per image (usually the one the solver returned) and re-fits it over the inliers by iteratively
 * re-weighted Levenberg-Marquardt: cell i, whose network-predicted standard deviation is sigma_i metres, enters the normal
 * equations with the weight w_i = 1 / (s0^2 + (f sigma_i / z_i)^2) - the inverse variance in pixels^2 of its reprojection
 * residual under an isotropic 3-D Gaussian of that sigma at camera depth z_i, floored by the pixel noise s0.  Same conventions
 * as xl_dsac_math.h and xl_dsac_quality_math.h, on which this header sits: the common subset of C99 and HIP C++, only
 * + - * / sqrt and comparisons, compiled with -ffp-contract=off on both sides.  The weighted per-cell normal equations
 * (pnp_cell_normal_eq_w), the step-size stop (lm_step_small) and the LM constants are the solver's, in xl_dsac_math.h; this
 * header keeps the weight, the row and what the rounds report.  Two consumers:
 *
 *   crossloc_amd/csrc/xl_dsac_refine.hip   the product: one 256-thread workgroup per image, the canonical block reduction
 *   tests/pose_refine_ref.c                test infrastructure: the same orchestration restated serially in C99 for gcc
 *
 * A ROUND starts at pose P_k.  Its inlier set { i : cell_err(P_k, i) < thr, sigma_i usable } and its weights (from the depths
 * at P_k) stay fixed while Levenberg-Marquardt moves the pose; the weights are recomputed from P_k at every evaluation, not
 * stored.  Fixed weights keep the estimating equation sum w_i J_i^T r_i = 0 unbiased: weights that followed the moving pose
 * would reward poses that push the cells to larger depths.  Parameters and increment: the world -> camera pose {R, t} with
 * apply_step, as everywhere else.  Row layout and status codes: include/crossloc_dsac.h.
 */
#ifndef XL_DSAC_REFINE_MATH_H
#define XL_DSAC_REFINE_MATH_H

#include "xl_dsac_quality_math.h"

#define XLR_ROW 64                     /* doubles per output row */
#define XLR_COL_N_MASKED 63            /* masked pass: the cells the mask ruled out (quality_row_n_masked; 0.0 in the unmasked row) */
#define XLR_MAX_ROUNDS 16              /* upper limit of the max_rounds argument */
#define XLR_LG_RAISES 34               /* damping raises per iteration: lg climbs from >= -16 to 17 at most */
#define XLR_STATUS_OK 0.0
#define XLR_STATUS_FEW_INLIERS 1.0     /* fewer than 4 inliers at the input pose */
#define XLR_STATUS_FIRST_ROUND 2.0     /* the first round failed: not positive definite / LM breakdown / pose not finite */
#define XLR_STATUS_BAD_POSE 3.0        /* an input pose entry is not finite */

/* a sigma the model cannot use: not finite, or negative */
XL_MATH_FN bool refine_sigma_bad(double sigma) { return !quality_finite(sigma) || sigma < 0.0; }

/* weight of a cell with scene coordinate (X, Y, Z) and standard deviation sigma at the round's pose pk; s0sq = s0 * s0.
 * The inverse depth is formed as XL_PNP_CELL_ROWS forms it (z == 0 is read as 1).  sigma == 0 with s0 == 1 gives
 * exactly 1.0. */
XL_MATH_FN double refine_weight(const Pose *pk, double X, double Y, double Z, double sigma, double s0sq, const Cam *cam)
{
    double qz = pk->R[6] * X + pk->R[7] * Y + pk->R[8] * Z;
    double zc = qz + pk->t[2];
    double z = (zc != 0.0) ? 1.0 / zc : 1.0;
    double g = cam->f * sigma * z;
    return 1.0 / (s0sq + g * g);
}

/* the weighted per-cell normal equations, the step-size stop and the iteration cap under the names this pass had for them,
 * kept for restatements and hooks written against those: one-line forwards to xl_dsac_math.h (pnp_cell_normal_eq_w,
 * lm_step_small, XLM_LM_MAX_ITER), which the kernels and refine_cell use directly */
#define XLR_LM_MAX_ITER XLM_LM_MAX_ITER
XL_MATH_FN void refine_cell_normal_eq(const Pose *p, double X, double Y, double Z, double w, int y, int x, const Cam *cam,
                                      double *a)
{
    pnp_cell_normal_eq_w(p, X, Y, Z, w, y, x, cam, a);
}
XL_MATH_FN bool refine_step_small(const double *d, const Pose *prev) { return lm_step_small(d, prev); }

/* everything an inlier cell adds to a thread's 28 partials in one evaluation: the weight from the round's pose pk (1.0 without
 * a sigma map), the normal equations at the moving pose p */
XL_MATH_FN void refine_cell(const Pose *pk, const Pose *p, double X, double Y, double Z, double sigma, bool hasSigma, double s0sq,
                            int y, int x, const Cam *cam, double *a)
{
    double w = hasSigma ? refine_weight(pk, X, Y, Z, sigma, s0sq, cam) : 1.0;
    pnp_cell_normal_eq_w(p, X, Y, Z, w, y, x, cam, a);
}

/* [61], [62] of the row: the angle of Rout Rin^T in degrees and the distance of the two camera centres C = -R^T t */
XL_MATH_CALL_FN void refine_moved(const Pose *in, const Pose *out, double *deg, double *metres)
{
    double D[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            D[3 * i + j] = out->R[3 * i] * in->R[3 * j] + out->R[3 * i + 1] * in->R[3 * j + 1] + out->R[3 * i + 2] * in->R[3 * j + 2];
    double sx = D[7] - D[5], sy = D[2] - D[6], sz = D[3] - D[1];
    double s = 0.5 * sqrt(sx * sx + sy * sy + sz * sz);
    double c = 0.5 * (D[0] + D[4] + D[8] - 1.0);
    *deg = det_atan2(s, c) * (180.0 / XLM_CV_PI);
    double d2 = 0.0;
    for (int i = 0; i < 3; ++i) {
        double ci = -(in->R[i] * in->t[0] + in->R[3 + i] * in->t[1] + in->R[6 + i] * in->t[2]);
        double co = -(out->R[i] * out->t[0] + out->R[3 + i] * out->t[1] + out->R[6 + i] * out->t[2]);
        d2 += (co - ci) * (co - ci);
    }
    *metres = sqrt(d2);
}

/* the per-image step from what the rounds left to the output row (layout: include/crossloc_dsac.h).
 *   status     XLR_STATUS_*;  with BAD_POSE nothing else is read
 *   n0, bad    inliers at the input pose, cells with an unusable sigma
 *   cost0      weighted cost of the first evaluation (input pose)
 *   nLast, ne  inliers of the last completed round and the 28 weighted sums of its last evaluation, which is at the output
 *              pose over that round's set and weights; when no round completed (status 1, 2): n0 and the first evaluation
 *   in, out    world -> camera poses; out == in when no round completed
 * NaN pattern as in the pose-quality row: status 1, 2 leave [7..9] and [31..57] NaN, status 3 everything but [0] and [6]. */
XL_MATH_CALL_FN void refine_row(double status, const Cam *cam, double n0, double bad, double cost0, double nLast,
                                const double *ne, int rounds, int evals, int converged, const Pose *in, const Pose *out,
                                double *row)
{
    const double qnan = quality_nan();
    row[0] = (double)cam->N;
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
    for (int i = 0; i < 21; ++i) row[10 + i] = ne[i];
    for (int i = 31; i < 58; ++i) row[i] = qnan;
    row[58] = (double)rounds;
    row[59] = (double)evals;
    row[60] = (double)converged;
    row[61] = 0.0; row[62] = 0.0; row[63] = 0.0;
    if (status != XLR_STATUS_OK) return;
    refine_moved(in, out, &row[61], &row[62]);

    const double chi2 = ne[27] / (2.0 * nLast - 6.0);    /* 2n residuals, 6 parameters; n >= 4 */
    row[7] = sqrt(chi2);
    double inv[36];
    if (!quality_inv6(ne, inv)) return;                  /* J^T W J at the output pose not positive definite: no covariance */
    double S[36];
    for (int i = 0; i < 36; ++i) S[i] = chi2 * inv[i];
    {
        int k = 0;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) row[31 + k++] = S[6 * r + c];
    }
    quality_center_tail(S, out, row);
}

#endif  /* XL_DSAC_REFINE_MATH_H */
