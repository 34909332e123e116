/*
 * xl_dsac_quality_math.h — the lane-local arithmetic of the per-frame pose-quality pass, written once.
 *
 * The pass looks at ONE pose per image (usually the one the solver returned) and reports how far it can be trusted: the
 * inlier statistics at that pose, JtJ of the reprojection residuals over the inliers, and the covariance that follows
 * from it.  Same conventions as xl_dsac_math.h, which this header includes: the common subset of C99 and HIP C++, only
 * + - * / sqrt and comparisons, compiled with -ffp-contract=off on both sides.  What a cell adds to the sums is the solver's
 * own arithmetic and lives there (cell_err, soft_inlier_st, pnp_cell_normal_eq, cam_make); this header keeps what only the
 * quality passes need: the finiteness tests, the 6x6 inverse, the covariance and the row.  Two consumers:
 *
 *   crossloc_amd/csrc/xl_dsac_quality.hip   the product: one 256-thread workgroup per image, the canonical block reduction
 *   tests/pose_quality_ref.c                test infrastructure: the same orchestration restated serially in C99 for gcc
 *
 * Parameters of the covariance: (wx, wy, wz, tx, ty, tz) with R' = Exp(w) R, t' = t + d on the world -> camera pose
 * {R, t} - the increment the Levenberg-Marquardt refinement uses (apply_step in xl_dsac_math.h).
 */
#ifndef XL_DSAC_QUALITY_MATH_H
#define XL_DSAC_QUALITY_MATH_H

#include "xl_dsac_math.h"

#define XLQ_SUMS 32                    /* reduced per image: 28 normal-equation sums + the four below */
#define XLQ_S_COUNT 28                 /* number of inliers */
#define XLQ_S_SOFT 29                  /* soft-inlier sum over ALL cells */
#define XLQ_S_ERR 30                   /* sum of e over the inliers (e: the float cell error, widened) */
#define XLQ_S_ERR2 31                  /* sum of e^2 over the inliers */

#define XLQ_ROW 64                     /* doubles per output row; layout: include/crossloc_dsac.h */
#define XLQ_COL_N_MASKED 58            /* masked passes: the cells the mask ruled out (0.0 in the unmasked row) */
#define XLQ_STATUS_OK 0.0
#define XLQ_STATUS_FEW_INLIERS 1.0     /* fewer than 4 inliers */
#define XLQ_STATUS_NOT_PD 2.0          /* JtJ is not positive definite */
#define XLQ_STATUS_BAD_POSE 3.0        /* a pose entry is not finite */

XL_MATH_FN double quality_nan(void) { return bits_f64(0x7ff8000000000000ULL); }

/* finite <=> x - x is zero (inf - inf and nan - nan are NaN) */
XL_MATH_FN bool quality_finite(double x) { return x - x == 0.0; }

/* the entries of a float 4x4 cam->world pose that gt_from_pose16 reads (rows 0..2) are all finite */
XL_MATH_FN bool quality_pose16_finite(const float *p16)
{
    bool ok = true;
    for (int i = 0; i < 12; ++i) if (!quality_finite((double)p16[i])) ok = false;
    return ok;
}

XL_MATH_FN bool quality_pose_finite(const Pose *p)
{
    bool ok = true;
    for (int i = 0; i < 9; ++i) if (!quality_finite(p->R[i])) ok = false;
    for (int i = 0; i < 3; ++i) if (!quality_finite(p->t[i])) ok = false;
    return ok;
}

/* the world -> camera pose a float 4x4 cam->world matrix stands for: gt_from_pose16's {R2, t2}, what backward_rgb uses */
XL_MATH_CALL_FN void quality_pose_from16(const float *p16, Pose *p)
{
    Gt g;
    gt_from_pose16(p16, &g);
    for (int i = 0; i < 9; ++i) p->R[i] = g.R2[i];
    for (int i = 0; i < 3; ++i) p->t[i] = g.t2[i];
}

/* the pass's earlier name for the solver's per-cell normal equations, kept for restatements and hooks written against it:
 * a one-line forward to pnp_cell_normal_eq of xl_dsac_math.h.  quality_cell calls the target itself: through one more
 * force-inlined layer hipcc orders the kernel's cell loop differently (tools/kernel_asm_diff.py) */
XL_MATH_FN void quality_cell_normal_eq(const Pose *p, double X, double Y, double Z, int y, int x, const Cam *cam, double *a)
{
    pnp_cell_normal_eq(p, X, Y, Z, y, x, cam, a);
}

/* everything one cell adds to the 32 per-thread partials: the solver's soft-inlier term (soft_inlier_st) over all cells,
 * and for an inlier the solver's 28 normal-equation sums (pnp_cell_normal_eq), both of xl_dsac_math.h */
XL_MATH_FN void quality_cell(const Pose *p, double X, double Y, double Z, int y, int x, const Cam *cam, float beta, double *a)
{
    float e = cell_err(p, X, Y, Z, y, x, cam);
    a[XLQ_S_SOFT] += 1.0 - soft_inlier_st(e, cam->thr, beta);
    if (e < cam->thr) {                                  /* the float comparison the refinement makes */
        pnp_cell_normal_eq(p, X, Y, Z, y, x, cam, a);
        a[XLQ_S_COUNT] += 1.0;
        a[XLQ_S_ERR] += (double)e;
        a[XLQ_S_ERR2] += (double)e * (double)e;
    }
}

/* inverse of the symmetric 6x6 whose upper triangle (row-major, 21 values) is ut: Cholesky A = L L^T, M = L^-1,
 * A^-1 = M^T M; inv is the full matrix, row-major.  false on breakdown (a pivot that is not positive, or a result that
 * is not finite), as solve6 reports it. */
XL_MATH_FN bool quality_inv6(const double *ut, double *inv)
{
    double A[6][6], L[6][6], M[6][6];
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
        for (int j = 0; j < 6; ++j) { L[i][j] = 0.0; M[i][j] = 0.0; }
    bool ok = true;
    XL_MATH_UNROLL
    for (int j = 0; j < 6; ++j) {
        double s = A[j][j];
        XL_MATH_UNROLL
        for (int m = 0; m < j; ++m) s -= L[j][m] * L[j][m];
        if (!(s > 0.0)) ok = false;
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
    if (!ok) return false;
    /* M = L^-1 by forward substitution, column by column */
    XL_MATH_UNROLL
    for (int c = 0; c < 6; ++c) {
        M[c][c] = 1.0 / L[c][c];
        XL_MATH_UNROLL
        for (int i = c + 1; i < 6; ++i) {
            double v = 0.0;
            XL_MATH_UNROLL
            for (int m = c; m < i; ++m) v -= L[i][m] * M[m][c];
            M[i][c] = v / L[i][i];
        }
    }
    XL_MATH_UNROLL
    for (int r = 0; r < 6; ++r)
        XL_MATH_UNROLL
        for (int c = r; c < 6; ++c) {
            double v = 0.0;
            XL_MATH_UNROLL
            for (int m = c; m < 6; ++m) v += M[m][r] * M[m][c];
            inv[6 * r + c] = v;
            inv[6 * c + r] = v;
            if (!quality_finite(v)) ok = false;
        }
    return ok;
}

/* what follows from the pose covariance S (full 6x6, row-major, parameters (w, d) as above) at the world -> camera pose:
 * row[52..57] the covariance of the camera centre, row[8] sigma_pos_m, row[9] sigma_rot_deg.  Shared with the RGB-D row
 * (xl_dsac_rgbd_quality_math.h). */
XL_MATH_CALL_FN void quality_center_tail(const double *S, const Pose *pose, double *row)
{
    /* camera centre C = -R^T t in world coordinates: dC = A (w, d) with A = [ -R^T [t]x , -R^T ] (3x6) */
    const double *R = pose->R, *t = pose->t;
    const double tx[9] = { 0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0 };
    double A[18], AS[18];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            A[6 * i + j] = -(R[i] * tx[j] + R[3 + i] * tx[3 + j] + R[6 + i] * tx[6 + j]);
            A[6 * i + 3 + j] = -R[3 * j + i];
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 6; ++j) {
            double v = 0.0;
            for (int m = 0; m < 6; ++m) v += A[6 * i + m] * S[6 * m + j];
            AS[6 * i + j] = v;
        }
    double SC[9];
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            double v = 0.0;
            for (int m = 0; m < 6; ++m) v += AS[6 * i + m] * A[6 * j + m];
            SC[3 * i + j] = v;
        }
    row[52] = SC[0]; row[53] = SC[1]; row[54] = SC[2]; row[55] = SC[4]; row[56] = SC[5]; row[57] = SC[8];
    row[8] = sqrt(SC[0] + SC[4] + SC[8]);
    row[9] = sqrt(S[0] + S[7] + S[14]) * (180.0 / XLM_CV_PI);
}

/* the per-image step from the 32 reduced sums to the output row (layout: include/crossloc_dsac.h).  pose: world -> camera;
 * poseOk false: a pose entry was not finite and the sums were not formed. */
XL_MATH_CALL_FN void quality_row(const double *s, const Pose *pose, const Cam *cam, bool poseOk, double *row)
{
    const double qnan = quality_nan();
    row[0] = (double)cam->N;
    if (!poseOk) {
        for (int i = 1; i < XLQ_ROW; ++i) row[i] = qnan;
        row[6] = XLQ_STATUS_BAD_POSE;
        return;
    }
    const float fac = cam->alpha / (float)cam->Wo / (float)cam->Ho;
    const double n = s[XLQ_S_COUNT];
    row[1] = n;
    row[2] = s[XLQ_S_SOFT] * (double)fac;
    row[3] = s[XLQ_S_ERR];
    row[4] = s[XLQ_S_ERR2];
    row[5] = s[27];
    for (int i = 0; i < 21; ++i) row[10 + i] = s[i];
    for (int i = 7; i < 10; ++i) row[i] = qnan;
    for (int i = 31; i < 58; ++i) row[i] = qnan;
    for (int i = 58; i < XLQ_ROW; ++i) row[i] = 0.0;
    if (n < 4.0) { row[6] = XLQ_STATUS_FEW_INLIERS; return; }
    double inv[36];
    if (!quality_inv6(s, inv)) { row[6] = XLQ_STATUS_NOT_PD; return; }
    row[6] = XLQ_STATUS_OK;

    const double var = s[27] / (2.0 * n - 6.0);          /* 2n residuals, 6 parameters */
    row[7] = sqrt(var);
    double S[36];
    for (int i = 0; i < 36; ++i) S[i] = var * inv[i];
    {
        int k = 0;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) row[31 + k++] = S[6 * r + c];
    }
    quality_center_tail(S, pose, row);
}

/* the masked passes' one change to a finished row (quality_row: col XLQ_COL_N_MASKED, refine_row: XLR_COL_N_MASKED): the
 * number of masked-out cells in place of the unmasked row's 0.0; with status 3 the column stays NaN like its neighbours
 * (both rows keep their status in [6], and XLR_STATUS_BAD_POSE == XLQ_STATUS_BAD_POSE) */
XL_MATH_FN void quality_row_n_masked(double *row, int col, double nMasked)
{
    if (row[6] != XLQ_STATUS_BAD_POSE) row[col] = nMasked;
}

#endif  /* XL_DSAC_QUALITY_MATH_H */
