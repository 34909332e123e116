/*
 * xl_dsac_rgbd_math.h — the lane-local arithmetic of the RGB-D DSAC* solver, written once on top of xl_dsac_math.h.
 *
 * Everything one GPU lane (or one iteration of a CPU loop) computes on its own: the depth -> camera-coordinate formula,
 * the sums a Kabsch fit is made of, the fit itself (Horn's quaternion form: largest eigenvector of a symmetric 4x4 by
 * cyclic Jacobi with a fixed number of sweeps), the three-point sampling try and the per-cell distance error with its
 * soft-inlier term.  Two consumers include it:
 *
 *   crossloc_amd/csrc/xl_dsac_rgbd.hip   the product: staging, ballots, wave / block reductions, selection, refinement loop
 *   tests/dsac_rgbd_ref.c                test infrastructure: the same orchestration restated serially in C99 for gcc
 * (and, through xl_dsac_rgbd_bwd_math.h, the backward pass: xl_dsac_rgbd_bwd.hip and tests/dsac_rgbd_bwd_ref.c)
 *
 * Arithmetic contract as in xl_dsac_math.h: + - * / sqrt and the header's polynomials only, -ffp-contract=off on both
 * sides, expression order is part of the interface.  Reference line numbers are relative to the reference project's
 * dsacstar/ directory.  Poses are world -> camera: p_cam = R X + t, with p the camera coordinate (metres) of a cell and
 * X its scene coordinate.
 */
#ifndef XL_DSAC_RGBD_MATH_H
#define XL_DSAC_RGBD_MATH_H

#include "xl_dsac_math.h"

#define XLR_JACOBI_SWEEPS 8            /* cyclic sweeps over the 6 off-diagonal pairs of the 4x4 (quadratic convergence) */
#define XLR_SUMS_CENTROID 7            /* count, sum p (3), sum X (3) */
#define XLR_SUMS_COV 9                 /* A = sum (p - c_p)(X - c_X)^T, row-major */

/* camera coordinates of cell (y, x) from its depth (dataloader/dataloader.py:456-475 of the reference project): the ray
 * through the cell's pixel centre times the depth, in float */
XL_MATH_FN void rgbd_cam_from_depth(float d, int y, int x, float f, float ppx, float ppy, int sub,
                                    float *cx, float *cy, float *cz)
{
    float rx = ((float)(x * sub + sub / 2) - ppx) / f;
    float ry = ((float)(y * sub + sub / 2) - ppy) / f;
    *cx = rx * d;
    *cy = ry * d;
    *cz = d;
}

/* ------------------------------------------------------------------------------ Kabsch (dsacstar_util_rgbd.h:237-302) */

/* first pass over a point set: count and coordinate sums */
XL_MATH_FN void rgbd_acc_centroid(double *s, double px, double py, double pz, double X, double Y, double Z)
{
    s[0] += 1.0;
    s[1] += px; s[2] += py; s[3] += pz;
    s[4] += X;  s[5] += Y;  s[6] += Z;
}

XL_MATH_FN void rgbd_centroids(const double *s, double *cp, double *cX)
{
    double n = s[0];
    cp[0] = s[1] / n; cp[1] = s[2] / n; cp[2] = s[3] / n;
    cX[0] = s[4] / n; cX[1] = s[5] / n; cX[2] = s[6] / n;
}

/* second pass: centred cross-covariance A[3 i + j] += (p - c_p)_i (X - c_X)_j */
XL_MATH_FN void rgbd_acc_cov(double *a, const double *cp, const double *cX,
                             double px, double py, double pz, double X, double Y, double Z)
{
    double dp0 = px - cp[0], dp1 = py - cp[1], dp2 = pz - cp[2];
    double dX0 = X - cX[0], dX1 = Y - cX[1], dX2 = Z - cX[2];
    a[0] += dp0 * dX0; a[1] += dp0 * dX1; a[2] += dp0 * dX2;
    a[3] += dp1 * dX0; a[4] += dp1 * dX1; a[5] += dp1 * dX2;
    a[6] += dp2 * dX0; a[7] += dp2 * dX1; a[8] += dp2 * dX2;
}

/* one Jacobi rotation of the symmetric 4x4 M in the (P, Q) plane, eigenvectors accumulated in the columns of V; an
 * off-diagonal entry that no longer changes either diagonal entry is set to zero instead (the sweeps after convergence
 * then cost comparisons only) */
#define XLR_ROTATE(P, Q)                                                            \
    do {                                                                            \
        double apq = M[P][Q];                                                       \
        double g = 100.0 * fabs(apq);                                               \
        if (fabs(M[P][P]) + g == fabs(M[P][P]) && fabs(M[Q][Q]) + g == fabs(M[Q][Q])) { \
            M[P][Q] = 0.0; M[Q][P] = 0.0;      /* below the rounding of both diagonal entries: converged */ \
        } else {                                                                    \
            double tau = (M[Q][Q] - M[P][P]) / (2.0 * apq);                         \
            double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau)); \
            double c = 1.0 / sqrt(1.0 + tt * tt), s = tt * c;                       \
            XL_MATH_UNROLL                                                          \
            for (int k = 0; k < 4; ++k) {                                           \
                double akp = M[k][P], akq = M[k][Q];                                \
                M[k][P] = c * akp - s * akq;                                        \
                M[k][Q] = s * akp + c * akq;                                        \
            }                                                                       \
            XL_MATH_UNROLL                                                          \
            for (int k = 0; k < 4; ++k) {                                           \
                double apk = M[P][k], aqk = M[Q][k];                                \
                M[P][k] = c * apk - s * aqk;                                        \
                M[Q][k] = s * apk + c * aqk;                                        \
            }                                                                       \
            XL_MATH_UNROLL                                                          \
            for (int k = 0; k < 4; ++k) {                                           \
                double vkp = V[k][P], vkq = V[k][Q];                                \
                V[k][P] = c * vkp - s * vkq;                                        \
                V[k][Q] = s * vkp + c * vkq;                                        \
            }                                                                       \
        }                                                                           \
    } while (0)

/* what the Jacobi sweeps leave behind: all four eigenpairs of N(A) (eigenvector m is the column V[4 i + m], i = 0..3), the
 * index of the FIRST largest eigenvalue and its eigenvector normalised once more (the quaternion of R).  The backward pass
 * (xl_dsac_rgbd_bwd_math.h) differentiates the fit through them. */
typedef struct { double lam[4]; double V[16]; double q[4]; int top; } HornEig;

/* The rigid fit from the centroids and the centred cross-covariance: the proper rotation R maximising trace(R A^T)
 * (= U diag(1, 1, det(U V^T)) V^T of the SVD A = U W V^T) and t = c_p - R c_X.  Horn's closed form: R is the rotation of
 * the unit quaternion that is the eigenvector of the largest eigenvalue of the symmetric 4x4 N(A).  A rank-2 A (three
 * points) or rank <= 1 A (repeated draws) needs no special case: a repeated largest eigenvalue only means that several
 * rotations are optimal, Jacobi still returns an orthonormal eigenbasis, the FIRST largest diagonal entry is taken, and
 * A == 0 leaves V = I, i.e. the identity rotation. */
XL_MATH_FN void rgbd_kabsch_fit_eig(const double *cp, const double *cX, const double *A, Pose *out, HornEig *e)
{
    /* S_ab = sum X_a p_b = A[b][a] */
    double Sxx = A[0], Sxy = A[3], Sxz = A[6];
    double Syx = A[1], Syy = A[4], Syz = A[7];
    double Szx = A[2], Szy = A[5], Szz = A[8];
    double M[4][4], V[4][4];
    M[0][0] = Sxx + Syy + Szz; M[0][1] = Syz - Szy;       M[0][2] = Szx - Sxz;        M[0][3] = Sxy - Syx;
    M[1][0] = M[0][1];         M[1][1] = Sxx - Syy - Szz; M[1][2] = Sxy + Syx;        M[1][3] = Szx + Sxz;
    M[2][0] = M[0][2];         M[2][1] = M[1][2];         M[2][2] = -Sxx + Syy - Szz; M[2][3] = Syz + Szy;
    M[3][0] = M[0][3];         M[3][1] = M[1][3];         M[3][2] = M[2][3];          M[3][3] = -Sxx - Syy + Szz;
    XL_MATH_UNROLL
    for (int i = 0; i < 4; ++i)
        XL_MATH_UNROLL
        for (int j = 0; j < 4; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    XL_MATH_NO_UNROLL
    for (int sweep = 0; sweep < XLR_JACOBI_SWEEPS; ++sweep) {
        XLR_ROTATE(0, 1); XLR_ROTATE(0, 2); XLR_ROTATE(0, 3);
        XLR_ROTATE(1, 2); XLR_ROTATE(1, 3); XLR_ROTATE(2, 3);
    }
    double lam = M[0][0];
    int top = 0;
    double q0 = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
    if (M[1][1] > lam) { lam = M[1][1]; top = 1; q0 = V[0][1]; qx = V[1][1]; qy = V[2][1]; qz = V[3][1]; }
    if (M[2][2] > lam) { lam = M[2][2]; top = 2; q0 = V[0][2]; qx = V[1][2]; qy = V[2][2]; qz = V[3][2]; }
    if (M[3][3] > lam) { lam = M[3][3]; top = 3; q0 = V[0][3]; qx = V[1][3]; qy = V[2][3]; qz = V[3][3]; }
    double nq = sqrt(q0 * q0 + qx * qx + qy * qy + qz * qz);
    q0 = q0 / nq; qx = qx / nq; qy = qy / nq; qz = qz / nq;
    XL_MATH_UNROLL
    for (int i = 0; i < 4; ++i) {
        e->lam[i] = M[i][i];
        XL_MATH_UNROLL
        for (int j = 0; j < 4; ++j) e->V[4 * i + j] = V[i][j];
    }
    e->q[0] = q0; e->q[1] = qx; e->q[2] = qy; e->q[3] = qz;
    e->top = top;
    double *R = out->R;
    R[0] = q0 * q0 + qx * qx - qy * qy - qz * qz; R[1] = 2.0 * (qx * qy - q0 * qz); R[2] = 2.0 * (qx * qz + q0 * qy);
    R[3] = 2.0 * (qy * qx + q0 * qz); R[4] = q0 * q0 - qx * qx + qy * qy - qz * qz; R[5] = 2.0 * (qy * qz - q0 * qx);
    R[6] = 2.0 * (qz * qx - q0 * qy); R[7] = 2.0 * (qz * qy + q0 * qx); R[8] = q0 * q0 - qx * qx - qy * qy + qz * qz;
    out->t[0] = cp[0] - (R[0] * cX[0] + R[1] * cX[1] + R[2] * cX[2]);
    out->t[1] = cp[1] - (R[3] * cX[0] + R[4] * cX[1] + R[5] * cX[2]);
    out->t[2] = cp[2] - (R[6] * cX[0] + R[7] * cX[1] + R[8] * cX[2]);
}

#undef XLR_ROTATE

/* the fit alone (the forward pass): the eigen-decomposition is dropped */
XL_MATH_FN void rgbd_kabsch_fit(const double *cp, const double *cX, const double *A, Pose *out)
{
    HornEig e;
    rgbd_kabsch_fit_eig(cp, cX, A, out, &e);
}

/* ------------------------------------------------------------------------------ cell error, score term, sampling try */

/* || p - (R X + t) || in centimetres (dsacstar_util.h:296, 502) */
XL_MATH_FN double rgbd_dist_cm(const Pose *p, double X, double Y, double Z, double px, double py, double pz)
{
    double dx = px - (p->R[0] * X + p->R[1] * Y + p->R[2] * Z + p->t[0]);
    double dy = py - (p->R[3] * X + p->R[4] * Y + p->R[5] * Z + p->t[1]);
    double dz = pz - (p->R[6] * X + p->R[7] * Y + p->R[8] * Z + p->t[2]);
    return sqrt(dx * dx + dy * dy + dz * dz) * 100.0;
}

/* get3DDistErrs, dsacstar_util.h:498-503: float error of a valid cell, clamped with std::min(err, maxDist) */
XL_MATH_FN float rgbd_cell_err(const Pose *p, double X, double Y, double Z, double px, double py, double pz, float maxDist)
{
    float a = (float)rgbd_dist_cm(p, X, Y, Z, px, py, pz);
    return (maxDist < a) ? maxDist : a;
}

/* one term of getHypScores (dsacstar_util.h:331-333): 1 - sigmoid(beta (e - thr)), the product in float */
XL_MATH_FN double rgbd_soft_term(float e, float beta, float thr)
{
    double st = (double)(beta * (e - thr));
    st = 1.0 / (1.0 + det_exp(-st));
    return 1.0 - st;
}

/* one sampling try (sampleHypothesesRGBD, dsacstar_util.h:266-305) from its three drawn pairs pc[3 j ..] (camera) and
 * Xw[3 j ..] (scene): Kabsch on the three, accepted iff all three are reconstructed within thr centimetres */
XL_MATH_FN bool rgbd_try_fit(const double *pc, const double *Xw, float thr, Pose *out)
{
    double s[XLR_SUMS_CENTROID], a[XLR_SUMS_COV], cp[3], cX[3];
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
    rgbd_kabsch_fit(cp, cX, a, out);
    bool ok = true;
    XL_MATH_UNROLL
    for (int j = 0; j < 3; ++j) {
        double n = rgbd_dist_cm(out, Xw[3 * j], Xw[3 * j + 1], Xw[3 * j + 2], pc[3 * j], pc[3 * j + 1], pc[3 * j + 2]);
        if (ok && !(n < (double)thr)) ok = false;
    }
    return ok;
}

#endif  /* XL_DSAC_RGBD_MATH_H */
