/*
 * tests/pose_refine_ref.c — CPU restatement of the uncertainty-weighted pose refinement (crossloc_amd/csrc/xl_dsac_refine.hip).
 *
 * TEST INFRASTRUCTURE ONLY.  The per-cell and per-image arithmetic is the product's xl_dsac_refine_math.h, compiled here by gcc
 * as C99 with -ffp-contract=off.  This file restates serially what the kernel does in parallel around it: the walk of 256
 * virtual threads over the cells (thread t: cells t, t + 256, ... in ascending order), the canonical block sum (block_sum of
 * xl_dsac_reduce.h, which states the order), the rounds and the Levenberg-Marquardt state machine.  Bitwise GPU == this file
 * therefore checks the kernel's orchestration and that gcc and hipcc agree on the same IEEE operations; the model itself is
 * checked against tests/indep_pose_refine.py (tests/test_pose_refine_cpu.py).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "xl_dsac_refine_math.h"      /* crossloc_amd/csrc: shared with the kernel */
#include "xl_dsac_reduce.h"           /* the canonical block sum and its order */

#define XR_T XL_BLOCK_THREADS         /* threads of the kernel's workgroup: 4 waves of 64 */

typedef struct {
    const float *coords; int64_t sc, sy, sx;
    const float *sigma; int64_t gy, gx;
    Cam cam;
    double s0sq;
} XrIn;

static void xr_fetch(const XrIn *in, int i, double *X, double *Y, double *Z, double *s)
{
    const int y = i / in->cam.Wo, x = i - y * in->cam.Wo;
    const float *q = in->coords + (int64_t)y * in->sy + (int64_t)x * in->sx;
    *X = (double)q[0]; *Y = (double)q[in->sc]; *Z = (double)q[2 * in->sc];
    *s = in->sigma ? (double)in->sigma[(int64_t)y * in->gy + (int64_t)x * in->gx] : 0.0;
}

/* one evaluation: per-thread partials over the inliers, canonical reduction */
static void xr_normal_eq(const XrIn *in, const Pose *pk, const Pose *p, const unsigned char *inl, double *ne)
{
    double (*part)[28] = (double (*)[28])malloc(sizeof(double) * XR_T * 28);
    for (int tid = 0; tid < XR_T; ++tid) {
        double *a = part[tid];
        for (int k = 0; k < 28; ++k) a[k] = 0.0;
        for (int i = tid; i < in->cam.N; i += XR_T) {
            if (!inl[i]) continue;
            const int y = i / in->cam.Wo, x = i - y * in->cam.Wo;
            double X, Y, Z, s;
            xr_fetch(in, i, &X, &Y, &Z, &s);
            refine_cell(pk, p, X, Y, Z, s, in->sigma != NULL, in->s0sq, y, x, &in->cam, a);
        }
    }
    block_sum(&part[0][0], 28, ne);
    free(part);
}

/* the round's inlier set at `pose`; returns the count, *bad the cells with an unusable sigma */
static double xr_inliers(const XrIn *in, const Pose *pose, unsigned char *inl, double *bad)
{
    double cnt = 0.0;
    *bad = 0.0;
    for (int i = 0; i < in->cam.N; ++i) {
        const int y = i / in->cam.Wo, x = i - y * in->cam.Wo;
        double X, Y, Z, s;
        xr_fetch(in, i, &X, &Y, &Z, &s);
        inl[i] = 0;
        if (in->sigma && refine_sigma_bad(s)) { *bad += 1.0; continue; }
        if (cell_err(pose, X, Y, Z, y, x, &in->cam) < in->cam.thr) { inl[i] = 1; cnt += 1.0; }
    }
    return cnt;
}

/* What the kernel must produce for one image.  coords float32 [3,Ho,Wo] through (sc, sy, sx); sigma float32 [Ho,Wo] through
 * (gy, gx) or NULL; pose16 float32 cam->world.  Out: pose16 float32, row 64 doubles, w2c 12 doubles, mask [Ho*Wo] bytes: the
 * inlier set of the last completed round (all zero when none completed). */
int xr_refine_pose(const float *coords, int64_t sc, int64_t sy, int64_t sx, const float *sigma, int64_t gy, int64_t gx,
                   int Ho, int Wo, const float *pose16, float thr, float focal, float ppx, float ppy, float maxReproj, int sub,
                   float s0, int maxRounds, float *outPose16, double *row, double *w2c, unsigned char *mask)
{
    if (!coords || !pose16 || !outPose16 || !row || !w2c || !mask || Ho <= 0 || Wo <= 0 || sub <= 0) return -1;
    if (!(s0 > 0.0f) || maxRounds < 1 || maxRounds > XLR_MAX_ROUNDS) return -1;
    XrIn in;
    in.coords = coords; in.sc = sc; in.sy = sy; in.sx = sx;
    in.sigma = sigma; in.gy = gy; in.gx = gx;
    in.cam = cam_make(Ho, Wo, thr, focal, ppx, ppy, 0.0f, maxReproj, sub);
    in.s0sq = (double)s0 * (double)s0;
    const int N = in.cam.N;

    const bool poseOk = quality_pose16_finite(pose16);
    Pose poseIn;
    if (poseOk) quality_pose_from16(pose16, &poseIn);
    else pose_identity(&poseIn);

    double status = poseOk ? XLR_STATUS_OK : XLR_STATUS_BAD_POSE;
    Pose pose = poseIn;
    double neOut[28];
    for (int k = 0; k < 28; ++k) neOut[k] = 0.0;
    double n0 = 0.0, bad = 0.0, cost0 = 0.0, nLast = 0.0;
    int rounds = 0, evals = 0, converged = 0;
    unsigned char *inl = (unsigned char *)malloc((size_t)N);
    memset(mask, 0, (size_t)N);

    for (int r = 0; poseOk && r < maxRounds; ++r) {
        double badNow;
        const double cnt = xr_inliers(&in, &pose, inl, &badNow);
        if (r > 0 && memcmp(inl, mask, (size_t)N) == 0) { converged = 1; break; }
        if (r > 0 && cnt < 4.0) break;

        const Pose pk = pose;
        Pose cur = pose, prev;
        double ne[28], neNew[28];
        xr_normal_eq(&in, &pk, &cur, inl, ne); ++evals;
        if (r == 0) {
            n0 = cnt; bad = badNow; cost0 = ne[27]; nLast = cnt;
            for (int k = 0; k < 28; ++k) neOut[k] = ne[k];
            if (cnt < 4.0) { status = XLR_STATUS_FEW_INLIERS; break; }
        }
        int lg = -3;
        double inv[36];
        bool failed = !quality_inv6(ne, inv);           /* J^T W J at the round's pose must be positive definite */
        for (int it = 0; !failed && it < XLM_LM_MAX_ITER; ++it) {
            double d[6];
            prev = cur;
            if (!solve6(ne, lambda_of(lg), d)) { failed = true; break; }
            apply_step(&prev, d, &cur);
            const double prevErr = ne[27];
            xr_normal_eq(&in, &pk, &cur, inl, neNew); ++evals;
            for (int up = 0; up < XLR_LG_RAISES; ++up) {
                if (!(neNew[27] > prevErr)) break;
                if (++lg > 16) break;
                if (!solve6(ne, lambda_of(lg), d)) { failed = true; break; }
                apply_step(&prev, d, &cur);
                xr_normal_eq(&in, &pk, &cur, inl, neNew); ++evals;
            }
            if (failed) break;
            lg = (lg - 1 > -16) ? lg - 1 : -16;
            if (lm_step_small(d, &prev)) break;
            for (int k = 0; k < 28; ++k) ne[k] = neNew[k];
        }
        if (!failed && !quality_pose_finite(&cur)) failed = true;
        if (failed) {
            if (r == 0) status = XLR_STATUS_FIRST_ROUND;
            break;
        }
        pose = cur;
        nLast = cnt;
        memcpy(mask, inl, (size_t)N);
        for (int k = 0; k < 28; ++k) neOut[k] = neNew[k];
        ++rounds;
    }
    free(inl);

    refine_row(status, &in.cam, n0, bad, cost0, nLast, neOut, rounds, evals, converged, &poseIn, &pose, row);
    if (status == XLR_STATUS_OK) pose_to_c2w16(&pose, outPose16);
    else memcpy(outPose16, pose16, 16 * sizeof(float));
    if (poseOk) pose_store12(&pose, w2c);
    else for (int i = 0; i < 12; ++i) w2c[i] = quality_nan();
    return 0;
}

/* --- hooks for the header-piece tests: thin calls into the shared headers --- */

/* the 28 sums one cell adds at pose Rt12: weighted with w through pnp_cell_normal_eq_w (out28w), and through the
 * unweighted pnp_cell_normal_eq (out28q) */
void xr_test_cell_normal_eq(const double *Rt12, const double *xyz, double w, int y, int x, float focal, float ppx, float ppy, int sub,
                            double *out28w, double *out28q)
{
    Pose p;
    pose_load12(Rt12, &p);
    const Cam cam = cam_make(0, 0, 0.0f, focal, ppx, ppy, 0.0f, 0.0f, sub);
    for (int k = 0; k < 28; ++k) { out28w[k] = 0.0; out28q[k] = 0.0; }
    pnp_cell_normal_eq_w(&p, xyz[0], xyz[1], xyz[2], w, y, x, &cam, out28w);
    pnp_cell_normal_eq(&p, xyz[0], xyz[1], xyz[2], y, x, &cam, out28q);
}

double xr_test_weight(const double *Rt12, const double *xyz, double sigma, double s0, float focal)
{
    Pose p;
    pose_load12(Rt12, &p);
    const Cam cam = cam_make(0, 0, 0.0f, focal, 0.0, 0.0, 0.0f, 0.0f, 0);
    return refine_weight(&p, xyz[0], xyz[1], xyz[2], sigma, s0 * s0, &cam);
}

void xr_test_pose_to_c2w16(const double *Rt12, float *out16)
{
    Pose p;
    pose_load12(Rt12, &p);
    pose_to_c2w16(&p, out16);
}
