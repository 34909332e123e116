/*
 * tests/pose_refine_masked_ref.c — CPU restatement of the MASKED uncertainty-weighted pose refinement
 * (crossloc_amd/csrc/xl_dsac_refine.hip, xl_dsac_refine_pose_masked_batch).
 *
 * TEST INFRASTRUCTURE ONLY, the sibling of tests/pose_refine_ref.c: the per-cell and per-image arithmetic is the product's
 * xl_dsac_refine_math.h, compiled here by gcc as C99 with -ffp-contract=off; this file restates serially the masked kernel's
 * orchestration around it - the walk of 256 virtual threads over the cells, the canonical block sum, the rounds and the
 * Levenberg-Marquardt state machine, and the mask: a masked-out cell is passed by in every round's marking loop before its sigma
 * is checked and before its error is formed.  Neither its coordinate nor its sigma is dereferenced.
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
    const unsigned char *usable;      /* [N], nonzero = usable */
    Cam cam;
    double s0sq;
} XrmIn;

static void xrm_fetch(const XrmIn *in, int i, double *X, double *Y, double *Z, double *s)
{
    const int y = i / in->cam.Wo, x = i - y * in->cam.Wo;
    const float *q = in->coords + (int64_t)y * in->sy + (int64_t)x * in->sx;
    *X = (double)q[0]; *Y = (double)q[in->sc]; *Z = (double)q[2 * in->sc];
    *s = in->sigma ? (double)in->sigma[(int64_t)y * in->gy + (int64_t)x * in->gx] : 0.0;
}

/* one evaluation: per-thread partials over the inliers (all of them usable cells), canonical reduction */
static void xrm_normal_eq(const XrmIn *in, const Pose *pk, const Pose *p, const unsigned char *inl, double *ne)
{
    double (*part)[28] = (double (*)[28])malloc(sizeof(double) * XR_T * 28);
    for (int tid = 0; tid < XR_T; ++tid) {
        double *a = part[tid];
        for (int k = 0; k < 28; ++k) a[k] = 0.0;
        for (int i = tid; i < in->cam.N; i += XR_T) {
            if (!inl[i]) continue;
            const int y = i / in->cam.Wo, x = i - y * in->cam.Wo;
            double X, Y, Z, s;
            xrm_fetch(in, i, &X, &Y, &Z, &s);
            refine_cell(pk, p, X, Y, Z, s, in->sigma != NULL, in->s0sq, y, x, &in->cam, a);
        }
    }
    block_sum(&part[0][0], 28, ne);
    free(part);
}

/* the round's inlier set at `pose` over the usable cells; returns the count, *bad the usable cells with an unusable sigma */
static double xrm_inliers(const XrmIn *in, const Pose *pose, unsigned char *inl, double *bad)
{
    double cnt = 0.0;
    *bad = 0.0;
    for (int i = 0; i < in->cam.N; ++i) {
        inl[i] = 0;
        if (!in->usable[i]) continue;
        const int y = i / in->cam.Wo, x = i - y * in->cam.Wo;
        double X, Y, Z, s;
        xrm_fetch(in, i, &X, &Y, &Z, &s);
        if (in->sigma && refine_sigma_bad(s)) { *bad += 1.0; continue; }
        if (cell_err(pose, X, Y, Z, y, x, &in->cam) < in->cam.thr) { inl[i] = 1; cnt += 1.0; }
    }
    return cnt;
}

/* What the masked kernel must produce for one image.  Arguments as xr_refine_pose of tests/pose_refine_ref.c plus
 * usable [Ho*Wo] bytes (nonzero = usable).  Out: pose16 float32, row 64 doubles, w2c 12 doubles, mask [Ho*Wo] bytes: the inlier
 * set of the last completed round (all zero when none completed). */
int xrm_refine_pose(const float *coords, int64_t sc, int64_t sy, int64_t sx, const float *sigma, int64_t gy, int64_t gx,
                    int Ho, int Wo, const unsigned char *usable, const float *pose16, float thr, float focal, float ppx, float ppy,
                    float maxReproj, int sub, float s0, int maxRounds, float *outPose16, double *row, double *w2c,
                    unsigned char *mask)
{
    if (!coords || !usable || !pose16 || !outPose16 || !row || !w2c || !mask || Ho <= 0 || Wo <= 0 || sub <= 0) return -1;
    if (!(s0 > 0.0f) || maxRounds < 1 || maxRounds > XLR_MAX_ROUNDS) return -1;
    XrmIn in;
    in.coords = coords; in.sc = sc; in.sy = sy; in.sx = sx;
    in.sigma = sigma; in.gy = gy; in.gx = gx;
    in.usable = usable;
    in.cam = cam_make(Ho, Wo, thr, focal, ppx, ppy, 0.0f, maxReproj, sub);
    in.s0sq = (double)s0 * (double)s0;
    const int N = in.cam.N;

    const bool poseOk = quality_pose16_finite(pose16);
    Pose poseIn;
    if (poseOk) quality_pose_from16(pose16, &poseIn);
    else pose_identity(&poseIn);

    double nMasked = 0.0;
    for (int i = 0; i < N; ++i) if (!usable[i]) nMasked += 1.0;

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
        const double cnt = xrm_inliers(&in, &pose, inl, &badNow);
        if (r > 0 && memcmp(inl, mask, (size_t)N) == 0) { converged = 1; break; }
        if (r > 0 && cnt < 4.0) break;

        const Pose pk = pose;
        Pose cur = pose, prev;
        double ne[28], neNew[28];
        xrm_normal_eq(&in, &pk, &cur, inl, ne); ++evals;
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
            xrm_normal_eq(&in, &pk, &cur, inl, neNew); ++evals;
            for (int up = 0; up < XLR_LG_RAISES; ++up) {
                if (!(neNew[27] > prevErr)) break;
                if (++lg > 16) break;
                if (!solve6(ne, lambda_of(lg), d)) { failed = true; break; }
                apply_step(&prev, d, &cur);
                xrm_normal_eq(&in, &pk, &cur, inl, neNew); ++evals;
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
    quality_row_n_masked(row, XLR_COL_N_MASKED, nMasked);
    if (status == XLR_STATUS_OK) pose_to_c2w16(&pose, outPose16);
    else memcpy(outPose16, pose16, 16 * sizeof(float));
    if (poseOk) pose_store12(&pose, w2c);
    else for (int i = 0; i < 12; ++i) w2c[i] = quality_nan();
    return 0;
}
