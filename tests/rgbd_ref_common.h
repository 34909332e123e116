/*
 * tests/rgbd_ref_common.h — what the three RGB-D restatements (dsac_rgbd_ref.c, dsac_rgbd_bwd_ref.c, rgbd_quality_ref.c) share.
 *
 * TEST INFRASTRUCTURE ONLY: where an image comes from and the load of one cell, the staged valid list, the cell error and the
 * serial model of the refinement loop (rgbd_refine of crossloc_amd/csrc/xl_dsac_rgbd_dev.h).  The lane-local arithmetic is the
 * product's xl_dsac_rgbd_math.h, the canonical block sum and its order the plain-C half of xl_dsac_reduce.h.
 */
#ifndef RGBD_REF_COMMON_H
#define RGBD_REF_COMMON_H

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xl_dsac_rgbd_math.h"        /* crossloc_amd/csrc: shared with the kernels */
#include "xl_dsac_reduce.h"

#define XR_T XL_BLOCK_THREADS         /* threads of the kernels' workgroup: 4 waves of 64 */
#define XR_MAX_REF_STEPS 100

/* where an image comes from: exactly one of cam ([3,Ho,Wo] strides cc, cy, cx) and depth ([Ho,Wo] strides dy, dx) is non-null */
typedef struct {
    const float *coords; int64_t sc, sy, sx;
    const float *cam; int64_t cc, cy, cx;
    const float *depth; int64_t dy, dx;
    float focal, ppx, ppy; int sub;
} RgbdSrc;

static RgbdSrc xr_src(const float *coords, int64_t sc, int64_t sy, int64_t sx, const float *cam, int64_t cc, int64_t cy, int64_t cx,
                      const float *depth, int64_t dy, int64_t dx, float focal, float ppx, float ppy, int sub)
{
    const RgbdSrc in = { coords, sc, sy, sx, cam, cc, cy, cx, depth, dy, dx, focal, ppx, ppy, sub };
    return in;
}

/* scene coordinate X and camera coordinate p of cell (y, x) */
static void xr_load(const RgbdSrc *in, int y, int x, float *X, float *p)
{
    const float *q = in->coords + (int64_t)y * in->sy + (int64_t)x * in->sx;
    X[0] = q[0]; X[1] = q[in->sc]; X[2] = q[2 * in->sc];
    if (in->cam) {
        const float *m = in->cam + (int64_t)y * in->cy + (int64_t)x * in->cx;
        p[0] = m[0]; p[1] = m[in->cc]; p[2] = m[2 * in->cc];
    } else {
        rgbd_cam_from_depth(in->depth[(int64_t)y * in->dy + (int64_t)x * in->dx], y, x, in->focal, in->ppx, in->ppy, in->sub,
                            p, p + 1, p + 2);
    }
}

/* the staged image: six floats per valid cell in valid-list order (x-major), and the list itself (cell = y * Wo + x) */
typedef struct { float *p[3], *X[3]; int *cell; int n; } Staged;

static void xr_free(Staged *s)
{
    for (int c = 0; c < 3; ++c) { free(s->p[c]); free(s->X[c]); }
    free(s->cell);
}

static int xr_stage(Staged *s, const RgbdSrc *in, int Ho, int Wo)
{
    const int N = Ho * Wo;
    for (int c = 0; c < 3; ++c) {
        s->p[c] = (float *)malloc(sizeof(float) * (size_t)N);
        s->X[c] = (float *)malloc(sizeof(float) * (size_t)N);
    }
    s->cell = (int *)malloc(sizeof(int) * (size_t)N);
    s->n = 0;
    for (int x = 0; x < Wo; ++x)
        for (int y = 0; y < Ho; ++y) {
            float X[3], p[3];
            xr_load(in, y, x, X, p);
            if (!(p[2] != 0.0f)) continue;
            const int k = s->n++;
            for (int c = 0; c < 3; ++c) { s->p[c][k] = p[c]; s->X[c][k] = X[c]; }
            s->cell[k] = y * Wo + x;
        }
    return s->n;
}

static float xr_err(const Staged *s, const Pose *p, int k, float maxDist)
{
    return rgbd_cell_err(p, (double)s->X[0][k], (double)s->X[1][k], (double)s->X[2][k],
                         (double)s->p[0][k], (double)s->p[1][k], (double)s->p[2][k], maxDist);
}

/* what the refinement leaves behind besides the pose: of the last FITTED round the inlier count, centroids and covariance sums */
typedef struct { unsigned finalInl; int rounds; double cp[3], cX[3], a[XLR_SUMS_COV]; } XrRefine;

/* the refinement loop (refineHypRGBD, dsacstar_util.h:611-677): the walk of 256 virtual threads, block sums in the canonical
 * order.  Optional recorders: inlOut [n] the inlier set of the last fitted round; roundCounts [100] the inlier count of every
 * round entered, the rejected last one included (-1 beyond); roundPoses [100,12]; roundMasks [100, N] the cells fitted in an
 * accepted round. */
static void xr_refine(const Staged *S, float thr, float maxDist, Pose *pose, XrRefine *ro, uint8_t *inlOut,
                      int32_t *roundCounts, double *roundPoses, uint8_t *roundMasks, int N)
{
    const int nValid = S->n;
    unsigned best = 3;
    memset(ro, 0, sizeof(*ro));
    if (inlOut) memset(inlOut, 0, (size_t)(nValid > 0 ? nValid : 1));
    if (roundCounts) for (int r = 0; r < XR_MAX_REF_STEPS; ++r) roundCounts[r] = -1;
    uint8_t *inl = (uint8_t *)malloc((size_t)(nValid > 0 ? nValid : 1));
    double *part = (double *)malloc(sizeof(double) * XR_T * XLR_SUMS_COV);
    for (int step = 0; step < XR_MAX_REF_STEPS; ++step) {
        unsigned cnt = 0;
        for (int k = 0; k < nValid; ++k) {
            inl[k] = xr_err(S, pose, k, maxDist) < thr;
            cnt += inl[k];
        }
        if (roundCounts) roundCounts[step] = (int32_t)cnt;
        if (cnt <= best) break;
        best = cnt;
        double s[XLR_SUMS_CENTROID], a[XLR_SUMS_COV], cp[3], cX[3];
        for (int tid = 0; tid < XR_T; ++tid) {
            double *v = part + tid * XLR_SUMS_CENTROID;
            for (int k = 0; k < XLR_SUMS_CENTROID; ++k) v[k] = 0.0;
            for (int k = tid; k < nValid; k += XR_T)
                if (inl[k]) rgbd_acc_centroid(v, (double)S->p[0][k], (double)S->p[1][k], (double)S->p[2][k],
                                              (double)S->X[0][k], (double)S->X[1][k], (double)S->X[2][k]);
        }
        block_sum(part, XLR_SUMS_CENTROID, s);
        rgbd_centroids(s, cp, cX);
        for (int tid = 0; tid < XR_T; ++tid) {
            double *v = part + tid * XLR_SUMS_COV;
            for (int k = 0; k < XLR_SUMS_COV; ++k) v[k] = 0.0;
            for (int k = tid; k < nValid; k += XR_T)
                if (inl[k]) rgbd_acc_cov(v, cp, cX, (double)S->p[0][k], (double)S->p[1][k], (double)S->p[2][k],
                                         (double)S->X[0][k], (double)S->X[1][k], (double)S->X[2][k]);
        }
        block_sum(part, XLR_SUMS_COV, a);
        rgbd_kabsch_fit(cp, cX, a, pose);
        if (roundPoses) pose_store12(pose, roundPoses + 12 * ro->rounds);
        if (roundMasks) {
            uint8_t *m = roundMasks + (size_t)ro->rounds * (size_t)N;
            memset(m, 0, (size_t)N);
            for (int k = 0; k < nValid; ++k) if (inl[k]) m[S->cell[k]] = 1;
        }
        if (inlOut) memcpy(inlOut, inl, (size_t)nValid);
        ro->finalInl = cnt;
        ++ro->rounds;
        for (int i = 0; i < 3; ++i) { ro->cp[i] = cp[i]; ro->cX[i] = cX[i]; }
        for (int i = 0; i < XLR_SUMS_COV; ++i) ro->a[i] = a[i];
    }
    free(part);
    free(inl);
}

#endif  /* RGBD_REF_COMMON_H */
