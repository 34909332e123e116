/*
 * tests/rgbd_refine_ref.c — CPU restatement of the ray-aware pose refinement behind the RGB-D solver
 * (crossloc_amd/csrc/xl_dsac_rgbd_refine.hip).
 *
 * TEST INFRASTRUCTURE ONLY.  The per-cell and per-image arithmetic is the product's xl_dsac_rgbd_refine_math.h, compiled here by
 * gcc as C99 with -ffp-contract=off.  This file restates serially what the kernel does in parallel around it: the walk of 256
 * virtual threads over the cells (thread t: cells t, t + 256, ... in ascending order), the canonical block sum (block_sum of
 * xl_dsac_reduce.h, which states the order), the rounds and the Levenberg-Marquardt state machine.  Bitwise GPU == this file
 * therefore checks the kernel's orchestration and that gcc and hipcc agree on the same IEEE operations; the model itself is
 * checked against tests/indep_rgbd_refine.py (tests/test_rgbd_refine_cpu.py).
 */
#include "rgbd_ref_common.h"
#include "xl_dsac_rgbd_refine_math.h"   /* crossloc_amd/csrc: shared with the kernel */

typedef struct {
    RgbdSrc src;
    const float *sigma; int64_t gy, gx;
    const float *sigmaZ; int64_t zy, zx;
    RgbdR q;
} XrrIn;

typedef struct { double X, Y, Z, sigma, sigmaZ; float p[3]; } XrrCell;

static XrrCell xrr_fetch(const XrrIn *in, int i)
{
    XrrCell ce;
    const int y = i / in->q.Wo, x = i - y * in->q.Wo;
    float X[3];
    xr_load(&in->src, y, x, X, ce.p);
    ce.X = (double)X[0]; ce.Y = (double)X[1]; ce.Z = (double)X[2];
    ce.sigma = in->sigma ? (double)in->sigma[(int64_t)y * in->gy + (int64_t)x * in->gx] : 0.0;
    ce.sigmaZ = in->sigmaZ ? (double)in->sigmaZ[(int64_t)y * in->zy + (int64_t)x * in->zx] : 0.0;
    return ce;
}

/* the round-start walk: per-thread partials, canonical reduction */
static void xrr_start(const XrrIn *in, const Pose *pose, const Pose *prev, bool hasPrev, double *s0)
{
    double *part = (double *)malloc(sizeof(double) * XR_T * XLRR_SUMS0);
    for (int tid = 0; tid < XR_T; ++tid) {
        double *a = part + tid * XLRR_SUMS0;
        for (int k = 0; k < XLRR_SUMS0; ++k) a[k] = 0.0;
        for (int i = tid; i < in->q.N; i += XR_T) {
            const XrrCell ce = xrr_fetch(in, i);
            rgbdr_cell_start(pose, prev, hasPrev, ce.X, ce.Y, ce.Z, ce.p[0], ce.p[1], ce.p[2], ce.sigma, ce.sigmaZ, &in->q, a);
        }
    }
    block_sum(part, XLRR_SUMS0, s0);
    free(part);
}

/* one evaluation: per-thread partials over the inliers at pk, canonical reduction */
static void xrr_normal_eq(const XrrIn *in, const Pose *pk, const Pose *p, const double *c, double *ne)
{
    double *part = (double *)malloc(sizeof(double) * XR_T * 28);
    for (int tid = 0; tid < XR_T; ++tid) {
        double *a = part + tid * 28;
        for (int k = 0; k < 28; ++k) a[k] = 0.0;
        for (int i = tid; i < in->q.N; i += XR_T) {
            const XrrCell ce = xrr_fetch(in, i);
            rgbdr_cell_eval(pk, p, ce.X, ce.Y, ce.Z, ce.p[0], ce.p[1], ce.p[2], ce.sigma, ce.sigmaZ, &in->q, c, a);
        }
    }
    block_sum(part, 28, ne);
    free(part);
}

/* the inlier set at `pose` as a byte mask (for the tests; the kernel keeps no mask) */
static void xrr_mask(const XrrIn *in, const Pose *pose, unsigned char *mask)
{
    for (int i = 0; i < in->q.N; ++i) {
        const XrrCell ce = xrr_fetch(in, i);
        mask[i] = (ce.p[2] != 0.0f) && !rgbdr_unusable(ce.sigma, ce.sigmaZ)
                  && rgbdr_inlier(pose, ce.X, ce.Y, ce.Z, ce.p[0], ce.p[1], ce.p[2], &in->q);
    }
}

/* What the kernel must produce for one image.  coords float32 [3,Ho,Wo] through (sc, sy, sx); exactly one of cam [3,Ho,Wo] and
 * depth [Ho,Wo]; sigma, sigmaZ float32 [Ho,Wo] or NULL; pose16 float32 cam->world.  Out: pose16 float32, row 64 doubles, w2c 12
 * doubles, mask [Ho*Wo] bytes: the inlier set of the last completed round (all zero when none completed). */
int xrr_refine_pose(const float *coords, int64_t sc, int64_t sy, int64_t sx, const float *cam, int64_t cc, int64_t cy, int64_t cx,
                    const float *depth, int64_t dy, int64_t dx, int Ho, int Wo,
                    const float *sigma, int64_t gy, int64_t gx, const float *sigmaZ, int64_t zy, int64_t zx,
                    const float *pose16, float thr, float maxDist, float focal, float ppx, float ppy, int sub,
                    float s0, float depthRel, int maxRounds, float *outPose16, double *row, double *w2c, unsigned char *mask)
{
    if (!coords || (cam == NULL) == (depth == NULL) || !pose16 || !outPose16 || !row || !w2c || !mask || Ho <= 0 || Wo <= 0 || sub <= 0)
        return -1;
    if (!(s0 > 0.0f) || !(depthRel >= 0.0f) || !(depthRel <= 3.0e38f) || maxRounds < 1 || maxRounds > XLR_MAX_ROUNDS) return -1;
    XrrIn in;
    in.src = xr_src(coords, sc, sy, sx, cam, cc, cy, cx, depth, dy, dx, focal, ppx, ppy, sub);
    in.sigma = sigma; in.gy = gy; in.gx = gx;
    in.sigmaZ = sigmaZ; in.zy = zy; in.zx = zx;
    in.q.thr = thr; in.q.maxDist = maxDist; in.q.Ho = Ho; in.q.Wo = Wo; in.q.N = Ho * Wo;
    in.q.s0sq = rgbdr_s0sq(sigma != NULL, sigmaZ != NULL, depthRel, s0);
    in.q.k = (double)depthRel;
    const int N = in.q.N;

    const bool poseOk = quality_pose16_finite(pose16);
    Pose poseIn;
    if (poseOk) quality_pose_from16(pose16, &poseIn);
    else pose_identity(&poseIn);

    double status = poseOk ? XLR_STATUS_OK : XLR_STATUS_BAD_POSE;
    Pose pose = poseIn, prevPk = poseIn;
    double neOut[28], cOut[3] = { 0.0, 0.0, 0.0 };
    for (int k = 0; k < 28; ++k) neOut[k] = 0.0;
    double n0 = 0.0, bad = 0.0, nValid = 0.0, cost0 = 0.0, nLast = 0.0;
    int rounds = 0, evals = 0, converged = 0;
    memset(mask, 0, (size_t)N);

    for (int r = 0; poseOk && r < maxRounds; ++r) {
        double s[XLRR_SUMS0], c[3];
        xrr_start(&in, &pose, &prevPk, r > 0, s);
        const double cnt = s[XLRR_S_COUNT];
        if (r > 0 && s[XLRR_S_DIFF] == 0.0) { converged = 1; break; }
        if (r > 0 && cnt < 3.0) break;
        rgbdr_centroid(s, c);

        const Pose pk = pose;
        Pose cur = pose, prev;
        double ne[28], neNew[28];
        xrr_normal_eq(&in, &pk, &cur, c, ne); ++evals;
        if (r == 0) {
            n0 = cnt; bad = s[XLRR_S_BAD]; nValid = s[XLRR_S_VALID]; cost0 = ne[27]; nLast = cnt;
            for (int k = 0; k < 28; ++k) neOut[k] = ne[k];
            for (int k = 0; k < 3; ++k) cOut[k] = c[k];
            if (cnt < 3.0) { status = XLR_STATUS_FEW_INLIERS; break; }
        }
        int lg = -3;
        bool failed = !rgbdr_well_posed(ne);
        for (int it = 0; !failed && it < XLM_LM_MAX_ITER; ++it) {
            double d[6];
            prev = cur;
            if (!solve6(ne, lambda_of(lg), d)) { failed = true; break; }
            rgbdr_apply_step(&prev, c, d, &cur);
            const double prevErr = ne[27];
            xrr_normal_eq(&in, &pk, &cur, c, neNew); ++evals;
            for (int up = 0; up < XLR_LG_RAISES; ++up) {
                if (!(neNew[27] > prevErr)) break;
                if (++lg > 16) break;
                if (!solve6(ne, lambda_of(lg), d)) { failed = true; break; }
                rgbdr_apply_step(&prev, c, d, &cur);
                xrr_normal_eq(&in, &pk, &cur, c, neNew); ++evals;
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
        prevPk = pk;
        nLast = cnt;
        xrr_mask(&in, &pk, mask);
        for (int k = 0; k < 28; ++k) neOut[k] = neNew[k];
        for (int k = 0; k < 3; ++k) cOut[k] = c[k];
        ++rounds;
    }

    /* the row rates the float pose the caller receives: one more evaluation there, over the last round's set */
    Pose poseOut = pose;
    if (status == XLR_STATUS_OK) {
        pose_to_c2w16(&pose, outPose16);
        quality_pose_from16(outPose16, &poseOut);
        xrr_normal_eq(&in, &prevPk, &poseOut, cOut, neOut); ++evals;
    } else {
        memcpy(outPose16, pose16, 16 * sizeof(float));
    }
    rgbdr_row(status, &in.q, n0, bad, nValid, cost0, nLast, neOut, cOut, rounds, evals, converged, &poseIn, &poseOut, row);
    if (poseOk) pose_store12(&pose, w2c);
    else for (int i = 0; i < 12; ++i) w2c[i] = quality_nan();
    return 0;
}

/* --- hooks for the header-piece tests: thin calls into the shared header --- */

/* noise of a cell with camera coordinate p: out = a, b, rho (3), W row-major (9) */
void xrr_test_noise(const double *p, double sigma, double sigmaZ, double s0sq, double k, double *out14)
{
    double a, b, rho[3];
    rgbdr_noise(p[0], p[1], p[2], sigma, sigmaZ, s0sq, k, &a, &b, rho);
    out14[0] = a; out14[1] = b;
    for (int i = 0; i < 3; ++i) out14[2 + i] = rho[i];
    for (int j = 0; j < 3; ++j) {
        double e[3] = { 0.0, 0.0, 0.0 }, col[3];
        e[j] = 1.0;
        rgbdr_apply_w(a, b, rho, e, col);
        for (int i = 0; i < 3; ++i) out14[5 + 3 * i + j] = col[i];
    }
}

/* the 28 sums one cell adds at pose Rt12 about c */
void xrr_test_cell_normal_eq(const double *Rt12, const double *xyz, const double *p, const double *c, double sigma, double sigmaZ,
                             double s0sq, double k, double *out28)
{
    Pose pose;
    pose_load12(Rt12, &pose);
    double a, b, rho[3];
    rgbdr_noise(p[0], p[1], p[2], sigma, sigmaZ, s0sq, k, &a, &b, rho);
    for (int i = 0; i < 28; ++i) out28[i] = 0.0;
    rgbdr_cell_normal_eq(&pose, xyz[0], xyz[1], xyz[2], p[0], p[1], p[2], c, a, b, rho, out28);
}

/* the step in (rotation about c, centroid translation) */
void xrr_test_apply_step(const double *Rt12, const double *c, const double *d, double *out12)
{
    Pose prev, out;
    pose_load12(Rt12, &prev);
    rgbdr_apply_step(&prev, c, d, &out);
    pose_store12(&out, out12);
}
