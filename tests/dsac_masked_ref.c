/*
 * tests/dsac_masked_ref.c — CPU restatement of the masked RGB DSAC* solver (xl_dsac_forward_rgb_masked_batch,
 * crossloc_amd/csrc/xl_dsac.hip with MASKED = true).
 *
 * TEST INFRASTRUCTURE ONLY.  The lane-local arithmetic (per-cell normal equations, LM stop rule, soft-inlier term and pose
 * write included) is the product's xl_dsac_math.h and the order of the sums is xl_dsac_reduce.h, compiled here by gcc as
 * C99 with -ffp-contract=off.  This file restates serially what the kernel does in
 * parallel around them, in the manner of oracle/dsac_oracle.c (with which it shares no code, only the product's headers): the tries of
 * a hypothesis in ascending order (the kernel's ballot picks the lowest accepted lane), lane l summing cells l, l + 64, ... and
 * the xor butterfly (the order of xo_score), first-maximum-wins selection, the 256 virtual threads of the normal equations (the
 * order of xo_normal_eq) and the LM state machine.  The mask enters at the four points include/crossloc_dsac.h names: a try
 * that drew a masked-out cell is rejected before P3P and never reads that cell; the score sums usable cells only; an inlier is
 * a usable cell below the threshold; fewer than four usable cells make the image dead.  A masked-out cell's coordinates are
 * never read here at all, so identity B (their values influence no output bit) holds in this file by construction;
 * tests/test_dsac_masked_cpu.py ties the file to the pinned oracle through identity A (all-ones mask == oracle, bit for bit).
 *
 * With -DXM_MAIN the file is a program of its own (for the sanitizer run): see main() at the end.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xl_dsac_math.h"
#include "xl_dsac_reduce.h"
#include "../../include/crossloc_dsac.h"      /* beside crossloc_amd/csrc, as the kernels include it: XL_DSAC_MAX_REF_STEPS */

#define XM_DBG 28
#define XM_MAX_CELLS 16384
#define XM_T XL_BLOCK_THREADS

typedef struct {
    const float *base; int64_t sc, sy, sx;
    const uint8_t *mask;                          /* [Ho*Wo], nonzero = usable */
    int Ho, Wo;
} xm_image;

static void xm_fetch(const xm_image *im, int i, double X[3])
{
    const int y = i / im->Wo, x = i - y * im->Wo;
    const float *p = im->base + (int64_t)y * im->sy + (int64_t)x * im->sx;
    X[0] = (double)p[0]; X[1] = (double)p[im->sc]; X[2] = (double)p[2 * im->sc];
}

static float xm_cell_err(const xm_image *im, const Pose *p, int i, const Cam *cam)
{
    const int y = i / cam->Wo, x = i - y * cam->Wo;
    double X[3];
    xm_fetch(im, i, X);
    return cell_err(p, X[0], X[1], X[2], y, x, cam);
}

/* one try: the draws of the unmasked solver; rejected before P3P (identity pose) when a drawn cell is masked out */
static int xm_sample_try(const xm_image *im, const Cam *cam, uint64_t imageKey, uint32_t hyp, uint32_t t, Pose *pose, int cells[4])
{
    const uint64_t st = try_state(imageKey, hyp, t);
    V3 P[4];
    double uv[4][2];
    float px[4], py[4];
    int usable = 1;
    for (int j = 0; j < 4; ++j) {
        const int x = draw(st, 2 * j, cam->Wo);
        const int y = draw(st, 2 * j + 1, cam->Ho);
        cells[j] = y * cam->Wo + x;
        px[j] = cell_px(cam, x);
        py[j] = cell_px(cam, y);
        uv[j][0] = (double)px[j]; uv[j][1] = (double)py[j];
        if (!im->mask[cells[j]]) usable = 0;
    }
    if (!usable) { pose_identity(pose); return 0; }
    for (int j = 0; j < 4; ++j) {
        double X[3];
        xm_fetch(im, cells[j], X);
        P[j].x = X[0]; P[j].y = X[1]; P[j].z = X[2];
    }
    if (!p3p(P[0], P[1], P[2], P[3], uv, cam, pose)) { pose_identity(pose); return 0; }
    for (int j = 0; j < 4; ++j) {
        float u, v;
        project(pose, P[j].x, P[j].y, P[j].z, cam, &u, &v);
        const float dx = px[j] - u, dy = py[j] - v;
        const double n = sqrt((double)dx * (double)dx + (double)dy * (double)dy);
        if (!(n < (double)cam->thr)) return 0;
    }
    return 1;
}

/* lane l accumulates the usable cells among l, l + 64, ... in ascending order, then the butterfly; the factor is alpha / Wo / Ho */
static double xm_score(const xm_image *im, const Pose *pose, const Cam *cam)
{
    const float beta = 5.0f / cam->thr;
    double part[64];
    for (int l = 0; l < 64; ++l) {
        double acc = 0.0;
        for (int i = l; i < cam->N; i += 64) {
            if (!im->mask[i]) continue;
            acc += 1.0 - soft_inlier_st(xm_cell_err(im, pose, i, cam), cam->thr, beta);
        }
        part[l] = acc;
    }
    const double total = butterfly64(part);
    const float fac = cam->alpha / (float)cam->Wo / (float)cam->Ho;
    return total * (double)fac;
}

/* normal equations over the inlier set at pose p: thread t accumulates cells t, t + 256, ..., then the canonical block sum */
static void xm_normal_eq(const xm_image *im, const unsigned char *inl, const Pose *p, const Cam *cam, double out[28])
{
    double *part = (double *)malloc(sizeof(double) * 28 * XM_T);
    for (int tdx = 0; tdx < XM_T; ++tdx) {
        double a[28];
        for (int k = 0; k < 28; ++k) a[k] = 0.0;
        for (int i = tdx; i < cam->N; i += XM_T) {
            if (!inl[i]) continue;
            const int y = i / cam->Wo, x = i - y * cam->Wo;
            double X[3];
            xm_fetch(im, i, X);
            pnp_cell_normal_eq(p, X[0], X[1], X[2], y, x, cam, a);
        }
        for (int k = 0; k < 28; ++k) part[tdx * 28 + k] = a[k];
    }
    block_sum(part, 28, out);
    free(part);
}

/* the LM state machine of the kernel's refine_pose; returns 0 on failure (pose untouched) */
static int xm_lm_pnp(const xm_image *im, const unsigned char *inl, const Cam *cam, Pose *pose, int *evals)
{
    Pose cur = *pose, prev;
    double ne[28], neNew[28];
    int lg = -3, iters = 0;
    xm_normal_eq(im, inl, &cur, cam, ne);
    ++*evals;
    for (;;) {
        double d[6];
        prev = cur;
        if (!solve6(ne, lambda_of(lg), d)) return 0;
        apply_step(&prev, d, &cur);
        const double prevErr = ne[27];
        xm_normal_eq(im, inl, &cur, cam, neNew);
        ++*evals;
        while (neNew[27] > prevErr) {
            if (++lg <= 16) {
                if (!solve6(ne, lambda_of(lg), d)) return 0;
                apply_step(&prev, d, &cur);
                xm_normal_eq(im, inl, &cur, cam, neNew);
                ++*evals;
            } else break;
        }
        lg = (lg - 1 > -16) ? lg - 1 : -16;
        ++iters;
        if (iters >= XLM_LM_MAX_ITER || lm_step_small(d, &prev)) break;
        memcpy(ne, neNew, sizeof(ne));
    }
    if (!pose_not_nan(&cur)) return 0;
    *pose = cur;
    return 1;
}

/* the dead image's pose as the kernel writes it: not pose_to_c2w16 of the identity, whose translation column is -0.0f */
static void xm_identity16(float *pose16)
{
    for (int i = 0; i < 16; ++i) pose16[i] = (i % 5 == 0) ? 1.0f : 0.0f;
}

/*
 * One image.  coords [3,Ho,Wo] float32 with element strides (sc, sy, sx); mask [Ho*Wo] uint8, nonzero = usable.  Outputs
 * (nullable except pose16): status, cells [nHyp,4], tries [nHyp], scores [nHyp], dbg [28] as the kernel writes it.
 */
int xm_forward_rgb_masked(const float *coords, int64_t sc, int64_t sy, int64_t sx, int Ho, int Wo, const uint8_t *mask,
                          float *pose16, int32_t *status, int nHyp, float thr, float focal, float ppx, float ppy,
                          float alpha, float maxReproj, int sub, uint64_t seed, uint64_t image, uint32_t maxTries,
                          int32_t *cells, int32_t *tries, double *scores, double *dbg)
{
    if (!coords || !mask || !pose16 || nHyp <= 0 || Ho <= 0 || Wo <= 0 || sub <= 0 || maxTries == 0) return -1;
    const int N = Ho * Wo;
    if (N > XM_MAX_CELLS) return -2;
    const xm_image im = { coords, sc, sy, sx, mask, Ho, Wo };
    const Cam cam = cam_make(Ho, Wo, thr, focal, ppx, ppy, alpha, maxReproj, sub);
    const uint64_t imageKey = image_key(seed, image);

    int nUsable = 0;
    for (int i = 0; i < N; ++i) nUsable += mask[i] ? 1 : 0;
    if (nUsable < 4) {
        /* dead image: nothing is sampled */
        xm_identity16(pose16);
        if (status) *status = 1;
        for (int h = 0; h < nHyp; ++h) {
            if (cells) for (int j = 0; j < 4; ++j) cells[4 * h + j] = -1;
            if (tries) tries[h] = 0;
            if (scores) scores[h] = 0.0;
        }
        if (dbg) {
            Pose id;
            pose_identity(&id);
            dbg[0] = -1.0; dbg[1] = 0.0; dbg[2] = 0.0; dbg[3] = 0.0;
            pose_store12(&id, dbg + 4);
            pose_store12(&id, dbg + 16);
        }
        return 0;
    }

    /* ---- sample + score */
    int win = -1, anyNan = 0;
    double winScore = 0.0;
    Pose winPose, pose0;
    pose_identity(&winPose);
    pose_identity(&pose0);
    for (int h = 0; h < nHyp; ++h) {
        Pose pose;
        int c4[4] = { 0, 0, 0, 0 };
        int triesUsed = -(int)maxTries;                   /* exhausted: pose and cells are the last try's */
        for (uint32_t t = 0; t < maxTries; ++t)
            if (xm_sample_try(&im, &cam, imageKey, (uint32_t)h, t, &pose, c4)) { triesUsed = (int)t + 1; break; }
        const double score = xm_score(&im, &pose, &cam);
        if (cells) for (int j = 0; j < 4; ++j) cells[4 * h + j] = c4[j];
        if (tries) tries[h] = triesUsed;
        if (scores) scores[h] = score;
        if (score != score) anyNan = 1;
        if (h == 0) pose0 = pose;
        if (win < 0 || score > winScore) { win = h; winScore = score; winPose = pose; }
    }
    if (anyNan) { win = 0; winPose = pose0; }             /* a NaN score makes every soft-max probability NaN: draw() returns 0 */

    Pose pose = winPose;
    if (dbg) { dbg[0] = (double)win; pose_store12(&pose, dbg + 4); }

    /* ---- refine: inliers are the usable cells below the threshold */
    unsigned char *inl = (unsigned char *)malloc((size_t)N);
    unsigned best = 4, finalInl = 0;
    int rounds = 0, evals = 0;
    for (int step = 0; step < XL_DSAC_MAX_REF_STEPS; ++step) {
        unsigned cnt = 0;
        for (int i = 0; i < N; ++i) {
            inl[i] = (mask[i] && xm_cell_err(&im, &pose, i, &cam) < cam.thr) ? 1 : 0;
            cnt += inl[i];
        }
        if (cnt <= best) break;
        best = cnt;
        Pose upd = pose;
        if (!xm_lm_pnp(&im, inl, &cam, &upd, &evals)) break;
        pose = upd;
        finalInl = cnt;
        ++rounds;
    }
    free(inl);

    /* ---- write (pose2trans): inverse rigid transform, float row-major */
    pose_to_c2w16(&pose, pose16);
    if (status) *status = 0;
    if (dbg) {
        dbg[1] = (double)rounds; dbg[2] = (double)finalInl; dbg[3] = (double)evals;
        pose_store12(&pose, dbg + 16);
    }
    return 0;
}

#ifdef XM_MAIN
/* dsac_masked_ref FILE Ho Wo nHyp thr maxTries: FILE holds float32 coords [3,Ho,Wo] then the uint8 mask [Ho,Wo].  Runs the
 * image with every optional output, then with none, then with an all-zero mask (the dead path); prints the results. */
int main(int argc, char **argv)
{
    if (argc != 7) { fprintf(stderr, "usage: %s FILE Ho Wo nHyp thr maxTries\n", argv[0]); return 2; }
    const int Ho = atoi(argv[2]), Wo = atoi(argv[3]), nHyp = atoi(argv[4]);
    const float thr = (float)atof(argv[5]);
    const long maxTries = atol(argv[6]);
    if (Ho <= 0 || Wo <= 0 || nHyp <= 0 || maxTries <= 0 || Ho * Wo > XM_MAX_CELLS) return 2;
    const size_t N = (size_t)Ho * (size_t)Wo;
    float *buf = (float *)malloc(sizeof(float) * 3 * N);
    uint8_t *mask = (uint8_t *)malloc(N);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(buf, sizeof(float), 3 * N, f) != 3 * N || fread(mask, 1, N, f) != N) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    fclose(f);
    int32_t *cells = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)nHyp), *tries = (int32_t *)malloc(sizeof(int32_t) * (size_t)nHyp);
    double *scores = (double *)malloc(sizeof(double) * (size_t)nHyp);
    double dbg[XM_DBG];
    float pose[16];
    int32_t status = -1, status2 = -1, status3 = -1;
    const int st = xm_forward_rgb_masked(buf, (int64_t)N, Wo, 1, Ho, Wo, mask, pose, &status, nHyp, thr, 480.0f, Wo * 4.0f, Ho * 4.0f,
                                         100.0f, 100.0f, 8, 1305, 0, (uint32_t)maxTries, cells, tries, scores, dbg);
    printf("masked: rc %d status %d winner %d rounds %d inliers %d centre %.6f %.6f %.6f\n", st, (int)status, (int)dbg[0], (int)dbg[1],
           (int)dbg[2], pose[3], pose[7], pose[11]);
    const int st2 = xm_forward_rgb_masked(buf, (int64_t)N, Wo, 1, Ho, Wo, mask, pose, &status2, nHyp, thr, 480.0f, Wo * 4.0f, Ho * 4.0f,
                                          100.0f, 100.0f, 8, 1305, 0, (uint32_t)maxTries, NULL, NULL, NULL, NULL);
    memset(mask, 0, N);
    const int st3 = xm_forward_rgb_masked(buf, (int64_t)N, Wo, 1, Ho, Wo, mask, pose, &status3, nHyp, thr, 480.0f, Wo * 4.0f, Ho * 4.0f,
                                          100.0f, 100.0f, 8, 1305, 0, (uint32_t)maxTries, cells, tries, scores, dbg);
    printf("no outputs: rc %d status %d; dead: rc %d status %d winner %d\n", st2, (int)status2, st3, (int)status3, (int)dbg[0]);
    free(scores); free(tries); free(cells); free(mask); free(buf);
    return (st == 0 && st2 == 0 && st3 == 0 && status == 0 && status2 == 0 && status3 == 1) ? 0 : 1;
}
#endif
