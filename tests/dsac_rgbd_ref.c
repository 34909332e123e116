/*
 * tests/dsac_rgbd_ref.c — CPU restatement of the RGB-D DSAC* solver (crossloc_amd/csrc/xl_dsac_rgbd.hip).
 *
 * TEST INFRASTRUCTURE ONLY.  The lane-local arithmetic is the product's xl_dsac_rgbd_math.h, compiled here by gcc as C99
 * with -ffp-contract=off.  This file restates serially what the kernel does in parallel around it: the x-major list of
 * valid cells, the tries of a hypothesis in ascending order (the kernel's ballot picks the lowest accepted lane), the
 * 64-lane walk over the valid list with its xor butterfly, first-maximum-wins selection, and the refinement's walk of 256
 * virtual threads (xr_refine, rgbd_ref_common.h; the order of its block sums: xl_dsac_reduce.h).  Bitwise GPU == this file checks the kernel's orchestration
 * and that gcc and hipcc agree on the same IEEE operations; the formulas themselves are checked against
 * tests/indep_dsac_rgbd.py (numpy, SVD Kabsch), which shares no code with the header.
 *
 * With -DXR_MAIN the file is a program of its own (for the sanitizer run): see main() at the end.
 */
#include "rgbd_ref_common.h"          /* the input record, staging, the cell error, the refinement loop; xl_dsac_rgbd_math.h */

#define XR_DBG 16
#define XR_MAX_CELLS 6144

/*
 * One image.  Exactly one of cam ([3,Ho,Wo] strides cc, cy, cx) and depth ([Ho,Wo] strides dy, dx) is non-null.
 * Outputs (all nullable except pose16): cells [nHyp,3] cell indices of the accepted try (-1: not sampled), tries [nHyp],
 * scores [nHyp], dbg [16] as the kernel writes it, hypPoses [nHyp,12], and of the refinement roundCounts [100] (inlier
 * count of every round entered, the rejected last one included; -1 beyond), roundPoses [100,12] and roundMasks
 * [100, Ho*Wo] (cells fitted in an accepted round).
 */
int xr_forward_rgbd(const float *coords, int64_t sc, int64_t sy, int64_t sx,
                    const float *cam, int64_t cc, int64_t cy, int64_t cx, const float *depth, int64_t dy, int64_t dx,
                    int Ho, int Wo, int nHyp, float thr, float alpha, float maxDist,
                    float focal, float ppx, float ppy, int sub, uint64_t seed, uint64_t image, uint32_t maxTries,
                    float *pose16, int32_t *cells, int32_t *tries, double *scores, double *dbg, double *hypPoses,
                    int32_t *roundCounts, double *roundPoses, uint8_t *roundMasks)
{
    if (!coords || !pose16 || (cam == NULL) == (depth == NULL) || Ho <= 0 || Wo <= 0 || nHyp <= 0 || maxTries == 0) return -1;
    if (!cam && sub <= 0) return -1;
    const int N = Ho * Wo;
    if (N > XR_MAX_CELLS) return -2;
    const RgbdSrc in = xr_src(coords, sc, sy, sx, cam, cc, cy, cx, depth, dy, dx, focal, ppx, ppy, sub);
    Staged S;
    const int nValid = xr_stage(&S, &in, Ho, Wo);
    const uint64_t imageKey = image_key(seed, image);
    const float beta = 5.0f / thr;
    const float fac = alpha / (float)Wo / (float)Ho;
    const double invalidTerm = rgbd_soft_term(maxDist, beta, thr);

    /* ---- sample + score */
    int win = -1, anyNan = 0;
    double winScore = 0.0;
    Pose winPose, pose0;
    pose_identity(&winPose);
    pose_identity(&pose0);
    for (int h = 0; h < nHyp; ++h) {
        Pose pose;
        pose_identity(&pose);
        int ks[3] = { -1, -1, -1 };
        int triesUsed = 0;
        if (nValid > 0) {
            triesUsed = -(int)maxTries;
            for (uint32_t t = 0; t < maxTries; ++t) {
                const uint64_t st = try_state(imageKey, (uint32_t)h, t);
                double pc[9], Xw[9];
                for (int j = 0; j < 3; ++j) {
                    ks[j] = draw(st, j, nValid);
                    for (int c = 0; c < 3; ++c) { pc[3 * j + c] = (double)S.p[c][ks[j]]; Xw[3 * j + c] = (double)S.X[c][ks[j]]; }
                }
                if (rgbd_try_fit(pc, Xw, thr, &pose)) { triesUsed = (int)t + 1; break; }
            }
        }
        double part[64];
        for (int l = 0; l < 64; ++l) {
            double acc = 0.0;
            for (int k = l; k < nValid; k += 64) acc += rgbd_soft_term(xr_err(&S, &pose, k, maxDist), beta, thr);
            part[l] = acc;
        }
        double total = butterfly64(part);      /* the order: xl_dsac_reduce.h */
        total = total + (double)(N - nValid) * invalidTerm;
        const double score = total * (double)fac;
        if (cells) for (int j = 0; j < 3; ++j) cells[3 * h + j] = (ks[j] >= 0) ? S.cell[ks[j]] : -1;
        if (tries) tries[h] = triesUsed;
        if (scores) scores[h] = score;
        if (hypPoses) pose_store12(&pose, hypPoses + 12 * h);
        if (score != score) anyNan = 1;
        if (h == 0) pose0 = pose;
        if (win < 0 || score > winScore) { win = h; winScore = score; winPose = pose; }
    }
    if (anyNan) { win = 0; winPose = pose0; }       /* a NaN score makes every soft-max probability NaN: draw() returns 0 */

    /* ---- refine (refineHypRGBD, dsacstar_util.h:611-677) */
    Pose pose = winPose;
    XrRefine ro;
    xr_refine(&S, thr, maxDist, &pose, &ro, NULL, roundCounts, roundPoses, roundMasks, N);

    /* ---- write (pose2trans): inverse rigid transform, float row-major */
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) pose16[4 * i + j] = (float)pose.R[3 * j + i];
        pose16[4 * i + 3] = (float)(-(pose.R[i] * pose.t[0] + pose.R[3 + i] * pose.t[1] + pose.R[6 + i] * pose.t[2]));
    }
    pose16[12] = 0.0f; pose16[13] = 0.0f; pose16[14] = 0.0f; pose16[15] = 1.0f;
    if (dbg) {
        dbg[0] = (double)win; dbg[1] = (double)nValid; dbg[2] = (double)ro.rounds; dbg[3] = (double)ro.finalInl;
        pose_store12(&pose, dbg + 4);
    }
    xr_free(&S);
    return 0;
}

/* --- hooks for the formula tests: thin calls into the shared header --- */

/* Kabsch on n pairs (p camera, X scene, [n,3] doubles), sums taken serially: out12 = R row-major, t */
void xr_test_kabsch(int n, const double *p, const double *X, double *out12)
{
    double s[XLR_SUMS_CENTROID] = { 0 }, a[XLR_SUMS_COV] = { 0 }, cp[3], cX[3];
    for (int i = 0; i < n; ++i) rgbd_acc_centroid(s, p[3 * i], p[3 * i + 1], p[3 * i + 2], X[3 * i], X[3 * i + 1], X[3 * i + 2]);
    rgbd_centroids(s, cp, cX);
    for (int i = 0; i < n; ++i) rgbd_acc_cov(a, cp, cX, p[3 * i], p[3 * i + 1], p[3 * i + 2], X[3 * i], X[3 * i + 1], X[3 * i + 2]);
    Pose o;
    rgbd_kabsch_fit(cp, cX, a, &o);
    pose_store12(&o, out12);
}

void xr_test_cam_from_depth(float d, int y, int x, float f, float ppx, float ppy, int sub, float *out3)
{
    rgbd_cam_from_depth(d, y, x, f, ppx, ppy, sub, out3, out3 + 1, out3 + 2);
}

#ifdef XR_MAIN
/* dsac_rgbd_ref FILE Ho Wo nHyp thr maxDist: FILE holds float32 coords [3,Ho,Wo] then camera coordinates [3,Ho,Wo].  Runs
 * the camera form with every optional output, then the depth form on the camera tensor's z plane; prints both poses. */
int main(int argc, char **argv)
{
    if (argc != 7) { fprintf(stderr, "usage: %s FILE Ho Wo nHyp thr maxDist\n", argv[0]); return 2; }
    const int Ho = atoi(argv[2]), Wo = atoi(argv[3]), nHyp = atoi(argv[4]);
    const float thr = (float)atof(argv[5]), maxDist = (float)atof(argv[6]);
    if (Ho <= 0 || Wo <= 0 || nHyp <= 0 || Ho * Wo > XR_MAX_CELLS) return 2;
    const size_t N = (size_t)Ho * (size_t)Wo;
    float *buf = (float *)malloc(sizeof(float) * 6 * N);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(buf, sizeof(float), 6 * N, f) != 6 * N) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fclose(f);
    int32_t *cells = (int32_t *)malloc(sizeof(int32_t) * 3 * (size_t)nHyp), *tries = (int32_t *)malloc(sizeof(int32_t) * (size_t)nHyp);
    double *scores = (double *)malloc(sizeof(double) * (size_t)nHyp), *hyp = (double *)malloc(sizeof(double) * 12 * (size_t)nHyp);
    int32_t *rc = (int32_t *)malloc(sizeof(int32_t) * XR_MAX_REF_STEPS);
    double *rp = (double *)malloc(sizeof(double) * 12 * XR_MAX_REF_STEPS);
    uint8_t *rm = (uint8_t *)malloc(N * XR_MAX_REF_STEPS);
    double dbg[XR_DBG];
    float pose[16];
    int st = xr_forward_rgbd(buf, (int64_t)N, Wo, 1, buf + 3 * N, (int64_t)N, Wo, 1, NULL, 0, 0, Ho, Wo, nHyp, thr, 100.0f, maxDist,
                             480.0f, Wo * 4.0f, Ho * 4.0f, 8, 1305, 0, 1000000u, pose, cells, tries, scores, dbg, hyp, rc, rp, rm);
    printf("camera form: status %d winner %d nValid %d rounds %d inliers %d centre %.6f %.6f %.6f\n", st, (int)dbg[0], (int)dbg[1],
           (int)dbg[2], (int)dbg[3], pose[3], pose[7], pose[11]);
    int st2 = xr_forward_rgbd(buf, (int64_t)N, Wo, 1, NULL, 0, 0, 0, buf + 5 * N, Wo, 1, Ho, Wo, nHyp, thr, 100.0f, maxDist,
                              480.0f, Wo * 4.0f, Ho * 4.0f, 8, 1305, 0, 1000000u, pose, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
    printf("depth form: status %d centre %.6f %.6f %.6f\n", st2, pose[3], pose[7], pose[11]);
    free(rm); free(rp); free(rc); free(hyp); free(scores); free(tries); free(cells); free(buf);
    return (st == 0 && st2 == 0) ? 0 : 1;
}
#endif
