/*
 * tests/rgbd_quality_ref.c — CPU restatement of the RGB-D pose-quality pass (crossloc_amd/csrc/xl_dsac_rgbd_quality.hip).
 *
 * TEST INFRASTRUCTURE ONLY.  The per-cell and per-image arithmetic is the product's xl_dsac_rgbd_quality_math.h, compiled
 * here by gcc as C99 with -ffp-contract=off.  This file restates serially what the kernel does in parallel around it: the
 * two walks of 256 virtual threads over the cells (thread t: cells t, t + 256, ... in ascending order), the canonical
 * block sum (xl_dsac_reduce.h states its order), the centroid formed between the walks.  Bitwise GPU == this
 * file therefore checks the kernel's orchestration and that gcc and hipcc agree on the same IEEE operations; the formulas
 * themselves are checked by tests/test_rgbd_quality_cpu.py (an uncentred numpy restatement, numeric Jacobians, Monte-Carlo
 * calibration, the solver restatement's scores).
 *
 * With -DXRQ_MAIN the file is a program of its own (for the sanitizer run): see main() at the end.
 */
#include "rgbd_ref_common.h"             /* the input record and the per-cell load; the block sum of xl_dsac_reduce.h */
#include "xl_dsac_rgbd_quality_math.h"   /* crossloc_amd/csrc: shared with the kernel */

#define XRQ_T XR_T
#define XRQ_SUMS (XLQR_SUMS1 + XLQR_SUMS2 + 4)   /* what xrq_test_sums exports: both walks, the centroid, the pivot ratio */

/* the kernel from its pose on: walk 1, reduction, centroid, walk 2, reduction, final step */
static void xrq_run(const RgbdSrc *in, const RgbdQ *q, const Pose *pose, bool poseOk, double *row, double *sums)
{
    double *part = (double *)malloc(sizeof(double) * XRQ_T * XLQR_SUMS2);
    const float beta = 5.0f / q->thr;
    double s1[XLQR_SUMS1], s2[XLQR_SUMS2], c[3], ratio;
    for (int tid = 0; tid < XRQ_T; ++tid) {
        double *a = part + tid * XLQR_SUMS1;
        for (int k = 0; k < XLQR_SUMS1; ++k) a[k] = 0.0;
        if (!poseOk) continue;
        for (int i = tid; i < q->N; i += XRQ_T) {
            const int y = i / q->Wo, x = i - y * q->Wo;
            float X[3], p[3];
            xr_load(in, y, x, X, p);
            rgbdq_cell1(pose, (double)X[0], (double)X[1], (double)X[2], p[0], p[1], p[2], q, beta, a);
        }
    }
    block_sum(part, XLQR_SUMS1, s1);
    rgbdq_centroid(s1, c);
    for (int tid = 0; tid < XRQ_T; ++tid) {
        double *a = part + tid * XLQR_SUMS2;
        for (int k = 0; k < XLQR_SUMS2; ++k) a[k] = 0.0;
        if (!poseOk) continue;
        for (int i = tid; i < q->N; i += XRQ_T) {
            const int y = i / q->Wo, x = i - y * q->Wo;
            float X[3], p[3];
            xr_load(in, y, x, X, p);
            rgbdq_cell2(pose, (double)X[0], (double)X[1], (double)X[2], p[0], p[1], p[2], q, c, a);
        }
    }
    block_sum(part, XLQR_SUMS2, s2);
    free(part);
    double tmp[XLQ_ROW];
    rgbdq_row(s1, s2, c, pose, q, poseOk, row ? row : tmp, &ratio);
    if (sums) {
        for (int k = 0; k < XLQR_SUMS1; ++k) sums[k] = s1[k];
        for (int k = 0; k < XLQR_SUMS2; ++k) sums[XLQR_SUMS1 + k] = s2[k];
        for (int k = 0; k < 3; ++k) sums[XLQR_SUMS1 + XLQR_SUMS2 + k] = c[k];
        sums[XLQR_SUMS1 + XLQR_SUMS2 + 3] = ratio;
    }
}

static int xrq_args(RgbdSrc *in, RgbdQ *q, const float *coords, int64_t sc, int64_t sy, int64_t sx,
                    const float *cam, int64_t cc, int64_t cy, int64_t cx, const float *depth, int64_t dy, int64_t dx,
                    int Ho, int Wo, float thr, float alpha, float maxDist, float focal, float ppx, float ppy, int sub)
{
    if (!coords || (cam == NULL) == (depth == NULL) || Ho <= 0 || Wo <= 0 || sub <= 0) return -1;
    *in = xr_src(coords, sc, sy, sx, cam, cc, cy, cx, depth, dy, dx, focal, ppx, ppy, sub);
    q->thr = thr; q->alpha = alpha; q->maxDist = maxDist; q->Ho = Ho; q->Wo = Wo; q->N = Ho * Wo;
    return 0;
}

/* the row the kernel must produce for one image: float32 cam->world 4x4 in, 64 doubles out */
int xrq_pose_quality(const float *coords, int64_t sc, int64_t sy, int64_t sx,
                     const float *cam, int64_t cc, int64_t cy, int64_t cx, const float *depth, int64_t dy, int64_t dx,
                     int Ho, int Wo, const float *pose16, float thr, float alpha, float maxDist,
                     float focal, float ppx, float ppy, int sub, double *row)
{
    RgbdSrc in;
    RgbdQ q;
    if (!pose16 || !row) return -1;
    if (xrq_args(&in, &q, coords, sc, sy, sx, cam, cc, cy, cx, depth, dy, dx, Ho, Wo, thr, alpha, maxDist, focal, ppx, ppy, sub)) return -1;
    const bool poseOk = quality_pose16_finite(pose16);
    Pose pose;
    if (poseOk) quality_pose_from16(pose16, &pose);
    else pose_identity(&pose);
    xrq_run(&in, &q, &pose, poseOk, row, NULL);
    return 0;
}

static bool xrq_pose12(const double *Rt12, Pose *pose)
{
    pose_load12(Rt12, pose);
    const bool ok = quality_pose_finite(pose);
    if (!ok) pose_identity(pose);
    return ok;
}

/* the same at a double world -> camera pose (R row-major, t): the solver restatement's refined pose and hypotheses */
int xrq_pose_quality_w2c(const float *coords, int64_t sc, int64_t sy, int64_t sx,
                         const float *cam, int64_t cc, int64_t cy, int64_t cx, const float *depth, int64_t dy, int64_t dx,
                         int Ho, int Wo, const double *Rt12, float thr, float alpha, float maxDist,
                         float focal, float ppx, float ppy, int sub, double *row)
{
    RgbdSrc in;
    RgbdQ q;
    if (!Rt12 || !row) return -1;
    if (xrq_args(&in, &q, coords, sc, sy, sx, cam, cc, cy, cx, depth, dy, dx, Ho, Wo, thr, alpha, maxDist, focal, ppx, ppy, sub)) return -1;
    Pose pose;
    const bool poseOk = xrq_pose12(Rt12, &pose);
    xrq_run(&in, &q, &pose, poseOk, row, NULL);
    return 0;
}

/* the reduced sums at a double world -> camera pose, XRQ_SUMS = 25 doubles: walk 1 [0..8] (n_valid, n, sum m, soft sum over
 * the valid cells, sum e, sum e^2, SSE), walk 2 [9..20] (C xx xy xz yy yz zz, the gradient sum u x r, sum r), the
 * centroid c [21..23] and the smallest relative Cholesky pivot of M [24] (NaN when M was not factored) */
int xrq_test_sums_w2c(const float *coords, int64_t sc, int64_t sy, int64_t sx,
                      const float *cam, int64_t cc, int64_t cy, int64_t cx, const float *depth, int64_t dy, int64_t dx,
                      int Ho, int Wo, const double *Rt12, float thr, float alpha, float maxDist,
                      float focal, float ppx, float ppy, int sub, double *sums)
{
    RgbdSrc in;
    RgbdQ q;
    if (!Rt12 || !sums) return -1;
    if (xrq_args(&in, &q, coords, sc, sy, sx, cam, cc, cy, cx, depth, dy, dx, Ho, Wo, thr, alpha, maxDist, focal, ppx, ppy, sub)) return -1;
    Pose pose;
    const bool poseOk = xrq_pose12(Rt12, &pose);
    xrq_run(&in, &q, &pose, poseOk, NULL, sums);
    return 0;
}

/* --- hooks for the formula tests: thin calls into the shared headers --- */

/* the world -> camera pose the kernel derives from a float cam->world 4x4 */
void xrq_test_pose_from16(const float *pose16, double *Rt12)
{
    Pose p;
    quality_pose_from16(pose16, &p);
    pose_store12(&p, Rt12);
}

/* apply_step: out = prev (-) d, i.e. R = Exp(-d_w) R_prev, t = t_prev - d_t */
void xrq_test_apply_step(const double *Rt12, const double *d6, double *out12)
{
    Pose prev, out;
    pose_load12(Rt12, &prev);
    apply_step(&prev, d6, &out);
    pose_store12(&out, out12);
}

int xrq_test_inv3(const double *ut6, double *inv9, double *minRatio) { return rgbdq_inv3(ut6, inv9, minRatio) ? 1 : 0; }

#ifdef XRQ_MAIN
/* rgbd_quality_ref FILE Ho Wo thr maxDist: FILE holds float32 coords [3,Ho,Wo], camera coordinates [3,Ho,Wo] and a cam->world
 * pose [16].  Takes the row in camera form, in depth form on the camera tensor's z plane, at the double pose and the sums;
 * prints status, counts and sigma of each. */
int main(int argc, char **argv)
{
    if (argc != 6) { fprintf(stderr, "usage: %s FILE Ho Wo thr maxDist\n", argv[0]); return 2; }
    const int Ho = atoi(argv[2]), Wo = atoi(argv[3]);
    const float thr = (float)atof(argv[4]), maxDist = (float)atof(argv[5]);
    if (Ho <= 0 || Wo <= 0) return 2;
    const size_t N = (size_t)Ho * (size_t)Wo;
    float *buf = (float *)malloc(sizeof(float) * (6 * N + 16));
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(buf, sizeof(float), 6 * N + 16, f) != 6 * N + 16) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fclose(f);
    const float *pose16 = buf + 6 * N;
    double row[XLQ_ROW], row2[XLQ_ROW], row3[XLQ_ROW], sums[XRQ_SUMS], Rt12[12];
    int st = xrq_pose_quality(buf, (int64_t)N, Wo, 1, buf + 3 * N, (int64_t)N, Wo, 1, NULL, 0, 0, Ho, Wo, pose16, thr, 100.0f, maxDist,
                              480.0f, Wo * 4.0f, Ho * 4.0f, 8, row);
    printf("camera form: rc %d status %d n_valid %d n_inliers %d sigma_m %.6g sigma_pos_m %.6g\n", st, (int)row[6], (int)row[58],
           (int)row[1], row[7], row[8]);
    int st2 = xrq_pose_quality(buf, (int64_t)N, Wo, 1, NULL, 0, 0, 0, buf + 5 * N, Wo, 1, Ho, Wo, pose16, thr, 100.0f, maxDist,
                               480.0f, Wo * 4.0f, Ho * 4.0f, 8, row2);
    printf("depth form: rc %d status %d n_valid %d n_inliers %d\n", st2, (int)row2[6], (int)row2[58], (int)row2[1]);
    xrq_test_pose_from16(pose16, Rt12);
    int st3 = xrq_pose_quality_w2c(buf, (int64_t)N, Wo, 1, buf + 3 * N, (int64_t)N, Wo, 1, NULL, 0, 0, Ho, Wo, Rt12, thr, 100.0f, maxDist,
                                   480.0f, Wo * 4.0f, Ho * 4.0f, 8, row3);
    int st4 = xrq_test_sums_w2c(buf, (int64_t)N, Wo, 1, buf + 3 * N, (int64_t)N, Wo, 1, NULL, 0, 0, Ho, Wo, Rt12, thr, 100.0f, maxDist,
                                480.0f, Wo * 4.0f, Ho * 4.0f, 8, sums);
    printf("double pose: rc %d %d same row %d pivot ratio %.3g\n", st3, st4, memcmp(row, row3, sizeof(row)) == 0, sums[XRQ_SUMS - 1]);
    free(buf);
    return (st == 0 && st2 == 0 && st3 == 0 && st4 == 0) ? 0 : 1;
}
#endif
