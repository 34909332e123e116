/*
 * oracle/dsac_oracle.c — CPU restatement of CrossLoc's `dsacstar.forward_rgb`.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in the product path (crossloc_amd/, dsacstar.py)
 * may include, link or call this file; only tests/, __graft_entry__.smoke() and
 * bench.py's cpu_baseline leg use it, as the checker / reported CPU baseline.
 *
 * The dependency runs the other way, and only to the product's headers: the lane-local arithmetic (deterministic exp /
 * sincos / atan2, RNG, the camera record, projection, cell error and the soft-inlier sigmoid, quartic, P3P, the per-cell
 * normal equations, Cholesky step, the LM stop rule and its constants, the float 4x4 write, the backward pass's
 * derivatives) is the product's crossloc_amd/csrc/xl_dsac_math.h, compiled here by gcc as C99; the round limit is the public
 * header's.  This file restates serially what the kernels do in
 * parallel around it: the try loop (first accepted try), the lane-strided partial sums and the xor-butterfly, the
 * 256-thread reduction of the normal equations (block_sum of xl_dsac_reduce.h, where the order is stated), the LM state machine, refinement, both drivers.  So bitwise GPU == oracle
 * checks that orchestration and that gcc and hipcc agree on the same IEEE operations; it does NOT check the shared
 * formulas.  Those are guarded by the known answers below, by the independent implementation (tests/indep_dsac.py) and,
 * against a change of rounding or expression order, by tests/test_oracle_dsac_pin.py.
 *
 * PARITY UNPINNED vs the reference binary: the reference extension delegates all of its
 * geometry to OpenCV 3.4.2 (cv::solvePnP P3P / ITERATIVE, cv::projectPoints,
 * cv::Rodrigues), which is neither vendored in /root/reference nor installed in the
 * build image, and the reference ships no tests or golden vectors for this path.  The
 * restatement is therefore pinned by analytic known answers (tests/test_oracle_dsac.py):
 * exact-coordinate scenes recover the ground-truth pose, P3P recovers a known pose,
 * closed-form soft-inlier scores, refinement monotonicity, hypothesis-order invariance.
 *
 * What is restated (reference file:line, relative to /root/reference/):
 *   orchestration, constants      dsacstar/dsacstar.cpp:47-48, 63-178
 *   createSampling                dsacstar/dsacstar_util.h:59-76
 *   sampleHypotheses/safeSolvePnP dsacstar/dsacstar_util.h:91-120, 135-221
 *   getReproErrs (calcJ=false)    dsacstar/dsacstar_util.h:356-446
 *   getHypScores                  dsacstar/dsacstar_util.h:316-343
 *   softMax / draw(argmax)        dsacstar/dsacstar_util.h:684-752
 *   refineHyp                     dsacstar/dsacstar_util.h:522-597
 *   pose2trans + write-back       dsacstar/dsacstar_util.h:759-770, dsacstar.cpp:172-177
 *   ThreadRand semantics          dsacstar/thread_rand.cpp:13-54, 68-71
 *
 * Third-party arithmetic (OpenCV 3.4.2, pinned by setup/environment.yml:11) restated
 * from its published algorithms, see DESIGN.md §"Solver arithmetic":
 *   - projectPoints: Xc = R*X + t in double, z = Z ? 1/Z : 1 (no cheirality test),
 *     u = x*f + cx, stored as float.
 *   - P3P + 4th point: law-of-cosines quartic (Grunert form of the Gao et al. system
 *     OpenCV solves), Ferrari resolution with a Newton root of the resolvent cubic,
 *     two Newton polish steps on the three distances, rigid alignment through the two
 *     triangle frames; the candidate with the smallest squared pixel error on the 4th
 *     point wins (OpenCV p3p::solve four-point overload behaviour).
 *   - ITERATIVE PnP with extrinsic guess: CvLevMarq state machine (max 20 outer
 *     iterations, eps FLT_EPSILON, lambda = 10^k, k0 = -3, k+1 on error increase up to
 *     16, k-1 on accept, damping JtJ.diag *= 1+lambda), 6x6 solve by Cholesky, on a
 *     left-multiplicative rotation increment instead of OpenCV's global Rodrigues vector.
 *
 * Deliberate, documented deviations that make "bit-exact hypothesis indices" definable
 * (SURVEY.md §7 hard parts): the RNG is counter-based (seed, image, hypothesis, try),
 * not std::mt19937 per OpenMP thread; every transcendental is a fixed polynomial built
 * from + - * / sqrt so gcc and hipcc produce identical bits (compile with
 * -ffp-contract=off); reductions over cells use a fixed order (lane-strided partials +
 * xor-butterfly) instead of the reference's x-major serial order.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "xl_dsac_math.h"             /* crossloc_amd/csrc: the lane-local arithmetic, shared with the kernels */
#include "xl_dsac_reduce.h"           /* the canonical block sum and its order (plain-C half) */
#include "../../include/crossloc_dsac.h"      /* beside crossloc_amd/csrc, as the kernels include it: XL_DSAC_MAX_REF_STEPS */

/* ------------------------------------------------------------------ small helpers */

typedef struct {
    const float *base; int64_t sc, sy, sx;   /* strides in elements */
    int Ho, Wo;
} xo_coords;

static void xo_fetch(const xo_coords *c, int x, int y, double X[3])
{
    const float *p = c->base + (int64_t)y * c->sy + (int64_t)x * c->sx;
    X[0] = (double)p[0];
    X[1] = (double)p[c->sc];
    X[2] = (double)p[2 * c->sc];
}

static Cam xo_cam(int Ho, int Wo, float thr, float focal, float ppx, float ppy, float alpha, float maxReproj, int sub)
{
    return cam_make(Ho, Wo, thr, focal, ppx, ppy, alpha, maxReproj, sub);
}

/* the unit-test hooks pass the intrinsics as doubles and no grid */
static Cam xo_test_cam(double f, double cx, double cy, float maxReproj)
{
    return cam_make(0, 0, 0.0f, f, cx, cy, 0.0f, maxReproj, 0);
}

/* clamped reprojection error of cell i */
static float xo_cell_err(const xo_coords *co, const Pose *p, int i, const Cam *cam)
{
    int y = i / cam->Wo, x = i - y * cam->Wo;
    double X[3];
    xo_fetch(co, x, y, X);
    return cell_err(p, X[0], X[1], X[2], y, x, cam);
}

/* ------------------------------------------------------------------ one sampling try */

/* returns true if the try is accepted; pose holds the try's result (identity if P3P failed: safeSolvePnP zeroes
 * rvec/tvec, dsacstar_util.h:114-116), cells[4] the sampled (y*Wo + x) indices (dsacstar_util.h:159-219). */
static bool xo_sample_try(const xo_coords *co, const Cam *cam, uint64_t imageKey, uint32_t hyp, uint32_t t,
                          Pose *pose, int cells[4])
{
    uint64_t st = try_state(imageKey, hyp, t);
    V3 P[4];
    double uv[4][2];
    float px[4], py[4];
    for (int j = 0; j < 4; ++j) {
        int x = draw(st, 2 * j, cam->Wo);         /* x first, then y (dsacstar_util.h:171-172) */
        int y = draw(st, 2 * j + 1, cam->Ho);
        double X[3];
        cells[j] = y * cam->Wo + x;
        px[j] = cell_px(cam, x);
        py[j] = cell_px(cam, y);
        uv[j][0] = (double)px[j]; uv[j][1] = (double)py[j];
        xo_fetch(co, x, y, X);
        P[j].x = X[0]; P[j].y = X[1]; P[j].z = X[2];
    }
    if (!p3p(P[0], P[1], P[2], P[3], uv, cam, pose)) {
        pose_identity(pose);
        return false;
    }
    for (int j = 0; j < 4; ++j) {
        float u, v;
        project(pose, P[j].x, P[j].y, P[j].z, cam, &u, &v);
        float dx = px[j] - u, dy = py[j] - v;
        double n = sqrt((double)dx * (double)dx + (double)dy * (double)dy);
        if (!(n < (double)cam->thr)) return false;
    }
    return true;
}

/* the try loop of one hypothesis: the first accepted try wins (on the GPU: 64 tries at a time, lowest set ballot bit);
 * returns the number of tries used, negative if none was accepted (pose and cells are then the last try's) */
static int32_t xo_sample_hyp(const xo_coords *co, const Cam *cam, uint64_t imageKey, uint32_t hyp, uint32_t maxTries,
                             Pose *pose, int cells[4])
{
    for (uint32_t t = 0; t < maxTries; ++t)
        if (xo_sample_try(co, cam, imageKey, hyp, t, pose, cells)) return (int32_t)(t + 1);
    return -(int32_t)maxTries;
}

/* soft-inlier score of one pose (dsacstar_util.h:316-343 over the map of :356-446):
 * lane l accumulates cells l, l+64, ... in row-major cell order, then the butterfly. */
static double xo_score(const xo_coords *co, const Pose *pose, const Cam *cam)
{
    float beta = 5.0f / cam->thr;
    double part[64];
    for (int l = 0; l < 64; ++l) {
        double acc = 0.0;
        for (int i = l; i < cam->N; i += 64) {
            acc += 1.0 - soft_inlier_st(xo_cell_err(co, pose, i, cam), cam->thr, beta);
        }
        part[l] = acc;
    }
    double total = butterfly64(part);
    float fac = cam->alpha / (float)cam->Wo / (float)cam->Ho;
    return total * (double)fac;
}

/* ------------------------------------------------------------------ LM refinement */

#define XO_T XL_BLOCK_THREADS

/* per-thread 28-vectors of the canonical block sum (block_sum, xl_dsac_reduce.h): [XO_T][28] contiguous */
typedef struct { double v[28]; } xo_vec28;

/* normal equations of the reprojection residuals over the inlier set at pose p:
 * out[0..20] upper triangle of JtJ (row-major), out[21..26] Jt r, out[27] sum r^2 */
static void xo_normal_eq(const xo_coords *co, const unsigned char *inl, const Pose *p, const Cam *cam, double out[28])
{
    xo_vec28 *part = (xo_vec28 *)malloc(sizeof(xo_vec28) * XO_T);
    for (int tdx = 0; tdx < XO_T; ++tdx) {
        double a[28];
        for (int k = 0; k < 28; ++k) a[k] = 0.0;
        for (int i = tdx; i < cam->N; i += XO_T) {
            if (!inl[i]) continue;
            int y = i / co->Wo, x = i - y * co->Wo;
            double X[3];
            xo_fetch(co, x, y, X);
            pnp_cell_normal_eq(p, X[0], X[1], X[2], y, x, cam, a);
        }
        for (int k = 0; k < 28; ++k) part[tdx].v[k] = a[k];
    }
    block_sum(part[0].v, 28, out);
    free(part);
}

/* cv::solvePnP(ITERATIVE, useExtrinsicGuess=true) restated: the CvLevMarq state machine (max 20 outer iterations, eps
 * FLT_EPSILON, lambda = 10^k, k0 = -3, k+1 on error increase up to 16, k-1 on accept); returns 0 on failure (pose
 * untouched) */
static int xo_lm_pnp(const xo_coords *co, const unsigned char *inl, const Cam *cam, Pose *pose, int *evals)
{
    Pose cur = *pose, prev;
    double ne[28], ne_new[28];
    int lg = -3, iters = 0;
    xo_normal_eq(co, inl, &cur, cam, ne);
    ++*evals;
    for (;;) {
        double d[6];
        prev = cur;
        if (!solve6(ne, lambda_of(lg), d)) return 0;
        apply_step(&prev, d, &cur);
        double prevErr = ne[27];
        xo_normal_eq(co, inl, &cur, cam, ne_new);
        ++*evals;
        while (ne_new[27] > prevErr) {
            if (++lg <= 16) {
                if (!solve6(ne, lambda_of(lg), d)) return 0;
                apply_step(&prev, d, &cur);
                xo_normal_eq(co, inl, &cur, cam, ne_new);
                ++*evals;
            } else break;
        }
        lg = (lg - 1 > -16) ? lg - 1 : -16;
        ++iters;
        if (iters >= XLM_LM_MAX_ITER || lm_step_small(d, &prev)) break;
        memcpy(ne, ne_new, sizeof(ne));
    }
    if (!pose_not_nan(&cur)) return 0;
    *pose = cur;
    return 1;
}

/* refineHyp (dsacstar_util.h:522-597): pose is refined in place; inlAcc (may be NULL) receives the inlier map of the
 * last successful re-fit (all zero if none), *nAcc its size. */
static void xo_refine(const xo_coords *co, const Cam *cam, Pose *pose, unsigned char *inlAcc, unsigned *nAcc,
                      int *roundsOut, int *evalsOut)
{
    const int N = cam->N;
    float *errs = (float *)malloc(sizeof(float) * (size_t)N);
    unsigned char *inl = (unsigned char *)malloc((size_t)N);
    for (int i = 0; i < N; ++i) errs[i] = xo_cell_err(co, pose, i, cam);
    if (inlAcc) memset(inlAcc, 0, (size_t)N);
    unsigned best = 4, finalInl = 0;
    int rounds = 0, evals = 0;
    for (int step = 0; step < XL_DSAC_MAX_REF_STEPS; ++step) {
        unsigned cnt = 0;
        for (int i = 0; i < N; ++i) { inl[i] = (errs[i] < cam->thr) ? 1 : 0; cnt += inl[i]; }
        if (cnt <= best) break;
        best = cnt;
        Pose upd = *pose;
        if (!xo_lm_pnp(co, inl, cam, &upd, &evals)) break;
        *pose = upd;
        finalInl = cnt;
        if (inlAcc) memcpy(inlAcc, inl, (size_t)N);
        ++rounds;
        for (int i = 0; i < N; ++i) errs[i] = xo_cell_err(co, pose, i, cam);
    }
    free(errs); free(inl);
    if (nAcc) *nAcc = finalInl;
    if (roundsOut) *roundsOut = rounds;
    if (evalsOut) *evalsOut = evals;
}

/* ------------------------------------------------------------------ public entry points */

/*
 * Debug record layout (dbg may be NULL), doubles:
 *   [0] winner index   [1] refinement rounds accepted   [2] final inlier count
 *   [3] LM normal-equation evaluations   [4..15] winner pose before refinement (R row-major, t)
 *   [16..27] refined pose (R, t)
 */
int xo_dsac_forward_rgb(const float *coords, int64_t sc, int64_t sy, int64_t sx, int Ho, int Wo,
                        float *out_pose16, int nHyp, float thr, float focal, float ppx, float ppy,
                        float alpha, float maxReproj, int sub, uint64_t seed, uint64_t image,
                        uint32_t maxTries,
                        int32_t *out_cells /*[nHyp*4] or NULL*/, int32_t *out_tries /*[nHyp] or NULL*/,
                        double *out_scores /*[nHyp] or NULL*/, double *dbg /*[28] or NULL*/)
{
    if (!coords || !out_pose16 || nHyp <= 0 || Ho <= 0 || Wo <= 0 || sub <= 0 || maxTries == 0) return -1;
    xo_coords co = { coords, sc, sy, sx, Ho, Wo };
    const Cam cam = xo_cam(Ho, Wo, thr, focal, ppx, ppy, alpha, maxReproj, sub);
    const uint64_t imageKey = image_key(seed, image);

    Pose *hyps = (Pose *)malloc(sizeof(Pose) * (size_t)nHyp);
    double *scores = (double *)malloc(sizeof(double) * (size_t)nHyp);
    int32_t *cells = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)nHyp);
    int32_t *tries = (int32_t *)malloc(sizeof(int32_t) * (size_t)nHyp);

    /* sampleHypotheses + getReproErrs + getHypScores, parallel over hypotheses like the reference */
#pragma omp parallel for schedule(dynamic, 1)
    for (int h = 0; h < nHyp; ++h) {
        int c4[4];
        tries[h] = xo_sample_hyp(&co, &cam, imageKey, (uint32_t)h, maxTries, &hyps[h], c4);
        for (int j = 0; j < 4; ++j) cells[4 * h + j] = c4[j];
        scores[h] = xo_score(&co, &hyps[h], &cam);
    }

    /* softMax + draw(argmax): first maximum wins; any NaN score makes every prob NaN -> index 0 */
    int win = 0, anyNan = 0;
    for (int h = 0; h < nHyp; ++h) if (scores[h] != scores[h]) anyNan = 1;
    if (!anyNan)
        for (int h = 1; h < nHyp; ++h) if (scores[h] > scores[win]) win = h;

    Pose pose = hyps[win];
    if (dbg) {
        dbg[0] = (double)win;
        pose_store12(&pose, dbg + 4);
    }

    int rounds = 0, evals = 0;
    unsigned finalInl = 0;
    xo_refine(&co, &cam, &pose, NULL, &finalInl, &rounds, &evals);

    pose_to_c2w16(&pose, out_pose16);     /* pose2trans: inverse of [R t; 0 1], stored float row-major */

    if (out_cells) memcpy(out_cells, cells, sizeof(int32_t) * 4 * (size_t)nHyp);
    if (out_tries) memcpy(out_tries, tries, sizeof(int32_t) * (size_t)nHyp);
    if (out_scores) memcpy(out_scores, scores, sizeof(double) * (size_t)nHyp);
    if (dbg) {
        dbg[1] = (double)rounds; dbg[2] = (double)finalInl; dbg[3] = (double)evals;
        pose_store12(&pose, dbg + 16);
    }
    free(hyps); free(scores); free(cells); free(tries);
    return 0;
}

/* --- unit-test hooks (known-answer tests call these directly): thin calls into xl_dsac_math.h --- */

int xo_test_p3p(const double *P12, const double *uv8, double f, double cx, double cy, double *Rt12)
{
    V3 P[4];
    double uv[4][2];
    for (int i = 0; i < 4; ++i) {
        P[i].x = P12[3 * i]; P[i].y = P12[3 * i + 1]; P[i].z = P12[3 * i + 2];
        uv[i][0] = uv8[2 * i]; uv[i][1] = uv8[2 * i + 1];
    }
    const Cam cam = xo_test_cam(f, cx, cy, 0.0f);
    Pose p;
    int ok = p3p(P[0], P[1], P[2], P[3], uv, &cam, &p);
    if (ok) pose_store12(&p, Rt12);
    return ok;
}

double xo_test_score(const float *coords, int64_t sc, int64_t sy, int64_t sx, int Ho, int Wo,
                     const double *Rt12, float thr, float alpha, float maxReproj,
                     float focal, float ppx, float ppy, int sub)
{
    xo_coords co = { coords, sc, sy, sx, Ho, Wo };
    const Cam cam = xo_cam(Ho, Wo, thr, focal, ppx, ppy, alpha, maxReproj, sub);
    Pose p;
    pose_load12(Rt12, &p);
    return xo_score(&co, &p, &cam);
}

double xo_test_exp(double x) { return det_exp(x); }
void xo_test_sincos(double x, double *s, double *c) { det_sincos(x, s, c); }
int xo_test_quartic(const double *A5, double *roots4)
{
    /* the roots in slot order, packed */
    double x[4];
    unsigned mask = quartic(A5[0], A5[1], A5[2], A5[3], A5[4], &x[0], &x[1], &x[2], &x[3]);
    int n = 0;
    for (int i = 0; i < 4; ++i) if ((mask >> i) & 1u) roots4[n++] = x[i];
    return n;
}
void xo_test_draws(uint64_t seed, uint64_t image, uint32_t hyp, uint32_t t, int Wo, int Ho, int32_t *xy8)
{
    uint64_t st = try_state(image_key(seed, image), hyp, t);
    for (int j = 0; j < 4; ++j) { xy8[2 * j] = draw(st, 2 * j, Wo); xy8[2 * j + 1] = draw(st, 2 * j + 1, Ho); }
}
void xo_set_num_threads(int n)
{
#ifdef _OPENMP
    if (n > 0) omp_set_num_threads(n);
#else
    (void)n;
#endif
}
int xo_num_threads(void)
{
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

/* backward_rgb restatement (same translation unit: it uses the static helpers above) */
#include "dsac_bwd_oracle.c"
