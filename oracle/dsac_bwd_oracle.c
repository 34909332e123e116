/*
 * oracle/dsac_bwd_oracle.c — CPU restatement of CrossLoc's `dsacstar.backward_rgb` (DSAC* expected pose loss and its
 * gradient with respect to the scene coordinates).  Included at the end of dsac_oracle.c (one translation unit).
 *
 * TEST INFRASTRUCTURE ONLY — same rules as dsac_oracle.c, and the same split: Rodrigues maps, residual rows, dProjectdObj,
 * pseudo-inverse, loss and dLoss come from the product's crossloc_amd/csrc/xl_dsac_math.h (the oracle depends on that header,
 * never the product on the oracle); this file keeps the serial dPNP, the reductions and the driver.  PARITY UNPINNED vs
 * the reference binary (OpenCV absent); pinned by numeric-derivative known answers in tests/test_oracle_dsac_bwd.py.
 *
 * What is restated (reference file:line, relative to /root/reference/dsacstar/):
 *   orchestration                    dsacstar.cpp:200-483
 *   getReproErrs(calcJ=true)         dsacstar_util.h:403-434   (rows d err / d (rvec, tvec), zero above maxReproj)
 *   softMax                          dsacstar_util.h:684-704
 *   loss / calcAngularDistance       dsacstar_loss.h:47-88
 *   dLoss                            dsacstar_loss.h:99-212
 *   dProjectdObj                     dsacstar_derivative.h:51-106
 *   dPNP (central differences)       dsacstar_derivative.h:131-190
 *   dScore / dSMScore                dsacstar_derivative.h:209-402
 *   trans2pose / pose2trans / getMax dsacstar_util.h:759-790, 821-834
 *
 * Third-party arithmetic restated from its published behaviour (OpenCV 3.4.2): cv::Rodrigues in both directions with
 * its analytic Jacobian (exact derivative of R = cos t I + (1-cos t) k k^T + sin t [k]x), the pose Jacobian of
 * cv::projectPoints (chain rule through Xc = R X + t, same z guard as the projection), cv::Mat::inv(DECOMP_SVD) of the
 * symmetric 6x6 J^T J as an eigen-decomposition pseudo-inverse with OpenCV's threshold 2*DBL_EPSILON*sum(w).
 *
 * Deliberate, documented deviations (on top of those of the forward restatement): sums over cells use the canonical
 * fixed order (thread-strided partials + butterfly) instead of x-major serial order; sum_c dRepro(c) J(c) is formed
 * before the product with dPNP (associativity); the ground-truth pose is inverted as a rigid transform (the reference
 * takes a general 4x4 inverse and lets cv::Rodrigues re-orthonormalise); R -> rvec uses atan2(sin, cos) where OpenCV
 * uses acos(cos); a non-finite dLoss is zeroed like a NaN one; the entropy print-out is not computed.
 */

/* ------------------------------------------------------------------ dPNP (central differences over P3P) */

/* 6x12 jacobian (row-major, [6][12]) of the P3P pose w.r.t. the four sampled scene coordinates; columns 9..11 stay
 * zero (the 4th point only disambiguates).  dsacstar_derivative.h:131-190: float points, float eps, the
 * += eps / -= 2 eps / += eps sequence is carried from column to column exactly as written there. */
static void xo_dpnp(const float obj[4][3], const double uv[4][2], const Cam *cam, double J[72])
{
    const float eps = 0.001f;
    float pts[4][3];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 3; ++j) pts[i][j] = obj[i][j];
    for (int i = 0; i < 72; ++i) J[i] = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            V3 P[4];
            Pose fwd, bwd;
            pts[i][j] += eps;
            for (int a = 0; a < 4; ++a) { P[a].x = (double)pts[a][0]; P[a].y = (double)pts[a][1]; P[a].z = (double)pts[a][2]; }
            int okf = p3p(P[0], P[1], P[2], P[3], uv, cam, &fwd);
            pts[i][j] -= 2 * eps;
            for (int a = 0; a < 4; ++a) { P[a].x = (double)pts[a][0]; P[a].y = (double)pts[a][1]; P[a].z = (double)pts[a][2]; }
            int okb = okf ? p3p(P[0], P[1], P[2], P[3], uv, cam, &bwd) : 0;
            if (!okf || !okb) { for (int k = 0; k < 72; ++k) J[k] = 0.0; return; }
            pts[i][j] += eps;
            double rf[3], rb[3];
            log_so3(fwd.R, rf);
            log_so3(bwd.R, rb);
            double den = (double)(2 * eps);
            int col = i * 3 + j, bad = 0;
            for (int k = 0; k < 3; ++k) {
                double a = (rf[k] - rb[k]) / den, b = (fwd.t[k] - bwd.t[k]) / den;
                J[k * 12 + col] = a;
                J[(3 + k) * 12 + col] = b;
                if (!(a == a) || !(b == b)) bad = 1;
            }
            if (bad) { for (int k = 0; k < 72; ++k) J[k] = 0.0; return; }
        }
}

/* ------------------------------------------------------------------ the entry point */

/* per-hypothesis record exported for parity tests (doubles) */
#define XO_BWD_REC 64
/*  [0] prob  [1] loss  [2] active  [3] accepted inliers  [4] clampI (path I zeroed)  [5] sog
 *  [6..17] refined pose (R, t)  [18..23] dLoss/dHyp  [24..29] w = pinv(JtJ) dLoss^T  [30..41] support-point gradients
 *  [42] max |jacobeanR|  [43] max |dPNP|  [44..49] g6 = sum_c dRepro(c) J_init(c)  [50..52] rvec of the refined pose */

int xo_dsac_backward_rgb(const float *coords, int64_t sc, int64_t sy, int64_t sx, int Ho, int Wo,
                         float *grad, int64_t gsc, int64_t gsy, int64_t gsx,      /* accumulated (+=) */
                         const float *gtPose16, int nHyp, float thr, float focal, float ppx, float ppy,
                         float wRot, float wTrans, float softClamp, float alpha, float maxReproj, int sub,
                         uint64_t seed, uint64_t image, uint32_t maxTries,
                         double *outLoss, double *rec /*[nHyp*XO_BWD_REC] or NULL*/)
{
    if (!coords || !grad || !gtPose16 || !outLoss || nHyp <= 0 || Ho <= 0 || Wo <= 0 || sub <= 0 || maxTries == 0) return -1;
    xo_coords co = { coords, sc, sy, sx, Ho, Wo };
    const Cam cam = xo_cam(Ho, Wo, thr, focal, ppx, ppy, alpha, maxReproj, sub);
    const uint64_t imageKey = image_key(seed, image);
    const int N = Ho * Wo;
    Gt gt;
    gt_from_pose16(gtPose16, &gt);

    Pose *init = (Pose *)malloc(sizeof(Pose) * (size_t)nHyp);
    Pose *ref = (Pose *)malloc(sizeof(Pose) * (size_t)nHyp);
    double *scores = (double *)malloc(sizeof(double) * (size_t)nHyp);
    double *probs = (double *)malloc(sizeof(double) * (size_t)nHyp);
    double *losses = (double *)malloc(sizeof(double) * (size_t)nHyp);
    double *sog = (double *)calloc((size_t)nHyp, sizeof(double));
    int32_t *cells = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)nHyp);
    unsigned char *inlAcc = (unsigned char *)calloc((size_t)nHyp * (size_t)N, 1);
    unsigned *nAcc = (unsigned *)calloc((size_t)nHyp, sizeof(unsigned));
    double *dRinit = (double *)calloc((size_t)nHyp * 27, sizeof(double));
    double *dRref = (double *)calloc((size_t)nHyp * 27, sizeof(double));
    double *wv = (double *)calloc((size_t)nHyp * 6, sizeof(double));
    double *spg = (double *)calloc((size_t)nHyp * 12, sizeof(double));
    int *clampI = (int *)calloc((size_t)nHyp, sizeof(int));
    double *recs = rec;
    if (recs) memset(recs, 0, sizeof(double) * (size_t)nHyp * XO_BWD_REC);

    /* 1. sampleHypotheses + soft-inlier scores (same sampler as the forward pass, keyed by randomSeed) */
#pragma omp parallel for schedule(dynamic, 1)
    for (int h = 0; h < nHyp; ++h) {
        int c4[4];
        xo_sample_hyp(&co, &cam, imageKey, (uint32_t)h, maxTries, &init[h], c4);
        for (int j = 0; j < 4; ++j) cells[4 * h + j] = c4[j];
        scores[h] = xo_score(&co, &init[h], &cam);
    }

    /* 2. softMax (dsacstar_util.h:684-704) */
    {
        double maxScore = 0.0, sum = 0.0;
        for (int i = 0; i < nHyp; ++i) if (i == 0 || scores[i] > maxScore) maxScore = scores[i];
        for (int i = 0; i < nHyp; ++i) { probs[i] = det_exp(scores[i] - maxScore); sum += probs[i]; }
        for (int i = 0; i < nHyp; ++i) probs[i] /= sum;
    }

    /* 3. refinement of every hypothesis that matters + 4. losses + path I per-hypothesis quantities */
#pragma omp parallel for schedule(dynamic, 1)
    for (int h = 0; h < nHyp; ++h) {
        ref[h] = init[h];
        int active = !(probs[h] < XLM_PROB_THRESH);
        double dLossH[6] = { 0, 0, 0, 0, 0, 0 }, maxJR = 0.0, rv[3] = { 0, 0, 0 };
        if (active) xo_refine(&co, &cam, &ref[h], inlAcc + (size_t)h * N, &nAcc[h], NULL, NULL);
        losses[h] = pose_loss(&ref[h], &gt, (double)wRot, (double)wTrans, (double)softClamp);
        if (active) {
            double r0[3];
            log_so3(init[h].R, r0);
            rodrigues_jac(r0, dRinit + (size_t)h * 27);
            log_so3(ref[h].R, rv);
            rodrigues_jac(rv, dRref + (size_t)h * 27);
            dloss(&ref[h], dRref + (size_t)h * 27, &gt, (double)wRot, (double)wTrans, (double)softClamp, dLossH);
            if (nAcc[h] >= 4) {
                /* J^T J over the accepted inliers, canonical reduction */
                xo_vec28 *part = (xo_vec28 *)malloc(sizeof(xo_vec28) * XO_T);
                const unsigned char *ia = inlAcc + (size_t)h * N;
                for (int tdx = 0; tdx < XO_T; ++tdx) {
                    double a[28];
                    for (int k = 0; k < 28; ++k) a[k] = 0.0;
                    for (int i = tdx; i < N; i += XO_T) {
                        if (!ia[i]) continue;
                        int y = i / Wo, x = i - y * Wo;
                        double X[3], J6[6];
                        xo_fetch(&co, x, y, X);
                        resid_row(&ref[h], dRref + (size_t)h * 27, X[0], X[1], X[2], cell_px(&cam, x), cell_px(&cam, y),
                                  &cam, J6);
                        int k = 0;
                        for (int r = 0; r < 6; ++r)
                            for (int c = r; c < 6; ++c) a[k++] += J6[r] * J6[c];
                    }
                    for (int k = 0; k < 28; ++k) part[tdx].v[k] = a[k];
                }
                double ne[28], A[36], Ainv[36];
                block_sum(part[0].v, 28, ne);
                free(part);
                int k = 0;
                for (int r = 0; r < 6; ++r)
                    for (int c = r; c < 6; ++c) { A[6 * r + c] = ne[k]; A[6 * c + r] = ne[k]; ++k; }
                pinv6(A, Ainv);
                /* jacobeanR = -(JtJ)^-1 J^T: clamp if any entry exceeds 10 (dsacstar.cpp:408-412) */
                for (int i = 0; i < N; ++i) {
                    if (!ia[i]) continue;
                    int y = i / Wo, x = i - y * Wo;
                    double X[3], J6[6];
                    xo_fetch(&co, x, y, X);
                    resid_row(&ref[h], dRref + (size_t)h * 27, X[0], X[1], X[2], cell_px(&cam, x), cell_px(&cam, y),
                              &cam, J6);
                    for (int r = 0; r < 6; ++r) {
                        double u = 0.0;
                        for (int c = 0; c < 6; ++c) u += Ainv[6 * r + c] * J6[c];
                        u = fabs(u);
                        if (u > maxJR) maxJR = u;
                    }
                }
                clampI[h] = (maxJR > 10.0) ? 1 : 0;
                for (int r = 0; r < 6; ++r) {
                    double v = 0.0;
                    for (int c = 0; c < 6; ++c) v += Ainv[6 * r + c] * dLossH[c];
                    wv[(size_t)h * 6 + r] = v;
                }
            }
        }
        if (recs) {
            double *q = recs + (size_t)h * XO_BWD_REC;
            q[0] = probs[h]; q[1] = losses[h]; q[2] = (double)active; q[3] = (double)nAcc[h]; q[4] = (double)clampI[h];
            pose_store12(&ref[h], q + 6);
            for (int i = 0; i < 6; ++i) { q[18 + i] = dLossH[i]; q[24 + i] = wv[(size_t)h * 6 + i]; }
            q[42] = maxJR;
            for (int i = 0; i < 3; ++i) q[50 + i] = rv[i];
        }
    }

    /* 5. expected loss; gradient of the soft-max selection (dsacstar_derivative.h:345-356) */
    double expected = 0.0;
    for (int h = 0; h < nHyp; ++h) expected += probs[h] * losses[h];
    *outLoss = expected;
    for (int i = 0; i < nHyp; ++i) {
        if (probs[i] < XLM_PROB_THRESH) continue;
        double g = probs[i] * losses[i];
        for (int j = 0; j < nHyp; ++j) g -= probs[i] * probs[j] * losses[j];
        sog[i] = g;
    }

    /* 6. path II per-hypothesis quantities: g6 = sum_c dRepro(c) J_init(c), dPNP, support-point gradients */
    const float beta = 5.0f / thr;
    const float facf = alpha / (float)Wo / (float)Ho;
#pragma omp parallel for schedule(dynamic, 1)
    for (int h = 0; h < nHyp; ++h) {
        if (probs[h] < XLM_PROB_THRESH) continue;
        xo_vec28 *part = (xo_vec28 *)malloc(sizeof(xo_vec28) * XO_T);
        for (int tdx = 0; tdx < XO_T; ++tdx) {
            double a[28];
            for (int k = 0; k < 28; ++k) a[k] = 0.0;
            for (int i = tdx; i < N; i += XO_T) {
                int y = i / Wo, x = i - y * Wo;
                double X[3], J6[6];
                xo_fetch(&co, x, y, X);
                float px = cell_px(&cam, x), py = cell_px(&cam, y);
                double st = soft_inlier_st(cell_err(&init[h], X[0], X[1], X[2], y, x, &cam), thr, beta);
                double dRep = -st * (1.0 - st) * (double)beta * sog[h];
                dRep *= (double)facf;
                resid_row(&init[h], dRinit + (size_t)h * 27, X[0], X[1], X[2], px, py, &cam, J6);
                for (int k = 0; k < 6; ++k) a[k] += dRep * J6[k];
            }
            for (int k = 0; k < 28; ++k) part[tdx].v[k] = a[k];
        }
        double g28[28];
        block_sum(part[0].v, 28, g28);
        free(part);
        float obj[4][3];
        double uv[4][2];
        for (int j = 0; j < 4; ++j) {
            int cidx = cells[4 * h + j];
            int y = cidx / Wo, x = cidx - y * Wo;
            const float *p = co.base + (int64_t)y * co.sy + (int64_t)x * co.sx;
            obj[j][0] = p[0]; obj[j][1] = p[co.sc]; obj[j][2] = p[2 * co.sc];
            uv[j][0] = (double)cell_px(&cam, x);
            uv[j][1] = (double)cell_px(&cam, y);
        }
        double J[72], maxH = 0.0;
        xo_dpnp(obj, uv, &cam, J);
        for (int k = 0; k < 72; ++k) { double v = fabs(J[k]); if (v > maxH) maxH = v; }
        if (maxH > 10.0) for (int k = 0; k < 72; ++k) J[k] = 0.0;      /* dsacstar_derivative.h:288 */
        for (int c = 0; c < 12; ++c) {
            double v = 0.0;
            for (int r = 0; r < 6; ++r) v += g28[r] * J[r * 12 + c];
            spg[(size_t)h * 12 + c] = v;
        }
        if (recs) {
            double *q = recs + (size_t)h * XO_BWD_REC;
            q[5] = sog[h]; q[43] = maxH;
            for (int c = 0; c < 12; ++c) q[30 + c] = spg[(size_t)h * 12 + c];
            for (int k = 0; k < 6; ++k) q[44 + k] = g28[k];
        }
    }

    /* 7. assemble: per cell, hypotheses in ascending order, float accumulation like the reference's tensor += */
#pragma omp parallel for schedule(static)
    for (int i = 0; i < N; ++i) {
        int y = i / Wo, x = i - y * Wo;
        double X[3];
        xo_fetch(&co, x, y, X);
        float px = cell_px(&cam, x), py = cell_px(&cam, y);
        float *g = grad + (int64_t)y * gsy + (int64_t)x * gsx;
        float acc[3] = { g[0], g[gsc], g[2 * gsc] };
        for (int h = 0; h < nHyp; ++h) {
            if (probs[h] < XLM_PROB_THRESH) continue;
            double gI[3] = { 0.0, 0.0, 0.0 };
            if (nAcc[h] >= 4 && !clampI[h] && inlAcc[(size_t)h * N + i]) {
                double J6[6], dNdO[3];
                resid_row(&ref[h], dRref + (size_t)h * 27, X[0], X[1], X[2], px, py, &cam, J6);
                double s = 0.0;
                for (int k = 0; k < 6; ++k) s += J6[k] * wv[(size_t)h * 6 + k];
                s = -s;
                dproject_dobj(&ref[h], X[0], X[1], X[2], px, py, &cam, dNdO);
                for (int k = 0; k < 3; ++k) gI[k] = s * dNdO[k];
            }
            double st = soft_inlier_st(cell_err(&init[h], X[0], X[1], X[2], y, x, &cam), thr, beta);
            double dRep = -st * (1.0 - st) * (double)beta * sog[h];
            dRep *= (double)facf;
            double dPdO[3];
            dproject_dobj(&init[h], X[0], X[1], X[2], px, py, &cam, dPdO);
            double jac[3] = { dPdO[0] * dRep, dPdO[1] * dRep, dPdO[2] * dRep };
            for (int j = 0; j < 4; ++j)
                if (cells[4 * h + j] == i)
                    for (int k = 0; k < 3; ++k) jac[k] += spg[(size_t)h * 12 + 3 * j + k];
            for (int k = 0; k < 3; ++k)
                acc[k] = (float)((double)acc[k] + (probs[h] * gI[k] + jac[k]));
        }
        g[0] = acc[0]; g[gsc] = acc[1]; g[2 * gsc] = acc[2];
    }

    free(init); free(ref); free(scores); free(probs); free(losses); free(sog); free(cells); free(inlAcc); free(nAcc);
    free(dRinit); free(dRref); free(wv); free(spg); free(clampI);
    return 0;
}

/* --- unit-test hooks: thin calls into xl_dsac_math.h --- */
double xo_test_atan2(double y, double x) { return det_atan2(y, x); }
void xo_test_log_so3(const double *R9, double *r3) { log_so3(R9, r3); }
void xo_test_rodrigues_jac(const double *r3, double *dR27) { rodrigues_jac(r3, dR27); }
void xo_test_pinv6(const double *A36, double *Ainv36) { pinv6(A36, Ainv36); }
double xo_test_resid_row(const double *Rt12, const double *r3, const double *X3, float px, float py,
                         double f, double cx, double cy, float maxReproj, double *J6)
{
    const Cam cam = xo_test_cam(f, cx, cy, maxReproj);
    Pose p;
    double dR[27];
    pose_load12(Rt12, &p);
    rodrigues_jac(r3, dR);
    return resid_row(&p, dR, X3[0], X3[1], X3[2], px, py, &cam, J6);
}
void xo_test_dproject_dobj(const double *Rt12, const double *X3, float px, float py, double f, double cx, double cy,
                           float maxReproj, double *out3)
{
    const Cam cam = xo_test_cam(f, cx, cy, maxReproj);
    Pose p;
    pose_load12(Rt12, &p);
    dproject_dobj(&p, X3[0], X3[1], X3[2], px, py, &cam, out3);
}
double xo_test_pose_loss(const double *Rt12, const float *gt16, double wRot, double wTrans, double cut)
{
    Pose p;
    Gt g;
    pose_load12(Rt12, &p);
    gt_from_pose16(gt16, &g);
    return pose_loss(&p, &g, wRot, wTrans, cut);
}
void xo_test_dloss(const double *Rt12, const double *r3, const float *gt16, double wRot, double wTrans, double cut, double *jac6)
{
    Pose p;
    Gt g;
    double dR[27];
    pose_load12(Rt12, &p);
    gt_from_pose16(gt16, &g);
    rodrigues_jac(r3, dR);
    dloss(&p, dR, &g, wRot, wTrans, cut, jac6);
}
void xo_test_dpnp(const float *obj12, const double *uv8, double f, double cx, double cy, double *J72)
{
    const Cam cam = xo_test_cam(f, cx, cy, 0.0f);
    float o[4][3];
    double uv[4][2];
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 3; ++j) o[i][j] = obj12[3 * i + j];
        uv[i][0] = uv8[2 * i]; uv[i][1] = uv8[2 * i + 1];
    }
    xo_dpnp(o, uv, &cam, J72);
}
