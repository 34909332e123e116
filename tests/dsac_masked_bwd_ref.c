/*
 * tests/dsac_masked_bwd_ref.c — CPU restatement of the masked RGB backward pass (xl_dsac_backward_rgb_masked_batch,
 * crossloc_amd/csrc/xl_dsac.hip: xl_dsac_forward_kernel<1, true> and the MASKED instantiations of the four backward kernels).
 *
 * TEST INFRASTRUCTURE ONLY.  It includes tests/dsac_masked_ref.c for the masked sampler, score, normal equations and LM state
 * machine (static there), and with them the product's xl_dsac_math.h and xl_dsac_reduce.h.  What it restates serially is the
 * backward pass around them, step by step in the order of oracle/dsac_bwd_oracle.c (with which it shares no code, only the
 * product's headers) and with that file's reduction orders: the soft-max in ascending order, sums over cells as 256 thread-strided
 * partials and the canonical block sum, the expected loss and the soft-max gradient in ascending order, dPNP with the reference's
 * += eps / -= 2 eps / += eps sequence carried from column to column, the gradient per cell with the hypotheses in ascending
 * order and float accumulation.  The mask enters where include/crossloc_dsac.h says: the masked forward's hypotheses and scores;
 * inliers are usable cells; path II sums usable cells; a hypothesis that carries a masked-out cell has a zero dPNP and that cell
 * is not read; a masked-out cell's gradient is not touched; fewer than four usable cells make the image dead.  A masked-out
 * cell's coordinates are never read here, so identity B holds in this file by construction; tests/test_dsac_masked_bwd_cpu.py
 * ties the file to the pinned oracle through identity A (all-ones mask == oracle.backward_rgb, bit for bit).
 *
 * With -DXMB_MAIN the file is a program of its own (for the sanitizer run): see main() at the end.
 */
#include "dsac_masked_ref.c"

#define XMB_REC 64
/* the per-hypothesis record: the first 53 doubles of XL_DSAC_BWD_REC (layout: include/crossloc_dsac.h) */

/* refine_pose<true>: the refinement loop of xm_forward_rgb_masked, keeping the inlier map of the last successful re-fit */
static void xmb_refine(const xm_image *im, const Cam *cam, Pose *pose, unsigned char *inlAcc, unsigned *nAcc)
{
    const int N = cam->N;
    unsigned char *inl = (unsigned char *)malloc((size_t)N);
    unsigned best = 4;
    int evals = 0;
    memset(inlAcc, 0, (size_t)N);
    *nAcc = 0;
    for (int step = 0; step < XL_DSAC_MAX_REF_STEPS; ++step) {
        unsigned cnt = 0;
        for (int i = 0; i < N; ++i) {
            inl[i] = (im->mask[i] && xm_cell_err(im, pose, i, cam) < cam->thr) ? 1 : 0;
            cnt += inl[i];
        }
        if (cnt <= best) break;
        best = cnt;
        Pose upd = *pose;
        if (!xm_lm_pnp(im, inl, cam, &upd, &evals)) break;
        *pose = upd;
        *nAcc = cnt;
        memcpy(inlAcc, inl, (size_t)N);
    }
    free(inl);
}

/* dPNP by central differences (dsacstar_derivative.h:131-190): float points, float eps, the perturbation sequence carried
 * from column to column; a failed solve or a NaN entry zeroes the whole Jacobian; columns 9..11 stay zero */
static void xmb_dpnp(const float obj[4][3], const double uv[4][2], const Cam *cam, double J[72])
{
    const float eps = 0.001f;
    float pts[4][3];
    memcpy(pts, obj, sizeof(pts));
    for (int k = 0; k < 72; ++k) J[k] = 0.0;
    for (int col = 0; col < 9; ++col) {
        float *v = &pts[col / 3][col % 3];
        Pose sol[2];
        int ok = 1;
        for (int back = 0; back < 2 && ok; ++back) {
            V3 P[4];
            *v += back ? -2 * eps : eps;
            for (int a = 0; a < 4; ++a) { P[a].x = (double)pts[a][0]; P[a].y = (double)pts[a][1]; P[a].z = (double)pts[a][2]; }
            ok = p3p(P[0], P[1], P[2], P[3], uv, cam, &sol[back]);
        }
        int bad = !ok;
        if (ok) {
            *v += eps;
            double rf[3], rb[3];
            log_so3(sol[0].R, rf);
            log_so3(sol[1].R, rb);
            const double den = (double)(2 * eps);
            for (int k = 0; k < 3; ++k) {
                const double a = (rf[k] - rb[k]) / den, b = (sol[0].t[k] - sol[1].t[k]) / den;
                J[k * 12 + col] = a;
                J[(3 + k) * 12 + col] = b;
                if (!(a == a) || !(b == b)) bad = 1;
            }
        }
        if (bad) { for (int k = 0; k < 72; ++k) J[k] = 0.0; return; }
    }
}

/*
 * One image.  coords [3,Ho,Wo] float32 with element strides (sc, sy, sx); mask [Ho*Wo] uint8, nonzero = usable; grad like coords
 * with strides (gsc, gsy, gsx), accumulated.  Outputs: outLoss, status; nullable rec [nHyp*XMB_REC], tries [nHyp] (the masked
 * forward's: negative = exhausted) and cells [nHyp*4].
 */
int xmb_backward_rgb_masked(const float *coords, int64_t sc, int64_t sy, int64_t sx, int Ho, int Wo, const uint8_t *mask,
                            float *grad, int64_t gsc, int64_t gsy, int64_t gsx, const float *gtPose16, int nHyp, float thr,
                            float focal, float ppx, float ppy, float wRot, float wTrans, float softClamp, float alpha,
                            float maxReproj, int sub, uint64_t seed, uint64_t image, uint32_t maxTries,
                            double *outLoss, int32_t *status, double *rec, int32_t *tries, int32_t *cellsOut)
{
    if (!coords || !mask || !grad || !gtPose16 || !outLoss || nHyp <= 0 || Ho <= 0 || Wo <= 0 || sub <= 0 || maxTries == 0) return -1;
    const int N = Ho * Wo;
    if (N > XM_MAX_CELLS) return -2;
    const xm_image im = { coords, sc, sy, sx, mask, Ho, Wo };
    const Cam cam = cam_make(Ho, Wo, thr, focal, ppx, ppy, alpha, maxReproj, sub);
    const uint64_t imageKey = image_key(seed, image);
    if (rec) memset(rec, 0, sizeof(double) * (size_t)nHyp * XMB_REC);

    int nUsable = 0;
    for (int i = 0; i < N; ++i) nUsable += mask[i] ? 1 : 0;
    if (nUsable < 4) {
        /* dead image: nothing is sampled, the gradient is not touched */
        *outLoss = 0.0;
        if (status) *status = 1;
        for (int h = 0; h < nHyp; ++h) {
            if (tries) tries[h] = 0;
            if (cellsOut) for (int j = 0; j < 4; ++j) cellsOut[4 * h + j] = -1;
        }
        return 0;
    }
    if (status) *status = 0;
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
    double *part = (double *)malloc(sizeof(double) * 28 * XM_T);

    /* 1. the masked forward's hypotheses and scores (exhausted: the last try's result, the identity where the mask rejected it) */
    for (int h = 0; h < nHyp; ++h) {
        int c4[4] = { 0, 0, 0, 0 };
        int triesUsed = -(int)maxTries;
        for (uint32_t t = 0; t < maxTries; ++t)
            if (xm_sample_try(&im, &cam, imageKey, (uint32_t)h, t, &init[h], c4)) { triesUsed = (int)t + 1; break; }
        for (int j = 0; j < 4; ++j) cells[4 * h + j] = c4[j];
        if (tries) tries[h] = triesUsed;
        if (cellsOut) for (int j = 0; j < 4; ++j) cellsOut[4 * h + j] = c4[j];
        scores[h] = xm_score(&im, &init[h], &cam);
    }

    /* 2. softMax (dsacstar_util.h:684-704) */
    {
        double maxScore = 0.0, sum = 0.0;
        for (int i = 0; i < nHyp; ++i) if (i == 0 || scores[i] > maxScore) maxScore = scores[i];
        for (int i = 0; i < nHyp; ++i) { probs[i] = det_exp(scores[i] - maxScore); sum += probs[i]; }
        for (int i = 0; i < nHyp; ++i) probs[i] /= sum;
    }

    /* 3. refinement over the usable cells of every hypothesis that matters, losses, path I per-hypothesis quantities */
    for (int h = 0; h < nHyp; ++h) {
        ref[h] = init[h];
        const int active = !(probs[h] < XLM_PROB_THRESH);
        double dLossH[6] = { 0, 0, 0, 0, 0, 0 }, maxJR = 0.0, rv[3] = { 0, 0, 0 };
        const unsigned char *ia = inlAcc + (size_t)h * N;
        if (active) xmb_refine(&im, &cam, &ref[h], inlAcc + (size_t)h * N, &nAcc[h]);
        losses[h] = pose_loss(&ref[h], &gt, (double)wRot, (double)wTrans, (double)softClamp);
        if (active) {
            double r0[3];
            double *dRr = dRref + (size_t)h * 27;
            log_so3(init[h].R, r0);
            rodrigues_jac(r0, dRinit + (size_t)h * 27);
            log_so3(ref[h].R, rv);
            rodrigues_jac(rv, dRr);
            dloss(&ref[h], dRr, &gt, (double)wRot, (double)wTrans, (double)softClamp, dLossH);
            if (nAcc[h] >= 4) {
                /* J^T J over the accepted inliers (usable by construction), canonical reduction */
                for (int tdx = 0; tdx < XM_T; ++tdx) {
                    double a[28];
                    for (int k = 0; k < 28; ++k) a[k] = 0.0;
                    for (int i = tdx; i < N; i += XM_T) {
                        if (!ia[i]) continue;
                        const int y = i / Wo, x = i - y * Wo;
                        double X[3], J6[6];
                        xm_fetch(&im, i, X);
                        resid_row(&ref[h], dRr, X[0], X[1], X[2], cell_px(&cam, x), cell_px(&cam, y), &cam, J6);
                        int k = 0;
                        for (int r = 0; r < 6; ++r)
                            for (int c = r; c < 6; ++c) a[k++] += J6[r] * J6[c];
                    }
                    for (int k = 0; k < 28; ++k) part[tdx * 28 + k] = a[k];
                }
                double ne[28], A[36], Ainv[36];
                block_sum(part, 28, ne);
                int k = 0;
                for (int r = 0; r < 6; ++r)
                    for (int c = r; c < 6; ++c) { A[6 * r + c] = ne[k]; A[6 * c + r] = ne[k]; ++k; }
                pinv6(A, Ainv);
                /* jacobeanR = -(JtJ)^-1 J^T: clamp if any entry exceeds 10 (dsacstar.cpp:408-412); a maximum, order-free */
                for (int i = 0; i < N; ++i) {
                    if (!ia[i]) continue;
                    const int y = i / Wo, x = i - y * Wo;
                    double X[3], J6[6];
                    xm_fetch(&im, i, X);
                    resid_row(&ref[h], dRr, X[0], X[1], X[2], cell_px(&cam, x), cell_px(&cam, y), &cam, J6);
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
        if (rec) {
            double *q = rec + (size_t)h * XMB_REC;
            q[0] = probs[h]; q[1] = losses[h]; q[2] = (double)active; q[3] = (double)nAcc[h]; q[4] = (double)clampI[h];
            pose_store12(&ref[h], q + 6);
            for (int i = 0; i < 6; ++i) { q[18 + i] = dLossH[i]; q[24 + i] = wv[(size_t)h * 6 + i]; }
            q[42] = maxJR;
            for (int i = 0; i < 3; ++i) q[50 + i] = rv[i];
        }
    }

    /* 4. expected loss; gradient of the soft-max selection (dsacstar_derivative.h:345-356) */
    double expected = 0.0;
    for (int h = 0; h < nHyp; ++h) expected += probs[h] * losses[h];
    *outLoss = expected;
    for (int i = 0; i < nHyp; ++i) {
        if (probs[i] < XLM_PROB_THRESH) continue;
        double g = probs[i] * losses[i];
        for (int j = 0; j < nHyp; ++j) g -= probs[i] * probs[j] * losses[j];
        sog[i] = g;
    }

    /* 5. path II per hypothesis: g6 = sum over the usable cells of dRepro(c) J_init(c), dPNP, support-point gradients */
    const float beta = 5.0f / thr;
    const float facf = alpha / (float)Wo / (float)Ho;
    for (int h = 0; h < nHyp; ++h) {
        if (probs[h] < XLM_PROB_THRESH) continue;
        for (int tdx = 0; tdx < XM_T; ++tdx) {
            double a[28];
            for (int k = 0; k < 28; ++k) a[k] = 0.0;
            for (int i = tdx; i < N; i += XM_T) {
                if (!mask[i]) continue;
                const int y = i / Wo, x = i - y * Wo;
                double X[3], J6[6];
                xm_fetch(&im, i, X);
                const float px = cell_px(&cam, x), py = cell_px(&cam, y);
                const double st = soft_inlier_st(cell_err(&init[h], X[0], X[1], X[2], y, x, &cam), thr, beta);
                double dRep = -st * (1.0 - st) * (double)beta * sog[h];
                dRep *= (double)facf;
                resid_row(&init[h], dRinit + (size_t)h * 27, X[0], X[1], X[2], px, py, &cam, J6);
                for (int k = 0; k < 6; ++k) a[k] += dRep * J6[k];
            }
            for (int k = 0; k < 28; ++k) part[tdx * 28 + k] = a[k];
        }
        double g28[28], J[72], maxH = 0.0;
        block_sum(part, 28, g28);
        int carriesMasked = 0;
        for (int j = 0; j < 4; ++j) if (!mask[cells[4 * h + j]]) carriesMasked = 1;
        if (carriesMasked) {
            /* tries exhausted on a mask-rejected try: no cell is read, the zero Jacobian of a failed solve */
            for (int k = 0; k < 72; ++k) J[k] = 0.0;
        } else {
            float obj[4][3];
            double uv[4][2];
            for (int j = 0; j < 4; ++j) {
                const int cidx = cells[4 * h + j];
                const int y = cidx / Wo, x = cidx - y * Wo;
                const float *p = coords + (int64_t)y * sy + (int64_t)x * sx;
                obj[j][0] = p[0]; obj[j][1] = p[sc]; obj[j][2] = p[2 * sc];
                uv[j][0] = (double)cell_px(&cam, x);
                uv[j][1] = (double)cell_px(&cam, y);
            }
            xmb_dpnp(obj, uv, &cam, J);
        }
        for (int k = 0; k < 72; ++k) { const double v = fabs(J[k]); if (v > maxH) maxH = v; }
        if (maxH > 10.0) for (int k = 0; k < 72; ++k) J[k] = 0.0;      /* dsacstar_derivative.h:288 */
        for (int c = 0; c < 12; ++c) {
            double v = 0.0;
            for (int r = 0; r < 6; ++r) v += g28[r] * J[r * 12 + c];
            spg[(size_t)h * 12 + c] = v;
        }
        if (rec) {
            double *q = rec + (size_t)h * XMB_REC;
            q[5] = sog[h]; q[43] = maxH;
            for (int c = 0; c < 12; ++c) q[30 + c] = spg[(size_t)h * 12 + c];
            for (int k = 0; k < 6; ++k) q[44 + k] = g28[k];
        }
    }

    /* 6. assemble: per usable cell, hypotheses in ascending order, float accumulation like the reference's tensor += */
    for (int i = 0; i < N; ++i) {
        if (!mask[i]) continue;                                        /* neither read nor written */
        const int y = i / Wo, x = i - y * Wo;
        double X[3];
        xm_fetch(&im, i, X);
        const float px = cell_px(&cam, x), py = cell_px(&cam, y);
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
            const double st = soft_inlier_st(cell_err(&init[h], X[0], X[1], X[2], y, x, &cam), thr, beta);
            double dRep = -st * (1.0 - st) * (double)beta * sog[h];
            dRep *= (double)facf;
            double dPdO[3];
            dproject_dobj(&init[h], X[0], X[1], X[2], px, py, &cam, dPdO);
            double jac[3] = { dPdO[0] * dRep, dPdO[1] * dRep, dPdO[2] * dRep };
            for (int j = 0; j < 4; ++j)
                if (cells[4 * h + j] == i)
                    for (int k = 0; k < 3; ++k) jac[k] += spg[(size_t)h * 12 + 3 * j + k];
            for (int k = 0; k < 3; ++k) acc[k] = (float)((double)acc[k] + (probs[h] * gI[k] + jac[k]));
        }
        g[0] = acc[0]; g[gsc] = acc[1]; g[2 * gsc] = acc[2];
    }

    free(part);
    free(init); free(ref); free(scores); free(probs); free(losses); free(sog); free(cells); free(inlAcc); free(nAcc);
    free(dRinit); free(dRref); free(wv); free(spg); free(clampI);
    return 0;
}

#ifdef XMB_MAIN
/* dsac_masked_bwd_ref FILE Ho Wo nHyp thr maxTries: FILE holds float32 coords [3,Ho,Wo] then the uint8 mask [Ho,Wo].  Runs the
 * image against the identity as ground truth with every optional output, then with none, then with an all-zero mask (the dead
 * path); prints the results. */
int main(int argc, char **argv)
{
    if (argc != 7) { fprintf(stderr, "usage: %s FILE Ho Wo nHyp thr maxTries\n", argv[0]); return 2; }
    const int Ho = atoi(argv[2]), Wo = atoi(argv[3]), nHyp = atoi(argv[4]);
    const float thr = (float)atof(argv[5]);
    const long maxTries = atol(argv[6]);
    if (Ho <= 0 || Wo <= 0 || nHyp <= 0 || maxTries <= 0 || Ho * Wo > XM_MAX_CELLS) return 2;
    const size_t N = (size_t)Ho * (size_t)Wo;
    float *buf = (float *)malloc(sizeof(float) * 3 * N), *grad = (float *)calloc(3 * N, sizeof(float));
    uint8_t *mask = (uint8_t *)malloc(N);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(buf, sizeof(float), 3 * N, f) != 3 * N || fread(mask, 1, N, f) != N) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    fclose(f);
    float gt[16];
    xm_identity16(gt);
    double *rec = (double *)malloc(sizeof(double) * XMB_REC * (size_t)nHyp);
    int32_t *tries = (int32_t *)malloc(sizeof(int32_t) * (size_t)nHyp), *cells = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)nHyp);
    double loss = -1.0, loss2 = -1.0, loss3 = -1.0;
    int32_t status = -1, status2 = -1, status3 = -1;
    const int st = xmb_backward_rgb_masked(buf, (int64_t)N, Wo, 1, Ho, Wo, mask, grad, (int64_t)N, Wo, 1, gt, nHyp, thr, 480.0f,
                                           Wo * 4.0f, Ho * 4.0f, 1.0f, 100.0f, 100.0f, 100.0f, 100.0f, 8, 1305, 0,
                                           (uint32_t)maxTries, &loss, &status, rec, tries, cells);
    double gmax = 0.0;
    for (size_t i = 0; i < 3 * N; ++i) if (fabs((double)grad[i]) > gmax) gmax = fabs((double)grad[i]);
    printf("masked: rc %d status %d loss %.6f max |grad| %.6g prob[0] %.6f\n", st, (int)status, loss, gmax, rec[0]);
    const int st2 = xmb_backward_rgb_masked(buf, (int64_t)N, Wo, 1, Ho, Wo, mask, grad, (int64_t)N, Wo, 1, gt, nHyp, thr, 480.0f,
                                            Wo * 4.0f, Ho * 4.0f, 1.0f, 100.0f, 100.0f, 100.0f, 100.0f, 8, 1305, 0,
                                            (uint32_t)maxTries, &loss2, NULL, NULL, NULL, NULL);
    memset(mask, 0, N);
    const int st3 = xmb_backward_rgb_masked(buf, (int64_t)N, Wo, 1, Ho, Wo, mask, grad, (int64_t)N, Wo, 1, gt, nHyp, thr, 480.0f,
                                            Wo * 4.0f, Ho * 4.0f, 1.0f, 100.0f, 100.0f, 100.0f, 100.0f, 8, 1305, 0,
                                            (uint32_t)maxTries, &loss3, &status3, rec, tries, cells);
    printf("no outputs: rc %d loss %.6f; dead: rc %d status %d loss %.6f\n", st2, loss2, st3, (int)status3, loss3);
    free(cells); free(tries); free(rec); free(mask); free(grad); free(buf);
    (void)status2;
    return (st == 0 && st2 == 0 && st3 == 0 && status == 0 && status3 == 1 && loss == loss2 && loss3 == 0.0) ? 0 : 1;
}
#endif
