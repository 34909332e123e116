/*
 * tests/dsac_compact_ref.c — CPU restatement of the masked RGB DSAC* solver and its backward pass under the compact sampler
 * (xl_dsac_forward_rgb_masked_sampled_batch / xl_dsac_backward_rgb_masked_sampled_batch with XL_DSAC_SAMPLER_COMPACT,
 * crossloc_amd/csrc/xl_dsac.hip: xl_dsac_forward_kernel<PHASE, kMaskCompact> and the MASKED instantiations of the four backward
 * kernels).
 *
 * TEST INFRASTRUCTURE ONLY.  It includes tests/dsac_masked_bwd_ref.c (and through it tests/dsac_masked_ref.c) for what the two
 * samplers share and those files keep static: the score over the usable cells, the normal equations, the LM state machine,
 * the refinement loop and dPNP - and with them the product's xl_dsac_math.h and xl_dsac_reduce.h.  The bit plane, the rank plane
 * and the selection are the product's statements in xl_dsac_math.h (mask_rank_plane, mask_select, compact_try_cells); what is
 * restated here serially is the kernels' orchestration around them: the mask packed into words, a try that draws four ranks
 * and is never rejected by the mask, the tries of a hypothesis in ascending order, and then the forward and the backward pass
 * step by step as the two included files state them for the reject sampler, with one difference: every hypothesis carries
 * four usable cells, so the backward pass never skips dPNP and an exhausted hypothesis is treated as the unmasked pass treats
 * one (its last try's P3P result, or the identity where that P3P failed).  A masked-out cell's coordinates are never read here.
 * tests/test_dsac_compact_cpu.py checks the selection against numpy and the drawn cells against a restatement of the generator in
 * Python integers, so the file is not its own yardstick.
 *
 * With -DXC_MAIN the file is a program of its own (for the sanitizer run): see main() at the end.
 */
#include "dsac_masked_bwd_ref.c"

#define XC_MAX_WORDS (XM_MAX_CELLS / 32)

/* the mask as the kernel stages it: bit i & 31 of word i >> 5 <-> cell i; then its rank plane.  Returns the number of words */
static int xc_planes(const uint8_t *mask, int N, uint32_t *words, uint32_t *rank)
{
    const int nWords = (N + 31) >> 5;
    for (int w = 0; w < nWords; ++w) words[w] = 0u;
    for (int i = 0; i < N; ++i) if (mask[i]) words[i >> 5] |= 1u << (i & 31);
    mask_rank_plane(words, nWords, rank);
    return nWords;
}

/* mask_select on its own: the cell of rank k among the usable cells of mask [N], or -1 when k is out of range */
int xc_mask_select(const uint8_t *mask, int N, int k)
{
    if (!mask || N <= 0 || N > XM_MAX_CELLS) return -1;
    uint32_t words[XC_MAX_WORDS], rank[XC_MAX_WORDS + 1];
    const int nWords = xc_planes(mask, N, words, rank);
    if (k < 0 || (uint32_t)k >= rank[nWords]) return -1;
    return mask_select(words, rank, nWords, k);
}

typedef struct { const uint32_t *words, *rank; int nWords; } xc_planes_t;

/* one try: four ranks among the usable cells; everything behind the cells is the masked solver's */
static int xc_sample_try(const xm_image *im, const xc_planes_t *pl, const Cam *cam, uint64_t imageKey, uint32_t hyp, uint32_t t,
                         Pose *pose, int cells[4])
{
    const uint64_t st = try_state(imageKey, hyp, t);
    V3 P[4];
    double uv[4][2];
    float px[4], py[4];
    compact_try_cells(st, pl->words, pl->rank, pl->nWords, cells);
    for (int j = 0; j < 4; ++j) {
        const int y = cells[j] / cam->Wo, x = cells[j] - y * cam->Wo;
        double X[3];
        px[j] = cell_px(cam, x);
        py[j] = cell_px(cam, y);
        uv[j][0] = (double)px[j]; uv[j][1] = (double)py[j];
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

/* the tries of hypothesis h in ascending order; exhausted: pose and cells are the last try's, -maxTries returned */
static int xc_hypothesis(const xm_image *im, const xc_planes_t *pl, const Cam *cam, uint64_t imageKey, int h, uint32_t maxTries,
                         Pose *pose, int c4[4])
{
    for (uint32_t t = 0; t < maxTries; ++t)
        if (xc_sample_try(im, pl, cam, imageKey, (uint32_t)h, t, pose, c4)) return (int)t + 1;
    return -(int)maxTries;
}

/*
 * One image, forward.  Arguments and outputs as xm_forward_rgb_masked (tests/dsac_masked_ref.c).
 */
int xc_forward_rgb_compact(const float *coords, int64_t sc, int64_t sy, int64_t sx, int Ho, int Wo, const uint8_t *mask,
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

    uint32_t words[XC_MAX_WORDS], rank[XC_MAX_WORDS + 1];
    const xc_planes_t pl = { words, rank, xc_planes(mask, N, words, rank) };
    if (rank[pl.nWords] < 4u)                              /* dead image: the reject restatement's path, nothing is sampled */
        return xm_forward_rgb_masked(coords, sc, sy, sx, Ho, Wo, mask, pose16, status, nHyp, thr, focal, ppx, ppy, alpha,
                                     maxReproj, sub, seed, image, maxTries, cells, tries, scores, dbg);

    /* ---- sample + score */
    int win = -1, anyNan = 0;
    double winScore = 0.0;
    Pose winPose, pose0;
    pose_identity(&winPose);
    pose_identity(&pose0);
    for (int h = 0; h < nHyp; ++h) {
        Pose pose;
        int c4[4] = { 0, 0, 0, 0 };
        const int triesUsed = xc_hypothesis(&im, &pl, &cam, imageKey, h, maxTries, &pose, c4);
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

/*
 * One image, backward.  Arguments and outputs as xmb_backward_rgb_masked (tests/dsac_masked_bwd_ref.c); steps 2 - 6 are that
 * file's, with dPNP computed for every hypothesis above the probability threshold (none carries a masked-out cell).
 */
int xc_backward_rgb_compact(const float *coords, int64_t sc, int64_t sy, int64_t sx, int Ho, int Wo, const uint8_t *mask,
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

    uint32_t words[XC_MAX_WORDS], rank[XC_MAX_WORDS + 1];
    const xc_planes_t pl = { words, rank, xc_planes(mask, N, words, rank) };
    if (rank[pl.nWords] < 4u)                              /* dead image: the reject restatement's path, nothing is sampled */
        return xmb_backward_rgb_masked(coords, sc, sy, sx, Ho, Wo, mask, grad, gsc, gsy, gsx, gtPose16, nHyp, thr, focal, ppx, ppy,
                                       wRot, wTrans, softClamp, alpha, maxReproj, sub, seed, image, maxTries, outLoss, status, rec,
                                       tries, cellsOut);
    if (rec) memset(rec, 0, sizeof(double) * (size_t)nHyp * XMB_REC);
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

    /* 1. the compact forward's hypotheses and scores (exhausted: the last try's result) */
    for (int h = 0; h < nHyp; ++h) {
        int c4[4] = { 0, 0, 0, 0 };
        const int triesUsed = xc_hypothesis(&im, &pl, &cam, imageKey, h, maxTries, &init[h], c4);
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
        {
            /* the four cells are usable, whether the hypothesis was accepted or ran out of tries */
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

#ifdef XC_MAIN
/* dsac_compact_ref FILE Ho Wo nHyp thr maxTries: FILE holds float32 coords [3,Ho,Wo] then the uint8 mask [Ho,Wo].  Selects
 * every rank of the mask and checks it against a walk over the bytes; runs the forward and the backward pass (identity as
 * ground truth) with every optional output, then with none, then with an all-zero mask (the dead path); prints the results. */
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

    int k = 0, selectOk = 1;
    for (size_t i = 0; i < N; ++i)
        if (mask[i]) { if (xc_mask_select(mask, (int)N, k) != (int)i) selectOk = 0; ++k; }
    if (xc_mask_select(mask, (int)N, k) != -1 || xc_mask_select(mask, (int)N, -1) != -1) selectOk = 0;
    printf("select: %d usable cells, %s\n", k, selectOk ? "ok" : "MISMATCH");

    int32_t *cells = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)nHyp), *tries = (int32_t *)malloc(sizeof(int32_t) * (size_t)nHyp);
    double *scores = (double *)malloc(sizeof(double) * (size_t)nHyp);
    double *rec = (double *)malloc(sizeof(double) * XMB_REC * (size_t)nHyp);
    double dbg[XM_DBG];
    float pose[16], gt[16];
    xm_identity16(gt);
    int32_t status = -1, status2 = -1, status3 = -1, bstatus = -1, bstatus3 = -1;
    double loss = -1.0, loss2 = -1.0, loss3 = -1.0;
    const int st = xc_forward_rgb_compact(buf, (int64_t)N, Wo, 1, Ho, Wo, mask, pose, &status, nHyp, thr, 480.0f, Wo * 4.0f, Ho * 4.0f,
                                          100.0f, 100.0f, 8, 1305, 0, (uint32_t)maxTries, cells, tries, scores, dbg);
    printf("compact: rc %d status %d winner %d rounds %d inliers %d centre %.6f %.6f %.6f\n", st, (int)status, (int)dbg[0], (int)dbg[1],
           (int)dbg[2], pose[3], pose[7], pose[11]);
    const int st2 = xc_forward_rgb_compact(buf, (int64_t)N, Wo, 1, Ho, Wo, mask, pose, &status2, nHyp, thr, 480.0f, Wo * 4.0f, Ho * 4.0f,
                                           100.0f, 100.0f, 8, 1305, 0, (uint32_t)maxTries, NULL, NULL, NULL, NULL);
    const int bt = xc_backward_rgb_compact(buf, (int64_t)N, Wo, 1, Ho, Wo, mask, grad, (int64_t)N, Wo, 1, gt, nHyp, thr, 480.0f,
                                           Wo * 4.0f, Ho * 4.0f, 1.0f, 100.0f, 100.0f, 100.0f, 100.0f, 8, 1305, 0,
                                           (uint32_t)maxTries, &loss, &bstatus, rec, tries, cells);
    double gmax = 0.0;
    for (size_t i = 0; i < 3 * N; ++i) if (fabs((double)grad[i]) > gmax) gmax = fabs((double)grad[i]);
    printf("backward: rc %d status %d loss %.6f max |grad| %.6g prob[0] %.6f\n", bt, (int)bstatus, loss, gmax, rec[0]);
    const int bt2 = xc_backward_rgb_compact(buf, (int64_t)N, Wo, 1, Ho, Wo, mask, grad, (int64_t)N, Wo, 1, gt, nHyp, thr, 480.0f,
                                            Wo * 4.0f, Ho * 4.0f, 1.0f, 100.0f, 100.0f, 100.0f, 100.0f, 8, 1305, 0,
                                            (uint32_t)maxTries, &loss2, NULL, NULL, NULL, NULL);
    memset(mask, 0, N);
    const int st3 = xc_forward_rgb_compact(buf, (int64_t)N, Wo, 1, Ho, Wo, mask, pose, &status3, nHyp, thr, 480.0f, Wo * 4.0f, Ho * 4.0f,
                                           100.0f, 100.0f, 8, 1305, 0, (uint32_t)maxTries, cells, tries, scores, dbg);
    const int bt3 = xc_backward_rgb_compact(buf, (int64_t)N, Wo, 1, Ho, Wo, mask, grad, (int64_t)N, Wo, 1, gt, nHyp, thr, 480.0f,
                                            Wo * 4.0f, Ho * 4.0f, 1.0f, 100.0f, 100.0f, 100.0f, 100.0f, 8, 1305, 0,
                                            (uint32_t)maxTries, &loss3, &bstatus3, rec, tries, cells);
    printf("no outputs: rc %d %d status %d loss %.6f; dead: rc %d %d status %d %d winner %d loss %.6f\n", st2, bt2, (int)status2, loss2,
           st3, bt3, (int)status3, (int)bstatus3, (int)dbg[0], loss3);
    free(rec); free(scores); free(tries); free(cells); free(mask); free(grad); free(buf);
    return (selectOk && st == 0 && st2 == 0 && st3 == 0 && bt == 0 && bt2 == 0 && bt3 == 0 && status == 0 && status2 == 0 &&
            status3 == 1 && bstatus == 0 && bstatus3 == 1 && loss == loss2 && loss3 == 0.0) ? 0 : 1;
}
#endif
