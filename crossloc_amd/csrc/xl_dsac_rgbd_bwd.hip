// xl_dsac_rgbd_bwd.hip — the RGB-D DSAC* backward pass on MI355X (gfx950): the DSAC* expectation of the pose loss over the
// hypothesis distribution and its gradient w.r.t. the scene coordinates, Kabsch hypotheses from camera coordinates (depth),
// batched.  Replaces dsacstar_rgbd_backward (dsacstar/dsacstar.cpp:631-885 of the reference project) behind
// xl_dsac_backward_rgbd_batch (include/crossloc_dsac.h: semantics, deviations and the record layout).  Five launches on the
// caller's stream, the sequence of the RGB backward in xl_dsac.hip; all of 256 threads (4 wavefronts):
//
//   K0 (S x B)        stage; wave w of split s samples and scores hypotheses (s * 4 + w) + 4 S i with the forward kernel's
//                     sampler and scoring walk (xl_dsac_rgbd_dev.h): every hypothesis' pose, score and drawn places, and the
//                     place of every cell in the valid list.  A hypothesis is one wave's work: nothing depends on S
//   K1 (nHyp x B)     soft-max probability; inactive (prob < 1e-3): loss of the unrefined pose, leave before staging.  Active:
//                     stage, the forward kernel's refinement loop, loss, and for path I the adjoint H of the last fit for
//                     (G_R, g_t) = d loss / d (R, t), v = R^T g_t / n, c_p, and the per-thread inlier masks
//   K2 (B)            expected loss and the gradient of the soft-max selection
//   K3 (nHyp x B)     inactive: leave before staging.  Stage; the twelve score sums over the valid cells under the unrefined pose
//                     (two block reductions); the minimal fit once more with its eigen-decomposition, the rotation Jacobian
//                     of the support points (path-II guard) and the 3 x 3 support-point gradients
//   K4 (N/256 x B)    per cell, hypotheses in ascending order, float accumulation: prob * path I + path II
//
// LDS of K0, K1, K3: the forward kernel's layout (26 bytes per cell behind Smem; rgbd_lds_view), 138 KiB at 60 x 90, one workgroup
// per CU.  The input record (RgbdIn, rgbd_input) is in xl_dsac_rgbd_dev.h, the order of the block sums in xl_dsac_reduce.h.
// What one lane computes on its own is in xl_dsac_rgbd_bwd_math.h; tests/dsac_rgbd_bwd_ref.c compiles the same header with gcc
// and restates this file's orchestration serially, and tests/test_dsac_rgbd_bwd_gpu.py compares every output bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>                    // memcpy in the host half of xl_dsac_math.h (bits_f64), as that header asks

#include "../../include/crossloc_dsac.h"
#include "xl_common.h"

namespace {

#include "xl_dsac_rgbd_dev.h"

constexpr int kRec = XL_DSAC_RGBD_BWD_REC;
static_assert(kRec == XLR_BWD_REC, "one record size");

struct RgbdBwdParams : RgbdIn {
    float *grad; int64_t gsb, gsc, gsy, gsx;
    const float *gt;
    double *hypPoses; double *scores; int32_t *places; int32_t *placeOf;     // K0 -> K1, K3, K4
    double *rec; unsigned long long *masks; double *outLoss;
    uint64_t seed, image0, imageStride;
    uint32_t maxTries;
    int nHyp, S;
    float thr, alpha, maxDist, wRot, wTrans, softClamp;
};

// K0 (grid S x B): sample and score
__global__ __launch_bounds__(kThreads)
void xl_dsac_rgbd_bwd_sample_kernel(RgbdBwdParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const Lds L = rgbd_lds_view(smem_raw, P.Npad);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = blockIdx.x, b = blockIdx.y;
    const int N = P.Ho * P.Wo;
    int cntSel = 0;
    const int nValid = rgbd_stage(P, b, L.S, L.sF, L.sCell, cntSel, tid, lane, wave, split == 0 ? P.placeOf + (int64_t)b * N : nullptr);
    const Cells ce{ L.sF, L.sF + P.Npad, L.sF + 2 * P.Npad, L.sF + 3 * P.Npad, L.sF + 4 * P.Npad, L.sF + 5 * P.Npad };
    const uint64_t imageKey = image_key(P.seed, P.image0 + (uint64_t)b * P.imageStride);
    const float thr = P.thr, maxDist = P.maxDist;
    const ScoreConst sc(thr, P.alpha, P.Ho, P.Wo);
    const double invalidTerm = sc.invalid_term(maxDist, thr);
    for (int h = split * kWaves + wave; h < P.nHyp; h += P.S * kWaves) {
        Pose pose;
        int k3[3];
        (void)rgbd_sample_hyp(ce, nValid, thr, imageKey, h, P.maxTries, lane, pose, k3);
        const double score = rgbd_score_hyp(ce, nValid, N, pose, maxDist, thr, sc, invalidTerm, lane);
        if (lane == 0) {
            const int64_t o = (int64_t)b * P.nHyp + h;
            pose_store12(&pose, P.hypPoses + o * 12);
            P.scores[o] = score;
#pragma unroll
            for (int j = 0; j < 3; ++j) P.places[o * 3 + j] = k3[j];
        }
    }
}

// K1 (grid nHyp x B): probability; if active: stage, refine, loss, path-I quantities, inlier masks
__global__ __launch_bounds__(kThreads)
void xl_dsac_rgbd_bwd_hyp_kernel(RgbdBwdParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const Lds L = rgbd_lds_view(smem_raw, P.Npad);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.x, b = blockIdx.y;
    const int64_t o = (int64_t)b * P.nHyp + h;
    const double prob = rgbd_softmax_prob(P.scores + (int64_t)b * P.nHyp, P.nHyp, h);
    const bool active = !(prob < XLM_PROB_THRESH);
    double *rec = P.rec + o * kRec;
    Pose pose;
    pose_load12(P.hypPoses + o * 12, &pose);
    Gt gt;
    gt_from_pose16(P.gt + (int64_t)b * 16, &gt);
    if (!active) {                                           // (uniform over the workgroup: prob is computed alike by every thread)
        const double loss = pose_loss(&pose, &gt, (double)P.wRot, (double)P.wTrans, (double)P.softClamp);
        if (tid < kRec) rec[tid] = (tid == 0) ? prob : (tid == 1) ? loss : 0.0;
        return;
    }
    int cntSel = 0, redSel = 0;
    const int nValid = rgbd_stage(P, b, L.S, L.sF, L.sCell, cntSel, tid, lane, wave, nullptr);
    const Cells ce{ L.sF, L.sF + P.Npad, L.sF + 2 * P.Npad, L.sF + 3 * P.Npad, L.sF + 4 * P.Npad, L.sF + 5 * P.Npad };
    RefineOut ro;
    rgbd_refine(ce, nValid, P.thr, P.maxDist, L.S, cntSel, redSel, tid, wave, lane, pose, ro);
    const double loss = pose_loss(&pose, &gt, (double)P.wRot, (double)P.wTrans, (double)P.softClamp);
    P.masks[o * kThreads + tid] = ro.inl;

    // path I: adjoint of the last fit for the loss gradient; none when no round was fitted (the reference's eyePts.size() < 3)
    double H[9], v[3] = { 0.0, 0.0, 0.0 }, gap = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = 0.0;
    int guardI = 0;
    if (ro.rounds > 0) {
        Pose again;
        HornEig e;
        rgbd_kabsch_fit_eig(ro.cp, ro.cX, ro.a, &again, &e);
        guardI = rgbd_eig_gap(&e, &gap) ? 1 : 0;
        if (!guardI) {
            double GR[9], g3[3];
            rgbd_loss_grad(&pose, &gt, (double)P.wRot, (double)P.wTrans, (double)P.softClamp, GR, g3);
            rgbd_kabsch_adjoint(&e, ro.cX, GR, g3, H);
            rgbd_Rt_mul_div(pose.R, g3, (double)ro.finalInl, v);
        }
    }
    if (tid == 0) {
        rec[0] = prob; rec[1] = loss; rec[2] = 1.0; rec[3] = (double)ro.finalInl; rec[4] = (double)guardI; rec[5] = 0.0;
        pose_store12(&pose, rec + 6);
        for (int i = 0; i < 9; ++i) rec[18 + i] = H[i];
        for (int i = 0; i < 3; ++i) { rec[27 + i] = v[i]; rec[30 + i] = ro.cp[i]; }
        for (int i = 33; i < kRec; ++i) rec[i] = 0.0;
        rec[56] = gap;
    }
}

// K2 (grid B): expected loss and the gradient of the soft-max selection (dsacstar_derivative.h:345-356)
__global__ __launch_bounds__(kThreads)
void xl_dsac_rgbd_bwd_expect_kernel(RgbdBwdParams P)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    double *rec = P.rec + (int64_t)b * P.nHyp * kRec;
    if (tid == 0) {
        double e = 0.0;
        for (int h = 0; h < P.nHyp; ++h) e += rec[(int64_t)h * kRec] * rec[(int64_t)h * kRec + 1];
        P.outLoss[b] = e;
    }
    for (int i = tid; i < P.nHyp; i += kThreads) {
        const double pi = rec[(int64_t)i * kRec];
        if (pi < XLM_PROB_THRESH) continue;
        double g = pi * rec[(int64_t)i * kRec + 1];
        for (int j = 0; j < P.nHyp; ++j) g -= pi * rec[(int64_t)j * kRec] * rec[(int64_t)j * kRec + 1];
        rec[(int64_t)i * kRec + 5] = g;
    }
}

// K3 (grid nHyp x B): path II per hypothesis: the twelve sums, the minimal fit's adjoint, the support-point gradients
__global__ __launch_bounds__(kThreads)
void xl_dsac_rgbd_bwd_score_kernel(RgbdBwdParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const Lds L = rgbd_lds_view(smem_raw, P.Npad);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.x, b = blockIdx.y;
    const int64_t o = (int64_t)b * P.nHyp + h;
    double *rec = P.rec + o * kRec;
    if (rec[0] < XLM_PROB_THRESH) return;                     // inactive: before staging, the whole workgroup alike
    int cntSel = 0;
    const int nValid = rgbd_stage(P, b, L.S, L.sF, L.sCell, cntSel, tid, lane, wave, nullptr);
    const Cells ce{ L.sF, L.sF + P.Npad, L.sF + 2 * P.Npad, L.sF + 3 * P.Npad, L.sF + 4 * P.Npad, L.sF + 5 * P.Npad };
    Pose init;
    pose_load12(P.hypPoses + o * 12, &init);
    const double sog = rec[5];
    const ScoreConst sc(P.thr, P.alpha, P.Ho, P.Wo);

    double sR[9], sT[3];
    {
        double s[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) s[i] = 0.0;
        for (int k = tid; k < nValid; k += kThreads) {
            double w, dhat[3];
            const double X = (double)ce.X[k], Y = (double)ce.Y[k], Z = (double)ce.Z[k];
            if (rgbd_cell_weight(&init, X, Y, Z, (double)ce.px[k], (double)ce.py[k], (double)ce.pz[k], P.maxDist, sc.beta, P.thr, sog,
                                 sc.fac, &w, dhat))
                rgbd_acc_score_sums(s, w, dhat, X, Y, Z);
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) sR[i] = s[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) sT[i] = s[9 + i];
    }
    block_sum(sR, L.S.red[0], wave, lane);
    block_sum(sT, L.S.red[1], wave, lane);

    // the minimal fit once more (the bits of K0's fit), with its eigen-decomposition
    const int32_t *pl = P.places + o * 3;
    const int k0 = pl[0], k1 = pl[1], k2 = pl[2];
    double sup[9], maxW = 0.0, gap = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) sup[i] = 0.0;
    int guardII = 1;
    if (k0 >= 0 && k1 >= 0 && k2 >= 0 && k0 < nValid && k1 < nValid && k2 < nValid) {
        const int ks[3] = { k0, k1, k2 };
        double pc[9], Xw[9], cp[3], cX[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int k = ks[j];
            pc[3 * j] = (double)ce.px[k]; pc[3 * j + 1] = (double)ce.py[k]; pc[3 * j + 2] = (double)ce.pz[k];
            Xw[3 * j] = (double)ce.X[k];  Xw[3 * j + 1] = (double)ce.Y[k];  Xw[3 * j + 2] = (double)ce.Z[k];
        }
        Pose fit;
        HornEig e;
        rgbd_fit3_eig(pc, Xw, &fit, &e, cp, cX);
        guardII = rgbd_eig_gap(&e, &gap) ? 1 : 0;
        if (!guardII) {
            maxW = rgbd_max_domega(&e, &init, pc, cp, cX);
            if (!(maxW <= XLR_MAX_DOMEGA)) guardII = 1;
        }
        if (!guardII) {
            double H[9], v[3];
            rgbd_kabsch_adjoint(&e, cX, sR, sT, H);
            rgbd_Rt_mul_div(init.R, sT, 3.0, v);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double g[3];
                rgbd_Ht_mul(H, pc[3 * j] - cp[0], pc[3 * j + 1] - cp[1], pc[3 * j + 2] - cp[2], g);
                sup[3 * j] = g[0] - v[0]; sup[3 * j + 1] = g[1] - v[1]; sup[3 * j + 2] = g[2] - v[2];
            }
        }
    }
    if (tid == 0) {
        for (int i = 0; i < 9; ++i) rec[33 + i] = sup[i];
        rec[42] = maxW; rec[43] = (double)guardII;
        for (int i = 0; i < 9; ++i) rec[44 + i] = sR[i];
        for (int i = 0; i < 3; ++i) rec[53 + i] = sT[i];
        rec[57] = gap;
    }
}

// K4 (grid ceil(N/256) x B): assemble the gradient per cell, hypotheses in ascending order, float accumulation like the
// reference's tensor += (dsacstar.cpp:462-480)
__global__ __launch_bounds__(kThreads)
void xl_dsac_rgbd_bwd_assemble_kernel(RgbdBwdParams P)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const int N = P.Ho * P.Wo;
    if (i >= N) return;
    const int y = i / P.Wo, x = i - y * P.Wo;
    const float *q = P.coords + (int64_t)b * P.sb + (int64_t)y * P.sy + (int64_t)x * P.sx;
    const double X = (double)q[0], Y = (double)q[P.sc], Z = (double)q[2 * P.sc];
    float cxf, cyf, czf;
    rgbd_load_cam(P, b, P.focals ? P.focals[b] : P.focal, y, x, cxf, cyf, czf);
    const double px = (double)cxf, py = (double)cyf, pz = (double)czf;
    const int place = P.placeOf[(int64_t)b * N + i];
    float *g = P.grad + (int64_t)b * P.gsb + (int64_t)y * P.gsy + (int64_t)x * P.gsx;
    if (place < 0) return;                                    // an invalid cell gets nothing
    float acc[3] = { g[0], g[P.gsc], g[2 * P.gsc] };
    const ScoreConst sc(P.thr, P.alpha, P.Ho, P.Wo);
    const int mt = place % kThreads, mj = place / kThreads;
    for (int h = 0; h < P.nHyp; ++h) {
        const int64_t o = (int64_t)b * P.nHyp + h;
        const double *rec = P.rec + o * kRec;
        const double prob = rec[0];
        if (prob < XLM_PROB_THRESH) continue;
        double gI[3] = { 0.0, 0.0, 0.0 };
        if (rec[3] > 0.0 && rec[4] == 0.0 && ((P.masks[o * kThreads + mt] >> mj) & 1ull)) {
            rgbd_Ht_mul(rec + 18, px - rec[30], py - rec[31], pz - rec[32], gI);
            gI[0] = gI[0] - rec[27]; gI[1] = gI[1] - rec[28]; gI[2] = gI[2] - rec[29];
        }
        Pose init;
        pose_load12(P.hypPoses + o * 12, &init);
        double jac[3] = { 0.0, 0.0, 0.0 }, w, dhat[3];
        if (rgbd_cell_weight(&init, X, Y, Z, px, py, pz, P.maxDist, sc.beta, P.thr, rec[5], sc.fac, &w, dhat))
            rgbd_cell_direct(&init, w, dhat, jac);
        const int32_t *pl = P.places + o * 3;
        for (int j = 0; j < 3; ++j)
            if (pl[j] == place)
                for (int k = 0; k < 3; ++k) jac[k] += rec[33 + 3 * j + k];
        for (int k = 0; k < 3; ++k) acc[k] = (float)((double)acc[k] + (prob * gI[k] + jac[k]));
    }
    g[0] = acc[0]; g[P.gsc] = acc[1]; g[2 * P.gsc] = acc[2];
}

}  // namespace

extern "C" int xl_dsac_backward_rgbd_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                           const float *cam_dev, int64_t mb, int64_t mc, int64_t my, int64_t mx,
                                           const float *depth_dev, int64_t db, int64_t dy, int64_t dx,
                                           int B, int Ho, int Wo,
                                           float *grad_dev, int64_t gsb, int64_t gsc, int64_t gsy, int64_t gsx,
                                           const float *gt_poses_dev, double *out_loss_dev,
                                           int n_hyp, float thr, float alpha, float max_dist,
                                           float w_rot, float w_trans, float soft_clamp,
                                           float focal, float ppx, float ppy, int sub, const float *focals_dev,
                                           uint64_t seed, uint64_t image0, uint64_t image_stride, uint32_t max_tries,
                                           void *stream, double *rec_dev)
{
    RgbdBwdParams P;
    if (rgbd_input(P, coords_dev, sb, sc, sy, sx, cam_dev, mb, mc, my, mx, depth_dev, db, dy, dx, B, Ho, Wo, focal, ppx, ppy, sub,
                   focals_dev) != XL_OK || !grad_dev || !gt_poses_dev || !out_loss_dev || n_hyp <= 0 || max_tries == 0 ||
        max_tries > XL_DSAC_RGBD_MAX_TRIES)
        return XL_ERR_ARG;
    if ((int64_t)Ho * (int64_t)Wo > (int64_t)kMaxCells) return XL_ERR_GRID;
    if (B > 65535) return XL_ERR_GRID;                        // images ride on blockIdx.y
    const int N = Ho * Wo;
    P.Npad = (N + 3) & ~3;
    const size_t lds = rgbd_lds_bytes(P.Npad);
    if (lds > kMaxLds) return XL_ERR_GRID;
    hipStream_t st = (hipStream_t)stream;
    const size_t nh = (size_t)B * n_hyp;

    int S = 1;
    while (S * 2 * kWaves <= n_hyp && (long long)B * S * 2 <= 1024) S *= 2;

    // workspace: every hypothesis' pose, score and drawn places; the place of every cell; records and inlier masks
    const size_t bPoses = sizeof(double) * nh * 12, bScores = sizeof(double) * nh, bPlaces = sizeof(int32_t) * nh * 3;
    const size_t bPlaceOf = sizeof(int32_t) * (size_t)B * N;
    const size_t bRec = rec_dev ? 0 : sizeof(double) * nh * kRec, bMasks = sizeof(unsigned long long) * nh * kThreads;
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    unsigned char *ws = nullptr;
    if (hipMallocAsync((void **)&ws, up(bPoses) + up(bScores) + up(bPlaces) + up(bPlaceOf) + up(bRec) + up(bMasks), st) != hipSuccess)
        return XL_ERR_HIP;
    unsigned char *cur = ws;
    P.hypPoses = (double *)cur; cur += up(bPoses);
    P.scores = (double *)cur; cur += up(bScores);
    P.places = (int32_t *)cur; cur += up(bPlaces);
    P.placeOf = (int32_t *)cur; cur += up(bPlaceOf);
    P.rec = rec_dev ? rec_dev : (double *)cur; cur += up(bRec);
    P.masks = (unsigned long long *)cur;
    P.grad = grad_dev; P.gsb = gsb; P.gsc = gsc; P.gsy = gsy; P.gsx = gsx;
    P.gt = gt_poses_dev; P.outLoss = out_loss_dev;
    P.seed = seed; P.image0 = image0; P.imageStride = image_stride; P.maxTries = max_tries;
    P.nHyp = n_hyp; P.S = S;
    P.thr = thr; P.alpha = alpha; P.maxDist = max_dist; P.wRot = w_rot; P.wTrans = w_trans; P.softClamp = soft_clamp;

    static XlLdsLimit configured;
    const void *const kernels[] = { reinterpret_cast<const void *>(xl_dsac_rgbd_bwd_sample_kernel),
                                    reinterpret_cast<const void *>(xl_dsac_rgbd_bwd_hyp_kernel),
                                    reinterpret_cast<const void *>(xl_dsac_rgbd_bwd_score_kernel) };
    if (!rgbd_raise_lds_limit(configured, kernels, lds)) {
        (void)hipFreeAsync(ws, st);
        return XL_ERR_HIP;
    }
    hipLaunchKernelGGL(xl_dsac_rgbd_bwd_sample_kernel, dim3(S, B), dim3(kThreads), lds, st, P);
    hipLaunchKernelGGL(xl_dsac_rgbd_bwd_hyp_kernel, dim3(n_hyp, B), dim3(kThreads), lds, st, P);
    hipLaunchKernelGGL(xl_dsac_rgbd_bwd_expect_kernel, dim3(B), dim3(kThreads), 0, st, P);
    hipLaunchKernelGGL(xl_dsac_rgbd_bwd_score_kernel, dim3(n_hyp, B), dim3(kThreads), lds, st, P);
    hipLaunchKernelGGL(xl_dsac_rgbd_bwd_assemble_kernel, dim3((N + kThreads - 1) / kThreads, B), dim3(kThreads), 0, st, P);
    const hipError_t launched = hipGetLastError();
    if (hipFreeAsync(ws, st) != hipSuccess || launched != hipSuccess) return XL_ERR_HIP;
    return XL_OK;
}
