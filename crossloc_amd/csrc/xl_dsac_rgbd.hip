// xl_dsac_rgbd.hip — the RGB-D DSAC* pose solver on MI355X (gfx950): Kabsch hypotheses from camera coordinates (depth),
// batched.  Replaces the forward pass of dsacstar_rgbd_forward (dsacstar/dsacstar.cpp:495-612 of the reference project)
// behind xl_dsac_forward_rgbd_batch (include/crossloc_dsac.h, semantics and debug layout there).  The RGB kernels of
// xl_dsac.hip are not involved.  One 256-thread workgroup (4 wavefronts) per image, one launch per batch:
//
//   stage      the cells are walked x-major (x outer, y inner, the order of the reference's validPts) in chunks of 256; a
//              cell is valid iff its camera z is nonzero; ballot + popcount give every valid cell its place in the valid
//              list, and its six floats (camera x y z, scene X Y Z) go to LDS as SoA planes in that order, with the cell
//              index beside them.  In depth form the camera coordinate is formed here (rgbd_cam_from_depth)
//   sample     wavefront w owns hypotheses w, w+4, ...; the 64 lanes evaluate 64 consecutive tries of one hypothesis (three
//              draws from the valid list, Kabsch, three residuals); __ballot picks the lowest accepted try
//              (sampleHypothesesRGBD, dsacstar_util.h:236-307)
//   score      the same wavefront walks the valid list (lanes stride it), distance error, soft-inlier term, xor butterfly;
//              the invalid cells all have the error maxDist and enter as one product (get3DDistErrs + getHypScores,
//              dsacstar_util.h:457-507, 316-343); error maps never leave registers
//   select     first maximum wins, across the 4 wavefronts through LDS
//   refine     all 256 threads: inlier set, two block sums (centroids, centred cross-covariance; order: xl_dsac_reduce.h), Kabsch redundantly
//              in every thread so control flow stays uniform, while the inlier count grows (refineHypRGBD,
//              dsacstar_util.h:611-677)
//   write      inverse rigid transform as float 4x4 (pose2trans)
//
// LDS: 26 bytes per cell (6 floats + a 16-bit cell index) behind the 1152 bytes of Smem: 141 552 bytes (138 KiB of the CU's
// 160 KiB) at 60 x 90, one workgroup per CU.  Arithmetic contract as in xl_dsac.hip: -ffp-contract=off, fixed reduction order.  What one lane computes
// on its own is in xl_dsac_rgbd_math.h; tests/dsac_rgbd_ref.c compiles the same header with gcc and restates this file's
// orchestration serially, and tests/test_dsac_rgbd_gpu.py compares every output bit for bit.  Staging, the sampling and scoring
// of a hypothesis and the refinement loop are __device__ functions of xl_dsac_rgbd_dev.h, shared with the backward pass
// (xl_dsac_rgbd_bwd.hip); so are the input record (RgbdIn, rgbd_input), the LDS view (rgbd_lds_view) and the score constants.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>                    // memcpy in the host half of xl_dsac_math.h (bits_f64), as that header asks

#include "../../include/crossloc_dsac.h"
#include "xl_common.h"

namespace {

#include "xl_dsac_rgbd_dev.h"           // staging, sampling, scoring and refinement: shared with xl_dsac_rgbd_bwd.hip

struct RgbdParams : RgbdIn {
    float *outPoses;
    int32_t *cells; int32_t *tries; double *scores; double *dbg;
    uint64_t seed, image0, imageStride;
    uint32_t maxTries;
    int nHyp;
    float thr, alpha, maxDist;
};

__global__ __launch_bounds__(kThreads)
void xl_dsac_rgbd_forward_kernel(RgbdParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const Lds L = rgbd_lds_view(smem_raw, P.Npad);
    Smem &S = L.S;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const int N = P.Ho * P.Wo;
    int cntSel = 0;

    // ---- stage: valid list (x-major) and the valid cells' six floats
    const int nValid = rgbd_stage(P, b, L.S, L.sF, L.sCell, cntSel, tid, lane, wave, nullptr);
    const Cells ce{ L.sF, L.sF + P.Npad, L.sF + 2 * P.Npad, L.sF + 3 * P.Npad, L.sF + 4 * P.Npad, L.sF + 5 * P.Npad };

    const uint64_t imageIdx = P.image0 + (uint64_t)b * P.imageStride;
    const uint64_t imageKey = image_key(P.seed, imageIdx);
    const float thr = P.thr, maxDist = P.maxDist;
    const ScoreConst sc(thr, P.alpha, P.Ho, P.Wo);
    const double invalidTerm = sc.invalid_term(maxDist, thr);

    // ---- sample + score: this wave's hypotheses
    double bestScore = 0.0;
    int bestIdx = -1;
    int anyNan = 0;
    for (int h = wave; h < P.nHyp; h += kWaves) {
        Pose pose;
        int k3[3];
        const int triesUsed = rgbd_sample_hyp(ce, nValid, thr, imageKey, h, P.maxTries, lane, pose, k3);
        const double score = rgbd_score_hyp(ce, nValid, N, pose, maxDist, thr, sc, invalidTerm, lane);

        if (lane == 0) {
            if (P.cells) {
                int32_t *o = P.cells + ((int64_t)b * P.nHyp + h) * 3;
#pragma unroll
                for (int j = 0; j < 3; ++j) o[j] = (k3[j] >= 0) ? (int32_t)L.sCell[k3[j]] : -1;
            }
            if (P.tries) P.tries[(int64_t)b * P.nHyp + h] = triesUsed;
            if (P.scores) P.scores[(int64_t)b * P.nHyp + h] = score;
        }
        if (score != score) anyNan = 1;
        const bool better = (bestIdx < 0) || (score > bestScore);
        if (h == 0 && lane == 0) pose_store12(&pose, S.pose0);
        if (better) {
            bestScore = score; bestIdx = h;
            if (lane == 0) pose_store12(&pose, S.bestPose[wave]);
        }
    }
    if (lane == 0) { S.bestScore[wave] = bestScore; S.bestIdx[wave] = bestIdx; S.anyNan[wave] = anyNan; }
    __syncthreads();

    // ---- select: first maximum wins; any NaN score makes every soft-max probability NaN and draw() return 0
    int win = -1, winWave = 0, nanAny = 0;
    {
        double ws = 0.0;
        for (int w = 0; w < kWaves; ++w) {
            const double sc = S.bestScore[w];
            const int idx = S.bestIdx[w];
            nanAny |= S.anyNan[w];
            if (idx < 0) continue;
            if (win < 0 || sc > ws || (sc == ws && idx < win)) { win = idx; ws = sc; winWave = w; }
        }
        if (nanAny) win = 0;
    }
    Pose pose;
    pose_load12(nanAny ? S.pose0 : S.bestPose[winWave], &pose);

    // ---- refine
    RefineOut ro;
    int redSel = 0;
    rgbd_refine(ce, nValid, thr, maxDist, S, cntSel, redSel, tid, wave, lane, pose, ro);
    const int rounds = ro.rounds;
    const unsigned finalInl = ro.finalInl;

    // ---- write (pose2trans): inverse rigid transform, float row-major
    if (tid == 0) {
        float *o = P.outPoses + (int64_t)b * 16;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) o[4 * i + j] = (float)pose.R[3 * j + i];
            o[4 * i + 3] = (float)(-(pose.R[i] * pose.t[0] + pose.R[3 + i] * pose.t[1] + pose.R[6 + i] * pose.t[2]));
        }
        o[12] = 0.0f; o[13] = 0.0f; o[14] = 0.0f; o[15] = 1.0f;
        if (P.dbg) {
            double *q = P.dbg + (int64_t)b * XL_DSAC_RGBD_DBG_DOUBLES;
            q[0] = (double)win; q[1] = (double)nValid; q[2] = (double)rounds; q[3] = (double)finalInl;
            pose_store12(&pose, q + 4);
        }
    }
}

}  // namespace

extern "C" int xl_dsac_forward_rgbd_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                          const float *cam_dev, int64_t mb, int64_t mc, int64_t my, int64_t mx,
                                          const float *depth_dev, int64_t db, int64_t dy, int64_t dx,
                                          int B, int Ho, int Wo, float *out_poses_dev,
                                          int n_hyp, float thr, float alpha, float max_dist,
                                          float focal, float ppx, float ppy, int sub, const float *focals_dev,
                                          uint64_t seed, uint64_t image0, uint64_t image_stride, uint32_t max_tries,
                                          void *stream,
                                          int32_t *cells_dev, int32_t *tries_dev, double *scores_dev, double *dbg_dev)
{
    RgbdParams P;
    if (rgbd_input(P, coords_dev, sb, sc, sy, sx, cam_dev, mb, mc, my, mx, depth_dev, db, dy, dx, B, Ho, Wo, focal, ppx, ppy, sub,
                   focals_dev) != XL_OK || !out_poses_dev || n_hyp <= 0 || max_tries == 0 || max_tries > XL_DSAC_RGBD_MAX_TRIES)
        return XL_ERR_ARG;
    if ((int64_t)Ho * (int64_t)Wo > (int64_t)kMaxCells) return XL_ERR_GRID;
    P.Npad = (Ho * Wo + 3) & ~3;
    P.outPoses = out_poses_dev;
    P.cells = cells_dev; P.tries = tries_dev; P.scores = scores_dev; P.dbg = dbg_dev;
    P.seed = seed; P.image0 = image0; P.imageStride = image_stride; P.maxTries = max_tries;
    P.nHyp = n_hyp; P.thr = thr; P.alpha = alpha; P.maxDist = max_dist;

    const size_t lds = rgbd_lds_bytes(P.Npad);
    if (lds > kMaxLds) return XL_ERR_GRID;
    static XlLdsLimit configured;
    const void *const kernels[] = { reinterpret_cast<const void *>(xl_dsac_rgbd_forward_kernel) };
    if (!rgbd_raise_lds_limit(configured, kernels, lds)) return XL_ERR_HIP;
    hipLaunchKernelGGL(xl_dsac_rgbd_forward_kernel, dim3(B), dim3(kThreads), lds, (hipStream_t)stream, P);
    return hipGetLastError() == hipSuccess ? XL_OK : XL_ERR_HIP;
}
