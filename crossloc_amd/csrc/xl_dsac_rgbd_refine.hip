// xl_dsac_rgbd_refine.hip — ray-aware uncertainty-weighted pose refinement behind the RGB-D DSAC* solver on MI355X (gfx950): ONE
// given pose per image is re-fitted over its inliers by Levenberg-Marquardt under a 3x3 information matrix per cell, built from
// the standard deviation the coordinate network predicts (isotropic) and the depth noise along the viewing ray (model, rounds
// and parameters: xl_dsac_rgbd_refine_math.h).
//
// A stand-alone pass behind xl_dsac_refine_pose_rgbd_batch (include/crossloc_dsac.h, row layout there; the input record RgbdIn and
// its shared checks, rgbd_input, are in xl_dsac_rgbd_dev.h), the sibling of xl_dsac_refine.hip and xl_dsac_rgbd_quality.hip; the
// solver's kernels in xl_dsac_rgbd.hip are not involved.  One 256-thread workgroup (4 wavefronts) per image:
//
//   read       thread tid walks cells tid, tid + 256, ... in ascending order; scene and camera coordinates (or depth), sigma and
//              sigma_z come straight from global memory through the caller's strides on every walk.  Nothing is staged in LDS
//              and no per-thread inlier mask is kept, so the pass has no cell limit of its own: a walk re-reads what the last
//              one left in the cache
//   round      at the round's pose P_k, one walk: valid cells, cells with an unusable sigma, the inliers (clamped float error
//              < thr, the solver's comparison), their sum of m, and - from the second round on - the cells whose decision differs
//              under the previous round's pose (no mismatch: equal sets, converged).  One block_sum of 8 doubles; every thread
//              forms the centre c itself
//   LM         the control flow of xl_dsac_refine.hip: damping from 10^-3, solve6 / lambda_of, the step applied as a rotation
//              about c and a centroid translation, the accept test on the cost, the iteration cap and the step-size stop; every
//              evaluation is one walk (the inlier decision at P_k again, with the same bits) and one block_sum of 28 doubles
//   finish     one more evaluation at the float cam->world pose the caller receives (read back as a pass reads a pose), over the
//              last round's set; thread 0: the maps to the row's parameters, the covariance, the row, both poses
//
// The pose is uniform over the workgroup: every thread runs the same LM state machine on the same reduced sums, there are no
// broadcasts.  Every loop is bounded by a constant or by max_rounds.  Arithmetic contract as in xl_dsac_rgbd.hip:
// -ffp-contract=off, fixed reduction order; tests/rgbd_refine_ref.c compiles the same header with gcc and restates this file's
// orchestration serially, and tests/test_rgbd_refine_gpu.py compares poses and rows bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/crossloc_dsac.h"
#include "xl_common.h"

namespace {

#include "xl_dsac_rgbd_dev.h"          // RgbdIn, rgbd_input, rgbd_load_cam, block_sum, kThreads, kWaves
#include "xl_dsac_rgbd_refine_math.h"

static_assert(XLR_ROW == XL_DSAC_REFINE_DOUBLES, "row width of the shared arithmetic and of the C ABI");
static_assert(XLR_MAX_ROUNDS == XL_DSAC_REFINE_MAX_ROUNDS, "round limit of the shared arithmetic and of the C ABI");

struct RgbdRefineParams : RgbdIn {
    const float *sigma; int64_t gb, gy, gx;       // nullptr: sigma = 0
    const float *sigmaZ; int64_t zb, zy, zx;      // nullptr: sigma_z = 0
    const float *poses;                           // [B][16] cam->world
    float *outPoses;                              // [B][16]
    double *rows;                                 // [B][64]
    double *w2c;                                  // optional [B][12]
    float thr, maxDist, s0, depthRel;
    int maxRounds;
};

// what a walk reads of cell (y, x) of image b
struct CellIn {
    double X, Y, Z, sigma, sigmaZ;
    float px, py, pz;
};

__device__ __forceinline__ CellIn load_cell(const RgbdRefineParams &P, int b, float f, int i)
{
    CellIn ce;
    const int y = i / P.Wo, x = i - y * P.Wo;
    rgbd_load_cam(P, b, f, y, x, ce.px, ce.py, ce.pz);
    const float *X = P.coords + (int64_t)b * P.sb + (int64_t)y * P.sy + (int64_t)x * P.sx;
    ce.X = (double)X[0]; ce.Y = (double)X[P.sc]; ce.Z = (double)X[2 * P.sc];
    ce.sigma = P.sigma ? (double)P.sigma[(int64_t)b * P.gb + (int64_t)y * P.gy + (int64_t)x * P.gx] : 0.0;
    ce.sigmaZ = P.sigmaZ ? (double)P.sigmaZ[(int64_t)b * P.zb + (int64_t)y * P.zy + (int64_t)x * P.zx] : 0.0;
    return ce;
}

// one evaluation: this thread's part of the 28 sums at pose p about c, over the inliers at the round's pose pk
__device__ __forceinline__ void normal_eq_thread(const RgbdRefineParams &P, int b, float f, const RgbdR &q, const Pose &pk,
                                                 const Pose &p, const double (&c)[3], int tid, double (&a)[28])
{
#pragma unroll
    for (int k = 0; k < 28; ++k) a[k] = 0.0;
    for (int i = tid; i < q.N; i += kThreads) {
        const CellIn ce = load_cell(P, b, f, i);
        rgbdr_cell_eval(&pk, &p, ce.X, ce.Y, ce.Z, ce.px, ce.py, ce.pz, ce.sigma, ce.sigmaZ, &q, c, a);
    }
}

__global__ __launch_bounds__(kThreads)
void xl_dsac_rgbd_refine_kernel(RgbdRefineParams P)
{
    __shared__ double red[2][kWaves * 28];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;

    RgbdR q;
    q.thr = P.thr; q.maxDist = P.maxDist;
    q.Ho = P.Ho; q.Wo = P.Wo; q.N = P.Ho * P.Wo;
    q.s0sq = rgbdr_s0sq(P.sigma != nullptr, P.sigmaZ != nullptr, P.depthRel, P.s0);
    q.k = (double)P.depthRel;
    const float f = P.focals ? P.focals[b] : P.focal;

    // every thread derives the pose itself (uniform over the workgroup, no broadcast)
    float p16[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) p16[i] = P.poses[(int64_t)b * 16 + i];
    const bool poseOk = quality_pose16_finite(p16);
    Pose poseIn;
    if (poseOk) quality_pose_from16(p16, &poseIn);
    else pose_identity(&poseIn);

    double status = poseOk ? XLR_STATUS_OK : XLR_STATUS_BAD_POSE;
    Pose pose = poseIn, prevPk = poseIn;
    double neOut[28], cOut[3] = { 0.0, 0.0, 0.0 };
#pragma unroll
    for (int k = 0; k < 28; ++k) neOut[k] = 0.0;
    double n0 = 0.0, bad = 0.0, nValid = 0.0, cost0 = 0.0, nLast = 0.0;
    int rounds = 0, evals = 0, converged = 0;

    int redSel = 0;
    if (poseOk) {
        for (int r = 0; r < P.maxRounds; ++r) {
            // ---- the round's inlier set at its pose, compared with the previous round's in the same walk
            double s0[XLRR_SUMS0];
#pragma unroll
            for (int k = 0; k < XLRR_SUMS0; ++k) s0[k] = 0.0;
            for (int i = tid; i < q.N; i += kThreads) {
                const CellIn ce = load_cell(P, b, f, i);
                rgbdr_cell_start(&pose, &prevPk, r > 0, ce.X, ce.Y, ce.Z, ce.px, ce.py, ce.pz, ce.sigma, ce.sigmaZ, &q, s0);
            }
            block_sum(s0, red[redSel], wave, lane); redSel ^= 1;
            const double cnt = s0[XLRR_S_COUNT];
            if (r > 0 && s0[XLRR_S_DIFF] == 0.0) { converged = 1; break; }
            if (r > 0 && cnt < 3.0) break;
            double c[3];
            rgbdr_centroid(s0, c);

            // ---- Levenberg-Marquardt over the set (the loop of xl_dsac_refine.hip in the centred parameters)
            const Pose pk = pose;
            Pose cur = pose, prev;
            double ne[28], neNew[28];
            normal_eq_thread(P, b, f, q, pk, cur, c, tid, ne);
            block_sum(ne, red[redSel], wave, lane); redSel ^= 1; ++evals;
            if (r == 0) {
                n0 = cnt; bad = s0[XLRR_S_BAD]; nValid = s0[XLRR_S_VALID]; cost0 = ne[27]; nLast = cnt;
#pragma unroll
                for (int k = 0; k < 28; ++k) neOut[k] = ne[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) cOut[k] = c[k];
                if (cnt < 3.0) { status = XLR_STATUS_FEW_INLIERS; break; }
            }
            int lg = -3;
            bool failed = !rgbdr_well_posed(ne);            // J^T W J at the round's pose must have a sound Cholesky factor
            for (int it = 0; !failed && it < XLM_LM_MAX_ITER; ++it) {
                double d[6];
                prev = cur;
                if (!solve6(ne, lambda_of(lg), d)) { failed = true; break; }
                rgbdr_apply_step(&prev, c, d, &cur);
                const double prevErr = ne[27];
                normal_eq_thread(P, b, f, q, pk, cur, c, tid, neNew);
                block_sum(neNew, red[redSel], wave, lane); redSel ^= 1; ++evals;
                for (int up = 0; up < XLR_LG_RAISES; ++up) {
                    if (!(neNew[27] > prevErr)) break;
                    if (++lg > 16) break;
                    if (!solve6(ne, lambda_of(lg), d)) { failed = true; break; }
                    rgbdr_apply_step(&prev, c, d, &cur);
                    normal_eq_thread(P, b, f, q, pk, cur, c, tid, neNew);
                    block_sum(neNew, red[redSel], wave, lane); redSel ^= 1; ++evals;
                }
                if (failed) break;
                lg = (lg - 1 > -16) ? lg - 1 : -16;
                if (lm_step_small(d, &prev)) break;
#pragma unroll
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
#pragma unroll
            for (int k = 0; k < 28; ++k) neOut[k] = neNew[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) cOut[k] = c[k];
            ++rounds;
        }
    }

    // ---- the row rates the pose the caller receives: the float cam->world matrix, read back as every pass reads a pose (the
    // RGB-D quality pass behind this one sees exactly that pose).  One more evaluation there, over the last round's set
    float o16[16];
    Pose poseOut = pose;
    if (status == XLR_STATUS_OK) {                                       // at least one round completed; uniform
        pose_to_c2w16(&pose, o16);
        quality_pose_from16(o16, &poseOut);
        normal_eq_thread(P, b, f, q, prevPk, poseOut, cOut, tid, neOut);
        block_sum(neOut, red[redSel], wave, lane); ++evals;
    }

    if (tid != 0) return;
    double row[XLR_ROW];
    rgbdr_row(status, &q, n0, bad, nValid, cost0, nLast, neOut, cOut, rounds, evals, converged, &poseIn, &poseOut, row);
    double *o = P.rows + (int64_t)b * XLR_ROW;
    for (int i = 0; i < XLR_ROW; ++i) o[i] = row[i];
    float *op = P.outPoses + (int64_t)b * 16;
    if (status == XLR_STATUS_OK) {
        for (int i = 0; i < 16; ++i) op[i] = o16[i];
    } else {
        for (int i = 0; i < 16; ++i) op[i] = p16[i];                 // no round completed: the input pose, bit for bit
    }
    if (P.w2c) {
        double *w = P.w2c + (int64_t)b * 12;
        if (poseOk) pose_store12(&pose, w);
        else for (int i = 0; i < 12; ++i) w[i] = quality_nan();
    }
}

}  // namespace

extern "C" int xl_dsac_refine_pose_rgbd_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                              const float *cam_dev, int64_t mb, int64_t mc, int64_t my, int64_t mx,
                                              const float *depth_dev, int64_t db, int64_t dy, int64_t dx,
                                              const float *sigma_dev, int64_t gb, int64_t gy, int64_t gx,
                                              const float *depth_sigma_dev, int64_t zb, int64_t zy, int64_t zx,
                                              int B, int Ho, int Wo, const float *poses_dev, float *out_poses_dev,
                                              double *rows_dev, double *w2c_dev, float thr, float max_dist,
                                              float focal, float ppx, float ppy, int sub, const float *focals_dev,
                                              float s0, float depth_rel, int max_rounds, void *stream)
{
    RgbdRefineParams P;
    if (rgbd_input(P, coords_dev, sb, sc, sy, sx, cam_dev, mb, mc, my, mx, depth_dev, db, dy, dx, B, Ho, Wo, focal, ppx, ppy, sub,
                   focals_dev) != XL_OK || !poses_dev || !out_poses_dev || !rows_dev || sub <= 0)
        return XL_ERR_ARG;
    if (!(s0 > 0.0f) || !(depth_rel >= 0.0f) || !(depth_rel <= 3.0e38f) || max_rounds < 1 || max_rounds > XL_DSAC_REFINE_MAX_ROUNDS)
        return XL_ERR_ARG;
    if ((int64_t)Ho * (int64_t)Wo > (int64_t)INT32_MAX - kThreads) return XL_ERR_GRID;       // the cell index is an int
    P.sigma = sigma_dev; P.gb = gb; P.gy = gy; P.gx = gx;
    P.sigmaZ = depth_sigma_dev; P.zb = zb; P.zy = zy; P.zx = zx;
    P.poses = poses_dev; P.outPoses = out_poses_dev; P.rows = rows_dev; P.w2c = w2c_dev;
    P.thr = thr; P.maxDist = max_dist; P.s0 = s0; P.depthRel = depth_rel; P.maxRounds = max_rounds;
    hipLaunchKernelGGL(xl_dsac_rgbd_refine_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, P);
    return hipGetLastError() == hipSuccess ? XL_OK : XL_ERR_HIP;
}
