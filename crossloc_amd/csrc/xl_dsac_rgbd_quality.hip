// xl_dsac_rgbd_quality.hip — per-frame pose quality for the RGB-D DSAC* solver on MI355X (gfx950): inlier statistics of the metric
// 3-D residuals, their JtJ over the inliers and the pose covariance at ONE given pose per image.
//
// A stand-alone pass behind xl_dsac_pose_quality_rgbd_batch (include/crossloc_dsac.h, row layout there; the input record RgbdIn and
// its shared checks, rgbd_input, are in xl_dsac_rgbd_dev.h), the sibling of
// xl_dsac_quality.hip; the solver's kernels in xl_dsac_rgbd.hip are not involved.  One 256-thread workgroup (4 wavefronts) per
// image, two walks over the cells:
//
//   read       thread tid walks cells tid, tid + 256, ... in ascending order (consecutive lanes read consecutive x); scene and
//              camera coordinates (or depth) come straight from global memory through the caller's strides.  Nothing is staged
//              in LDS, so the pass has no cell limit of its own (XL_DSAC_RGBD_MAX_CELLS does not apply); the second walk
//              re-reads what the first one left in the cache
//   walk 1     valid cells (camera z != 0): distance error in cm (rgbd_cell_err), soft-inlier term; for inliers (e < thr, the
//              float comparison the refinement makes) the count, sum m, sum e, sum e^2 and SSE
//   reduce     9 per-thread double partials in the solver's canonical order (block_sum, xl_dsac_reduce.h);
//              every thread forms the inlier centroid c from the LDS totals itself (uniform, no broadcast)
//   walk 2     the same inlier decision with the same bits; about c: C = sum u u^T, sum u x r, sum r; reduced the same way
//   finish     thread 0: 3x3 Cholesky inverse with a relative pivot test, the maps to the row's pose parameters, the row
//
// Arithmetic contract as in xl_dsac_rgbd.hip: -ffp-contract=off, fixed reduction order.  What one lane computes on its own is
// in xl_dsac_rgbd_quality_math.h; tests/rgbd_quality_ref.c compiles the same header with gcc and restates this file's
// orchestration serially, and tests/test_rgbd_quality_gpu.py compares all 64 doubles of a row bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/crossloc_dsac.h"
#include "xl_common.h"

namespace {

#include "xl_dsac_rgbd_dev.h"          // RgbdIn, rgbd_input, rgbd_load_cam, block_sum, kThreads, kWaves
#include "xl_dsac_rgbd_quality_math.h"

static_assert(XLQ_ROW == XL_DSAC_QUALITY_DOUBLES, "row width of the shared arithmetic and of the C ABI");

struct RgbdQualityParams : RgbdIn {
    const float *poses;               // [B][16] cam->world
    double *rows;                     // [B][64]
    float thr, alpha, maxDist;
};

__global__ __launch_bounds__(kThreads)
void xl_dsac_rgbd_quality_kernel(RgbdQualityParams P)
{
    __shared__ double red1[kWaves * XLQR_SUMS1];
    __shared__ double red2[kWaves * XLQR_SUMS2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const int N = P.Ho * P.Wo;

    RgbdQ q;
    q.thr = P.thr; q.alpha = P.alpha; q.maxDist = P.maxDist;
    q.Ho = P.Ho; q.Wo = P.Wo; q.N = N;
    const float f = P.focals ? P.focals[b] : P.focal;
    const float beta = 5.0f / q.thr;

    // every thread derives the pose itself (uniform over the workgroup, no broadcast)
    float p16[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) p16[i] = P.poses[(int64_t)b * 16 + i];
    const bool poseOk = quality_pose16_finite(p16);
    Pose pose;
    if (poseOk) quality_pose_from16(p16, &pose);
    else pose_identity(&pose);

    const float *g = P.coords + (int64_t)b * P.sb;
    double s1[XLQR_SUMS1];              // per-thread partials, then the totals
#pragma unroll
    for (int k = 0; k < XLQR_SUMS1; ++k) s1[k] = 0.0;
    if (poseOk) {
        for (int i = tid; i < N; i += kThreads) {
            const int y = i / P.Wo, x = i - y * P.Wo;
            float cx, cy, cz;
            rgbd_load_cam(P, b, f, y, x, cx, cy, cz);
            const float *X = g + (int64_t)y * P.sy + (int64_t)x * P.sx;
            rgbdq_cell1(&pose, (double)X[0], (double)X[P.sc], (double)X[2 * P.sc], cx, cy, cz, &q, beta, s1);
        }
    }
    block_sum(s1, red1, wave, lane);
    double c[3];
    rgbdq_centroid(s1, c);

    double s2[XLQR_SUMS2];
#pragma unroll
    for (int k = 0; k < XLQR_SUMS2; ++k) s2[k] = 0.0;
    if (poseOk) {
        for (int i = tid; i < N; i += kThreads) {
            const int y = i / P.Wo, x = i - y * P.Wo;
            float cx, cy, cz;
            rgbd_load_cam(P, b, f, y, x, cx, cy, cz);
            const float *X = g + (int64_t)y * P.sy + (int64_t)x * P.sx;
            rgbdq_cell2(&pose, (double)X[0], (double)X[P.sc], (double)X[2 * P.sc], cx, cy, cz, &q, c, s2);
        }
    }
    block_sum(s2, red2, wave, lane);
    if (tid != 0) return;
    double row[XLQ_ROW];
    rgbdq_row(s1, s2, c, &pose, &q, poseOk, row, nullptr);
    double *o = P.rows + (int64_t)b * XLQ_ROW;
    for (int i = 0; i < XLQ_ROW; ++i) o[i] = row[i];
}

}  // namespace

extern "C" int xl_dsac_pose_quality_rgbd_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                               const float *cam_dev, int64_t mb, int64_t mc, int64_t my, int64_t mx,
                                               const float *depth_dev, int64_t db, int64_t dy, int64_t dx,
                                               int B, int Ho, int Wo, const float *poses_dev,
                                               float thr, float alpha, float max_dist,
                                               float focal, float ppx, float ppy, int sub, const float *focals_dev,
                                               double *rows_dev, void *stream)
{
    RgbdQualityParams P;
    if (rgbd_input(P, coords_dev, sb, sc, sy, sx, cam_dev, mb, mc, my, mx, depth_dev, db, dy, dx, B, Ho, Wo, focal, ppx, ppy, sub,
                   focals_dev) != XL_OK || !poses_dev || !rows_dev || sub <= 0)
        return XL_ERR_ARG;
    if ((int64_t)Ho * (int64_t)Wo > (int64_t)INT32_MAX - kThreads) return XL_ERR_GRID;       // the cell index is an int
    P.poses = poses_dev; P.rows = rows_dev;
    P.thr = thr; P.alpha = alpha; P.maxDist = max_dist;
    hipLaunchKernelGGL(xl_dsac_rgbd_quality_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, P);
    return hipGetLastError() == hipSuccess ? XL_OK : XL_ERR_HIP;
}
