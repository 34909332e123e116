// xl_dsac_quality.hip — per-frame pose quality for the DSAC* solver on MI355X (gfx950): inlier statistics, JtJ of the
// reprojection residuals over the inliers and the pose covariance at ONE given pose per image.
//
// A stand-alone pass behind xl_dsac_pose_quality_batch (include/crossloc_dsac.h, row layout there); the solver's kernels in
// xl_dsac.hip are not involved.  One 256-thread workgroup (4 wavefronts) per image, one pass over the cells:
//
//   read       thread tid walks cells tid, tid + 256, ... in ascending order; the scene coordinate comes straight from
//              global memory through the caller's strides (each cell is read once, so there is nothing to stage in LDS and
//              the pass has no cell limit of its own)
//   cell       clamped reprojection error (cell_err), soft-inlier term over all cells; for inliers (e < thr, the float
//              comparison the refinement makes) the 28 normal-equation sums, the count, sum e and sum e^2
//   reduce     32 per-thread double partials in the solver's canonical order (block_sum, xl_dsac_reduce.h)
//   finish     thread 0: 6x6 Cholesky inverse, covariance of the pose and of the camera centre, the row
//
// Arithmetic contract as in xl_dsac.hip: -ffp-contract=off, fixed reduction order.  What one lane computes on its own is in
// xl_dsac_quality_math.h (on top of xl_dsac_math.h); tests/pose_quality_ref.c compiles the same header with gcc and restates
// this file's orchestration serially, and tests/test_pose_quality_gpu.py compares all 64 doubles of a row bit for bit.
//
// MASKED (xl_dsac_pose_quality_masked_batch): the same pass over the cells a per-cell validity mask admits, the masked solver's
// rules carried over.  A thread reads the mask byte of a cell before anything else of it; a masked-out cell is counted and
// skipped - its coordinate is not loaded, it is no inlier and adds to no sum - and the count rides the block sum as a 33rd
// value (exact integers; the 32 sums keep their order, so an all-ones mask gives the unmasked bits).  The unmasked
// instantiation is the kernel as it was.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/crossloc_dsac.h"
#include "xl_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

#include "xl_dsac_quality_math.h"
#include "xl_dsac_reduce.h"

static_assert(XLQ_ROW == XL_DSAC_QUALITY_DOUBLES, "row width of the shared arithmetic and of the C ABI");

struct QualityParams {
    const float *coords; int64_t sb, sc, sy, sx;
    const float *poses;               // [B][16] cam->world
    const float *focals;
    double *rows;                     // [B][64]
    int Ho, Wo, sub;
    float thr, focal, ppx, ppy, alpha, maxReproj;
    const uint8_t *mask;              // masked pass: [B][Ho*Wo], nonzero = usable cell
};

template <bool MASKED = false>
__global__ __launch_bounds__(kThreads)
void xl_dsac_quality_kernel(QualityParams P)
{
    constexpr int kSums = XLQ_SUMS + (MASKED ? 1 : 0);          // masked: [XLQ_SUMS] counts the masked-out cells
    __shared__ double red[kWaves * kSums];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const int N = P.Ho * P.Wo;

    const Cam cam = cam_make(P.Ho, P.Wo, P.thr, P.focals ? P.focals[b] : P.focal, P.ppx, P.ppy, P.alpha, P.maxReproj, P.sub);

    // every thread derives the pose itself (uniform over the workgroup, no broadcast), like the backward pass does
    float p16[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) p16[i] = P.poses[(int64_t)b * 16 + i];
    const bool poseOk = quality_pose16_finite(p16);
    Pose pose;
    if (poseOk) quality_pose_from16(p16, &pose);
    else pose_identity(&pose);

    double a[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) a[k] = 0.0;
    if (poseOk) {
        const float beta = 5.0f / cam.thr;
        const float *g = P.coords + (int64_t)b * P.sb;
        for (int i = tid; i < N; i += kThreads) {
            if constexpr (MASKED) {
                if (P.mask[(int64_t)b * N + i] == 0) { a[XLQ_SUMS] += 1.0; continue; }
            }
            const int y = i / P.Wo, x = i - y * P.Wo;
            const float *q = g + (int64_t)y * P.sy + (int64_t)x * P.sx;
            quality_cell(&pose, (double)q[0], (double)q[P.sc], (double)q[2 * P.sc], y, x, &cam, beta, a);
        }
    }

    block_sum(a, red, wave, lane);                              // the canonical order: xl_dsac_reduce.h
    if (tid != 0) return;
    double row[XLQ_ROW];
    quality_row(a, &pose, &cam, poseOk, row);
    if constexpr (MASKED) quality_row_n_masked(row, XLQ_COL_N_MASKED, a[XLQ_SUMS]);
    double *o = P.rows + (int64_t)b * XLQ_ROW;
    for (int i = 0; i < XLQ_ROW; ++i) o[i] = row[i];
}

// the launch of both entry points: MASKED adds the mask and launches the masked instantiation.  Everything is validated before
// the first HIP call.
template <bool MASKED>
int quality_launch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx, int B, int Ho, int Wo,
                   const uint8_t *mask_dev, const float *poses_dev, float thr, float focal, float ppx, float ppy, float alpha,
                   float max_reproj, int sub, const float *focals_dev, double *rows_dev, void *stream)
{
    if (!coords_dev || !poses_dev || !rows_dev || B <= 0 || Ho <= 0 || Wo <= 0 || sub <= 0) return XL_ERR_ARG;
    if (MASKED && !mask_dev) return XL_ERR_ARG;
    if ((int64_t)Ho * (int64_t)Wo > (int64_t)INT32_MAX - kThreads) return XL_ERR_GRID;       // the cell index is an int
    QualityParams P;
    P.coords = coords_dev; P.sb = sb; P.sc = sc; P.sy = sy; P.sx = sx;
    P.poses = poses_dev; P.focals = focals_dev; P.rows = rows_dev;
    P.Ho = Ho; P.Wo = Wo; P.sub = sub;
    P.thr = thr; P.focal = focal; P.ppx = ppx; P.ppy = ppy; P.alpha = alpha; P.maxReproj = max_reproj;
    P.mask = mask_dev;
    hipLaunchKernelGGL((xl_dsac_quality_kernel<MASKED>), dim3(B), dim3(kThreads), 0, (hipStream_t)stream, P);
    return hipGetLastError() == hipSuccess ? XL_OK : XL_ERR_HIP;
}

}  // namespace

extern "C" int xl_dsac_pose_quality_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                          int B, int Ho, int Wo, const float *poses_dev,
                                          float thr, float focal, float ppx, float ppy, float alpha, float max_reproj, int sub,
                                          const float *focals_dev, double *rows_dev, void *stream)
{
    return quality_launch<false>(coords_dev, sb, sc, sy, sx, B, Ho, Wo, nullptr, poses_dev, thr, focal, ppx, ppy, alpha, max_reproj,
                                 sub, focals_dev, rows_dev, stream);
}

extern "C" int xl_dsac_pose_quality_masked_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                                 int B, int Ho, int Wo, const uint8_t *mask_dev, const float *poses_dev,
                                                 float thr, float focal, float ppx, float ppy, float alpha, float max_reproj, int sub,
                                                 const float *focals_dev, double *rows_dev, void *stream)
{
    return quality_launch<true>(coords_dev, sb, sc, sy, sx, B, Ho, Wo, mask_dev, poses_dev, thr, focal, ppx, ppy, alpha, max_reproj,
                                sub, focals_dev, rows_dev, stream);
}
