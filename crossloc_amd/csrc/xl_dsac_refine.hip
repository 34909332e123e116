// xl_dsac_refine.hip — uncertainty-weighted pose refinement behind the DSAC* solver on MI355X (gfx950): ONE given pose per image
// is re-fitted over its inliers by iteratively re-weighted Levenberg-Marquardt, every cell weighted by the standard deviation
// the network predicts for it (model, rounds and weights: xl_dsac_refine_math.h).
//
// A stand-alone pass behind xl_dsac_refine_pose_batch (include/crossloc_dsac.h, row layout there); the solver's kernels in
// xl_dsac.hip are not involved.  One 256-thread workgroup (4 wavefronts) per image:
//
//   stage      X, Y, Z and sigma of every cell as four float planes in dynamic LDS, read once through the caller's strides
//              (16 bytes per cell): a frame takes some tens of evaluations, each of which reads every cell
//   round      at the round's pose P_k: thread tid marks its inlier cells tid, tid + 256, ... in a 64-bit mask (clamped float
//              error < thr, the solver's comparison; cells with an unusable sigma are left out), the workgroup sums the count
//              and whether any thread's mask differs from the previous round's (equal sets: converged)
//   LM         the control flow of the solver's refine_pose restated: damping from 10^-3, solve6 / lambda_of / apply_step, the
//              accept test on the weighted cost, the iteration cap and the step-size stop; every evaluation is one walk over
//              this thread's inliers and one block_sum of 28 doubles (xl_dsac_reduce.h: the canonical order)
//   finish     thread 0: covariance under the sigma model, the row, the float cam->world pose, optionally the double pose
//
// The pose is uniform over the workgroup: every thread runs the same LM state machine on the same reduced sums, there are no
// broadcasts.  Every loop is bounded by a constant or by max_rounds.  Arithmetic contract as in xl_dsac.hip:
// -ffp-contract=off, fixed reduction order; tests/pose_refine_ref.c compiles the same header with gcc and restates this file's
// orchestration serially, and tests/test_pose_refine_gpu.py compares poses and rows bit for bit.
//
// MASKED (xl_dsac_refine_pose_masked_batch): the same pass over the cells a per-cell validity mask admits, the masked solver's
// rules carried over.  The LDS holds no fifth plane (the exported cell limit stays): thread tid reads its own mask bytes once
// into a 64-bit word `usable` in the layout of its inlier word (bit j <-> cell tid + 256 j).  A masked-out cell is not staged,
// and the marking loop of every round passes it by before the sigma check and before cell_err, so it is neither an unusable
// sigma nor an inlier; the evaluations walk the inlier word and need nothing more.  The count of masked-out cells rides the
// round's block sum in its free fourth slot.  The unmasked instantiation is the kernel as it was.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/crossloc_dsac.h"
#include "xl_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

#include "xl_dsac_refine_math.h"
#include "xl_dsac_reduce.h"

static_assert(XLR_ROW == XL_DSAC_REFINE_DOUBLES, "row width of the shared arithmetic and of the C ABI");
static_assert(XLR_MAX_ROUNDS == XL_DSAC_REFINE_MAX_ROUNDS, "round limit of the shared arithmetic and of the C ABI");

// LDS: the double-buffered reduction scratch, then the four planes
struct Smem {
    double red[2][kWaves * 28];
};
constexpr size_t kSmemBytes = (sizeof(Smem) + 15) & ~size_t(15);
constexpr size_t kLdsLimit = 160 * 1024;
static_assert(kSmemBytes + (size_t)4 * XL_DSAC_REFINE_MAX_CELLS * sizeof(float) <= kLdsLimit, "the exported cell limit fits the LDS");
static_assert(kSmemBytes + (size_t)4 * (XL_DSAC_REFINE_MAX_CELLS + 4) * sizeof(float) > kLdsLimit, "the exported cell limit is the largest");
static_assert(XL_DSAC_REFINE_MAX_CELLS % 4 == 0, "planes are padded to 4 cells");
static_assert(XL_DSAC_REFINE_MAX_CELLS <= 64 * kThreads, "a thread's inlier mask has 64 bits");

struct RefineParams {
    const float *coords; int64_t sb, sc, sy, sx;
    const float *sigma; int64_t gb, gy, gx;       // nullptr: all weights 1
    const float *poses;                           // [B][16] cam->world
    const float *focals;
    float *outPoses;                              // [B][16]
    double *rows;                                 // [B][64]
    double *w2c;                                  // optional [B][12]
    int Ho, Wo, sub, Npad, maxRounds;
    float thr, focal, ppx, ppy, maxReproj, s0;
    const uint8_t *mask;                          // masked pass: [B][Ho*Wo], nonzero = usable cell
};

struct Planes { const float *x, *y, *z, *s; };

// one evaluation: this thread's part of the 28 weighted sums at pose p over the inliers `inl`, weights from the round's pose pk
__device__ __forceinline__ void normal_eq_thread(const Planes &pl, const Cam &cam, const Pose &pk, const Pose &p,
                                                 unsigned long long inl, bool hasSigma, double s0sq, int tid, double (&a)[28])
{
#pragma unroll
    for (int k = 0; k < 28; ++k) a[k] = 0.0;
    int j = 0;
    for (int i = tid; i < cam.N; i += kThreads, ++j) {
        if (!((inl >> j) & 1ull)) continue;
        const int y = i / cam.Wo, x = i - y * cam.Wo;
        refine_cell(&pk, &p, (double)pl.x[i], (double)pl.y[i], (double)pl.z[i], (double)pl.s[i], hasSigma, s0sq, y, x, &cam, a);
    }
}

template <bool MASKED = false>
__global__ __launch_bounds__(kThreads)
void xl_dsac_refine_kernel(RefineParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Smem &S = *reinterpret_cast<Smem *>(smem_raw);
    float *sCo = reinterpret_cast<float *>(smem_raw + kSmemBytes);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const int N = P.Ho * P.Wo;
    const bool hasSigma = P.sigma != nullptr;
    const double s0sq = (double)P.s0 * (double)P.s0;

    const Cam cam = cam_make(P.Ho, P.Wo, P.thr, P.focals ? P.focals[b] : P.focal, P.ppx, P.ppy, 0.0f, P.maxReproj, P.sub);

    // every thread derives the pose itself (uniform over the workgroup, no broadcast)
    float p16[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) p16[i] = P.poses[(int64_t)b * 16 + i];
    const bool poseOk = quality_pose16_finite(p16);
    Pose poseIn;
    if (poseOk) quality_pose_from16(p16, &poseIn);
    else pose_identity(&poseIn);

    double status = poseOk ? XLR_STATUS_OK : XLR_STATUS_BAD_POSE;
    Pose pose = poseIn;
    double neOut[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) neOut[k] = 0.0;
    double n0 = 0.0, bad = 0.0, cost0 = 0.0, nLast = 0.0;
    double nMasked = 0.0;                                       // masked: the cells the mask ruled out
    int rounds = 0, evals = 0, converged = 0;

    if (poseOk) {
        // ---- masked: this thread's slice of the mask, bit j <-> cell tid + 256 j, and how many of its cells are ruled out
        unsigned long long usable = ~0ull;
        double myMasked = 0.0;
        if constexpr (MASKED) {
            const uint8_t *gm = P.mask + (int64_t)b * N;
            usable = 0ull;
            int j = 0;
            for (int i = tid; i < N; i += kThreads, ++j) {
                if (gm[i] != 0) usable |= (1ull << j);
                else myMasked += 1.0;
            }
        }
        // ---- stage the four planes (a NULL sigma map is staged as zeros; its values are never used: every weight is 1)
        {
            const float *g = P.coords + (int64_t)b * P.sb;
            const float *gs = hasSigma ? P.sigma + (int64_t)b * P.gb : nullptr;
            int j = 0;
            for (int i = tid; i < N; i += kThreads, ++j) {
                if constexpr (MASKED) {
                    if (!((usable >> j) & 1ull)) continue;      // not read; its LDS slots are never read either
                }
                const int y = i / P.Wo, x = i - y * P.Wo;
                const float *q = g + (int64_t)y * P.sy + (int64_t)x * P.sx;
                sCo[i] = q[0];
                sCo[P.Npad + i] = q[P.sc];
                sCo[2 * P.Npad + i] = q[2 * P.sc];
                sCo[3 * P.Npad + i] = hasSigma ? gs[(int64_t)y * P.gy + (int64_t)x * P.gx] : 0.0f;
            }
        }
        __syncthreads();
        const Planes pl{ sCo, sCo + P.Npad, sCo + 2 * P.Npad, sCo + 3 * P.Npad };

        int redSel = 0;
        unsigned long long prevInl = 0ull;
        for (int r = 0; r < P.maxRounds; ++r) {
            // ---- the round's inlier set at its pose
            unsigned long long inl = 0ull;
            double c4[4] = { 0.0, 0.0, 0.0, 0.0 };      // inliers, unusable sigmas, mask differs from the previous round's, -
            {
                int j = 0;
                for (int i = tid; i < N; i += kThreads, ++j) {
                    if constexpr (MASKED) {
                        if (!((usable >> j) & 1ull)) continue;
                    }
                    if (hasSigma && refine_sigma_bad((double)pl.s[i])) { c4[1] += 1.0; continue; }
                    const int y = i / cam.Wo, x = i - y * cam.Wo;
                    const float e = cell_err(&pose, (double)pl.x[i], (double)pl.y[i], (double)pl.z[i], y, x, &cam);
                    if (e < cam.thr) inl |= (1ull << j);
                }
            }
            c4[0] = (double)__popcll(inl);
            c4[2] = (inl != prevInl) ? 1.0 : 0.0;       // the OR over the workgroup, as a sum of flags
            if constexpr (MASKED) c4[3] = myMasked;
            block_sum(c4, S.red[redSel], wave, lane); redSel ^= 1;
            const double cnt = c4[0];
            if (r > 0 && c4[2] == 0.0) { converged = 1; break; }
            if (r > 0 && cnt < 4.0) break;

            // ---- Levenberg-Marquardt over the set, weights fixed at the round's pose (refine_pose of xl_dsac.hip restated)
            const Pose pk = pose;
            Pose cur = pose, prev;
            double ne[28], neNew[28];
            normal_eq_thread(pl, cam, pk, cur, inl, hasSigma, s0sq, tid, ne);
            block_sum(ne, S.red[redSel], wave, lane); redSel ^= 1; ++evals;
            if (r == 0) {
                n0 = cnt; bad = c4[1]; cost0 = ne[27]; nLast = cnt;
                if constexpr (MASKED) nMasked = c4[3];
#pragma unroll
                for (int k = 0; k < 28; ++k) neOut[k] = ne[k];
                if (cnt < 4.0) { status = XLR_STATUS_FEW_INLIERS; break; }
            }
            int lg = -3;
            double inv[36];
            bool failed = !quality_inv6(ne, inv);           // J^T W J at the round's pose must be positive definite
            for (int it = 0; !failed && it < XLM_LM_MAX_ITER; ++it) {
                double d[6];
                prev = cur;
                if (!solve6(ne, lambda_of(lg), d)) { failed = true; break; }
                apply_step(&prev, d, &cur);
                const double prevErr = ne[27];
                normal_eq_thread(pl, cam, pk, cur, inl, hasSigma, s0sq, tid, neNew);
                block_sum(neNew, S.red[redSel], wave, lane); redSel ^= 1; ++evals;
                for (int up = 0; up < XLR_LG_RAISES; ++up) {
                    if (!(neNew[27] > prevErr)) break;
                    if (++lg > 16) break;
                    if (!solve6(ne, lambda_of(lg), d)) { failed = true; break; }
                    apply_step(&prev, d, &cur);
                    normal_eq_thread(pl, cam, pk, cur, inl, hasSigma, s0sq, tid, neNew);
                    block_sum(neNew, S.red[redSel], wave, lane); redSel ^= 1; ++evals;
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
            nLast = cnt;
            prevInl = inl;
#pragma unroll
            for (int k = 0; k < 28; ++k) neOut[k] = neNew[k];
            ++rounds;
        }
    }

    if (tid != 0) return;
    double row[XLR_ROW];
    refine_row(status, &cam, n0, bad, cost0, nLast, neOut, rounds, evals, converged, &poseIn, &pose, row);
    if constexpr (MASKED) quality_row_n_masked(row, XLR_COL_N_MASKED, nMasked);
    double *o = P.rows + (int64_t)b * XLR_ROW;
    for (int i = 0; i < XLR_ROW; ++i) o[i] = row[i];
    float *op = P.outPoses + (int64_t)b * 16;
    if (status == XLR_STATUS_OK) {
        float o16[16];
        pose_to_c2w16(&pose, o16);
        for (int i = 0; i < 16; ++i) op[i] = o16[i];
    } else {
        for (int i = 0; i < 16; ++i) op[i] = p16[i];                 // no round completed: the input pose, bit for bit
    }
    if (P.w2c) {
        double *q = P.w2c + (int64_t)b * 12;
        if (poseOk) pose_store12(&pose, q);
        else for (int i = 0; i < 12; ++i) q[i] = quality_nan();
    }
}

// the launch of both entry points: MASKED adds the mask and launches the masked instantiation (which keeps an LDS limit of its
// own).  Everything is validated before the first HIP call.
template <bool MASKED>
int refine_launch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                  const float *sigma_dev, int64_t gb, int64_t gy, int64_t gx,
                  int B, int Ho, int Wo, const uint8_t *mask_dev, const float *poses_dev, float *out_poses_dev,
                  double *rows_dev, double *w2c_dev,
                  float thr, float focal, float ppx, float ppy, float max_reproj, int sub,
                  const float *focals_dev, float s0, int max_rounds, void *stream)
{
    if (!coords_dev || !poses_dev || !out_poses_dev || !rows_dev || B <= 0 || Ho <= 0 || Wo <= 0 || sub <= 0) return XL_ERR_ARG;
    if (MASKED && !mask_dev) return XL_ERR_ARG;
    if (!(s0 > 0.0f) || max_rounds < 1 || max_rounds > XL_DSAC_REFINE_MAX_ROUNDS) return XL_ERR_ARG;
    if ((int64_t)Ho * (int64_t)Wo > (int64_t)XL_DSAC_REFINE_MAX_CELLS) return XL_ERR_GRID;
    const int N = Ho * Wo;
    RefineParams P;
    P.coords = coords_dev; P.sb = sb; P.sc = sc; P.sy = sy; P.sx = sx;
    P.sigma = sigma_dev; P.gb = gb; P.gy = gy; P.gx = gx;
    P.poses = poses_dev; P.focals = focals_dev; P.outPoses = out_poses_dev; P.rows = rows_dev; P.w2c = w2c_dev;
    P.Ho = Ho; P.Wo = Wo; P.sub = sub; P.Npad = (N + 3) & ~3; P.maxRounds = max_rounds;
    P.thr = thr; P.focal = focal; P.ppx = ppx; P.ppy = ppy; P.maxReproj = max_reproj; P.s0 = s0;
    P.mask = mask_dev;

    const size_t lds = kSmemBytes + (size_t)4 * P.Npad * sizeof(float);
    if (lds > kLdsLimit) return XL_ERR_GRID;
    static XlLdsLimit configured;
    if (configured.configure(reinterpret_cast<const void *>(xl_dsac_refine_kernel<MASKED>), lds) != XL_OK) return XL_ERR_HIP;
    hipLaunchKernelGGL((xl_dsac_refine_kernel<MASKED>), dim3(B), dim3(kThreads), lds, (hipStream_t)stream, P);
    return hipGetLastError() == hipSuccess ? XL_OK : XL_ERR_HIP;
}

}  // namespace

extern "C" int xl_dsac_refine_pose_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                         const float *sigma_dev, int64_t gb, int64_t gy, int64_t gx,
                                         int B, int Ho, int Wo, const float *poses_dev, float *out_poses_dev,
                                         double *rows_dev, double *w2c_dev,
                                         float thr, float focal, float ppx, float ppy, float max_reproj, int sub,
                                         const float *focals_dev, float s0, int max_rounds, void *stream)
{
    return refine_launch<false>(coords_dev, sb, sc, sy, sx, sigma_dev, gb, gy, gx, B, Ho, Wo, nullptr, poses_dev, out_poses_dev,
                                rows_dev, w2c_dev, thr, focal, ppx, ppy, max_reproj, sub, focals_dev, s0, max_rounds, stream);
}

extern "C" int xl_dsac_refine_pose_masked_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                                const float *sigma_dev, int64_t gb, int64_t gy, int64_t gx,
                                                int B, int Ho, int Wo, const uint8_t *mask_dev, const float *poses_dev,
                                                float *out_poses_dev, double *rows_dev, double *w2c_dev,
                                                float thr, float focal, float ppx, float ppy, float max_reproj, int sub,
                                                const float *focals_dev, float s0, int max_rounds, void *stream)
{
    return refine_launch<true>(coords_dev, sb, sc, sy, sx, sigma_dev, gb, gy, gx, B, Ho, Wo, mask_dev, poses_dev, out_poses_dev,
                               rows_dev, w2c_dev, thr, focal, ppx, ppy, max_reproj, sub, focals_dev, s0, max_rounds, stream);
}
