// xl_e2e.hip — the end-to-end training step's own op on MI355X (gfx950): per-image finishing of the DSAC* pose gradient
// (norm, acceptance, clipping scale, widening to the network's channels, accumulation onto a gradient that is already there).
//
// Behind xl_e2e_pose_gradient (include/crossloc_e2e.h: the rules, the row layout).  One 1024-thread workgroup (16 wavefronts)
// per image and two walks over it: thread tid owns cells tid, tid + 1024, ... through the caller's strides.  Both walks wait
// on memory, a few loads per thread and trip: 16 waves keep 60 x 90 cells to six trips each.
//
//   sums       float64 squares of the three channels of every cell, per thread in ascending cell order, then block_sum
//              (xl_dsac_reduce.h: the butterfly per wave, then the 16 wave sums in ascending order).  A non-finite element
//              makes the sum non-finite, so the sum is the finiteness test too.
//   apply      every thread holds n_b and s_b; the image (65 KB at 60 x 90) comes back from L2.  out is written whole.
//   stats      thread 0 stores its row write-through and counts the workgroup done (one agent-scope integer add); the
//              workgroup whose add came last reads the B rows past its L1, in ascending b, and writes stats[B].  The values
//              do not depend on which workgroup that is.  The counter is left at zero for the next call.
//
// Arithmetic contract as in the solver: -ffp-contract=off, fixed reduction order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crossloc_dsac.h"
#include "../../include/crossloc_e2e.h"
#include "xl_common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;

#include "xl_dsac_math.h"
#include "xl_dsac_reduce.h"

struct E2eParams {
    const float *g; int64_t gb, gc, gy, gx;
    const double *loss;
    float *out;
    double *stats;
    int B, Ho, Wo, C;
    float weight, clip, beta;
};

__device__ unsigned g_done;                 // workgroups of the running call that have stored their row; zero between calls

__device__ __forceinline__ void store_through(double *p, double v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ double load_past_l1(const double *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool is_clipped(double n, float clip) { return clip > 0.f && n > (double)clip; }

__global__ __launch_bounds__(kThreads)
void xl_e2e_pose_gradient_kernel(E2eParams P)
{
    __shared__ double red[kWaves];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const int N = P.Ho * P.Wo;
    const float *g = P.g + (int64_t)b * P.gb;

    double a[1] = { 0.0 };
    for (int i = tid; i < N; i += kThreads) {
        const int y = i / P.Wo, x = i - y * P.Wo;
        const float *q = g + (int64_t)y * P.gy + (int64_t)x * P.gx;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = (double)q[c * P.gc];
            a[0] = a[0] + v * v;
        }
    }
    block_sum(a, red, wave, lane);                              // the canonical order: xl_dsac_reduce.h

    const double lossb = P.loss[b];
    const double n = sqrt(a[0]);
    const bool accepted = isfinite(a[0]) && isfinite(lossb);
    const float s = accepted ? (float)((double)P.weight / P.B * (is_clipped(n, P.clip) ? (double)P.clip / n : 1.0)) : 0.f;

    float *o = P.out + (int64_t)b * P.C * N;
    for (int i = tid; i < N; i += kThreads) {
        const int y = i / P.Wo, x = i - y * P.Wo;
        const float *q = g + (int64_t)y * P.gy + (int64_t)x * P.gx;
        float t[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) t[c] = accepted ? s * q[c * P.gc] : 0.f;          // a rejected image: zeros, not 0 * NaN
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float *d = o + (int64_t)c * N + i;
            if (P.beta != 0.f) t[c] = P.beta * *d + t[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(int64_t)c * N + i] = t[c];
    }
    for (int64_t j = (int64_t)3 * N + tid; j < (int64_t)P.C * N; j += kThreads)
        o[j] = P.beta == 0.f ? 0.f : P.beta * o[j];

    if (tid != 0) return;
    double *row = P.stats + (int64_t)b * XL_E2E_STATS;
    store_through(row + 0, lossb);
    store_through(row + 1, n);
    store_through(row + 2, (double)s);
    store_through(row + 3, accepted ? 1.0 : 0.0);
    if (__hip_atomic_fetch_add(&g_done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != (unsigned)P.B - 1u) return;
    __hip_atomic_store(&g_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    double sumLoss = 0.0, nAccepted = 0.0, maxNorm = 0.0, nClipped = 0.0;
    for (int i = 0; i < P.B; ++i) {
        const double *r = P.stats + (int64_t)i * XL_E2E_STATS;
        if (load_past_l1(r + 3) == 0.0) continue;
        const double ni = load_past_l1(r + 1);
        sumLoss = sumLoss + load_past_l1(r + 0);
        nAccepted += 1.0;
        maxNorm = ni > maxNorm ? ni : maxNorm;
        if (is_clipped(ni, P.clip)) nClipped += 1.0;
    }
    double *sum = P.stats + (int64_t)P.B * XL_E2E_STATS;
    sum[0] = nAccepted > 0.0 ? sumLoss / nAccepted : 0.0;
    sum[1] = nAccepted;
    sum[2] = maxNorm;
    sum[3] = nClipped;
}

}  // namespace

extern "C" int xl_e2e_pose_gradient(const float *g, int64_t gb, int64_t gc, int64_t gy, int64_t gx, const double *loss,
                                    int B, int Ho, int Wo, int C, float weight, float clip_norm, float beta, float *out,
                                    double *stats, void *stream)
{
    if (!g || !loss || !out || !stats || B <= 0 || Ho <= 0 || Wo <= 0 || C < 3) return XL_ERR_ARG;
    if ((int64_t)Ho * (int64_t)Wo > (int64_t)INT32_MAX - kThreads) return XL_ERR_GRID;       // the cell index is an int
    E2eParams P;
    P.g = g; P.gb = gb; P.gc = gc; P.gy = gy; P.gx = gx;
    P.loss = loss; P.out = out; P.stats = stats;
    P.B = B; P.Ho = Ho; P.Wo = Wo; P.C = C;
    P.weight = weight; P.clip = clip_norm; P.beta = beta;
    hipLaunchKernelGGL(xl_e2e_pose_gradient_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, P);
    return hipGetLastError() == hipSuccess ? XL_OK : XL_ERR_HIP;
}
