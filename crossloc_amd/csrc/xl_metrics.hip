// xl_metrics.hip — fused per-image evaluation metrics of the depth, normal and semantics tasks.
//
// Reference (PyTorch eager on the CPU after a .cpu() of the prediction, utils/evaluation.py):
//   :247-267  depth_eval     abs-rel and RMS over has-data cells
//   :294-316  normal_eval    mean angular error (utils/learning.py:417-440: logits -> radian -> xyz)
//   :339-414  semantic_eval  arg-max, 6x6 confusion matrix per image
// Each metric is ONE streaming kernel here (reads prediction and label once) plus a tiny finalisation kernel, and produces one
// row per image (crossloc_metrics.h).  Sums are reduced in a fixed order (wave butterfly -> LDS -> per-chunk partial -> sequential
// finalise); the confusion matrix is a per-wave private LDS histogram (integer LDS adds), combined across waves, then integer
// partials.  No global atomics, no memset, nothing synchronises with the host.
//
// Cell -> lane mapping (the determinism contract): workgroup (x, b) owns the cells [x*kChunk, min(n, (x+1)*kChunk)) of image b;
// lane t owns the groups of 4 cells g = t, t + kT, ... of that chunk.  The mapping never depends on B or on pointer alignment;
// alignment only selects the load width per plane (load4 below).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crossloc_metrics.h"
#include "../../include/crossloc_dsac.h"

namespace {

constexpr int kT = 256;
constexpr int kChunk = XL_METRICS_CHUNK;
constexpr int kC = XL_METRICS_CLASSES;
constexpr int kBins = kC * kC;
constexpr double kPiD = 3.141592653589793;           // np.pi
static_assert(kChunk % (4 * kT) == 0, "a chunk is a whole number of 4-cell groups per lane");

// true when 16-byte loads of groups of 4 cells from `p` (a plane at the start of a chunk) are aligned
__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// cells off .. off+cnt-1 (cnt in 1..4) of a plane; slots past cnt are 0 and never used
__device__ __forceinline__ void load4(const float *p, int off, int cnt, bool al, float v[4])
{
    if (al && cnt == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p + off);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (j < cnt) ? p[off + j] : 0.f;
    }
}

// fixed-order block reduction of K doubles; result valid in thread 0
template <int K>
__device__ __forceinline__ void block_reduce(double (&v)[K], double *sm /* [kT/64][K] */)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += __shfl_xor(v[k], off);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) sm[wave * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double r = sm[k];
#pragma unroll
        for (int w = 1; w < kT / 64; ++w) r += sm[w * K + k];
        v[k] = r;
    }
}

struct Args {
    const float *pred, *gt;
    void *partials;
    long long sb, sc;                                // image / channel stride of pred, elements
    int n, nchunk;
    float nodata;
    uint8_t *cmap;
};

// ---------------------------------------------------------------------------------------------- depth

__global__ __launch_bounds__(kT)
void depth_metrics_kernel(Args a)
{
    __shared__ double sRed[(kT / 64) * 3];
    const int b = blockIdx.y;
    const int c0 = blockIdx.x * kChunk;
    const int len = min(kChunk, a.n - c0);
    const float *P = a.pred + (long long)b * a.sb + c0;
    const float *G = a.gt + (long long)b * a.n + c0;
    const bool alP = aligned16(P), alG = aligned16(G);
    double s[3] = { 0.0, 0.0, 0.0 };
    for (int g = threadIdx.x; g * 4 < len; g += kT) {
        const int off = g * 4, cnt = min(4, len - off);
        float p[4], q[4];
        load4(P, off, cnt, alP, p);
        load4(G, off, cnt, alG, q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < cnt) {
                const double m = (q[j] != a.nodata) ? 1.0 : 0.0;              // pick_valid_points, learning.py:63
                const double gd = (double)q[j];
                const double em = fabs((double)p[j] - gd) * m;               // evaluation.py:259, :264
                s[0] += em / gd;
                s[1] += em * em;                                             // :265
                s[2] += m;
            }
        }
    }
    block_reduce<3>(s, sRed);
    if (threadIdx.x == 0) {
        double *o = reinterpret_cast<double *>(a.partials) + ((long long)b * a.nchunk + blockIdx.x) * 3;
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
    }
}

// ---------------------------------------------------------------------------------------------- normal

// logits_to_radian (learning.py:431-440) in float64
__device__ __forceinline__ double logit_to_radian(float x)
{
    double r = 1.0 / (1.0 + exp(-(double)x));
    r = fmin(fmax(r, 1.e-7), 1.0 - 1.e-7);
    return (r * 2.0 - 1.0) * kPiD;
}

__global__ __launch_bounds__(kT)
void normal_metrics_kernel(Args a)
{
    __shared__ double sRed[(kT / 64) * 2];
    const int b = blockIdx.y;
    const int c0 = blockIdx.x * kChunk;
    const int len = min(kChunk, a.n - c0);
    const float *PA = a.pred + (long long)b * a.sb + c0, *PE = PA + a.sc;
    const float *GX = a.gt + (long long)b * 3 * a.n + c0, *GY = GX + a.n, *GZ = GY + a.n;
    const bool alA = aligned16(PA), alE = aligned16(PE), alX = aligned16(GX), alY = aligned16(GY), alZ = aligned16(GZ);
    double s[2] = { 0.0, 0.0 };
    for (int g = threadIdx.x; g * 4 < len; g += kT) {
        const int off = g * 4, cnt = min(4, len - off);
        float la[4], le[4], gx[4], gy[4], gz[4];
        load4(PA, off, cnt, alA, la);
        load4(PE, off, cnt, alE, le);
        load4(GX, off, cnt, alX, gx);
        load4(GY, off, cnt, alY, gy);
        load4(GZ, off, cnt, alZ, gz);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < cnt) {
                const double az = logit_to_radian(la[j]), el = logit_to_radian(le[j]);
                // ae2xyz (learning.py:417-428) with F.normalize (eps 1e-12)
                const double xyn = cos(el);
                double X = cos(az) * xyn, Y = sin(az) * xyn, Z = sin(el);
                const double pn = fmax(sqrt(X * X + Y * Y + Z * Z), 1.e-12);
                X /= pn; Y /= pn; Z /= pn;
                // cosine_similarity (evaluation.py:310; eps 1e-8): both vectors divided by their clamped norms, then the dot product
                const double x = (double)gx[j], y = (double)gy[j], z = (double)gz[j];
                const double n1 = fmax(sqrt(X * X + Y * Y + Z * Z), 1.e-8);
                const double n2 = fmax(sqrt(x * x + y * y + z * z), 1.e-8);
                double c = (X / n1) * (x / n2) + (Y / n1) * (y / n2) + (Z / n1) * (z / n2);
                c = fmin(fmax(c, -1.0 + 1.e-7), 1.0 - 1.e-7);                 // :311
                const double deg = acos(c) / kPiD * 180.0;                    // :312
                const double m = (gx[j] != a.nodata && gy[j] != a.nodata && gz[j] != a.nodata) ? 1.0 : 0.0;
                s[0] += deg * m;                                              // :315
                s[1] += m;
            }
        }
    }
    block_reduce<2>(s, sRed);
    if (threadIdx.x == 0) {
        double *o = reinterpret_cast<double *>(a.partials) + ((long long)b * a.nchunk + blockIdx.x) * 2;
        o[0] = s[0]; o[1] = s[1];
    }
}

// per image, thread k < K adds the chunk partials of component k in chunk order
template <int K>
__global__ __launch_bounds__(64)
void finalize_rows_kernel(const double *partials, int nchunk, double *rows)
{
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= K) return;
    const double *p = partials + (long long)b * nchunk * K + k;
    double r = 0.0;
    for (int c = 0; c < nchunk; ++c) r += p[(long long)c * K];
    rows[(long long)b * K + k] = r;
}

// ---------------------------------------------------------------------------------------------- semantics

__global__ __launch_bounds__(kT)
void semantics_metrics_kernel(Args a)
{
    __shared__ unsigned sHist[kT / 64][kBins];       // one private histogram per wave
    const int b = blockIdx.y;
    const int c0 = blockIdx.x * kChunk;
    const int len = min(kChunk, a.n - c0);
    const int wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < (kT / 64) * kBins; i += kT) (&sHist[0][0])[i] = 0u;
    __syncthreads();
    const float *L = a.pred + (long long)b * a.sb + c0;
    const float *G = a.gt + (long long)b * a.n + c0;
    uint8_t *M = a.cmap ? a.cmap + (long long)b * a.n + c0 : nullptr;
    bool alL[kC];
#pragma unroll
    for (int c = 0; c < kC; ++c) alL[c] = aligned16(L + (long long)c * a.sc);
    const bool alG = aligned16(G);
    const bool alM = M && (reinterpret_cast<uintptr_t>(M) & 3u) == 0;
    for (int g = threadIdx.x; g * 4 < len; g += kT) {
        const int off = g * 4, cnt = min(4, len - off);
        float best[4], v[4], lab[4];
        int arg[4] = { 0, 0, 0, 0 };
        load4(L, off, cnt, alL[0], best);
#pragma unroll
        for (int c = 1; c < kC; ++c) {
            load4(L + (long long)c * a.sc, off, cnt, alL[c], v);
#pragma unroll
            for (int j = 0; j < 4; ++j) if (v[j] > best[j]) { best[j] = v[j]; arg[j] = c; }   // strict: ties keep the lowest index
        }
        load4(G, off, cnt, alG, lab);
        if (M) {
            if (alM && cnt == 4) {
                *reinterpret_cast<uint32_t *>(M + off) = (uint32_t)arg[0] | ((uint32_t)arg[1] << 8) | ((uint32_t)arg[2] << 16) |
                                                         ((uint32_t)arg[3] << 24);
            } else {
                for (int j = 0; j < cnt; ++j) M[off + j] = (uint8_t)arg[j];
            }
        }
        // runs of equal bins within the 4 cells (the common case inside a segment) become one LDS add
        int runBin = -1;
        unsigned runLen = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int bin = -1;
            if (j < cnt && lab[j] >= 0.f && lab[j] < (float)kC) bin = (int)lab[j] * kC + arg[j];   // evaluation.py:374-375
            if (bin != runBin) {
                if (runBin >= 0) atomicAdd(&sHist[wave][runBin], runLen);
                runBin = bin; runLen = 0;
            }
            ++runLen;
        }
        if (runBin >= 0) atomicAdd(&sHist[wave][runBin], runLen);
    }
    __syncthreads();
    if (threadIdx.x < kBins) {
        unsigned r = sHist[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kT / 64; ++w) r += sHist[w][threadIdx.x];
        reinterpret_cast<unsigned *>(a.partials)[((long long)b * a.nchunk + blockIdx.x) * kBins + threadIdx.x] = r;
    }
}

__global__ __launch_bounds__(64)
void finalize_counts_kernel(const unsigned *partials, int nchunk, long long *counts)
{
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= kBins) return;
    const unsigned *p = partials + (long long)b * nchunk * kBins + k;
    long long r = 0;
    for (int c = 0; c < nchunk; ++c) r += (long long)p[(long long)c * kBins];
    counts[(long long)b * kBins + k] = r;
}

int launch_ok()
{
    return hipGetLastError() == hipSuccess ? XL_OK : XL_ERR_HIP;
}

bool fill(Args &a, const float *pred, int64_t sb, int64_t sc, const float *gt, int B, int n, float nodata, void *ws)
{
    if (!pred || !gt || !ws || B <= 0 || B > XL_METRICS_MAX_BATCH || n <= 0 || sb < 0 || sc < 0) return false;   // B is gridDim.y
    a.pred = pred; a.gt = gt; a.partials = ws; a.sb = sb; a.sc = sc; a.n = n; a.nchunk = (n + kChunk - 1) / kChunk;
    a.nodata = nodata; a.cmap = nullptr;
    return true;
}

}  // namespace

extern "C" {

int64_t xl_metrics_workspace_bytes(int B, int n_cells)
{
    if (B <= 0 || n_cells <= 0) return 0;
    return (int64_t)B * ((n_cells + kChunk - 1) / kChunk) * kBins * (int64_t)sizeof(unsigned);
}

int xl_metrics_depth(const float *pred, int64_t pred_sb, int64_t pred_sc, const float *gt_depth, int B, int n_cells,
                     float nodata, void *workspace, double *rows, void *stream)
{
    Args a;
    if (!rows || !fill(a, pred, pred_sb, pred_sc, gt_depth, B, n_cells, nodata, workspace)) return XL_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(depth_metrics_kernel, dim3(a.nchunk, B), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(finalize_rows_kernel<3>, dim3(B), dim3(64), 0, st, (const double *)workspace, a.nchunk, rows);
    return launch_ok();
}

int xl_metrics_normal(const float *logits, int64_t pred_sb, int64_t pred_sc, const float *gt_normals, int B, int n_cells,
                      float nodata, void *workspace, double *rows, void *stream)
{
    Args a;
    if (!rows || !fill(a, logits, pred_sb, pred_sc, gt_normals, B, n_cells, nodata, workspace)) return XL_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(normal_metrics_kernel, dim3(a.nchunk, B), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(finalize_rows_kernel<2>, dim3(B), dim3(64), 0, st, (const double *)workspace, a.nchunk, rows);
    return launch_ok();
}

int xl_metrics_semantics(const float *logits, int64_t pred_sb, int64_t pred_sc, int C, const float *labels, int B,
                         int n_cells, void *workspace, int64_t *counts, uint8_t *class_map, void *stream)
{
    Args a;
    if (C != kC || !counts || !fill(a, logits, pred_sb, pred_sc, labels, B, n_cells, 0.f, workspace)) return XL_ERR_ARG;
    a.cmap = class_map;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(semantics_metrics_kernel, dim3(a.nchunk, B), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(finalize_counts_kernel, dim3(B), dim3(64), 0, st, (const unsigned *)workspace, a.nchunk,
                       (long long *)counts);
    return launch_ok();
}

}  // extern "C"
