// xl_wino.hip — XL_OP_WINO_IN / XL_OP_WINO_OUT: the input and output transforms of Winograd F(2x2), F(4x4) and F(6x6, 3x3); the
// (m+2)^2 GEMMs between them are one batched XL_OP_CONV.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "xl_launch.h"
#include "xl_operand_math.h"

namespace {

// ---------------------------------------------------------------------------------------------- Winograd F(2x2, 3x3)

// The stride-1 3x3 convolutions of inference plans run as Winograd F(2x2,3x3): 16 multiplies per 2x2 output tile and
// (ci, co) pair instead of 36.  V[xi][t][c] = (B^T d B)[xi] for the 4x4 input patch d of output tile t (zero padded),
// M[xi] = V[xi] U[xi]^T (16 GEMMs through igemm_conv_kernel, one batched launch), Y = A^T M A + bias.
// HBM-bound elementwise passes, one tile x 4 channels per thread, coalesced along the channel.
// work item `it` of an input transform -> (tile t = (n, ty, tx), channel vector cv of CV per pixel)
__device__ __forceinline__ void wino_item(long long it, int CV, int Th, int Tw, int &cv, long long &t, int &tx, int &ty, int &n)
{
    cv = (int)(it % CV);
    t = it / CV;
    tx = (int)(t % Tw);
    ty = (int)((t / Tw) % Th);
    n = (int)(t / ((long long)Tw * Th));
}

__global__ __launch_bounds__(256)
void wino_in_kernel(const float *__restrict__ in, float *__restrict__ V, int B, int H, int W, int C, int ldIn, int Th, int Tw)
{
    const int C4 = C >> 2;
    const long long T = (long long)B * Th * Tw;
    const long long items = T * C4;
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long long)gridDim.x * 256) {
        int c4, tx, ty, n;
        long long t;
        wino_item(it, C4, Th, Tw, c4, t, tx, ty, n);
        f32x4 d[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int y = 2 * ty - 1 + a;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int x = 2 * tx - 1 + b;
                if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W)
                    d[a][b] = *reinterpret_cast<const f32x4 *>(in + (((long long)n * H + y) * W + x) * ldIn + 4 * c4);
                else
                    d[a][b] = f32x4{ 0.f, 0.f, 0.f, 0.f };
            }
        }
        f32x4 w[4][4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            w[0][b] = d[0][b] - d[2][b];
            w[1][b] = d[1][b] + d[2][b];
            w[2][b] = d[2][b] - d[1][b];
            w[3][b] = d[1][b] - d[3][b];
        }
        float *o = V + t * C + 4 * c4;
        const long long zs = T * C;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<f32x4 *>(o + (4 * i + 0) * zs) = w[i][0] - w[i][2];
            *reinterpret_cast<f32x4 *>(o + (4 * i + 1) * zs) = w[i][1] + w[i][2];
            *reinterpret_cast<f32x4 *>(o + (4 * i + 2) * zs) = w[i][2] - w[i][1];
            *reinterpret_cast<f32x4 *>(o + (4 * i + 3) * zs) = w[i][1] - w[i][3];
        }
    }
}

// grid (nchunks, B): block k of image n transforms tiles [k*tpb, (k+1)*tpb) and writes the fp64 GroupNorm partial sums
// of what it produced to stats[n][k][g] (fixed order: tiles per thread, then the S tile lanes, then the channels of
// the group).  256 threads = S tile lanes x C/4 channel quads.
__global__ __launch_bounds__(256)
void wino_out_kernel(const float *__restrict__ M, const float *__restrict__ bias, float *__restrict__ out,
                     double *__restrict__ stats, int B, int H, int W, int C, int ldOut, int Th, int Tw, int tpb,
                     int G, int nchunks)
{
    __shared__ double sS[256 * 8];
    const int tid = threadIdx.x;
    const int C4 = C >> 2, S = 256 / C4;
    const int c4 = tid % C4, sub = tid / C4;
    const int n = blockIdx.y, k = blockIdx.x;
    const int Timg = Th * Tw;
    const long long T = (long long)B * Timg;
    const long long zs = T * C;
    int t1 = (k + 1) * tpb; if (t1 > Timg) t1 = Timg;
    f32x4 bv = f32x4{ 0.f, 0.f, 0.f, 0.f };
    if (bias) bv = *reinterpret_cast<const f32x4 *>(bias + 4 * c4);
    f32x4 s1 = f32x4{ 0.f, 0.f, 0.f, 0.f }, s2 = f32x4{ 0.f, 0.f, 0.f, 0.f };
    for (int tl = k * tpb + sub; tl < t1; tl += S) {
        const int ty = tl / Tw, tx = tl - ty * Tw;
        const float *m = M + ((long long)n * Timg + tl) * C + 4 * c4;
        f32x4 r[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) r[i][j] = *reinterpret_cast<const f32x4 *>(m + (4 * i + j) * zs);
        f32x4 q[2][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            q[0][j] = r[0][j] + r[1][j] + r[2][j];
            q[1][j] = r[1][j] - r[2][j] - r[3][j];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const f32x4 y0 = q[i][0] + q[i][1] + q[i][2] + bv;
            const f32x4 y1 = q[i][1] - q[i][2] - q[i][3] + bv;
            float *o = out + (((long long)n * H + 2 * ty + i) * W + 2 * tx) * ldOut + 4 * c4;
            *reinterpret_cast<f32x4 *>(o) = y0;
            *reinterpret_cast<f32x4 *>(o + ldOut) = y1;
            s1 += y0; s1 += y1;
            s2 += y0 * y0; s2 += y1 * y1;
        }
    }
    if (!stats) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) { sS[tid * 8 + e] = (double)s1[e]; sS[tid * 8 + 4 + e] = (double)s2[e]; }
    __syncthreads();
    if (tid < G) {
        const int cpg = C / G;
        double a = 0.0, b = 0.0;
        for (int sb = 0; sb < S; ++sb)
            for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) {
                const int th = sb * C4 + (c >> 2);
                a += sS[th * 8 + (c & 3)];
                b += sS[th * 8 + 4 + (c & 3)];
            }
        double *o = stats + (((long long)n * nchunks + k) * G + tid) * 2;
        o[0] = a; o[1] = b;
    }
}

// F(4x4, 3x3): 36 multiplies per 4x4 output tile and (ci, co) pair instead of 144 (Lavin & Gray 2016, interpolation
// points 0, +-1, +-2, inf).  6x6 input patches at stride 4; H and W need not be multiples of 4 (partial tiles read zeros
// and their surplus outputs are neither stored nor counted).  Same launch structure as the F(2x2,3x3) pair.
template <typename V>
__device__ __forceinline__ void wino4_bt(const V (&d)[6], V (&o)[6])
{
    o[0] = 4.f * d[0] - 5.f * d[2] + d[4];
    o[1] = -4.f * d[1] - 4.f * d[2] + d[3] + d[4];
    o[2] = 4.f * d[1] - 4.f * d[2] - d[3] + d[4];
    o[3] = -2.f * d[1] - d[2] + 2.f * d[3] + d[4];
    o[4] = 2.f * d[1] - d[2] - 2.f * d[3] + d[4];
    o[5] = 4.f * d[1] - 5.f * d[3] + d[5];
}

template <typename V>
__device__ __forceinline__ void wino4_at(const V (&m)[6], V (&o)[4])
{
    o[0] = m[0] + m[1] + m[2] + m[3] + m[4];
    o[1] = m[1] - m[2] + 2.f * m[3] - 2.f * m[4];
    o[2] = m[1] + m[2] + 4.f * m[3] + 4.f * m[4];
    o[3] = m[1] - m[2] + 8.f * m[3] - 8.f * m[4] + m[5];
}

// one tile x 2 channels per thread
// DEFER: 0 = plain gather; 1 / 2 = the producer's GroupNorm (x*scale + shift; 2: + ReLU) is applied while gathering.
// The deferred form loads through clamped addresses and masks afterwards: a use inside the bounds branch would put a
// vmcnt(0) after every load and serialise the 36 gathers of a tile.
template <int DEFER>
__global__ __launch_bounds__(256)
void wino4_in_kernel(const float *__restrict__ in, float *__restrict__ V, int B, int H, int W, int C, int ldIn, int Th, int Tw,
                     const float *__restrict__ coeff)
{
    const int C2 = C >> 1;
    const long long T = (long long)B * Th * Tw;
    const long long items = T * C2;
    const long long zs = T * C;
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long long)gridDim.x * 256) {
        int c2, tx, ty, n;
        long long t;
        wino_item(it, C2, Th, Tw, c2, t, tx, ty, n);
        // deferred GroupNorm of the producer: x*scale + shift (+ReLU) applied to the pixels as they are gathered
        f32x4 ss = f32x4{ 1.f, 0.f, 1.f, 0.f };
        if (DEFER) ss = *reinterpret_cast<const f32x4 *>(coeff + ((long long)n * C + 2 * c2) * 2);
        f32x2 w[6][6];                               // w[i][b] = (B^T d)[i][b]
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const int x = 4 * tx - 1 + b;
            f32x2 col[6], o[6];
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const int y = 4 * ty - 1 + a;
                if (DEFER) {
                    const int yc = min(max(y, 0), H - 1), xc = min(max(x, 0), W - 1);
                    col[a] = *reinterpret_cast<const f32x2 *>(in + (((long long)n * H + yc) * W + xc) * ldIn + 2 * c2);
                } else if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W)
                    col[a] = *reinterpret_cast<const f32x2 *>(in + (((long long)n * H + y) * W + x) * ldIn + 2 * c2);
                else
                    col[a] = f32x2{ 0.f, 0.f };
            }
            if (DEFER) {
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    const int y = 4 * ty - 1 + a;
                    const bool inb = ((unsigned)y < (unsigned)H) & ((unsigned)x < (unsigned)W);
                    float v0 = fmaf(col[a][0], ss[0], ss[1]), v1 = fmaf(col[a][1], ss[2], ss[3]);   // one rounding, as every apply site
                    if (DEFER == 2) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
                    col[a] = f32x2{ inb ? v0 : 0.f, inb ? v1 : 0.f };
                }
            }
            wino4_bt(col, o);
#pragma unroll
            for (int i = 0; i < 6; ++i) w[i][b] = o[i];
        }
        float *op = V + t * C + 2 * c2;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            f32x2 o[6];
            wino4_bt(w[i], o);
#pragma unroll
            for (int j = 0; j < 6; ++j) *reinterpret_cast<f32x2 *>(op + (6 * i + j) * zs) = o[j];
        }
    }
}

// grid (nchunks, B); 256 threads = S tile lanes x C/2 channel pairs... C/2 may exceed 256: a block covers CB = min(C, 512)
// channels and blockIdx.z walks the channel blocks.  Statistics: one fp64 partial per (image, chunk, group).
__global__ __launch_bounds__(256)
void wino4_out_kernel(const float *__restrict__ M, const float *__restrict__ bias, float *__restrict__ out,
                      double *__restrict__ stats, int B, int H, int W, int C, int ldOut, int Th, int Tw, int tpb,
                      int G, int nchunks, int accumulate)
{
    __shared__ double sS[256 * 4];
    const int tid = threadIdx.x;
    const int CB = C < 512 ? C : 512;                 // channels per block
    const int C2 = CB >> 1, S = 256 / C2;
    const int cb0 = blockIdx.z * CB;
    const int c2 = tid % C2, sub = tid / C2;
    const int cch = cb0 + 2 * c2;                      // first of this thread's two channels
    const int n = blockIdx.y, k = blockIdx.x;
    const int Timg = Th * Tw;
    const long long T = (long long)B * Timg;
    const long long zs = T * C;
    int t1 = (k + 1) * tpb; if (t1 > Timg) t1 = Timg;
    f32x2 bv = f32x2{ 0.f, 0.f };
    if (bias) bv = *reinterpret_cast<const f32x2 *>(bias + cch);
    f32x2 s1 = f32x2{ 0.f, 0.f }, s2 = f32x2{ 0.f, 0.f };
    for (int tl = k * tpb + sub; tl < t1; tl += S) {
        const int ty = tl / Tw, tx = tl - ty * Tw;
        const float *m = M + ((long long)n * Timg + tl) * C + cch;
        f32x2 q[4][6];                               // q[p][j] = (A^T r)[p][j]
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            f32x2 col[6], o[4];
#pragma unroll
            for (int i = 0; i < 6; ++i) col[i] = *reinterpret_cast<const f32x2 *>(m + (6 * i + j) * zs);
            wino4_at(col, o);
#pragma unroll
            for (int pI = 0; pI < 4; ++pI) q[pI][j] = o[pI];
        }
#pragma unroll
        for (int pI = 0; pI < 4; ++pI) {
            f32x2 y[4];
            wino4_at(q[pI], y);
            const int oy = 4 * ty + pI;
            if (oy >= H) continue;
#pragma unroll
            for (int qI = 0; qI < 4; ++qI) {
                const int ox = 4 * tx + qI;
                if (ox >= W) continue;
                f32x2 v = y[qI] + bv;
                f32x2 *dst = reinterpret_cast<f32x2 *>(out + (((long long)n * H + oy) * W + ox) * ldOut + cch);
                if (accumulate) v += *dst;                     // data gradients: second producer of a gradient tensor
                *dst = v;
                s1 += v; s2 += v * v;
            }
        }
    }
    if (!stats) return;
    sS[tid * 4 + 0] = (double)s1[0]; sS[tid * 4 + 1] = (double)s1[1];
    sS[tid * 4 + 2] = (double)s2[0]; sS[tid * 4 + 3] = (double)s2[1];
    __syncthreads();
    const int cpg = C / G;
    const int gPerBlock = CB / cpg;                    // groups whose channels all live in this block
    if (tid < gPerBlock) {
        double a = 0.0, b = 0.0;
        for (int sb = 0; sb < S; ++sb)
            for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) {
                const int th = sb * C2 + (c >> 1);
                a += sS[th * 4 + (c & 1)];
                b += sS[th * 4 + 2 + (c & 1)];
            }
        const int g = cb0 / cpg + tid;
        double *o = stats + (((long long)n * nchunks + k) * G + g) * 2;
        o[0] = a; o[1] = b;
    }
}

// F(6x6, 3x3): 64 multiplies per 6x6 output tile and (ci, co) pair instead of 324 (5.06x fewer than the direct form,
// 1.27x fewer than F(4x4,3x3)); interpolation points 0, +-1, +-2, +-1/2, inf with the scaling of Lavin's wincnn set.
// Weights are transformed in float64 on the host side; measured error of a 256-channel layer against a float64
// convolution: 1.6e-5 of max|ref| (F(4x4,3x3): 1.2e-5, direct fp32: 2e-7).  8x8 input patches at stride 6; partial tiles
// as in the F(4x4,3x3) kernels.  Inference plans only.
template <typename V>
__device__ __forceinline__ void wino6_bt(const V (&d)[8], V (&o)[8])
{
    const V a = d[2] + d[6] - 4.25f * d[4], b = d[1] + d[5] - 4.25f * d[3];
    const V c = d[6] + 0.25f * d[2] - 1.25f * d[4], e = 0.5f * d[1] - 2.5f * d[3] + 2.f * d[5];
    const V f = d[6] + 4.f * d[2] - 5.f * d[4], g = 2.f * d[1] - 2.5f * d[3] + 0.5f * d[5];
    o[0] = d[0] - d[6] + 5.25f * (d[4] - d[2]);
    o[1] = a + b; o[2] = a - b;
    o[3] = c + e; o[4] = c - e;
    o[5] = f + g; o[6] = f - g;
    o[7] = d[7] - d[1] + 5.25f * (d[3] - d[5]);
}

template <typename V>
__device__ __forceinline__ void wino6_at(const V (&m)[8], V (&o)[6])
{
    const V s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
    const V s56 = m[5] + m[6], d56 = m[5] - m[6];
    o[0] = m[0] + s12 + s34 + 32.f * s56;
    o[1] = d12 + 2.f * d34 + 16.f * d56;
    o[2] = s12 + 4.f * s34 + 8.f * s56;
    o[3] = d12 + 8.f * d34 + 4.f * d56;
    o[4] = s12 + 16.f * s34 + 2.f * s56;
    o[5] = d12 + 32.f * d34 + d56 + m[7];
}

// The row transform of a tile accumulated column by column, for the forms that cannot hold the 6x8 intermediate:
// y[p][.] += (A^T)[., j] * o[p] with o = A^T (column j of the frequency block); j is a constant after unrolling.
template <typename V>
__device__ __forceinline__ void wino6_at_column(V (&y)[6][6], const V (&o)[6], int j)
{
    constexpr float AT[8][6] = { { 1.f, 0.f, 0.f, 0.f, 0.f, 0.f }, { 1.f, 1.f, 1.f, 1.f, 1.f, 1.f },
                                 { 1.f, -1.f, 1.f, -1.f, 1.f, -1.f }, { 1.f, 2.f, 4.f, 8.f, 16.f, 32.f },
                                 { 1.f, -2.f, 4.f, -8.f, 16.f, -32.f }, { 32.f, 16.f, 8.f, 4.f, 2.f, 1.f },
                                 { 32.f, -16.f, 8.f, -4.f, 2.f, -1.f }, { 0.f, 0.f, 0.f, 0.f, 0.f, 1.f } };
#pragma unroll
    for (int pI = 0; pI < 6; ++pI)
#pragma unroll
        for (int qI = 0; qI < 6; ++qI)
            if (AT[j][qI] != 0.f) y[pI][qI] += AT[j][qI] * o[pI];
}

// one tile x 2 channels per thread; DEFER as in wino4_in_kernel.  SPLIT: V is written as three bf16 planes
// ([plane][64][tiles][C], the operand form of csrc/xl_gemm_split.hip) instead of fp32.
// The interleaved-plane forms are held to 168 VGPRs = three waves per SIMD (the deferred one would take 178 and runs 20 %
// slower at two waves: 413 vs 346 us per 512-channel launch; at 168 it keeps 5 values in scratch and takes 364).
// FOLD (with DEFER = 1): `in` is the RAW output of a convolution whose GroupNorm(+ReLU, +residual, +ReLU) apply pass was not
// run: every in-image pixel becomes v = relu_out(relu_in(fmaf(x, scale, shift)) + res) on load (the arithmetic of
// gn_apply_kernel, flags as XL_GN_*), and the thread that owns a pixel - the tile whose 6 x 6 output footprint contains it -
// also writes v to `side`: the activation is materialised for its other consumers (the residual branch) by the pass that had
// to read it anyway.  `side` must not alias `in` or `res` (other tiles read their halo pixels from those).
// resCoef: the residual is itself the RAW output of a convolution whose GroupNorm + ReLU apply was deferred (its only consumer is
// this addition): {scale, shift} pairs like `coeff`, applied with ReLU while the residual is read.
struct WinoFold { const float *res; float *side; int ldRes, ldSide, flags; const float *resCoef; };

template <int DEFER, int SPLIT = 0, int FOLD = 0>
__global__ __launch_bounds__(256, (SPLIT == 2 ? 3 : 1))
void wino6_in_kernel(const float *__restrict__ in, float *__restrict__ V, int B, int H, int W, int C, int ldIn, int Th, int Tw,
                     const float *__restrict__ coeff, WinoFold fold, const float *__restrict__ pairScale)
{
    static_assert(!FOLD || DEFER == 1, "the fold form takes its ReLU / residual flags at run time");
    const int C2 = C >> 1;
    const long long T = (long long)B * Th * Tw;
    const long long items = T * C2;
    const long long zs = T * C;
    for (long long it = (long long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long long)gridDim.x * 256) {
        const int c2 = (int)(it % C2);
        const long long t = it / C2;
        const int tx = (int)(t % Tw);
        const int ty = (int)((t / Tw) % Th);
        const int n = (int)(t / ((long long)Tw * Th));
        f32x4 ss = f32x4{ 1.f, 0.f, 1.f, 0.f };
        if (DEFER) ss = *reinterpret_cast<const f32x4 *>(coeff + ((long long)n * C + 2 * c2) * 2);
        f32x4 rs = f32x4{ 1.f, 0.f, 1.f, 0.f };
        if constexpr (FOLD != 0) {
            if (fold.resCoef) rs = *reinterpret_cast<const f32x4 *>(fold.resCoef + ((long long)n * C + 2 * c2) * 2);
        }
        f32x2 w[8][8];                               // w[i][b] = (B^T d)[i][b]
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int x = 6 * tx - 1 + b;
            f32x2 col[8], o[8];
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                const int y = 6 * ty - 1 + a;
                if (DEFER) {
                    const int yc = min(max(y, 0), H - 1), xc = min(max(x, 0), W - 1);
                    col[a] = *reinterpret_cast<const f32x2 *>(in + (((long long)n * H + yc) * W + xc) * ldIn + 2 * c2);
                } else if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W)
                    col[a] = *reinterpret_cast<const f32x2 *>(in + (((long long)n * H + y) * W + x) * ldIn + 2 * c2);
                else
                    col[a] = f32x2{ 0.f, 0.f };
            }
            if (DEFER) {
                f32x2 rcol[8];
                if constexpr (FOLD != 0) {
                    if (fold.res) {
#pragma unroll
                        for (int a = 0; a < 8; ++a) {
                            const int yc = min(max(6 * ty - 1 + a, 0), H - 1), xc = min(max(x, 0), W - 1);
                            rcol[a] = *reinterpret_cast<const f32x2 *>(fold.res + (((long long)n * H + yc) * W + xc) * fold.ldRes + 2 * c2);
                        }
                        if (fold.resCoef) {                  // the residual's own deferred GroupNorm + ReLU (gn_apply's arithmetic)
#pragma unroll
                            for (int a = 0; a < 8; ++a)
                                rcol[a] = f32x2{ fmaxf(fmaf(rcol[a][0], rs[0], rs[1]), 0.f), fmaxf(fmaf(rcol[a][1], rs[2], rs[3]), 0.f) };
                        }
                    }
                }
#pragma unroll
                for (int a = 0; a < 8; ++a) {
                    const int y = 6 * ty - 1 + a;
                    const bool inb = ((unsigned)y < (unsigned)H) & ((unsigned)x < (unsigned)W);
                    float v0 = fmaf(col[a][0], ss[0], ss[1]), v1 = fmaf(col[a][1], ss[2], ss[3]);   // one rounding, as every apply site
                    if (DEFER == 2) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
                    if constexpr (FOLD != 0) {
                        if (fold.flags & XL_GN_RELU_IN) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
                        if (fold.res) { v0 += rcol[a][0]; v1 += rcol[a][1]; }
                        if (fold.flags & XL_GN_RELU_OUT) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
                        if (inb && a >= 1 && a <= 6 && b >= 1 && b <= 6)
                            *reinterpret_cast<f32x2 *>(fold.side + (((long long)n * H + y) * W + x) * fold.ldSide + 2 * c2) = f32x2{ v0, v1 };
                    }
                    col[a] = f32x2{ inb ? v0 : 0.f, inb ? v1 : 0.f };
                }
            }
            wino6_bt(col, o);
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i][b] = o[i];
        }
        if constexpr (SPLIT == 2) {
            // interleaved planes (256 x 256 split GEMM): V[xi][t][c / 16][plane][c % 16] bf16.  The 64 lanes of a wave hold
            // 128 consecutive channels of one tile = 8 chunks = one contiguous 768-byte piece per frequency, but a lane's
            // three words (its channel pair in the three planes) lie 32 bytes apart.  They are exchanged through a
            // wave-private LDS row so that every lane stores 12 contiguous bytes: one dwordx3 store instead of three
            // scattered dword stores per frequency (C % 128 == 0 and whole waves: checked by the launcher).
            __shared__ unsigned sX[4][2][192];
            const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
            const int c = 2 * c2;
            unsigned *op = reinterpret_cast<unsigned *>(V) + ((t * (C >> 4) + ((c - 2 * lane) >> 4)) * 48 >> 1) + 3 * lane;
            const long long zw = (zs * 3) >> 1;                                           // words per frequency
            const int wr = (lane >> 3) * 24 + (lane & 7);                                 // chunk, pair within the chunk
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                f32x2 o[8];
                wino6_bt(w[i], o);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    unsigned a1, a2, a3, b1, b2, b3;
                    xl_bf16_split3(o[j][0], a1, a2, a3);
                    xl_bf16_split3(o[j][1], b1, b2, b3);
                    unsigned *row = sX[wv][j & 1];
                    row[wr] = a1 | (b1 << 16); row[wr + 8] = a2 | (b2 << 16); row[wr + 16] = a3 | (b3 << 16);
                    const u32x3 v3 = u32x3{ row[3 * lane], row[3 * lane + 1], row[3 * lane + 2] };
                    *reinterpret_cast<u32x3 *>(op + (8 * i + j) * zw) = v3;
                }
            }
            continue;
        }
        if constexpr (SPLIT == 3) {
            // fp16 pairs (round 5, XL_CONV_PAIR_F16, csrc/xl_gemm_pair.hip): V[xi][t][c / 8][2][8] fp16 = {hi, (v - hi) 2^11} of
            // v = V * scale - a 16-byte slot of hi then one of lo' per 8 channels, so a K-step of 16 channels is the four slots
            // hi(k 0-7) lo'(k 0-7) hi(k 8-15) lo'(k 8-15).  A row is C words of 4 bytes like the fp32 form, and the four lanes
            // that hold 8 consecutive channels own the 32 bytes of their chunk: a lane's two words (hi and lo' of its channel pair)
            // are exchanged inside the QUAD on the DPP path - neighbours trade one word (even lanes collect the hi pair, odd lanes
            // the lo' pair), then lanes 1 and 2 swap - so that lane q stores bytes 8 q .. 8 q + 7: the same dwordx2 store, at the
            // same address, as the fp32 form.  (Through a wave-private LDS row instead: 0.60 / 1.07 ms per 512-channel launch at 95
            // frames, plain / fold form, against 0.51 / 0.83 for fp32.)
            const float sc = pairScale[0];
            const bool odd = (threadIdx.x & 1) != 0, mid = ((threadIdx.x + 1) & 2) != 0;      // lanes 1 and 2 of a quad
            unsigned *op = reinterpret_cast<unsigned *>(V) + t * C + 2 * c2;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                f32x2 o[8];
                wino6_bt(w[i], o);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    f16x2 h, l;
                    xl_f16_pair_scaled_pk(o[j] * sc, h, l);
                    const int H = __builtin_bit_cast(int, h), L = __builtin_bit_cast(int, l);
                    const int recv = __builtin_amdgcn_update_dpp(0, odd ? H : L, 0xB1, 0xF, 0xF, false);      // quad_perm [1,0,3,2]
                    int p0 = odd ? recv : H, p1 = odd ? L : recv;                 // even lanes: (hi, hi'), odd lanes: (lo', lo'')
                    const int s0 = __builtin_amdgcn_update_dpp(0, p0, 0xD8, 0xF, 0xF, false);                 // quad_perm [0,2,1,3]
                    const int s1 = __builtin_amdgcn_update_dpp(0, p1, 0xD8, 0xF, 0xF, false);
                    p0 = mid ? s0 : p0; p1 = mid ? s1 : p1;
                    *reinterpret_cast<u32x2 *>(op + (8 * i + j) * zs) = u32x2{ (unsigned)p0, (unsigned)p1 };
                }
            }
            continue;
        }
        if (SPLIT) {
            unsigned *op = reinterpret_cast<unsigned *>(V) + ((t * C + 2 * c2) >> 1);      // 2 bf16 per 32-bit word
            const long long plane = (64 * zs) >> 1;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                f32x2 o[8];
                wino6_bt(w[i], o);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    unsigned a1, a2, a3, b1, b2, b3;
                    xl_bf16_split3(o[j][0], a1, a2, a3);
                    xl_bf16_split3(o[j][1], b1, b2, b3);
                    unsigned *q = op + (((8 * i + j) * zs) >> 1);
                    q[0] = a1 | (b1 << 16); q[plane] = a2 | (b2 << 16); q[2 * plane] = a3 | (b3 << 16);
                }
            }
            continue;
        }
        float *op = V + t * C + 2 * c2;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            f32x2 o[8];
            wino6_bt(w[i], o);
#pragma unroll
            for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x2 *>(op + (8 * i + j) * zs) = o[j];
        }
    }
}

// grid (nchunks, B, C / CB), as wino4_out_kernel: M [64][B*Th*Tw][C] -> out [B,H,W,C] + bias + GroupNorm partial sums.
// VW channels per thread.  VW = 1: the factored transform on a 6x8 intermediate, one dword per lane and access.
// VW = 2 (channel counts that are multiples of 512): 8-byte accesses through a buffer descriptor with scalar plane
// offsets and a column-accumulated row transform - the factored form with two channels needs more than 256 VGPRs.
template <int VW> struct WinoVec { typedef float type; };
template <> struct WinoVec<2> { typedef f32x2 type; };
__device__ __forceinline__ float wino_lane(const float &v, int) { return v; }
__device__ __forceinline__ float wino_lane(const f32x2 &v, int i) { return v[i]; }

template <int VW>
__global__ __launch_bounds__(256)
void wino6_out_kernel(const float *__restrict__ M, const float *__restrict__ bias, float *__restrict__ out,
                      double *__restrict__ stats, int B, int H, int W, int C, int ldOut, int Th, int Tw, int tpb,
                      int G, int nchunks, int accumulate, int tileMajor)
{
    typedef typename WinoVec<VW>::type V;
    __shared__ double sS[256 * 2 * VW];
    const int tid = threadIdx.x;
    const int CB = C < 256 * VW ? C : 256 * VW;       // channels per block
    const int CV = CB / VW, S = 256 / CV;
    const int cb0 = blockIdx.z * CB;
    const int cv = tid % CV, sub = tid / CV;
    const int cch = cb0 + VW * cv;                     // first of this thread's channels
    const int n = blockIdx.y, k = blockIdx.x;
    const int Timg = Th * Tw;
    const long long T = (long long)B * Timg;
    // M is [64][tiles][C] (plane-major: what the fp32 GEMMs write) or - tileMajor, XL_CONV_M_TILE_MAJOR - [tiles][64][C]: the
    // 64 x C block of a tile is then ONE contiguous piece (128 KB at 512 channels) instead of 64 rows 14 MB apart
    const long long zs = tileMajor ? (long long)C : T * C;            // elements between frequency planes
    const long long ts = tileMajor ? 64LL * C : (long long)C;         // ... between tiles
    int t1 = (k + 1) * tpb; if (t1 > Timg) t1 = Timg;
    V bv = V(0.f);
    if (bias) bv = *reinterpret_cast<const V *>(bias + cch);
    V s1 = V(0.f), s2 = V(0.f);
    const __amdgpu_buffer_rsrc_t srdM = __builtin_amdgcn_make_buffer_rsrc((void *)M, 0, (int)(unsigned)(64 * T * C * 4 > 0xffffffffLL ? 0xffffffffLL : 64 * T * C * 4), 0x00020000);
    // VW = 2: the first frequency column of a tile is fetched while the tile BEFORE it is still being reduced and stored (round
    // 4): without that every tile started with an empty memory pipeline - 8 loads issued, one full HBM latency waited - and the
    // 36 stores of a tile went out with no read in flight behind them.
    const unsigned zsB = (unsigned)(zs * 4);
    auto tile_off = [&](int tl) { return (unsigned)(((long long)n * Timg + tl) * ts + cch) * 4u; };
    auto ldp = [&](unsigned vo, int plane) {
        // frequency planes through one buffer descriptor: the lane part of the address is ONE VGPR and the plane offset a
        // scalar (with flat pointers the compiler keeps 64 loop-invariant 64-bit addresses in registers)
        return __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(srdM, (int)vo, (int)(plane * zsB), 0));
    };
    f32x2 colN[8];
    if constexpr (VW == 2) {
        if (k * tpb + sub < t1) {
            const unsigned vo0 = tile_off(k * tpb + sub);
#pragma unroll
            for (int i = 0; i < 8; ++i) colN[i] = ldp(vo0, 8 * i);
        }
    }
    for (int tl = k * tpb + sub; tl < t1; tl += S) {
        const int ty = tl / Tw, tx = tl - ty * Tw;
        const float *m = M + ((long long)n * Timg + tl) * ts + cch;
        if constexpr (VW == 1) {
            V q[6][8];                               // q[p][j] = (A^T r)[p][j]
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                V col[8], o[6];
#pragma unroll
                for (int i = 0; i < 8; ++i) col[i] = *reinterpret_cast<const V *>(m + (8 * i + j) * zs);
                wino6_at(col, o);
#pragma unroll
                for (int pI = 0; pI < 6; ++pI) q[pI][j] = o[pI];
            }
#pragma unroll
            for (int pI = 0; pI < 6; ++pI) {
                V y[6];
                wino6_at(q[pI], y);
                const int oy = 6 * ty + pI;
                if (oy >= H) continue;
#pragma unroll
                for (int qI = 0; qI < 6; ++qI) {
                    const int ox = 6 * tx + qI;
                    if (ox >= W) continue;
                    V v = y[qI] + bv;
                    V *dst = reinterpret_cast<V *>(out + (((long long)n * H + oy) * W + ox) * ldOut + cch);
                    if (accumulate) v += *dst;                     // data gradients: second producer of a gradient tensor
                    *dst = v;
                    s1 += v; s2 += v * v;
                }
            }
        } else {
            // Two channels per lane: 8-byte accesses (a dword per lane caps the streaming rate of this pass near 4.5 TB/s).
            // The 6x8 intermediate of the factored form does not fit beside 16-byte-wide columns in flight, so the row
            // transform is accumulated column by column: y[p][.] += (A^T)[., j] * (A^T col_j)[p]; 36 accumulators, one
            // column being reduced and one in flight.
            V y[6][6];
#pragma unroll
            for (int pI = 0; pI < 6; ++pI)
#pragma unroll
                for (int qI = 0; qI < 6; ++qI) y[pI][qI] = bv;
            const unsigned vo = tile_off(tl);
            // the tile after this one (behind the last tile: this tile's own first column again - a valid address, L2 hits)
            const unsigned voNext = tile_off(tl + S < t1 ? tl + S : tl);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                V col[8], o[6];
#pragma unroll
                for (int i = 0; i < 8; ++i) col[i] = colN[i];
#pragma unroll
                for (int i = 0; i < 8; ++i) colN[i] = j + 1 < 8 ? ldp(vo, 8 * i + j + 1) : ldp(voNext, 8 * i);
                __builtin_amdgcn_sched_barrier(0);
                wino6_at(col, o);
                wino6_at_column(y, o, j);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int pI = 0; pI < 6; ++pI) {
                const int oy = 6 * ty + pI;
                if (oy >= H) continue;
#pragma unroll
                for (int qI = 0; qI < 6; ++qI) {
                    const int ox = 6 * tx + qI;
                    if (ox >= W) continue;
                    V v = y[pI][qI];
                    V *dst = reinterpret_cast<V *>(out + (((long long)n * H + oy) * W + ox) * ldOut + cch);
                    if (accumulate) v += *dst;
                    *dst = v;
                    s1 += v; s2 += v * v;
                }
            }
        }
    }
    if (!stats) return;
    const int cpg = C / G;
    const int lpg = cpg / VW;                          // lanes that hold one group
    if (S == 1 && lpg >= 1 && lpg <= 64 && (lpg & (lpg - 1)) == 0 && cpg == lpg * VW) {
        // every channel of the block lives in exactly one thread and a group in lpg neighbouring lanes of one wave: fp64
        // butterfly over those lanes (fixed order), one writer per (image, chunk, group) - no LDS, no barrier.  (The LDS
        // form below reads 16 doubles per group at a 256-byte lane stride: 32-way bank conflicts at the tail of every block.)
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int e = 0; e < VW; ++e) { a += (double)wino_lane(s1, e); b += (double)wino_lane(s2, e); }
        for (int off = 1; off < lpg; off <<= 1) { a += __shfl_xor(a, off, 64); b += __shfl_xor(b, off, 64); }
        if ((tid & (lpg - 1)) == 0) {
            double *o = stats + (((long long)n * nchunks + k) * G + cch / cpg) * 2;
            o[0] = a; o[1] = b;
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < VW; ++e) {
        sS[(tid * VW + e) * 2] = (double)wino_lane(s1, e);
        sS[(tid * VW + e) * 2 + 1] = (double)wino_lane(s2, e);
    }
    __syncthreads();
    const int gPerBlock = CB / cpg;                    // groups whose channels all live in this block
    if (tid < gPerBlock) {
        double a = 0.0, b = 0.0;
        for (int sb = 0; sb < S; ++sb)
            for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) {
                const int th = sb * CV + c / VW;
                a += sS[(th * VW + c % VW) * 2];
                b += sS[(th * VW + c % VW) * 2 + 1];
            }
        const int g = cb0 / cpg + tid;
        double *o = stats + (((long long)n * nchunks + k) * G + g) * 2;
        o[0] = a; o[1] = b;
    }
}

// F(6x6,3x3) output transform with the product M staged through LDS by DMA (round 3).  The register form above keeps one
// column of the 8 x 8 frequency block in flight per lane (8 loads of 8 bytes): ~32 KB per CU, and the pass runs at 4.8 TB/s.
// Here every WAVE is an independent unit - one (image, chunk of `tpb` tiles, 128-channel slice) - that owns a 32 KB ring
// in LDS: the 8 columns of a tile's frequency block, 8 planes x 512 bytes each, fetched by `buffer_load ... lds` (4
// instructions per column: lanes 0-31 one plane, lanes 32-63 the next), the column of the NEXT tile refilling a slot as
// soon as the current one has been reduced: 28-32 KB in flight per wave whatever the register pressure.  A lane reads its two
// channels of a plane with one ds_read_b64 (consecutive lanes, consecutive words).  In-order vmcnt bookkeeping: younger
// than the column being waited for are the other 7 columns (28 instructions) and, from the second tile on, the 36 stores
// of the tile before - every tile issues exactly 36, out-of-image pixels fall outside the buffer descriptor.
// GroupNorm partial sums: fp64 butterfly over the lanes of a group, one writer per (image, chunk, group).
__global__ __launch_bounds__(256, 1)
void wino6_out_dma_kernel(const float *__restrict__ M, const float *__restrict__ bias, float *__restrict__ out,
                          double *__restrict__ stats, int B, int H, int W, int C, int ldOut, int Th, int Tw, int tpb,
                          int G, int nchunks, long long units, int tileMajor)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dsmW[];
    typedef __attribute__((address_space(3))) void lds_void;
    constexpr unsigned OOB = 0x80000000u;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long unit = (long long)blockIdx.x * 4 + wave;            // (image, chunk, slice), slice fastest
    if (unit >= units) return;
    const int nsl = C >> 7;
    const int slice = (int)(unit % nsl);
    const int k = (int)((unit / nsl) % nchunks);
    const int n = (int)(unit / ((long long)nsl * nchunks));
    unsigned char *ring = dsmW + wave * 32768;
    const int Timg = Th * Tw;
    const long long T = (long long)B * Timg;
    const unsigned zsB = (unsigned)((tileMajor ? (long long)C : T * C) * 4);   // bytes between frequency planes (host: M < 2 GiB)
    const long long tsB = (tileMajor ? 64LL * C : (long long)C) * 4;     // ... between tiles
    const int t0 = k * tpb;
    int t1 = t0 + tpb; if (t1 > Timg) t1 = Timg;
    const int cch = slice * 128 + 2 * lane;                              // first of this lane's two channels
    const __amdgpu_buffer_rsrc_t srdM = __builtin_amdgcn_make_buffer_rsrc((void *)M, 0, (int)(unsigned)(64ull * T * C * 4), 0x00020000);
    // lane part of a DMA address: plane parity (lane >> 5) -> +8 planes... see dma_col: planes 8 (2h + (lane >> 5)) + j
    const unsigned laneOff = (unsigned)(lane >> 5) * 8u * zsB + (unsigned)(lane & 31) * 16u + (unsigned)slice * 512u;
    auto dma_col = [&](int tl, int j) {                                  // column j of tile tl (of this image) -> ring slot j
        const unsigned vo = tl < t1 ? (unsigned)(((long long)n * Timg + tl) * tsB) + laneOff : OOB;
#pragma unroll
        for (int h = 0; h < 4; ++h)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(srdM, (lds_void *)(ring + j * 4096 + h * 1024), 16, (int)vo,
                                                     (int)((unsigned)(16 * h + j) * zsB), 0, 0);
    };
    f32x2 bv = f32x2{ 0.f, 0.f };
    if (bias) bv = *reinterpret_cast<const f32x2 *>(bias + cch);
    f32x2 s1 = f32x2{ 0.f, 0.f }, s2 = f32x2{ 0.f, 0.f };
    const long long outBytes = ((long long)B * H * W - 1) * ldOut * 4 + (long long)C * 4;
    const __amdgpu_buffer_rsrc_t srdO = __builtin_amdgcn_make_buffer_rsrc((void *)out, 0, (int)(unsigned)outBytes, 0x00020000);
#pragma unroll
    for (int j = 0; j < 8; ++j) dma_col(t0, j);
    for (int tl = t0; tl < t1; ++tl) {
        const int ty = tl / Tw, tx = tl - ty * Tw;
        f32x2 y[6][6];
#pragma unroll
        for (int pI = 0; pI < 6; ++pI)
#pragma unroll
            for (int qI = 0; qI < 6; ++qI) y[pI][qI] = bv;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            // column j has landed when at most the 28 column fetches behind it (+ the 36 stores of the tile before) remain
            if (tl == t0) __builtin_amdgcn_s_waitcnt(0x0F70 | (28 & 15) | ((28 >> 4) << 14));
            else __builtin_amdgcn_s_waitcnt(0x0F70 | (63 & 15) | ((63 >> 4) << 14));
            __builtin_amdgcn_sched_barrier(0);
            f32x2 col[8], o[6];
#pragma unroll
            for (int i = 0; i < 8; ++i) col[i] = *reinterpret_cast<const f32x2 *>(ring + j * 4096 + i * 512 + lane * 8);
            wino6_at(col, o);
            wino6_at_column(y, o, j);
            // (the reads above have returned - their values were consumed - before the slot is refilled)
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(0xC07F);                          // lgkmcnt(0)
            dma_col(tl + 1, j);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int pI = 0; pI < 6; ++pI) {
            const int oy = 6 * ty + pI;
#pragma unroll
            for (int qI = 0; qI < 6; ++qI) {
                const int ox = 6 * tx + qI;
                const bool live = (oy < H) & (ox < W);
                const f32x2 v = y[pI][qI];
                const unsigned off = live ? (unsigned)(((((long long)n * H + oy) * W + ox) * ldOut + cch) * 4) : OOB;
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), srdO, (int)off, 0, 0);
                if (live) { s1 += v; s2 += v * v; }
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);                                  // vmcnt(0): the dummy fetches behind the last tile
    if (!stats) return;
    const int cpg = C / G, lpg = cpg >> 1;                               // lanes per group (host: a power of two, 1 .. 64)
    double a = (double)s1[0] + (double)s1[1], b = (double)s2[0] + (double)s2[1];
    if (lpg == 0) {                                                      // one channel per group (never with 32 groups of >= 128 channels)
        double *o = stats + (((long long)n * nchunks + k) * G + cch) * 2;
        o[0] = (double)s1[0]; o[1] = (double)s2[0]; o[2] = (double)s1[1]; o[3] = (double)s2[1];
        return;
    }
    for (int off = 1; off < lpg; off <<= 1) { a += __shfl_xor(a, off, 64); b += __shfl_xor(b, off, 64); }
    if ((lane & (lpg - 1)) == 0) {
        double *o = stats + (((long long)n * nchunks + k) * G + cch / cpg) * 2;
        o[0] = a; o[1] = b;
    }
}

}  // namespace

int xl_run_wino_in(const xl_op &op, hipStream_t st)
{
    if (op.ksize == 6) {                    // F(6x6,3x3): Ho x Wo tiles of 6x6 outputs, partial tiles allowed
        if (op.Cin % 4 != 0 || op.ld_in % 2 != 0 || op.Ho != (op.Hi + 5) / 6 || op.Wo != (op.Wi + 5) / 6) return XL_ERR_ARG;
        const unsigned blocks6 = xl_grid((long long)op.B * op.Ho * op.Wo * (op.Cin / 2), 256, 262144);
        auto kin = !op.aux2 ? wino6_in_kernel<0> : (op.flags & XL_GN_RELU_IN) ? wino6_in_kernel<2> : wino6_in_kernel<1>;
        if (op.flags & XL_CONV_SPLIT_BF16)
            kin = !op.aux2 ? wino6_in_kernel<0, 1> : (op.flags & XL_GN_RELU_IN) ? wino6_in_kernel<2, 1> : wino6_in_kernel<1, 1>;
        if ((op.flags & XL_CONV_SPLIT_BF16) && (op.flags & XL_CONV_SPLIT_IL)) {
            if (op.Cin % 128 != 0) return XL_ERR_ARG;          // a wave = 128 consecutive channels of one tile
            kin = !op.aux2 ? wino6_in_kernel<0, 2> : (op.flags & XL_GN_RELU_IN) ? wino6_in_kernel<2, 2> : wino6_in_kernel<1, 2>;
        }
        WinoFold fold = { nullptr, nullptr, 0, 0, 0, nullptr };
        if (op.out2) {
            // fold form: aux2 = coefficients, out2 = the materialised activation (pixel stride ld_out), aux = residual
            // (pixel stride ld_aux) when XL_GN_ADD is set; flags & (XL_GN_RELU_IN | XL_GN_ADD | XL_GN_RELU_OUT);
            // w (optional) = {scale, shift} pairs of the residual's own deferred GroupNorm + ReLU
            if (!op.aux2 || op.ld_out % 2 != 0 || ((op.flags & XL_GN_ADD) && (!op.aux || op.ld_aux % 2 != 0)) ||
                op.out2 == op.in || op.out2 == op.aux) return XL_ERR_ARG;
            fold.res = (op.flags & XL_GN_ADD) ? (const float *)op.aux : nullptr;
            fold.side = (float *)op.out2; fold.ldRes = op.ld_aux; fold.ldSide = op.ld_out;
            fold.flags = op.flags & (XL_GN_RELU_IN | XL_GN_RELU_OUT);
            fold.resCoef = (op.flags & XL_GN_ADD) ? (const float *)op.w : nullptr;
            if ((op.flags & XL_CONV_SPLIT_BF16) && !(op.flags & XL_CONV_PAIR_F16)) return XL_ERR_UNSUPPORTED;   // fp32 or fp16 pairs
            kin = (op.flags & XL_CONV_PAIR_F16) ? wino6_in_kernel<1, 3, 1> : wino6_in_kernel<1, 0, 1>;
        } else if (op.flags & XL_CONV_PAIR_F16)
            kin = !op.aux2 ? wino6_in_kernel<0, 3> : (op.flags & XL_GN_RELU_IN) ? wino6_in_kernel<2, 3> : wino6_in_kernel<1, 3>;
        if ((op.flags & XL_CONV_PAIR_F16) && (!op.scale || op.Cin % 16 != 0)) return XL_ERR_ARG;       // (a quad = 8 channels of one tile)
        hipLaunchKernelGGL(kin, dim3(blocks6), dim3(256), 0, st, (const float *)op.in,
                           (float *)op.out, op.B, op.Hi, op.Wi, op.Cin, op.ld_in, op.Ho, op.Wo,
                           (const float *)op.aux2, fold, (const float *)op.scale);
        return XL_OK;
    }
    if (op.ksize == 4) {                    // F(4x4,3x3): Ho x Wo tiles of 4x4 outputs, partial tiles allowed
        if (op.Cin % 4 != 0 || op.ld_in % 2 != 0 || op.Ho != (op.Hi + 3) / 4 || op.Wo != (op.Wi + 3) / 4) return XL_ERR_ARG;
        const unsigned blocks4 = xl_grid((long long)op.B * op.Ho * op.Wo * (op.Cin / 2), 256, 262144);
        auto kin = !op.aux2 ? wino4_in_kernel<0> : (op.flags & XL_GN_RELU_IN) ? wino4_in_kernel<2> : wino4_in_kernel<1>;
        hipLaunchKernelGGL(kin, dim3(blocks4), dim3(256), 0, st, (const float *)op.in,
                           (float *)op.out, op.B, op.Hi, op.Wi, op.Cin, op.ld_in, op.Ho, op.Wo,
                           (const float *)op.aux2);
        return XL_OK;
    }
    if (op.aux2) return XL_ERR_ARG;                      // the deferred GroupNorm exists for F(4x4,3x3) only
    if (op.Cin % 4 != 0 || op.ld_in % 4 != 0 || op.Hi != 2 * op.Ho || op.Wi != 2 * op.Wo) return XL_ERR_ARG;
    const unsigned blocks = xl_grid((long long)op.B * op.Ho * op.Wo * (op.Cin / 4), 256, 262144);
    hipLaunchKernelGGL(wino_in_kernel, dim3(blocks), dim3(256), 0, st, (const float *)op.in, (float *)op.out,
                       op.B, op.Hi, op.Wi, op.Cin, op.ld_in, op.Ho, op.Wo);
    return XL_OK;
}

int xl_run_wino_out(const xl_op &op, hipStream_t st)
{
    // in: M [16][B*Th*Tw][C]; out [B,H,W,C] (Hi x Wi = output size); reserved_i = tiles per block
    if (op.ksize == 6) {
        const int Th6 = (op.Hi + 5) / 6, Tw6 = (op.Wi + 5) / 6;
        // two channels per lane where the channel count allows (3.7 -> 3.3 ms per 44-frame step); XL_WINO_OUT_VW=1: one
        static const int vw = getenv("XL_WINO_OUT_VW") ? atoi(getenv("XL_WINO_OUT_VW")) : 2;
        const bool two = vw == 2 && op.Cin % 512 == 0 && 64LL * op.B * Th6 * Tw6 * op.Cin * 4 < 0xffffffffLL;
        const int CB = two ? 512 : (op.Cin < 256 ? op.Cin : 256);
        if (op.Cin % 2 != 0 || op.Cin % CB != 0 || (256 * (two ? 2 : 1)) % CB != 0 || op.ld_out % 2 != 0 || op.reserved_i < 1 ||
            op.nchunks != (Th6 * Tw6 + op.reserved_i - 1) / op.reserved_i)
            return XL_ERR_ARG;
        if (op.stats && (op.groups < 1 || op.Cin % op.groups != 0 || CB % (op.Cin / op.groups) != 0 ||
                         CB / (op.Cin / op.groups) > 256))
            return XL_ERR_ARG;
        // round 3: M staged through LDS by DMA, one wave per (image, chunk, 128-channel slice).  Measured at 47 frames:
        // 256 channels 0.155 vs 0.174 ms for the register form with one channel per lane; 512 channels 0.29 vs 0.28 ms
        // for the two-channels-per-lane register form (both ~5.1 TB/s: bytes in flight were not what limits this
        // pass) - so the DMA form takes the layers the 8-byte register form does not cover.  XL_WINO_OUT_DMA=1: all.
        static const bool noDma = getenv("XL_WINO_OUT_NO_DMA") != nullptr;
        static const bool allDma = getenv("XL_WINO_OUT_DMA") != nullptr;
        const int cpg6 = op.groups > 0 ? op.Cin / op.groups : 2;
        const long long outB = ((long long)op.B * op.Hi * op.Wi - 1) * op.ld_out * 4 + (long long)op.Cin * 4;
        if (!noDma && (allDma || !two) && !(op.flags & XL_CONV_ACCUMULATE) && op.Cin % 128 == 0 && 64LL * op.B * Th6 * Tw6 * op.Cin * 4 < 0x7fffffffLL &&
            outB < 0x7fffffffLL && (!op.stats || (cpg6 >= 2 && cpg6 <= 128 && (cpg6 & (cpg6 - 1)) == 0 && op.Cin % op.groups == 0))) {
            static XlLdsLimit configuredDma;
            if (configuredDma.configure(reinterpret_cast<const void *>(wino6_out_dma_kernel), 131072) != XL_OK) return XL_ERR_HIP;
            const long long units = (long long)op.B * op.nchunks * (op.Cin / 128);
            hipLaunchKernelGGL(wino6_out_dma_kernel, dim3((unsigned)((units + 3) / 4)), dim3(256), 131072, st, (const float *)op.in,
                               (const float *)op.bias, (float *)op.out, (double *)op.stats, op.B, op.Hi, op.Wi, op.Cin,
                               op.ld_out, Th6, Tw6, op.reserved_i, op.groups, op.nchunks, units,
                               (op.flags & XL_CONV_M_TILE_MAJOR) ? 1 : 0);
            return XL_OK;
        }
        hipLaunchKernelGGL(two ? wino6_out_kernel<2> : wino6_out_kernel<1>, dim3(op.nchunks, op.B, op.Cin / CB), dim3(256), 0, st, (const float *)op.in,
                           (const float *)op.bias, (float *)op.out, (double *)op.stats, op.B, op.Hi, op.Wi, op.Cin,
                           op.ld_out, Th6, Tw6, op.reserved_i, op.groups, op.nchunks,
                           (op.flags & XL_CONV_ACCUMULATE) ? 1 : 0, (op.flags & XL_CONV_M_TILE_MAJOR) ? 1 : 0);
        return XL_OK;
    }
    if (op.ksize == 4) {
        if (op.flags & XL_CONV_M_TILE_MAJOR) return XL_ERR_UNSUPPORTED;
        const int Th4 = (op.Hi + 3) / 4, Tw4 = (op.Wi + 3) / 4;
        const int CB = op.Cin < 512 ? op.Cin : 512;
        if (op.Cin % 2 != 0 || op.Cin % CB != 0 || 256 % (CB / 2) != 0 || op.ld_out % 2 != 0 || op.reserved_i < 1 ||
            op.nchunks != (Th4 * Tw4 + op.reserved_i - 1) / op.reserved_i)
            return XL_ERR_ARG;
        if (op.stats && (op.groups < 1 || op.Cin % op.groups != 0 || CB % (op.Cin / op.groups) != 0 ||
                         CB / (op.Cin / op.groups) > 256))
            return XL_ERR_ARG;
        hipLaunchKernelGGL(wino4_out_kernel, dim3(op.nchunks, op.B, op.Cin / CB), dim3(256), 0, st, (const float *)op.in,
                           (const float *)op.bias, (float *)op.out, (double *)op.stats, op.B, op.Hi, op.Wi, op.Cin,
                           op.ld_out, Th4, Tw4, op.reserved_i, op.groups, op.nchunks,
                           (op.flags & XL_CONV_ACCUMULATE) ? 1 : 0);
        return XL_OK;
    }
    const int C4 = op.Cin / 4;
    if (op.Cin % 4 != 0 || C4 > 256 || 256 % C4 != 0 || op.ld_out % 4 != 0 || op.reserved_i < 1) return XL_ERR_ARG;
    const int Th = op.Hi / 2, Tw = op.Wi / 2;
    if (op.Hi != 2 * Th || op.Wi != 2 * Tw || op.nchunks != (Th * Tw + op.reserved_i - 1) / op.reserved_i) return XL_ERR_ARG;
    if (op.stats && (op.groups < 1 || op.groups > 256 || op.Cin % op.groups != 0)) return XL_ERR_ARG;
    hipLaunchKernelGGL(wino_out_kernel, dim3(op.nchunks, op.B), dim3(256), 0, st, (const float *)op.in,
                       (const float *)op.bias, (float *)op.out, (double *)op.stats, op.B, op.Hi, op.Wi, op.Cin,
                       op.ld_out, Th, Tw, op.reserved_i, op.groups, op.nchunks);
    return XL_OK;
}
