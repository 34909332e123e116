// xl_gn.hip — GroupNorm as XL_OP_GN_STATS (fp64 partial sums), XL_OP_GN_FINAL (per-channel scale / shift) and XL_OP_GN_APPLY
// (+ ReLU / residual / ReLU), and the two heads XL_OP_HEAD and XL_OP_DUC_HEAD.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "xl_launch.h"
#include "xl_operand_math.h"

namespace {

// ---------------------------------------------------------------------------------------------- GroupNorm

// grid (nchunks, B); T threads with T % (C/4) == 0.  stats[((n*nchunks + chunk)*G + g)*2 + {0,1}] = sum, sumsq
__global__ void gn_stats_kernel(const float *__restrict__ x, double *__restrict__ stats, int HW, int C, int ld,
                                int G, int nchunks)
{
    extern __shared__ __attribute__((aligned(16))) double sPart[];     // [T][8]
    const int T = blockDim.x, tid = threadIdx.x;
    const int C4 = C >> 2;
    const int c4 = tid % C4, prow = tid / C4, rows = T / C4;
    const int chunk = blockIdx.x, n = blockIdx.y;
    const int per = (HW + nchunks - 1) / nchunks;
    const int p0 = chunk * per;
    int p1 = p0 + per; if (p1 > HW) p1 = HW;
    double s[4] = { 0, 0, 0, 0 }, ss[4] = { 0, 0, 0, 0 };
    const float *base = x + ((long long)n * HW) * ld + 4 * c4;
    for (int p = p0 + prow; p < p1; p += rows) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(base + (long long)p * ld);
#pragma unroll
        for (int j = 0; j < 4; ++j) { const double d = (double)v[j]; s[j] += d; ss[j] += d * d; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { sPart[tid * 8 + j] = s[j]; sPart[tid * 8 + 4 + j] = ss[j]; }
    __syncthreads();
    if (tid < G) {
        const int cpg = C / G;
        double a = 0.0, b = 0.0;
        for (int r = 0; r < rows; ++r)
            for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) {
                const int th = r * C4 + (c >> 2), sl = c & 3;
                a += sPart[th * 8 + sl];
                b += sPart[th * 8 + 4 + sl];
            }
        double *o = stats + (((long long)n * nchunks + chunk) * G + tid) * 2;
        o[0] = a; o[1] = b;
    }
}

// per-(image, channel) scale/shift from the fp64 partial sums, fixed summation order.  grid (B, slices), 256 threads: a workgroup
// finalises G / slices consecutive groups of one image.  slices > 1 for long entry lists only (the stem: conv2 leaves 2760 entries
// per image and group, 1.4 MB that ONE workgroup read in 41 us whatever the number of loads in flight - a single CU's miss queue -
// out of a single frame's 1.46 ms); the launcher derives it from the layer's geometry, never from the batch.
__global__ __launch_bounds__(256)
void gn_final_kernel(const double *__restrict__ stats, const float *__restrict__ gamma, const float *__restrict__ beta,
                     float *__restrict__ coeff, int HW, int C, int G, int nchunks, float eps, int statTile,
                     float *__restrict__ murs, int perTile)
{
    __shared__ double sG[2 * 64];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int cpg = C / G;
    const int Gw = G / (int)gridDim.y, g0 = (int)blockIdx.y * Gw;     // this workgroup's groups
    int valid = nchunks;
    if (statTile > 0)          // statistics came from a conv epilogue: one entry per conv tile overlapping image n
        valid = (int)((((long long)(n + 1) * HW - 1) / statTile) - (((long long)n * HW) / statTile)) + 1;
    else if (statTile < 0)     // ... from a conv whose tiles start at image boundaries (batch-invariant plans)
        valid = (HW - statTile - 1) / -statTile;
    valid *= perTile;          // (the stride-2 stem convolutions write one entry per tile and row block of waves)
    // P = 256 / (G rounded up to a power of two) threads per group (8 for 32 groups, 128 for the 2 groups of conv1) each sum
    // a contiguous slice of the chunks, then the P slices are added as a fixed binary tree.  P depends on the layer only.
    __shared__ double sP[256 * 2];
    int gp = 1;
    while (gp < Gw) gp <<= 1;
    const int P = 256 / gp;
    {
        const int gl = tid / P, part = tid - gl * P, g = g0 + gl;
        double a = 0.0, b = 0.0;
        if (gl < Gw) {
            const int per = (valid + P - 1) / P;
            int k0 = part * per, k1 = k0 + per;
            if (k1 > valid) k1 = valid;
            // four interleaved partial sums (k % 4), added in order: the loads of four entries are in flight together - as
            // one dependent chain a slice of 19 entries (a single frame: 150 one-tile chunks) took ~8 us of L2 latency
            const f64x2 *st = reinterpret_cast<const f64x2 *>(stats) + ((long long)n * nchunks * G + g);
            double pa[4] = { 0.0, 0.0, 0.0, 0.0 }, pb[4] = { 0.0, 0.0, 0.0, 0.0 };
            int k = k0;
            for (; k + 4 <= k1; k += 4) {
                f64x2 v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = st[(long long)(k + e) * G];
#pragma unroll
                for (int e = 0; e < 4; ++e) { pa[e] += v[e][0]; pb[e] += v[e][1]; }
            }
            for (int e = 0; k < k1; ++k, ++e) { const f64x2 v = st[(long long)k * G]; pa[e] += v[0]; pb[e] += v[1]; }
            a = (pa[0] + pa[1]) + (pa[2] + pa[3]);
            b = (pb[0] + pb[1]) + (pb[2] + pb[3]);
        }
        sP[2 * tid] = a; sP[2 * tid + 1] = b;
        for (int s = P >> 1; s >= 1; s >>= 1) {
            __syncthreads();
            if (part < s) {
                a += sP[2 * (tid + s)]; b += sP[2 * (tid + s) + 1];
                sP[2 * tid] = a; sP[2 * tid + 1] = b;
            }
        }
    }
    __syncthreads();
    for (int g = tid; g < Gw; g += 256) {                              // (sG: indexed by the group's number within the workgroup)
        const double a = sP[2 * (g * P)], b = sP[2 * (g * P) + 1];
        const double cnt = (double)HW * (double)cpg;
        const double mean = a / cnt;
        double var = b / cnt - mean * mean;
        if (var < 0.0) var = 0.0;
        sG[2 * g] = mean; sG[2 * g + 1] = 1.0 / sqrt(var + (double)eps);
    }
    __syncthreads();
    for (int c = g0 * cpg + tid; c < (g0 + Gw) * cpg; c += 256) {
        const int g = c / cpg - g0;
        const double sc = (double)gamma[c] * sG[2 * g + 1];
        coeff[((long long)n * C + c) * 2] = (float)sc;
        coeff[((long long)n * C + c) * 2 + 1] = (float)((double)beta[c] - sG[2 * g] * sc);
        if (murs) {                                  // training plans: mean / rstd for the GroupNorm backward kernels
            murs[((long long)n * C + c) * 2] = (float)sG[2 * g];
            murs[((long long)n * C + c) * 2 + 1] = (float)sG[2 * g + 1];
        }
    }
}

// grid (achunks, B), 256 threads. v = x*scale + shift; flags as in crossloc_cnn.h
__global__ __launch_bounds__(256)
void gn_apply_kernel(const float *__restrict__ x, const double *__restrict__ stats, const float *__restrict__ gamma,
                     const float *__restrict__ beta, const float *__restrict__ aux, float *__restrict__ out,
                     int HW, int C, int ldIn, int ldOut, int ldAux, int G, int nchunks, float eps, int flags, int statTile,
                     const float *__restrict__ coeff)
{
    extern __shared__ __attribute__((aligned(16))) float sSS[];        // scale[C], shift[C]
    const int tid = threadIdx.x, n = blockIdx.y;
    const int cpg = C / G;
    if (coeff) {
        for (int c = tid; c < C; c += 256) {
            sSS[c] = coeff[((long long)n * C + c) * 2];
            sSS[C + c] = coeff[((long long)n * C + c) * 2 + 1];
        }
    } else {
    for (int c = tid; c < C; c += 256) {
        const int g = c / cpg;
        double a = 0.0, b = 0.0;
        const double *st = stats + ((long long)n * nchunks * G + g) * 2;
        int valid = nchunks;
        if (statTile > 0)      // statistics came from the conv epilogue: one entry per conv tile overlapping image n
            valid = (int)((((long long)(n + 1) * HW - 1) / statTile) - (((long long)n * HW) / statTile)) + 1;
        else if (statTile < 0) // ... tiles that start at image boundaries
            valid = (HW - statTile - 1) / -statTile;
        for (int k = 0; k < valid; ++k) { a += st[(long long)k * G * 2]; b += st[(long long)k * G * 2 + 1]; }
        const double cnt = (double)HW * (double)cpg;
        const double mean = a / cnt;
        double var = b / cnt - mean * mean;
        if (var < 0.0) var = 0.0;
        const double rstd = 1.0 / sqrt(var + (double)eps);
        const double sc = (double)gamma[c] * rstd;
        sSS[c] = (float)sc;
        sSS[C + c] = (float)((double)beta[c] - mean * sc);
    }
    }
    __syncthreads();
    const int C4 = C >> 2;
    const int achunks = gridDim.x;
    const int per = (HW + achunks - 1) / achunks;
    const int p0 = blockIdx.x * per;
    int p1 = p0 + per; if (p1 > HW) p1 = HW;
    const long long nElem4 = (long long)(p1 - p0) * C4;
    const bool reluIn = flags & XL_GN_RELU_IN, add = flags & XL_GN_ADD, reluOut = flags & XL_GN_RELU_OUT;
    if (C4 <= 256 && 256 % C4 == 0) {
        // the usual case (C = 32 ... 1024, a power of two): a thread keeps ONE channel quad - {scale, shift} in registers, no
        // 64-bit division per element - and walks the pixels, four per trip with all loads issued first (round 4).  Element by
        // element the same arithmetic as the general loop below.
        const int c = 4 * (tid % C4), rows = 256 / C4;
        const f32x4 sc = *reinterpret_cast<const f32x4 *>(sSS + c), sh = *reinterpret_cast<const f32x4 *>(sSS + C + c);
        auto one = [&](long long pix, f32x4 v, const f32x4 &r) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float t = fmaf(v[j], sc[j], sh[j]);
                if (reluIn) t = fmaxf(t, 0.f);
                if (add) t += r[j];
                if (reluOut) t = fmaxf(t, 0.f);
                v[j] = t;
            }
            *reinterpret_cast<f32x4 *>(out + pix * ldOut + c) = v;
        };
        const f32x4 zero = { 0.f, 0.f, 0.f, 0.f };
        int p = p0 + tid / C4;
        for (; p + 3 * rows < p1; p += 4 * rows) {
            f32x4 v[4], r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long pix = (long long)n * HW + p + k * rows;
                v[k] = *reinterpret_cast<const f32x4 *>(x + pix * ldIn + c);
                r[k] = add ? *reinterpret_cast<const f32x4 *>(aux + pix * ldAux + c) : zero;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) one((long long)n * HW + p + k * rows, v[k], r[k]);
        }
        for (; p < p1; p += rows) {
            const long long pix = (long long)n * HW + p;
            one(pix, *reinterpret_cast<const f32x4 *>(x + pix * ldIn + c), add ? *reinterpret_cast<const f32x4 *>(aux + pix * ldAux + c) : zero);
        }
        return;
    }
    for (long long f = tid; f < nElem4; f += 256) {
        const int p = p0 + (int)(f / C4);
        const int c = (int)(f - (long long)(p - p0) * C4) * 4;
        const long long pix = (long long)n * HW + p;
        f32x4 v = *reinterpret_cast<const f32x4 *>(x + pix * ldIn + c);
        const f32x4 sc = *reinterpret_cast<const f32x4 *>(sSS + c);
        const f32x4 sh = *reinterpret_cast<const f32x4 *>(sSS + C + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float t = fmaf(v[j], sc[j], sh[j]);       // one rounding - the same arithmetic as the consumers that apply a
                                                      // deferred GroupNorm while loading (a frame must not depend on which form ran)
            if (reluIn) t = fmaxf(t, 0.f);
            v[j] = t;
        }
        if (add) {
            const f32x4 r = *reinterpret_cast<const f32x4 *>(aux + pix * ldAux + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += r[j];
        }
        if (reluOut) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
        }
        *reinterpret_cast<f32x4 *>(out + pix * ldOut + c) = v;
    }
}

// ---------------------------------------------------------------------------------------------- head

// in NHWC [B*HW][Cin], w [Cout][Cin], out NCHW [B][Cout][HW]; one wavefront per pixel (grid-stride)
template <int COUT_MAX>
__global__ __launch_bounds__(256)
void head_kernel(const float *__restrict__ in, const float *__restrict__ w, const float *__restrict__ bias,
                 const float *__restrict__ mean, float *__restrict__ out, int B, int HW, int Cin, int ldIn,
                 int Cout, int nTask, float lo, float hi, const float *__restrict__ coef, float normLo)
{
    // coef != NULL (512 -> <=4 form only): `in` is the raw output of the producing convolution and its GroupNorm (+ReLU)
    // is applied on load: x -> max(x*scale + shift, normLo) with {scale, shift} pairs [B][Cin][2] (XL_OP_GN_FINAL)
    const int lane = threadIdx.x & 63;
    const int waveGlobal = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const int nWaves = (gridDim.x * 256) >> 6;
    const int nq = (Cin + 255) >> 8;                          // float4 per lane (256 channels per trip), <= 8
    const long long total = (long long)B * HW;
    if (Cin == 512 && Cout <= 4) {
        // the coordinate head (512 -> 4): the lane's 8 x 4 weights stay in registers across the pixel loop (re-reading
        // them per pixel made 8 of the 10 loads of a pixel weight loads), two pixels in flight per iteration
        f32x4 wr[4][2];
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int q = 0; q < 2; ++q)
                wr[o][q] = o < Cout ? *reinterpret_cast<const f32x4 *>(w + (long long)o * Cin + q * 256 + lane * 4)
                                    : f32x4{ 0.f, 0.f, 0.f, 0.f };
        for (long long p0 = waveGlobal; p0 < total; p0 += 2LL * nWaves) {
            const long long p1 = p0 + nWaves;
            const bool two = p1 < total;
            const long long p1c = two ? p1 : p0;
            f32x4 v[2][2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                v[0][q] = *reinterpret_cast<const f32x4 *>(in + p0 * ldIn + q * 256 + lane * 4);
                v[1][q] = *reinterpret_cast<const f32x4 *>(in + p1c * ldIn + q * 256 + lane * 4);
            }
            if (coef) {
                const long long pp[2] = { p0, p1c };
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const float *cf = coef + ((pp[u] / HW) * Cin) * 2;
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const f32x4 c0 = *reinterpret_cast<const f32x4 *>(cf + 2 * (q * 256 + lane * 4));
                        const f32x4 c1 = *reinterpret_cast<const f32x4 *>(cf + 2 * (q * 256 + lane * 4) + 4);
                        v[u][q].x = fmaxf(fmaf(v[u][q].x, c0[0], c0[1]), normLo);
                        v[u][q].y = fmaxf(fmaf(v[u][q].y, c0[2], c0[3]), normLo);
                        v[u][q].z = fmaxf(fmaf(v[u][q].z, c1[0], c1[1]), normLo);
                        v[u][q].w = fmaxf(fmaf(v[u][q].w, c1[2], c1[3]), normLo);
                    }
                }
            }
            float acc[2][4];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    float t = 0.f;
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        t = fmaf(v[u][q].x, wr[o][q].x, t); t = fmaf(v[u][q].y, wr[o][q].y, t);
                        t = fmaf(v[u][q].z, wr[o][q].z, t); t = fmaf(v[u][q].w, wr[o][q].w, t);
                    }
                    acc[u][o] = t;
                }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int o = 0; o < 4; ++o) acc[u][o] += __shfl_xor(acc[u][o], off);
            if (lane < 2 * Cout) {
                const int u = lane / Cout, o = lane - u * Cout;
                if (u == 0 || two) {
                    float r = 0.f;
#pragma unroll
                    for (int uu = 0; uu < 2; ++uu)
#pragma unroll
                        for (int oo = 0; oo < 4; ++oo) if (uu == u && oo == o) r = acc[uu][oo];
                    r += bias[o];
                    if (o < nTask) r += mean[o];
                    else r = expf(fminf(fmaxf(r, lo), hi));
                    const long long p = u ? p1 : p0;
                    const int n = (int)(p / HW);
                    const int pix = (int)(p - (long long)n * HW);
                    out[((long long)n * Cout + o) * HW + pix] = r;
                }
            }
        }
        return;
    }
    for (long long p = waveGlobal; p < total; p += nWaves) {
        float acc[COUT_MAX];
#pragma unroll
        for (int o = 0; o < COUT_MAX; ++o) acc[o] = 0.f;
        for (int q = 0; q < nq; ++q) {
            const int c = q * 256 + lane * 4;
            if (c >= Cin) break;                                  // (Cin = 128 - the tiny network: lanes 32 .. 63 hold nothing)
            const f32x4 v = *reinterpret_cast<const f32x4 *>(in + p * ldIn + c);
#pragma unroll
            for (int o = 0; o < COUT_MAX; ++o) {
                if (o < Cout) {
                    const f32x4 wv = *reinterpret_cast<const f32x4 *>(w + (long long)o * Cin + c);
                    acc[o] = fmaf(v.x, wv.x, acc[o]); acc[o] = fmaf(v.y, wv.y, acc[o]);
                    acc[o] = fmaf(v.z, wv.z, acc[o]); acc[o] = fmaf(v.w, wv.w, acc[o]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < COUT_MAX; ++o)
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc[o] += __shfl_xor(acc[o], off);
        if (lane < Cout) {
            float v = 0.f;
#pragma unroll
            for (int o = 0; o < COUT_MAX; ++o) if (o == lane) v = acc[o];
            v += bias[lane];
            if (lane < nTask) v += mean[lane];                               // networks.py:351
            else v = expf(fminf(fmaxf(v, lo), hi));                          // networks.py:355-358
            const int n = (int)(p / HW);
            const int pix = (int)(p - (long long)n * HW);
            out[((long long)n * Cout + lane) * HW + pix] = v;
        }
    }
}

// Full-size (semantics) head, networks.py:259-273 + 344-358: the x8 pixel shuffle of the DUC activation is an index map
//   shuffled[b][c][8h+i][8w+j] = in[b][h][w][c*64 + i*8 + j]          (in: NHWC, GroupNorm + ReLU already applied)
// followed by F.interpolate(bilinear, align_corners=False) to H x W (the identity when H = 8 Hs and W = 8 Ws), the
// 1x1 fc3 over the C shuffled channels, the mean offset / exp(hardtanh) epilogue.  out NCHW [B][C][H][W]; one output
// pixel per thread (stores coalesced along x; the gathers of a wavefront fall into a few NHWC pixels).
template <int CMAX>
__global__ __launch_bounds__(256)
void duc_head_kernel(const float *__restrict__ in, const float *__restrict__ w, const float *__restrict__ bias,
                     const float *__restrict__ mean, float *__restrict__ out, int B, int Hs, int Ws, int C, int ldIn,
                     int H, int W, int nTask, float lo, float hi)
{
    const int Hu = 8 * Hs, Wu = 8 * Ws;
    const float sy = (float)Hu / (float)H, sx = (float)Wu / (float)W;       // area_pixel_compute_scale
    const bool ident = (Hu == H) && (Wu == W);
    const long long total = (long long)B * H * W;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long long)gridDim.x * 256) {
        const int x = (int)(p % W);
        const int y = (int)((p / W) % H);
        const int n = (int)(p / ((long long)W * H));
        float fy = sy * ((float)y + 0.5f) - 0.5f; if (fy < 0.f) fy = 0.f;
        float fx = sx * ((float)x + 0.5f) - 0.5f; if (fx < 0.f) fx = 0.f;
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + (y0 < Hu - 1 ? 1 : 0), x1 = x0 + (x0 < Wu - 1 ? 1 : 0);
        const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
        const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
        const float *img = in + (long long)n * Hs * Ws * ldIn;
        const long long a00 = ((long long)(y0 >> 3) * Ws + (x0 >> 3)) * ldIn + (y0 & 7) * 8 + (x0 & 7);
        const long long a01 = ((long long)(y0 >> 3) * Ws + (x1 >> 3)) * ldIn + (y0 & 7) * 8 + (x1 & 7);
        const long long a10 = ((long long)(y1 >> 3) * Ws + (x0 >> 3)) * ldIn + (y1 & 7) * 8 + (x0 & 7);
        const long long a11 = ((long long)(y1 >> 3) * Ws + (x1 >> 3)) * ldIn + (y1 & 7) * 8 + (x1 & 7);
        float v[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            v[c] = 0.f;
            if (c < C) {
                if (ident) v[c] = img[a00 + c * 64];
                else v[c] = ly0 * (lx0 * img[a00 + c * 64] + lx1 * img[a01 + c * 64])
                          + ly1 * (lx0 * img[a10 + c * 64] + lx1 * img[a11 + c * 64]);
            }
        }
#pragma unroll
        for (int o = 0; o < CMAX; ++o) {
            if (o < C) {
                float acc = bias[o];
#pragma unroll
                for (int c = 0; c < CMAX; ++c) if (c < C) acc = fmaf(w[o * C + c], v[c], acc);
                if (o < nTask) acc += mean[o];
                else acc = expf(fminf(fmaxf(acc, lo), hi));
                out[(((long long)n * C + o) * H + y) * W + x] = acc;
            }
        }
    }
}

}  // namespace

int xl_run_gn_stats(const xl_op &op, hipStream_t st)
{
    const int C4 = op.Cin / 4;
    if (op.Cin % 4 != 0 || op.Cin % op.groups != 0 || op.ld_in % 4 != 0) return XL_ERR_ARG;
    int T = 256;
    if (C4 > 256) T = C4;
    else if (256 % C4 != 0) {                        // e.g. 384 channels: 96 quads -> 192 threads (lcm with 64)
        T = C4;
        while (T % 64 != 0) T += C4;
    }
    if (T > 1024 || T % 64 != 0 || op.groups > T) return XL_ERR_ARG;
    hipLaunchKernelGGL(gn_stats_kernel, dim3(op.nchunks, op.B), dim3(T), sizeof(double) * 8 * T, st,
                       (const float *)op.in, (double *)op.stats, op.Hi * op.Wi, op.Cin, op.ld_in, op.groups,
                       op.nchunks);
    return XL_OK;
}

int xl_run_gn_apply(const xl_op &op, hipStream_t st)
{
    if (op.Cin % 4 != 0 || op.ld_in % 4 != 0 || op.ld_out % 4 != 0) return XL_ERR_ARG;
    const int HW = op.Hi * op.Wi;
    int achunks = (HW * (op.Cin / 4) + 256 * 16 - 1) / (256 * 16);     // ~16 float4 per thread
    if (achunks < 1) achunks = 1;
    if (achunks > 1024) achunks = 1024;
    hipLaunchKernelGGL(gn_apply_kernel, dim3(achunks, op.B), dim3(256), sizeof(float) * 2 * op.Cin, st,
                       (const float *)op.in, (const double *)op.stats, (const float *)op.w,
                       (const float *)op.bias, (const float *)op.aux, (float *)op.out, HW, op.Cin, op.ld_in,
                       op.ld_out, op.ld_aux, op.groups, op.nchunks, op.eps, op.flags, op.reserved_i, (const float *)op.aux2);
    return XL_OK;
}

int xl_run_gn_final(const xl_op &op, hipStream_t st)
{
    if (op.groups > 32 || op.Cin % op.groups != 0) return XL_ERR_ARG;
    if (op.reserved_i != 0) {
        // one entry (x stride) per producer tile overlapping an image: they must fit the nchunks slots the producer wrote,
        // or the finalisation sums the next image's entries / stale memory
        const long long rows = op.reserved_i < 0 ? -op.reserved_i : op.reserved_i, hw = (long long)op.Hi * op.Wi;
        const long long perTile = op.stride > 1 ? op.stride : 1;
        const long long tiles = op.reserved_i < 0 ? (hw + rows - 1) / rows : (hw + rows - 1) / rows + 1;
        if (tiles * perTile > op.nchunks) return XL_ERR_ARG;
    }
    // entries per image and group (an upper estimate from the layer's geometry): long lists are split over workgroups by
    // groups - 4 slices above 256 entries, 8 above 1024 (the stem; every other layer: one workgroup per image, as ever)
    long long entries = op.nchunks;
    if (op.reserved_i != 0) {
        const long long rows = op.reserved_i < 0 ? -op.reserved_i : op.reserved_i;
        entries = (((long long)op.Hi * op.Wi + rows - 1) / rows + 1) * (op.stride > 1 ? op.stride : 1);
    }
    int slices = entries > 1024 ? 8 : entries > 256 ? 4 : 1;
    static const char *noSlices = getenv("XL_GN_FINAL_ONE_WG");
    if (op.groups % slices != 0 || noSlices) slices = 1;
    hipLaunchKernelGGL(gn_final_kernel, dim3(op.B, slices), dim3(256), 0, st, (const double *)op.stats, (const float *)op.w,
                       (const float *)op.bias, (float *)op.out, op.Hi * op.Wi, op.Cin, op.groups, op.nchunks, op.eps,
                       op.reserved_i, (float *)op.out2, op.reserved_i != 0 && op.stride > 1 ? op.stride : 1);
    return XL_OK;
}

int xl_run_head(const xl_op &op, hipStream_t st)
{
    if (op.Cin % 4 != 0 || op.Cin < 4 || op.Cin > 2048 || op.Cout > 8 || op.Cout < 1 || op.ld_in % 4 != 0) return XL_ERR_ARG;
    const unsigned blocks = xl_grid((long long)op.B * op.Hi * op.Wi, 4, 4096);        // a wavefront per pixel
    if (op.aux2 && !(op.Cin == 512 && op.Cout <= 4)) return XL_ERR_UNSUPPORTED;    // normalise-on-load: 512 -> <=4 form
    hipLaunchKernelGGL(head_kernel<8>, dim3(blocks), dim3(256), 0, st, (const float *)op.in,
                       (const float *)op.w, (const float *)op.bias, (const float *)op.aux, (float *)op.out,
                       op.B, op.Hi * op.Wi, op.Cin, op.ld_in, op.Cout, op.n_task, op.clamp_lo, op.clamp_hi,
                       (const float *)op.aux2, (op.flags & XL_CONV_NORM_RELU) ? 0.f : -__builtin_huge_valf());
    return XL_OK;
}

int xl_run_duc_head(const xl_op &op, hipStream_t st)
{
    // in [B,Hi,Wi,Cout*64] NHWC, out [B,Cout,Ho,Wo] NCHW
    if (op.Cout < 1 || op.Cout > 8 || op.Cin != op.Cout * 64 || op.Ho < 1 || op.Wo < 1) return XL_ERR_ARG;
    const unsigned blocks = xl_grid((long long)op.B * op.Ho * op.Wo, 256, 65536);
    hipLaunchKernelGGL(duc_head_kernel<8>, dim3(blocks), dim3(256), 0, st, (const float *)op.in,
                       (const float *)op.w, (const float *)op.bias, (const float *)op.aux, (float *)op.out,
                       op.B, op.Hi, op.Wi, op.Cout, op.ld_in, op.Ho, op.Wo, op.n_task, op.clamp_lo, op.clamp_hi);
    return XL_OK;
}
