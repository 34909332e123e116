// xl_gn_bwd.hip — XL_OP_GNB_*: GroupNorm backward fused with the forward epilogue (ReLU / residual add / ReLU):
//   pass 1 per-(image, chunk, channel) sums of dv, dv*xhat, xhat; pass 2 dx (+ d residual);
//   then d gamma, d beta and the conv-bias gradient in closed form from the sums (no extra pass)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "xl_launch.h"
#include "xl_operand_math.h"

namespace {

struct GnbArgs {
    const float *x, *dout, *outAct, *gamma, *beta;
    const float *fco;        // forward coefficients from GN_FINAL: [B][C][2] {scale, shift}, then [B][C][2] {mean, rstd}
    double *bstats;          // [B][nchunks2][C][3]  (sum dv, sum dv*xhat, sum xhat)
    float *dx, *daux;
    double *ncsums;          // [B][C][6]: A, Bc, Xh, S1, S2, rstd (gnb_final_kernel)
    float *bco;              // [B][C][3]: rstd*gamma, rstd*S1/m, rstd*S2/m (gnb_final_kernel)
    int B, HW, C, ldX, ldD, ldO, ldDx, ldAux, G, nchunks2, flags;
    unsigned *amax;          // gnb_apply (optional): max |dx| of the pass, as float bits (xl_wave_max_commit)
    int rev;                 // gnb_stats: walk the images in descending order
};

// dv (gradient w.r.t. v = gn(x)) of one element
__device__ __forceinline__ float gnb_dv(float dout, float outAct, float v, int flags)
{
    float t = dout;
    if ((flags & XL_GN_RELU_OUT) && !(outAct > 0.f)) t = 0.f;
    if ((flags & XL_GN_RELU_IN) && !(v > 0.f)) t = 0.f;
    return t;
}

// grid (nchunks2, B), T threads, T % (C/4) == 0
__global__ void gnb_stats_kernel(GnbArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double smemD[];
    const int T = blockDim.x, tid = threadIdx.x;
    const int C4 = a.C >> 2;
    float *sCo = reinterpret_cast<float *>(smemD + (size_t)T * 12);          // mean, rstd, sc, sh per channel
    // images in DESCENDING order (a.rev; XL_GNB_REVERSE=0: ascending): the apply pass walks ascending and so starts with what this
    // pass read last - its first reads are still on the die (apply 118.9 -> 114.7 us per launch at batch 16; this pass itself does
    // not gain from meeting its producer's last writes: 85.7 -> 85.2)
    const int n = a.rev ? (int)gridDim.y - 1 - (int)blockIdx.y : (int)blockIdx.y, chunk = blockIdx.x;
    {
        const float *scsh = a.fco + (long long)n * a.C * 2;
        const float *murs = a.fco + ((long long)a.B + n) * a.C * 2;
        for (int c = tid; c < a.C; c += T) {
            sCo[c] = murs[2 * c]; sCo[a.C + c] = murs[2 * c + 1]; sCo[2 * a.C + c] = scsh[2 * c]; sCo[3 * a.C + c] = scsh[2 * c + 1];
        }
    }
    __syncthreads();
    const int c4 = tid % C4, prow = tid / C4, rows = T / C4;
    const int per = (a.HW + a.nchunks2 - 1) / a.nchunks2;
    const int p0 = chunk * per;
    int p1 = p0 + per; if (p1 > a.HW) p1 = a.HW;
    double sA[4] = { 0, 0, 0, 0 }, sB[4] = { 0, 0, 0, 0 }, sX[4] = { 0, 0, 0, 0 };
    const int c = 4 * c4;
    // the thread's channel quad is fixed: its coefficients live in registers; four pixels per trip with all their loads issued
    // before the first use (round 4: one pixel per trip left 2 - 3 loads in flight per thread, 3.8 TB/s).  The sums are
    // accumulated pixel by pixel in the same order as before.
    f32x4 cMu, cRs, cSc, cSh;
#pragma unroll
    for (int j = 0; j < 4; ++j) { cMu[j] = sCo[c + j]; cRs[j] = sCo[a.C + c + j]; cSc[j] = sCo[2 * a.C + c + j]; cSh[j] = sCo[3 * a.C + c + j]; }
    const bool hasOut = (a.flags & XL_GN_RELU_OUT) != 0;
    auto accumulate = [&](const f32x4 &xv, const f32x4 &dv4, const f32x4 &ov) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = xv[j] * cSc[j] + cSh[j];
            const float xh = (xv[j] - cMu[j]) * cRs[j];
            const float dv = gnb_dv(dv4[j], ov[j], v, a.flags);
            sA[j] += (double)dv; sB[j] += (double)dv * (double)xh; sX[j] += (double)xh;
        }
    };
    int p = p0 + prow;
    for (; p + 3 * rows < p1; p += 4 * rows) {
        f32x4 xv[4], dv4[4], ov[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long pix = (long long)n * a.HW + p + k * rows;
            xv[k] = *reinterpret_cast<const f32x4 *>(a.x + pix * a.ldX + c);
            dv4[k] = *reinterpret_cast<const f32x4 *>(a.dout + pix * a.ldD + c);
            ov[k] = f32x4{ 1.f, 1.f, 1.f, 1.f };
            if (hasOut) ov[k] = *reinterpret_cast<const f32x4 *>(a.outAct + pix * a.ldO + c);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) accumulate(xv[k], dv4[k], ov[k]);
    }
    for (; p < p1; p += rows) {
        const long long pix = (long long)n * a.HW + p;
        const f32x4 xv = *reinterpret_cast<const f32x4 *>(a.x + pix * a.ldX + c);
        const f32x4 dv4 = *reinterpret_cast<const f32x4 *>(a.dout + pix * a.ldD + c);
        f32x4 ov = { 1.f, 1.f, 1.f, 1.f };
        if (hasOut) ov = *reinterpret_cast<const f32x4 *>(a.outAct + pix * a.ldO + c);
        accumulate(xv, dv4, ov);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { smemD[tid * 12 + j] = sA[j]; smemD[tid * 12 + 4 + j] = sB[j]; smemD[tid * 12 + 8 + j] = sX[j]; }
    __syncthreads();
    for (int ch = tid; ch < a.C; ch += T) {
        double A = 0.0, Bc = 0.0, X = 0.0;
        for (int r = 0; r < rows; ++r) {
            const int th = r * C4 + (ch >> 2), sl = ch & 3;
            A += smemD[th * 12 + sl]; Bc += smemD[th * 12 + 4 + sl]; X += smemD[th * 12 + 8 + sl];
        }
        double *o = a.bstats + (((long long)n * a.nchunks2 + chunk) * a.C + ch) * 3;
        o[0] = A; o[1] = Bc; o[2] = X;
    }
}

// Totals of the per-chunk sums and everything the streaming apply pass needs per (image, channel), computed once per
// image instead of in the prologue of every apply workgroup.  grid (B, C / CB), 1024 threads; a workgroup owns CB
// channels (whole groups); 4 threads per channel each sum a contiguous quarter of the chunks, the quarters are added in
// a fixed order.
__global__ __launch_bounds__(1024)
void gnb_final_kernel(GnbArgs a, int CB)
{
    extern __shared__ __attribute__((aligned(16))) double dA[];      // A, Bc, Xh totals per channel, then S1, S2 per group
    const int tid = threadIdx.x, n = blockIdx.x;
    const int C = a.C, cpg = C / a.G;
    const int c0 = blockIdx.y * CB, g0 = c0 / cpg, GB = CB / cpg;
    double *sS = dA + 3 * (size_t)CB;
    const int part = tid & 3;
    const int per = (a.nchunks2 + 3) >> 2;
    const int k0 = part * per;
    int k1 = k0 + per; if (k1 > a.nchunks2) k1 = a.nchunks2;
    for (int cl = tid >> 2; cl < CB; cl += 256) {
        double A = 0.0, Bc = 0.0, X = 0.0;
        const double *bs = a.bstats + ((long long)n * a.nchunks2 * C + c0 + cl) * 3;
#pragma unroll 4
        for (int k = k0; k < k1; ++k) { A += bs[(long long)k * C * 3]; Bc += bs[(long long)k * C * 3 + 1]; X += bs[(long long)k * C * 3 + 2]; }
        // quarters 0+1 and 2+3, then the halves: the same order for every channel
        A += __shfl_xor(A, 1); Bc += __shfl_xor(Bc, 1); X += __shfl_xor(X, 1);
        A += __shfl_xor(A, 2); Bc += __shfl_xor(Bc, 2); X += __shfl_xor(X, 2);
        if (part == 0) { dA[3 * cl] = A; dA[3 * cl + 1] = Bc; dA[3 * cl + 2] = X; }
    }
    __syncthreads();
    for (int gl = tid; gl < GB; gl += 1024) {
        double S1 = 0.0, S2 = 0.0;
        for (int cl = gl * cpg; cl < (gl + 1) * cpg; ++cl) {
            S1 += (double)a.gamma[c0 + cl] * dA[3 * cl]; S2 += (double)a.gamma[c0 + cl] * dA[3 * cl + 1];
        }
        sS[2 * gl] = S1; sS[2 * gl + 1] = S2;
    }
    __syncthreads();
    const double m = (double)cpg * (double)a.HW;
    const float *murs = a.fco + ((long long)a.B + n) * C * 2;
    for (int cl = tid; cl < CB; cl += 1024) {
        const int c = c0 + cl, gl = cl / cpg;
        const double rs = (double)murs[2 * c + 1];
        float *bo = a.bco + ((long long)n * C + c) * 3;
        bo[0] = (float)(rs * (double)a.gamma[c]);
        bo[1] = (float)(rs * sS[2 * gl] / m);
        bo[2] = (float)(rs * sS[2 * gl + 1] / m);
        double *o = a.ncsums + ((long long)n * C + c) * 6;
        o[0] = dA[3 * cl]; o[1] = dA[3 * cl + 1]; o[2] = dA[3 * cl + 2]; o[3] = sS[2 * gl]; o[4] = sS[2 * gl + 1]; o[5] = rs;
    }
    (void)g0;
}

// grid (achunks, B), 256 threads
__global__ __launch_bounds__(256)
void gnb_apply_kernel(GnbArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float sK[];      // per channel: mean, rstd, sc, sh, k1, k2, k3
    const int tid = threadIdx.x, n = blockIdx.y;
    const int C = a.C;
    {
        const float *scsh = a.fco + (long long)n * C * 2;
        const float *murs = a.fco + ((long long)a.B + n) * C * 2;
        const float *bo = a.bco + (long long)n * C * 3;
        for (int c = tid; c < C; c += 256) {
            sK[c] = murs[2 * c]; sK[C + c] = murs[2 * c + 1]; sK[2 * C + c] = scsh[2 * c]; sK[3 * C + c] = scsh[2 * c + 1];
            sK[4 * C + c] = bo[3 * c]; sK[5 * C + c] = bo[3 * c + 1]; sK[6 * C + c] = bo[3 * c + 2];
        }
    }
    __syncthreads();
    const int C4 = C >> 2;
    const int achunks = gridDim.x;
    const int per = (a.HW + achunks - 1) / achunks;
    const int p0 = blockIdx.x * per;
    int p1 = p0 + per; if (p1 > a.HW) p1 = a.HW;
    const long long nElem4 = (long long)(p1 - p0) * C4;
    if (C4 <= 256 && 256 % C4 == 0) {
        // the usual case (C = 32 ... 1024, a power of two): a thread keeps ONE channel quad - its seven coefficients in
        // registers, no 64-bit division per element - and walks the pixels, four per trip with all loads issued first
        // (round 4: 4.5 -> TB/s).  Element by element the same arithmetic as the general loop below.
        const int c = 4 * (tid % C4), rows = 256 / C4;
        f32x4 kMu, kRs, kSc, kSh, k1, k2, k3;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            kMu[j] = sK[c + j]; kRs[j] = sK[C + c + j]; kSc[j] = sK[2 * C + c + j]; kSh[j] = sK[3 * C + c + j];
            k1[j] = sK[4 * C + c + j]; k2[j] = sK[5 * C + c + j]; k3[j] = sK[6 * C + c + j];
        }
        const bool hasOut = (a.flags & XL_GN_RELU_OUT) != 0, reluIn = (a.flags & XL_GN_RELU_IN) != 0;
        const bool add = (a.flags & XL_GN_ADD) != 0, accAux = (a.flags & XL_GN_ACC_AUX) != 0;
        float mx = 0.f;
        auto one = [&](long long pix, const f32x4 &xv, const f32x4 &d4, const f32x4 &ov, const f32x4 &old) {
            f32x4 dx, t4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = xv[j] * kSc[j] + kSh[j];
                const float xh = (xv[j] - kMu[j]) * kRs[j];
                float t = d4[j];
                if (hasOut && !(ov[j] > 0.f)) t = 0.f;
                t4[j] = t;
                const float dv = (reluIn && !(v > 0.f)) ? 0.f : t;
                dx[j] = k1[j] * dv - k2[j] - xh * k3[j];
            }
            if (add) {
                if (accAux) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) t4[j] += old[j];
                }
                *reinterpret_cast<f32x4 *>(a.daux + pix * a.ldAux + c) = t4;
            }
            *reinterpret_cast<f32x4 *>(a.dx + pix * a.ldDx + c) = dx;
            mx = fmaxf(fmaxf(mx, fmaxf(fabsf(dx[0]), fabsf(dx[1]))), fmaxf(fabsf(dx[2]), fabsf(dx[3])));
        };
        const f32x4 ones = { 1.f, 1.f, 1.f, 1.f };
        int p = p0 + tid / C4;
        for (; p + 3 * rows < p1; p += 4 * rows) {
            f32x4 xv[4], d4[4], ov[4], old[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long pix = (long long)n * a.HW + p + k * rows;
                xv[k] = *reinterpret_cast<const f32x4 *>(a.x + pix * a.ldX + c);
                d4[k] = *reinterpret_cast<const f32x4 *>(a.dout + pix * a.ldD + c);
                ov[k] = hasOut ? *reinterpret_cast<const f32x4 *>(a.outAct + pix * a.ldO + c) : ones;
                old[k] = (add && accAux) ? *reinterpret_cast<const f32x4 *>(a.daux + pix * a.ldAux + c) : ones;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) one((long long)n * a.HW + p + k * rows, xv[k], d4[k], ov[k], old[k]);
        }
        for (; p < p1; p += rows) {
            const long long pix = (long long)n * a.HW + p;
            const f32x4 xv = *reinterpret_cast<const f32x4 *>(a.x + pix * a.ldX + c);
            const f32x4 d4 = *reinterpret_cast<const f32x4 *>(a.dout + pix * a.ldD + c);
            const f32x4 ov = hasOut ? *reinterpret_cast<const f32x4 *>(a.outAct + pix * a.ldO + c) : ones;
            const f32x4 old = (add && accAux) ? *reinterpret_cast<const f32x4 *>(a.daux + pix * a.ldAux + c) : ones;
            one(pix, xv, d4, ov, old);
        }
        xl_wave_max_commit(mx, a.amax);
        return;
    }
    float mxs = 0.f;
    for (long long f = tid; f < nElem4; f += 256) {
        const int p = p0 + (int)(f / C4);
        const int c = (int)(f - (long long)(p - p0) * C4) * 4;
        const long long pix = (long long)n * a.HW + p;
        const f32x4 xv = *reinterpret_cast<const f32x4 *>(a.x + pix * a.ldX + c);
        const f32x4 d4 = *reinterpret_cast<const f32x4 *>(a.dout + pix * a.ldD + c);
        f32x4 ov = { 1.f, 1.f, 1.f, 1.f };
        if (a.flags & XL_GN_RELU_OUT) ov = *reinterpret_cast<const f32x4 *>(a.outAct + pix * a.ldO + c);
        f32x4 dx, t4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = xv[j] * sK[2 * C + c + j] + sK[3 * C + c + j];
            const float xh = (xv[j] - sK[c + j]) * sK[C + c + j];
            float t = d4[j];
            if ((a.flags & XL_GN_RELU_OUT) && !(ov[j] > 0.f)) t = 0.f;
            t4[j] = t;
            const float dv = ((a.flags & XL_GN_RELU_IN) && !(v > 0.f)) ? 0.f : t;
            dx[j] = sK[4 * C + c + j] * dv - sK[5 * C + c + j] - xh * sK[6 * C + c + j];
        }
        if (a.flags & XL_GN_ADD) {
            float *q = a.daux + pix * a.ldAux + c;
            if (a.flags & XL_GN_ACC_AUX) {
                const f32x4 old = *reinterpret_cast<const f32x4 *>(q);
#pragma unroll
                for (int j = 0; j < 4; ++j) t4[j] += old[j];
            }
            *reinterpret_cast<f32x4 *>(q) = t4;
        }
        *reinterpret_cast<f32x4 *>(a.dx + pix * a.ldDx + c) = dx;
        mxs = fmaxf(fmaxf(mxs, fmaxf(fabsf(dx[0]), fabsf(dx[1]))), fmaxf(fabsf(dx[2]), fabsf(dx[3])));
    }
    xl_wave_max_commit(mxs, a.amax);
}

// d gamma, d beta, d conv-bias from the per-(image, channel) sums; one thread per channel
__global__ void gnb_params_kernel(const double *ncsums, const float *gamma, int B, int C, int G, int HW,
                                  float *dgamma, float *dbeta, float *dbias)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int cpg = C / G;
    const double m = (double)cpg * (double)HW;
    double dg = 0.0, db = 0.0, dbi = 0.0;
    for (int n = 0; n < B; ++n) {
        const double *o = ncsums + ((long long)n * C + c) * 6;
        dg += o[1]; db += o[0];
        // sum over pixels of dx = rstd*(gamma*A - (HW*S1 + S2*sum_xhat)/m)
        dbi += o[5] * ((double)gamma[c] * o[0] - ((double)HW * o[3] + o[4] * o[2]) / m);
    }
    dgamma[c] = (float)dg; dbeta[c] = (float)db;
    // one channel per group = instance norm: a per-channel bias cancels exactly, its gradient is identically 0
    if (dbias) dbias[c] = (cpg == 1) ? 0.f : (float)dbi;
}

// the same for a list of layers: blockIdx.y = layer (XL_OP_GNB_PARAMS_LIST)
__global__ void gnb_params_list_kernel(const xl_gnb_params_item *__restrict__ items)
{
    const xl_gnb_params_item it = items[blockIdx.y];
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= it.C) return;
    const int cpg = it.C / it.G;
    const double m = (double)cpg * (double)it.HW;
    const double gam = (double)it.gamma[c];
    double dg = 0.0, db = 0.0, dbi = 0.0;
    for (int n = 0; n < it.B; ++n) {
        const double *o = it.sums + ((long long)n * it.C + c) * 6;
        dg += o[1]; db += o[0];
        dbi += o[5] * (gam * o[0] - ((double)it.HW * o[3] + o[4] * o[2]) / m);
    }
    it.dgamma[c] = (float)dg; it.dbeta[c] = (float)db;
    if (it.dbias) it.dbias[c] = (cpg == 1) ? 0.f : (float)dbi;
}

// threads of gnb_stats_kernel for C >= 4 channels (xl_run_gnb has checked), or -1
int gnb_threads(int C)
{
    const int C4 = C / 4;
    if (C4 > 256) return C4;
    if (256 % C4 == 0) return 256;
    int T = C4;                                         // e.g. 384 channels: 96 quads -> 192 threads (lcm with 64)
    while (T % 64 != 0) T += C4;
    return T <= 1024 ? T : -1;
}

}  // namespace

// XL_OP_GNB_STATS, XL_OP_GNB_FINAL, XL_OP_GNB_APPLY.  stats = forward coefficient table of the layer (GN_FINAL with out2: [B][C][2] {scale, shift} followed by
// [B][C][2] {mean, rstd}); stats2 = scratch: per-chunk sums, per-(image, channel) sums, apply coefficients
int xl_run_gnb(const xl_op &op, hipStream_t st)
{
    if (op.groups < 1 || op.Cin < 4) return XL_ERR_ARG;                    // (the divisors below)
    if (op.Cin % 4 != 0 || op.Cin % op.groups != 0 || op.groups > 64 || op.nchunks2 < 1 || !op.stats || !op.stats2)
        return XL_ERR_ARG;
    GnbArgs a;
    a.x = (const float *)op.in; a.dout = (const float *)op.aux; a.outAct = (const float *)op.aux2;
    a.gamma = (const float *)op.w; a.beta = (const float *)op.bias; a.fco = (const float *)op.stats;
    a.bstats = (double *)op.stats2; a.dx = (float *)op.out; a.daux = (float *)op.out2;
    a.ncsums = a.bstats + (long long)op.B * op.nchunks2 * op.Cin * 3;
    a.bco = reinterpret_cast<float *>(a.ncsums + (long long)op.B * op.Cin * 6);
    // (XL_OP_GNB_PARAMS_LIST: the per-(image, channel) sums of this layer go to a buffer of its own, read at the end of the pass)
    if (op.type == XL_OP_GNB_FINAL && op.scale) a.ncsums = (double *)const_cast<void *>(op.scale);
    a.B = op.B; a.HW = op.Hi * op.Wi; a.C = op.Cin; a.ldX = op.ld_in; a.ldD = op.ld_aux; a.ldO = op.ld_out; a.ldDx = op.ld_in;
    a.ldAux = op.Cout > 0 ? op.Cout : op.ld_out; a.G = op.groups; a.nchunks2 = op.nchunks2; a.flags = op.flags;
    static const int gnbRev = getenv("XL_GNB_REVERSE") ? atoi(getenv("XL_GNB_REVERSE")) : 1;
    a.rev = gnbRev;
    a.amax = op.type == XL_OP_GNB_APPLY ? (unsigned *)op.scale : nullptr;      // (round 5: max |dx| for the pair GEMMs that read dx)
    if (op.type == XL_OP_GNB_STATS) {
        const int T = gnb_threads(op.Cin);
        if (T < 0 || T > 1024) return XL_ERR_ARG;
        const size_t lds = sizeof(double) * 12 * T + sizeof(float) * 4 * op.Cin;
        hipLaunchKernelGGL(gnb_stats_kernel, dim3(op.nchunks2, op.B), dim3(T), lds, st, a);
    } else if (op.type == XL_OP_GNB_FINAL) {
        const int cpg = op.Cin / op.groups;
        const int CB = (op.Cin % 64 == 0 && 64 % cpg == 0) ? 64 : op.Cin;      // whole groups per workgroup
        const size_t lds = sizeof(double) * (3 * (size_t)CB + 2 * 64);
        hipLaunchKernelGGL(gnb_final_kernel, dim3(op.B, op.Cin / CB), dim3(1024), lds, st, a, CB);
    } else {
        int achunks = (a.HW * (op.Cin / 4) + 256 * 16 - 1) / (256 * 16);
        if (achunks < 1) achunks = 1;
        if (achunks > 1024) achunks = 1024;
        const size_t lds = sizeof(float) * 7 * op.Cin;
        hipLaunchKernelGGL(gnb_apply_kernel, dim3(achunks, op.B), dim3(256), lds, st, a);
    }
    return XL_OK;
}

int xl_run_gnb_params(const xl_op &op, hipStream_t st)
{
    const double *nc = (const double *)op.stats2 + (long long)op.B * op.nchunks2 * op.Cin * 3;
    float *dbias = (op.flags & XL_GN_NO_CONV_BIAS) ? nullptr : (float *)op.aux2;
    hipLaunchKernelGGL(gnb_params_kernel, dim3((op.Cin + 63) / 64), dim3(64), 0, st, nc, (const float *)op.w, op.B,
                       op.Cin, op.groups, op.Hi * op.Wi, (float *)op.out, (float *)op.out2, dbias);
    return XL_OK;
}

int xl_run_gnb_params_list(const xl_op &op, hipStream_t st)
{
    if (op.Cin < 1 || op.Cin > 65535 || !op.in || op.Cout < 1) return XL_ERR_ARG;      // Cout = the largest channel count
    hipLaunchKernelGGL(gnb_params_list_kernel, dim3((op.Cout + 63) / 64, op.Cin), dim3(64), 0, st,
                       (const xl_gnb_params_item *)op.in);
    return XL_OK;
}
