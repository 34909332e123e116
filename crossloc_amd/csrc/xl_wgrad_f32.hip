// xl_wgrad_f32.hip — the weight gradient of a convolution (what cuDNN wgrad did for `loss.backward()`): XL_OP_WGRAD and, for a
// Winograd layer, the transforms XL_OP_WINO_DY / XL_OP_WINO_WFINAL around its batched products.
//   wgrad_kernel       dW[o][tap][c] = sum_m dY[m][o] * X[m @ tap][c]: implicit GEMM with the PIXEL dimension as K,
//                      split-K over pixel ranges, fp32 MFMA 32x32x2 with operands read transposed from LDS
//                      ([pixel][channel] tiles, ds_read_b32 rows are conflict-free), fixed-order reduce -> OIHW
//   xl_run_wgrad       the dispatch: with XL_CONV_SPLIT_BF16 the products run on the matrix pipe (xl_wgrad_split.hip,
//                      xl_wgrad_pair.hip; one loop: xl_wgrad.h, xl_wgrad_body.h) and only the reduce over the splits is here
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xl_launch.h"
#include "xl_operand_math.h"

namespace {

struct WgradArgs {
    const float *x; const float *dy; float *partial;
    int B, Hi, Wi, Cin, Ho, Wo, Cout, ldX, ldY, ksize, stride;
    int M, splits, mPerSplit, nbo, nbc;
    unsigned xBytes, dyBytes;
    // batched launch (Winograd weight gradient: one [Cout x Cin] GEMM per frequency): zCount consecutive blocks of
    // x / dy (zX / zY elements apart) and of the partial buffer
    int zCount; long long zX, zY;
};

// tile BO (output channels) x BC (input channels) of ONE tap; K = output pixels of this split.
// waves WO x WC, wave tile (BO/WO) x (BC/WC) = TI x TJ MFMA tiles of 32x32.
// Both operand tiles are [pixel][channel] slices of dY / X, i.e. already K-major with the channel contiguous: they go
// global -> LDS by DMA (buffer_load ... lds, lane-linear = the natural row-major tile; out-of-range pixels and padding
// taps are zero-filled by the bounds check).  MFMA 32x32x2 takes ONE k per lane, so a lane cannot vectorise its
// fragment along k; it reads TI (TJ) CONSECUTIVE channels instead and feeds them to TI (TJ) different MFMAs: MFMA
// tile i of the wave holds the interleaved rows {TI*r + i} (columns {TJ*c + j}) — one ds_read_b64 per operand and
// k-pair instead of two ds_read_b32, and float2 stores in the epilogue.  The K-loop has the same shape as the
// forward kernel's: double-buffered, one barrier per K-step placed before its last chunk, the first fragments of
// the next step prefetched across the step boundary, DMA issue in the shadow of the last chunk's MFMAs.
template <int N> struct FragT { typedef float type; };
template <> struct FragT<2> { typedef f32x2 type; };
template <int N> __device__ __forceinline__ float frag_elem(const typename FragT<N>::type &v, int i);
template <> __device__ __forceinline__ float frag_elem<1>(const float &v, int) { return v; }
template <> __device__ __forceinline__ float frag_elem<2>(const FragT<2>::type &v, int i) { return v[i]; }

template <int BO, int BC, int WO, int WC>
__global__ __launch_bounds__(64 * WO * WC)
void wgrad_kernel(WgradArgs a)
{
    constexpr int NW = WO * WC, NT = 64 * NW;
    constexpr int TI = BO / WO / 32, TJ = BC / WC / 32;
    static_assert(TI <= 2 && TJ <= 2, "fragment width");
    constexpr int KB = 32;                                  // pixels per K-step
    constexpr int LA = (KB * BO / 4) / NT, LB = (KB * BC / 4) / NT;   // DMA instructions per wave and K-step
    constexpr int kWaitVm0 = 0x0F70;                        // s_waitcnt vmcnt(0)
    // ONE LDS object: with a second one hipcc waits vmcnt(0) before every ds_read that follows an LDS-DMA
    __shared__ __attribute__((aligned(16))) float smem[2 * KB * (BO + BC)];
    float (*sA)[KB * BO] = reinterpret_cast<float (*)[KB * BO]>(smem);                  // dY tile  [pixel][o]
    float (*sB)[KB * BC] = reinterpret_cast<float (*)[KB * BC]>(smem + 2 * KB * BO);    // X tile   [pixel][c]
    typedef __attribute__((address_space(3))) void lds_void;
    typedef typename FragT<TI>::type fragA_t;
    typedef typename FragT<TJ>::type fragB_t;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wo = wave / WC, wc = wave - wo * WC;
    const int PAD = (a.ksize == 3) ? 1 : 0;

    // Workgroup b runs on XCD b%8 (own L2).  Each XCD gets a contiguous run of the (split, tap, ob, cb) order, so
    // the ~64 workgroups resident on an XCD stream the SAME pixel range (one split) through its L2 — the dY / X rows
    // are fetched once per XCD and tap group instead of once per workgroup.
    const int taps = a.ksize * a.ksize;
    int t = xcd_remap(blockIdx.x, a.zCount * a.splits * taps * a.nbo * a.nbc);
    const int cb = t % a.nbc; t /= a.nbc;
    const int ob = t % a.nbo; t /= a.nbo;
    const int tap = t % taps; t /= taps;
    const int split = t % a.splits;
    const int z = t / a.splits;
    a.x += z * a.zX; a.dy += z * a.zY;
    a.partial += (long long)z * a.splits * taps * a.Cout * a.Cin;
    const int ky = tap / a.ksize, kx = tap - ky * a.ksize;
    const int o0 = ob * BO, c0 = cb * BC;
    const int mBeg = split * a.mPerSplit;
    int mEnd = mBeg + a.mPerSplit; if (mEnd > a.M) mEnd = a.M;

    const __amdgpu_buffer_rsrc_t srdX = __builtin_amdgcn_make_buffer_rsrc((void *)a.x, 0, (int)a.xBytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t srdY = __builtin_amdgcn_make_buffer_rsrc((void *)a.dy, 0, (int)a.dyBytes, 0x00020000);
    constexpr unsigned OOB = 0x80000000u;
    const int HoWo = a.Ho * a.Wo;

    // DMA slot q of this wave covers float4s (q*NW + wave)*64 .. +63 of the [KB][B?/4] tile
    int rowA[LA], colA[LA], rowB[LB], colB[LB];
#pragma unroll
    for (int q = 0; q < LA; ++q) { const int f = (q * NW + wave) * 64 + lane; rowA[q] = f / (BO / 4); colA[q] = (f - rowA[q] * (BO / 4)) * 4 + o0; }
#pragma unroll
    for (int q = 0; q < LB; ++q) { const int f = (q * NW + wave) * 64 + lane; rowB[q] = f / (BC / 4); colB[q] = (f - rowB[q] * (BC / 4)) * 4 + c0; }
    // Pixel coordinates of the X rows this lane fetches, advanced by KB pixels per K-step WITHOUT divisions
    // (straight-line selects only: the address arithmetic must stay in the MFMA basic block to overlap with it).
    // Requires Ho*Wo >= KB (one image wrap per step at most); checked by the launcher.
    int pn[LB], py[LB], px[LB];
    const int dOy = KB / a.Wo, dOx = KB - dOy * a.Wo;
#pragma unroll
    for (int q = 0; q < LB; ++q) {
        const int m = mBeg + rowB[q];
        pn[q] = m / HoWo;
        const int rem = m - pn[q] * HoWo;
        py[q] = rem / a.Wo; px[q] = rem - py[q] * a.Wo;
    }
    int mCur = mBeg;
    // offsets of the K-step starting at mCur, then advance to the next one
    auto offsets = [&](unsigned (&va)[LA], unsigned (&vb)[LB]) {
#pragma unroll
        for (int q = 0; q < LA; ++q) {
            const int m = mCur + rowA[q];
            va[q] = m < mEnd ? (unsigned)(m * a.ldY + colA[q]) * 4u : OOB;
        }
#pragma unroll
        for (int q = 0; q < LB; ++q) {
            const int m = mCur + rowB[q];
            const int iy = py[q] * a.stride - PAD + ky, ix = px[q] * a.stride - PAD + kx;
            const bool ok = m < mEnd && (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi;
            // mask arithmetic, not a select: hipcc turns the select into an exec-masked branch around the multiplies
            const unsigned msk = 0u - (unsigned)ok;
            vb[q] = (((unsigned)(((pn[q] * a.Hi + iy) * a.Wi + ix) * a.ldX + colB[q]) * 4u) & msk) | (OOB & ~msk);
            px[q] += dOx; py[q] += dOy;
            const bool cx = px[q] >= a.Wo;
            px[q] -= cx ? a.Wo : 0; py[q] += cx ? 1 : 0;
            const bool cy = py[q] >= a.Ho;
            py[q] -= cy ? a.Ho : 0; pn[q] += cy ? 1 : 0;
        }
        mCur += KB;
    };
    auto issue_a = [&](const unsigned (&va)[LA], int buf) {
#pragma unroll
        for (int q = 0; q < LA; ++q)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(srdY, (lds_void *)&sA[buf][(q * NW + wave) * 256], 16, (int)va[q], 0, 0, 0);
    };
    auto issue_b = [&](const unsigned (&vb)[LB], int buf) {
#pragma unroll
        for (int q = 0; q < LB; ++q)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(srdX, (lds_void *)&sB[buf][(q * NW + wave) * 256], 16, (int)vb[q], 0, 0, 0);
    };

    f32x16 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    int nk = (mEnd - mBeg + KB - 1) / KB;
    if (nk < 0) nk = 0;
    {
        unsigned va[LA], vb[LB];
        offsets(va, vb);
        issue_a(va, 0); issue_b(vb, 0);
        offsets(va, vb);
        issue_a(va, 1); issue_b(vb, 1);
    }
    __builtin_amdgcn_s_waitcnt(kWaitVm0);                   // the fence of __syncthreads() does not wait for LDS-DMA
    __syncthreads();

    const int fr = lane & 31, fk = lane >> 5;
    const float *Afrag = &sA[0][fk * BO + wo * (BO / WO) + TI * fr];
    const float *Bfrag = &sB[0][fk * BC + wc * (BC / WC) + TJ * fr];
    // fragments of a chunk of 4 k-pairs, ping-ponging between two register sets
    fragA_t fa[2][4];
    fragB_t fb[2][4];
    auto read_frags = [&](int set, int buf, int c) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            fa[set][u] = *reinterpret_cast<const fragA_t *>(Afrag + buf * (KB * BO) + 2 * (4 * c + u) * BO);
            fb[set][u] = *reinterpret_cast<const fragB_t *>(Bfrag + buf * (KB * BC) + 2 * (4 * c + u) * BC);
        }
    };
    auto multiply_u = [&](int set, int u) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(frag_elem<TI>(fa[set][u], i), frag_elem<TJ>(fb[set][u], j),
                                                                 acc[i][j], 0, 0, 0);
    };
    auto multiply = [&](int set) {
#pragma unroll
        for (int u = 0; u < 4; ++u) multiply_u(set, u);
    };
    constexpr int NM = 4 * TI * TJ, ND = 8;
    read_frags(0, 0, 0);
    for (int kk = 0; kk < nk; ++kk) {
        const int buf = kk & 1;
        unsigned vaN[LA], vbN[LB];                          // offsets of step kk+2, computed under this step's MFMAs
        offsets(vaN, vbN);
        read_frags(1, buf, 1);
        multiply(0);
        read_frags(0, buf, 2);
        multiply(1);
        read_frags(1, buf, 3);
        multiply(0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, ND, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, ND, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, ND, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, NM - 1, 0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(kWaitVm0);               // tile kk+1 has landed
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        multiply_u(1, 0);
        __builtin_amdgcn_sched_barrier(0x6);
        issue_a(vaN, buf);
        __builtin_amdgcn_sched_barrier(0x6);
        multiply_u(1, 1);
        __builtin_amdgcn_sched_barrier(0x6);
        issue_b(vbN, buf);
        read_frags(0, buf ^ 1, 0);
        __builtin_amdgcn_sched_barrier(0x6);
        multiply_u(1, 2);
        multiply_u(1, 3);
    }
    __builtin_amdgcn_s_waitcnt(kWaitVm0);                   // trailing DMAs must not outlive the workgroup's LDS

    // partial[split][tap][o][c]; MFMA tile (i, j): rows TI*row + i, columns TJ*col + j
    const int col = lane & 31, rhalf = (lane >> 5) * 4;
    float *P = a.partial + ((long long)split * a.ksize * a.ksize + tap) * a.Cout * a.Cin;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = o0 + wo * (BO / WO) + TI * ((r & 3) + 8 * (r >> 2) + rhalf) + i;
            const int c = c0 + wc * (BC / WC) + TJ * col;
            float *dst = P + (long long)o * a.Cin + c;
            if constexpr (TJ == 2) {
                *reinterpret_cast<f32x2 *>(dst) = f32x2{ acc[i][0][r], acc[i][1][r] };
            } else {
                *dst = acc[i][0][r];
            }
        }
}

// dW[o][c][ky][kx] = sum over splits (fixed order) of partial[s][tap][o][c]
__global__ void wgrad_reduce_kernel(const float *__restrict__ partial, float *__restrict__ dw, int splits, int taps,
                                    int Cout, int Cin)
{
    const long long total = (long long)taps * Cout * Cin;
    partial += (long long)blockIdx.y * splits * total;              // batched launch: one block of partials per GEMM
    dw += (long long)blockIdx.y * total;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int k = 0; k < splits; ++k) s += partial[(long long)k * total + i];
        const int c = (int)(i % Cin);
        long long t = i / Cin;
        const int o = (int)(t % Cout);
        const int tap = (int)(t / Cout);
        dw[((long long)o * Cin + c) * taps + tap] = s;
    }
}

template <int BO, int BC, int WO, int WC>
int launch_wgrad(const xl_op &op, hipStream_t st)
{
    WgradArgs a;
    a.x = (const float *)op.in; a.dy = (const float *)op.aux; a.partial = (float *)op.stats2;
    a.B = op.B; a.Hi = op.Hi; a.Wi = op.Wi; a.Cin = op.Cin; a.Ho = op.Ho; a.Wo = op.Wo; a.Cout = op.Cout;
    a.ldX = op.ld_in; a.ldY = op.ld_aux; a.ksize = op.ksize; a.stride = op.stride;
    a.M = op.B * op.Ho * op.Wo; a.splits = op.nchunks2;
    a.mPerSplit = ((a.M + a.splits - 1) / a.splits + 31) / 32 * 32;
    a.nbo = op.Cout / BO; a.nbc = op.Cin / BC;
    a.zCount = op.groups > 1 ? op.groups : 1;                     // WGRAD: groups = GEMMs per launch
    if (a.zCount > 1 && (op.ksize != 1 || op.ld_in != op.Cin || op.ld_aux != op.Cout)) return XL_ERR_ARG;
    a.zX = (long long)a.M * op.Cin; a.zY = (long long)a.M * op.Cout;
    const long long xb = (((long long)op.B * op.Hi * op.Wi - 1) * op.ld_in + op.Cin) * 4;
    const long long yb = (((long long)a.M - 1) * op.ld_aux + op.Cout) * 4;
    if (xb >= 0x7fffffffLL || yb >= 0x7fffffffLL) return XL_ERR_ARG;
    if (op.Ho * op.Wo < 32) return XL_ERR_UNSUPPORTED;          // the kernel advances pixel coordinates by one K-step (32)
    a.xBytes = (unsigned)xb; a.dyBytes = (unsigned)yb;
    const int taps = op.ksize * op.ksize;
    hipLaunchKernelGGL((wgrad_kernel<BO, BC, WO, WC>), dim3(a.zCount * taps * a.nbo * a.nbc * a.splits), dim3(64 * WO * WC), 0, st, a);
    const long long total = (long long)taps * op.Cout * op.Cin;
    const unsigned blocks = xl_grid(total, 256, 2048);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks, a.zCount), dim3(256), 0, st, (const float *)op.stats2,
                       (float *)op.out, a.splits, taps, op.Cout, op.Cin);
    return XL_OK;
}

// ---------------------------------------------------------------------------------------------- Winograd weight gradient

// Weight gradient of a stride-1 3x3 layer through F(4x4,3x3): with V = B^T x B (wino4_in_kernel) and dM = A dY A^T per
// 4x4 output tile, dU[xi][co][ci] = sum_tiles dM[xi][t][co] V[xi][t][ci] is 36 GEMMs with the TILES as the K dimension
// (the batched wgrad_kernel above, 4x fewer multiplies than the 9-tap form), and dg = G^T dU G.
template <typename V>
__device__ __forceinline__ void wino4_a(const V (&d)[4], V (&o)[6])      // A = (A^T)^T, 6x4
{
    o[0] = d[0];
    o[1] = d[0] + d[1] + d[2] + d[3];
    o[2] = d[0] - d[1] + d[2] - d[3];
    o[3] = d[0] + 2.f * d[1] + 4.f * d[2] + 8.f * d[3];
    o[4] = d[0] - 2.f * d[1] + 4.f * d[2] - 8.f * d[3];
    o[5] = d[3];
}

// dY [B,H,W,C] (pixel stride ld) -> dM [36][B*Th*Tw][C]; one tile x 2 channels per thread; pixels past H / W are zero
__global__ __launch_bounds__(256)
void wino4_dy_kernel(const float *__restrict__ dy, float *__restrict__ dM, int B, int H, int W, int C, int ld, int Th, int Tw)
{
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
        f32x2 w[6][4];                               // w[i][q] = (A dY)[i][q]
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int x = 4 * tx + q;
            f32x2 col[4], o[6];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int y = 4 * ty + p;
                if (y < H && x < W) col[p] = *reinterpret_cast<const f32x2 *>(dy + (((long long)n * H + y) * W + x) * ld + 2 * c2);
                else col[p] = f32x2{ 0.f, 0.f };
            }
            wino4_a(col, o);
#pragma unroll
            for (int i = 0; i < 6; ++i) w[i][q] = o[i];
        }
        float *op = dM + t * C + 2 * c2;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            f32x2 o[6];
            wino4_a(w[i], o);
#pragma unroll
            for (int j = 0; j < 6; ++j) *reinterpret_cast<f32x2 *>(op + (6 * i + j) * zs) = o[j];
        }
    }
}

// dg[o][c][a][b] = sum_ij G[i][a] dU[6i+j][o][c] G[j][b]  (G of F(4x4,3x3)); one (o, c) per thread, OIHW output
__global__ __launch_bounds__(256)
void wino4_wfinal_kernel(const float *__restrict__ dU, float *__restrict__ dw, int Cout, int Cin)
{
    const long long total = (long long)Cout * Cin;
    const float G[6][3] = { { 0.25f, 0.f, 0.f }, { -1.f / 6, -1.f / 6, -1.f / 6 }, { -1.f / 6, 1.f / 6, -1.f / 6 },
                            { 1.f / 24, 1.f / 12, 1.f / 6 }, { 1.f / 24, -1.f / 12, 1.f / 6 }, { 0.f, 0.f, 1.f } };
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        float u[6][6];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 6; ++b) u[a][b] = dU[(long long)(6 * a + b) * total + i];
        float t[3][6];                               // t = G^T u
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                float v = 0.f;
#pragma unroll
                for (int k = 0; k < 6; ++k) v = fmaf(G[k][a], u[k][b], v);
                t[a][b] = v;
            }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                float v = 0.f;
#pragma unroll
                for (int k = 0; k < 6; ++k) v = fmaf(t[a][k], G[k][b], v);
                dw[i * 9 + a * 3 + b] = v;
            }
    }
}

// The same through F(6x6,3x3): dM = A dY A^T per 6x6 output tile (A = (A^T)^T, 8x6), 64 GEMMs, dg = G^T dU G with the
// 8x3 G.  Measured against float64 on a 64-channel layer: 9e-6 of max|ref| (F(4x4,3x3): 6e-6).
template <typename V>
__device__ __forceinline__ void wino6_a(const V (&d)[6], V (&o)[8])
{
    const V e = d[0] + d[2] + d[4], f = d[1] + d[3] + d[5];
    const V g = d[0] + 4.f * d[2] + 16.f * d[4], h = 2.f * d[1] + 8.f * d[3] + 32.f * d[5];
    const V k = 32.f * d[0] + 8.f * d[2] + 2.f * d[4], l = 16.f * d[1] + 4.f * d[3] + d[5];
    o[0] = d[0];
    o[1] = e + f; o[2] = e - f;
    o[3] = g + h; o[4] = g - h;
    o[5] = k + l; o[6] = k - l;
    o[7] = d[5];
}

// dY [B,H,W,C] (pixel stride ld) -> dM [64][B*Th*Tw][C]; one tile x 2 channels per thread; pixels past H / W are zero.
// Round 5: the largest magnitude the pass writes goes to `amax`, for the fp16-pair GEMMs that consume its result (csrc/xl_gemm_pair.hip,
// csrc/xl_wgrad_pair.hip: a gradient has no static bound, so its power-of-two scale comes from the data): every thread keeps a
// running maximum, a wave combines its 64 with a DPP tree, at most one atomicMax per wave on the float's bits (xl_wave_max_commit,
// csrc/xl_common.h).  The slot is zeroed by an XL_OP_FILL0 at the head of the backward op list.
__global__ __launch_bounds__(256)
void wino6_dy_kernel(const float *__restrict__ dy, float *__restrict__ dM, int B, int H, int W, int C, int ld, int Th, int Tw,
                     unsigned *__restrict__ amax)
{
    float mx = 0.f;
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
        f32x2 w[8][6];                               // w[i][q] = (A dY)[i][q]
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const int x = 6 * tx + q;
            f32x2 col[6], o[8];
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                const int y = 6 * ty + p;
                if (y < H && x < W) col[p] = *reinterpret_cast<const f32x2 *>(dy + (((long long)n * H + y) * W + x) * ld + 2 * c2);
                else col[p] = f32x2{ 0.f, 0.f };
            }
            wino6_a(col, o);
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i][q] = o[i];
        }
        float *op = dM + t * C + 2 * c2;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            f32x2 o[8];
            wino6_a(w[i], o);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                *reinterpret_cast<f32x2 *>(op + (8 * i + j) * zs) = o[j];
                mx = fmaxf(mx, fmaxf(fabsf(o[j][0]), fabsf(o[j][1])));
            }
        }
    }
    xl_wave_max_commit(mx, amax);
}

// dg[o][c][a][b] = sum_ij G[i][a] dU[8i+j][o][c] G[j][b]  (G of F(6x6,3x3)); one (o, c) per thread, OIHW output
__global__ __launch_bounds__(256)
void wino6_wfinal_kernel(const float *__restrict__ dU, float *__restrict__ dw, int Cout, int Cin)
{
    const long long total = (long long)Cout * Cin;
    const float G[8][3] = { { 1.f, 0.f, 0.f }, { -2.f / 9, -2.f / 9, -2.f / 9 }, { -2.f / 9, 2.f / 9, -2.f / 9 },
                            { 1.f / 90, 1.f / 45, 2.f / 45 }, { 1.f / 90, -1.f / 45, 2.f / 45 },
                            { 1.f / 45, 1.f / 90, 1.f / 180 }, { 1.f / 45, -1.f / 90, 1.f / 180 }, { 0.f, 0.f, 1.f } };
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        float t[3][8];                               // t = G^T u, built row by row of u
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) t[a][b] = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const float u = dU[(long long)(8 * k + b) * total + i];
#pragma unroll
                for (int a = 0; a < 3; ++a) t[a][b] = fmaf(G[k][a], u, t[a][b]);
            }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                float v = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) v = fmaf(t[a][k], G[k][b], v);
                dw[i * 9 + a * 3 + b] = v;
            }
    }
}

}  // namespace

int xl_run_wgrad(const xl_op &op, hipStream_t st)
{
    if (op.nchunks2 < 1 || op.ld_in % 4 != 0 || op.ld_aux % 4 != 0) return XL_ERR_ARG;
    if (op.flags & XL_CONV_SPLIT_BF16) {                      // 1x1 / batched Winograd products on the bf16 pipe
        if (op.nchunks2 == 1) {
            // one split (the 64 batched products of a Winograd layer fill the chip without splitting K): the "partial"
            // tile IS the result, [z][Cout][Cin] - written in place, no reduce pass (it was a 134 MB copy per layer)
            xl_op direct = op;
            direct.stats2 = op.out;
            return (op.flags & XL_CONV_PAIR_F16) ? xl_run_wgrad_pair(direct, st) : xl_run_wgrad_split(direct, st);
        }
        const int rc = (op.flags & XL_CONV_PAIR_F16) ? xl_run_wgrad_pair(op, st) : xl_run_wgrad_split(op, st);
        if (rc != XL_OK) return rc;
        const unsigned blocks = xl_grid((long long)op.Cout * op.Cin, 256, 2048);
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks, op.groups > 1 ? op.groups : 1), dim3(256), 0, st,
                           (const float *)op.stats2, (float *)op.out, op.nchunks2, 1, op.Cout, op.Cin);
        return XL_OK;
    }
    if (op.Cout % 128 == 0 && op.Cin % 128 == 0) return launch_wgrad<128, 128, 2, 2>(op, st);
    if (op.Cout % 128 == 0 && op.Cin % 64 == 0) return launch_wgrad<128, 64, 2, 2>(op, st);
    if (op.Cout % 64 == 0 && op.Cin % 32 == 0) return launch_wgrad<64, 32, 2, 1>(op, st);
    return XL_ERR_UNSUPPORTED;
}

int xl_run_wino_dy(const xl_op &op, hipStream_t st)
{
    // ksize = output tile m of F(m x m, 3x3): 4 (default) or 6
    const int m = op.ksize == 6 ? 6 : 4;
    if (op.Cin % 2 != 0 || op.ld_in % 2 != 0 || op.Ho != (op.Hi + m - 1) / m || op.Wo != (op.Wi + m - 1) / m) return XL_ERR_ARG;
    const long long items = (long long)op.B * op.Ho * op.Wo * (op.Cin / 2);
    const unsigned blocks = xl_grid(items, 256, 262144);
    if (m == 6)
        hipLaunchKernelGGL(wino6_dy_kernel, dim3(blocks), dim3(256), 0, st, (const float *)op.in, (float *)op.out,
                           op.B, op.Hi, op.Wi, op.Cin, op.ld_in, op.Ho, op.Wo, (unsigned *)op.scale);   // scale: max |dM| slot (optional)
    else
        hipLaunchKernelGGL(wino4_dy_kernel, dim3(blocks), dim3(256), 0, st, (const float *)op.in, (float *)op.out,
                           op.B, op.Hi, op.Wi, op.Cin, op.ld_in, op.Ho, op.Wo);
    return XL_OK;
}

int xl_run_wino_wfinal(const xl_op &op, hipStream_t st)
{
    const unsigned blocks = xl_grid((long long)op.Cout * op.Cin, 256, 4096);
    hipLaunchKernelGGL(op.ksize == 6 ? wino6_wfinal_kernel : wino4_wfinal_kernel, dim3(blocks), dim3(256), 0, st,
                       (const float *)op.in, (float *)op.out, op.Cout, op.Cin);
    return XL_OK;
}
