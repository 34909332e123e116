// xl_igemm.hip — XL_OP_CONV on exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): every convolution the split and pair pipes do not take
// (fallbacks, data gradients, the fp32 Winograd GEMMs) as an implicit GEMM, M = B*Ho*Wo pixels, N = Cout, K = k*k*Cin.
#include <hip/hip_runtime.h>
#include <array>
#include <map>
#include <vector>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>

#include "xl_launch.h"
#include "xl_operand_math.h"

namespace {

// ---------------------------------------------------------------------------------------------- igemm conv

constexpr int kWaitVm0 = 0x0F70;                   // s_waitcnt vmcnt(0) (expcnt / lgkmcnt fields left at their maxima)
constexpr int kBK = 32;                            // K-step; one LDS tile row = 32 floats (128 B)

struct ConvArgs {
    const float *in; const float *w; const float *bias; float *out;
    int B, Hi, Wi, Cin, Ho, Wo, Cout, ldIn, ldOut;
    int M, K, nbm, nbn;
    unsigned inBytes, wBytes, outBytes;   // extents for the buffer descriptors (hardware bounds check)
    int accumulate;                 // epilogue: out += result (XL_CONV_ACCUMULATE)
    // fused GroupNorm statistics of the OUTPUT (forward only): fp64 partial sums per (image, tile-within-image, group)
    double *stats; int HW, G, cpg, nchunks;
    // MODE 2 (stride-2 data gradient, one parity class of result pixels per launch)
    int py, px, Hj, Wj, ntaps; unsigned tapList;
    // batched launch (Winograd: 16 independent GEMMs): tile t of the grid belongs to GEMM z = t / (nbm*nbn)
    int zCount; long long zIn, zW, zOut;   // element strides between consecutive GEMMs
    long long *clk;                 // diagnostics (XL_CONV_CLK=1): per-workgroup shader-clock phase timings, else NULL
    // NORM launches: the producer's GroupNorm is applied to the A operand on its way into LDS ("normalise on load"):
    // coef = {scale, shift} pairs [B][Cin][2] from GN_FINAL, x -> max(x*scale + shift, normLo), normLo = 0 (ReLU) or -inf
    const float *coef; float normLo;
};

// Tiles go global -> LDS directly (buffer_load ... lds through buffer descriptors): no register staging and no
// ds_write phase.  A padding tap gets an out-of-range offset and the hardware writes zeros (no branch, no select on
// the data).  LDS rows are unpadded (32 floats = 128 B = 8 lanes x 16 B, the lane-linear DMA destination); the 16-byte
// slots of a row are XOR-swizzled by (row>>1)&7, applied to the SOURCE offset of the lane that fills a slot and again
// to the fragment reads, which keeps ds_read_b128 conflict-free without padding.
// MODE 0: forward convolution.  MODE 1: data gradient — `in` is dY [B,Hi,Wi,Cin] (the forward OUTPUT, Cin = forward
// Cout), the result is dX [B,Ho,Wo,Cout] (forward input); output pixel (iy,ix) gathers dY[(iy+PAD-ky)/S][(ix+PAD-kx)/S]
// for the taps whose offset is divisible by the forward stride S (others are zero-filled by the bounds check).
// MODE 2: the stride-2 data gradient split by result-pixel parity (py,px): only the 1/2/2/4 taps that can reach a
// pixel of that class are multiplied (9 tap-GEMMs in total over the four launches instead of 36).
// NORM (1x1 forward launches only): the A operand is the RAW output of the producing convolution and its GroupNorm
// (+ReLU) is applied on the way into LDS, so the producer's separate apply pass (one read + one write of the
// activation) does not exist.  The A tile then goes global -> registers -> x*scale + shift -> ds_write instead of by
// DMA (the weights still go by DMA); the per-(image, channel) coefficients of the at most two images a tile touches
// sit in LDS behind the tiles.
template <int KS, int STRIDE, int BN, int CIN, int MODE = 0, int BM = 128, int ZB = 0, int NORM = 0>   // CIN = compile-time Cin tag (0: runtime);
                                         // BM = 64 for launches that would not fill the chip; ZB 1 = batched GEMMs (Winograd)
__global__ __launch_bounds__(256, 2)
void igemm_conv_kernel(ConvArgs a)
{
    static_assert(!NORM || (KS == 1 && STRIDE == 1 && MODE == 0 && ZB == 0), "normalise-on-load exists for 1x1 forward convs");
    constexpr int PAD = KS / 2;
    // The MFMA row operand is the WEIGHT fragment ("swapped"), so an accumulator register quad holds 4 consecutive output
    // channels of one pixel = 16 contiguous bytes of the NHWC result: the epilogue needs 16 dwordx4 stores per wave
    // instead of 64 dword stores.  It matters because the epilogue runs beside the co-resident workgroup's MFMA stream
    // and pays per INSTRUCTION there (XL_CONV_CLK: 27k ticks for the 64-store form with two workgroups per CU, 50k with
    // the per-element statistics on top, 6k for this form); while a workgroup sits in its epilogue its partner cannot
    // keep the matrix pipe full alone, so a long epilogue costs pipe time, not only latency: the 1x1 512->512 layers
    // ran at 78 % with the long one.  Forward launches start the accumulators at the bias instead of adding it per
    // element, and take the GroupNorm statistics from per-lane partial sums (below).
    constexpr int NJ = BN / 64;                 // 32-wide MFMA tiles per wave along N
    constexpr int BROWS = BN / 32;              // B-tile rows loaded per thread
    constexpr int AROWS = BM / 32;              // A-tile rows loaded per thread
    constexpr int TI = BM / 64;                 // 32-high MFMA tiles per wave along M
    constexpr unsigned OOB = 0x80000000u;       // > any legal extent: forces the zero-fill path
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *As = smem;                           // [2][BM][32]
    float *Bs = smem + 2 * BM * kBK;            // [2][BN][32]
    if (CIN != 0) a.Cin = CIN, a.K = KS * KS * CIN;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;

    // each XCD gets a contiguous run of (GEMM, m-tile, n-tile): the n-tiles of an m-tile share an L2
    int tile = xcd_remap(blockIdx.x, a.nbm * a.nbn * (ZB ? a.zCount : 1));
    if constexpr (ZB) {
        const int z = tile / (a.nbm * a.nbn);
        tile -= z * (a.nbm * a.nbn);
        a.in += z * a.zIn; a.w += z * a.zW; a.out += z * a.zOut;
    }
    const int mt = tile / a.nbn, nt = tile - mt * a.nbn;
    const int m0 = mt * BM, n0 = nt * BN;

    const __amdgpu_buffer_rsrc_t srdA = __builtin_amdgcn_make_buffer_rsrc((void *)a.in, 0, (int)a.inBytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t srdB = __builtin_amdgcn_make_buffer_rsrc((void *)a.w, 0, (int)a.wBytes, 0x00020000);

    // ---- per-thread load coordinates: AROWS A rows (and BROWS B rows); this lane fills physical slot tid&7 of its
    // rows with the logical k-slot kq
    const int lrow = tid >> 3;
    const int kq = (tid & 7) ^ ((lrow >> 1) & 7);
    unsigned aOff[AROWS];                           // byte offset of (n, iy0, ix0, 4*kq); wraps for padding rows
    int aIy[AROWS], aIx[AROWS];
    const int HoWo = (MODE == 2) ? a.Hj * a.Wj : a.Ho * a.Wo;
    const int rowW = (MODE == 2) ? a.Wj : a.Wo;
#pragma unroll
    for (int p = 0; p < AROWS; ++p) {
        const int m = m0 + lrow + 32 * p;
        if (m < a.M) {
            const int n = m / HoWo;
            const int rem = m - n * HoWo;
            const int oy = rem / rowW, ox = rem - oy * rowW;
            if constexpr (MODE == 0) {
                aIy[p] = oy * STRIDE - PAD;
                aIx[p] = ox * STRIDE - PAD;
                aOff[p] = (unsigned)(((n * a.Hi + aIy[p]) * a.Wi + aIx[p]) * a.ldIn + 4 * kq) * 4u;
            } else if constexpr (MODE == 1) {
                aIy[p] = oy + PAD;                   // numerators of the source row / column
                aIx[p] = ox + PAD;
                aOff[p] = (unsigned)(n * a.Hi * a.Wi * a.ldIn + 4 * kq) * 4u;
            } else {
                aIy[p] = 2 * oy + a.py + PAD;
                aIx[p] = 2 * ox + a.px + PAD;
                aOff[p] = (unsigned)(n * a.Hi * a.Wi * a.ldIn + 4 * kq) * 4u;
            }
        } else {
            aIy[p] = -100000; aIx[p] = -100000; aOff[p] = 0;
        }
    }
    unsigned bOff[BROWS];
#pragma unroll
    for (int p = 0; p < BROWS; ++p) bOff[p] = (unsigned)((n0 + lrow + 32 * p) * a.K + 4 * kq) * 4u;

    typedef __attribute__((address_space(3))) void lds_void;
    // Source offsets of K-step kk: A rows (per lane, OOB for padding taps) and the weight K position (scalar)
    auto tile_offsets = [&](int kk, unsigned (&voff)[AROWS], unsigned &kbytes) {
        // K order is (channel chunk of 32, tap, channel-in-chunk): the 9 taps of one chunk run back to back, so
        // the shifted re-reads of the same input pixels hit L1/L2 instead of going back to HBM 9 times
        int kbase = kk * kBK;
        int chunk, tap;
        if constexpr (MODE == 2) {
            chunk = kk / a.ntaps;
            tap = (int)((a.tapList >> (4 * (kk - chunk * a.ntaps))) & 15u);
            kbase = (chunk * (KS * KS) + tap) * kBK;             // position of this (chunk, tap) in the packed weights
        } else {
            chunk = kk / (KS * KS);
            tap = kk - chunk * (KS * KS);
        }
        kbytes = (unsigned)kbase * 4u;
        const int c0 = chunk * kBK;
        const int ky = tap / KS, kx = tap - ky * KS;
        const unsigned tapOff = (unsigned)((ky * a.Wi + kx) * a.ldIn + c0) * 4u;
#pragma unroll
        for (int p = 0; p < AROWS; ++p) {
            if constexpr (MODE == 0) {
                const bool ok = (unsigned)(aIy[p] + ky) < (unsigned)a.Hi && (unsigned)(aIx[p] + kx) < (unsigned)a.Wi;
                voff[p] = ok ? aOff[p] + tapOff : OOB;
            } else {
                const int ty = aIy[p] - ky, tx = aIx[p] - kx;
                const int sy = ty / STRIDE, sx = tx / STRIDE;               // STRIDE is 1 or 2 (shift)
                // (bitwise &: a short-circuit chain becomes nested exec-masked branches)
                const bool ok = ((ty | tx) >= 0) & (STRIDE == 1 || (((ty | tx) & 1) == 0)) & (sy < a.Hi) & (sx < a.Wi);
                // mask arithmetic, not a select: hipcc turns the select into an exec-masked branch around the
                // multiplies, which splits the K-loop into basic blocks that do not overlap with the MFMAs
                const unsigned msk = 0u - (unsigned)ok;
                voff[p] = ((aOff[p] + (unsigned)((sy * a.Wi + sx) * a.ldIn + c0) * 4u) & msk) | (OOB & ~msk);
            }
        }
    };
    // one wave instruction moves 8 rows x 128 B; destination = wave-uniform base (M0) + lane*16
    auto issue_dma_a = [&](const unsigned (&voff)[AROWS], int buf) {
#pragma unroll
        for (int p = 0; p < AROWS; ++p)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(srdA, (lds_void *)(As + (buf * BM + 32 * p + 8 * wave) * kBK), 16,
                                                     (int)voff[p], 0, 0, 0);
    };
    auto issue_dma_b = [&](unsigned kbytes, int buf) {
#pragma unroll
        for (int p = 0; p < BROWS; ++p)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(srdB, (lds_void *)(Bs + (buf * BN + 32 * p + 8 * wave) * kBK), 16,
                                                     (int)bOff[p], (int)kbytes, 0, 0);
    };
    auto load_dma = [&](int kk, int buf) {
        unsigned voff[AROWS], kbytes;
        tile_offsets(kk, voff, kbytes);
        if constexpr (!NORM) issue_dma_a(voff, buf);
        issue_dma_b(kbytes, buf);
    };
    // ---- NORM: A through registers.  This thread owns the 16-byte slot (row lrow + 32p, physical slot tid&7) of every
    // K-step - the slot the DMA form fills through it - holding channels 4*kq .. 4*kq+3 of the step's 32-channel chunk.
    float *sCoef = smem + 2 * (BM + BN) * kBK;                  // [2 image slots][Cin][2]
    int coefSlot[AROWS];                                        // float offset of this row's image slot in sCoef
    f32x4 aReg[AROWS];
    auto load_a_regs = [&](const unsigned (&voff)[AROWS]) {
#pragma unroll
        for (int p = 0; p < AROWS; ++p)
            aReg[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdA, (int)voff[p], 0, 0));
    };
    f32x4 cf[AROWS][2];                                         // {s0 t0 s1 t1}, {s2 t2 s3 t3} of the row's image
    auto load_coefs = [&](int kk) {                             // issued a K-step ahead: never waited for in the tail
        const int c = kk * kBK + 4 * kq;                        // first of this thread's 4 channels
#pragma unroll
        for (int p = 0; p < AROWS; ++p) {
            cf[p][0] = *reinterpret_cast<const f32x4 *>(sCoef + coefSlot[p] + 2 * c);
            cf[p][1] = *reinterpret_cast<const f32x4 *>(sCoef + coefSlot[p] + 2 * c + 4);
        }
    };
    auto store_a_regs = [&](int buf, int pLo, int pHi) {        // normalise + ds_write rows [pLo, pHi) into stage `buf`
#pragma unroll
        for (int p = 0; p < AROWS; ++p) {
            if (p < pLo || p >= pHi) continue;
            f32x4 v = aReg[p];
            v[0] = fmaxf(fmaf(v[0], cf[p][0][0], cf[p][0][1]), a.normLo);
            v[1] = fmaxf(fmaf(v[1], cf[p][0][2], cf[p][0][3]), a.normLo);
            v[2] = fmaxf(fmaf(v[2], cf[p][1][0], cf[p][1][1]), a.normLo);
            v[3] = fmaxf(fmaf(v[3], cf[p][1][2], cf[p][1][3]), a.normLo);
            *reinterpret_cast<f32x4 *>(As + (buf * BM + 32 * p + lrow) * kBK + 4 * (tid & 7)) = v;
        }
    };

    // C layout (swapped operands): pixel = tile column lane&31, channel = (r&3) + 8*(r>>2) + 4*(lane>>5) of a 32x32 block
    const int rhalf = (lane >> 5) * 4;
    const int nLane = n0 + wn * (BN / 2) + rhalf;                  // + j*32 + 8*q: first of 4 consecutive channels
    f32x16 acc[TI][NJ];
    if constexpr (MODE == 0 && ZB == 0) {
        // forward: the accumulators start at the bias (a null bias reads as zeros through the bounds check)
        const __amdgpu_buffer_rsrc_t srdBias = __builtin_amdgcn_make_buffer_rsrc((void *)a.bias, 0, a.bias ? a.Cout * 4 : 0, 0x00020000);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 b4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdBias, (nLane + j * 32 + 8 * q) * 4, 0, 0));
#pragma unroll
                for (int i = 0; i < TI; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[i][j][4 * q + e] = b4[e];
            }
    } else {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    }

    long long tc0 = 0, tw0 = 0, tc1 = 0, tc2 = 0;
    if (a.clk) { tc0 = clock64(); tw0 = wall_clock64(); }
    const int nk = (MODE == 2) ? a.ntaps * (a.Cin / kBK) : a.K / kBK;
    load_dma(0, 0);
    load_dma(1, 1);                                   // (nk == 1: an unused tile, drained with the others below)
    if constexpr (NORM) {
        // coefficient rows of the two images this tile can touch (HW >= BM) by DMA, the first two A stages through
        // registers; everything is issued before the first wait
        const int nLoN = m0 / a.HW;
        const int splitN = (nLoN + 1) * a.HW - m0;              // first tile row of the second image
#pragma unroll
        for (int p = 0; p < AROWS; ++p) coefSlot[p] = (lrow + 32 * p >= splitN) ? 2 * a.Cin : 0;
        const int n1 = (nLoN + 1 < a.B) ? nLoN + 1 : nLoN;
        const __amdgpu_buffer_rsrc_t srdC = __builtin_amdgcn_make_buffer_rsrc((void *)a.coef, 0, a.B * a.Cin * 8, 0x00020000);
        // a wave instruction moves 1 KB = 128 {scale, shift} pairs; wave w copies pieces w, w+4, ... of 2*Cin/128
        for (int pc = wave; pc < (2 * a.Cin) / 128; pc += 4) {
            const int img = pc / (a.Cin / 128), part = pc - img * (a.Cin / 128);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(srdC, (lds_void *)(sCoef + img * 2 * a.Cin + part * 256), 16,
                                                     (int)(((img ? n1 : nLoN) * a.Cin + part * 128) * 8 + lane * 16), 0, 0, 0);
        }
        unsigned v0[AROWS], v1[AROWS], kb;
        f32x4 aReg1[AROWS];
        tile_offsets(0, v0, kb);
        tile_offsets(1, v1, kb);
        load_a_regs(v0);
#pragma unroll
        for (int p = 0; p < AROWS; ++p)
            aReg1[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdA, (int)v1[p], 0, 0));
        __builtin_amdgcn_s_waitcnt(kWaitVm0);
        __syncthreads();                                        // the table is complete
        load_coefs(0);
        store_a_regs(0, 0, AROWS);
#pragma unroll
        for (int p = 0; p < AROWS; ++p) aReg[p] = aReg1[p];
        load_coefs(1);
        store_a_regs(1, 0, AROWS);
    }
    // An LDS-DMA is ordered for other waves' ds_reads only by the issuing wave's vmcnt wait followed by a barrier;
    // the workgroup fence of __syncthreads() waits for LDS operations (lgkmcnt) only, so the vmcnt(0) is explicit.
    __builtin_amdgcn_s_waitcnt(kWaitVm0);
    __syncthreads();
    if (a.clk) tc1 = clock64();

    // MFMA 32x32x2: lane l multiplies row l&31 at k = l>>5.  One ds_read_b128 per 32-row fragment holds the four
    // k-values 4*slot..4*slot+3 of logical slot 2c + (l>>5) of chunk c; the e-th element feeds the e-th MFMA.
    const int fragRow = lane & 31, khalf = lane >> 5;
    const int swz = (fragRow >> 1) & 7;
    const float *Afrag = As + (wm * (BM / 2) + fragRow) * kBK;
    const float *Bfrag = Bs + (wn * (BN / 2) + fragRow) * kBK;
    int cOff[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) cOff[c] = ((2 * c + khalf) ^ swz) * 4;
    // Fragments ping-pong between two register sets: chunk c+1 is read from LDS while chunk c multiplies, across
    // K-steps too (the last chunk of a step prefetches the first fragments of the next one from the other buffer).
    f32x4 fa[2][TI], fb[2][NJ];
    auto read_frags = [&](int set, int buf, int c) {
#pragma unroll
        for (int i = 0; i < TI; ++i) fa[set][i] = *reinterpret_cast<const f32x4 *>(Afrag + (buf * BM + i * 32) * kBK + cOff[c]);
#pragma unroll
        for (int j = 0; j < NJ; ++j) fb[set][j] = *reinterpret_cast<const f32x4 *>(Bfrag + (buf * BN + j * 32) * kBK + cOff[c]);
    };
    auto multiply_e = [&](int set, int e) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[set][j][e], fa[set][i][e], acc[i][j], 0, 0, 0);
    };
    auto multiply = [&](int set) {
#pragma unroll
        for (int e = 0; e < 4; ++e) multiply_e(set, e);
    };
    read_frags(0, 0, 0);
    // One barrier per K-step, placed before its LAST chunk: by then every wave has issued all its reads of the
    // current buffer (so the DMA of step kk+2 may overwrite it) and, after the vmcnt(0) of the fence, the tile of
    // step kk+1 has landed in the other buffer (so the cross-step prefetch may read it).  Each DMA has a full
    // K-step (4096 MFMA cycles) to land.  Within a chunk the order is pinned to [first MFMA] [fragment reads of the
    // next chunk] [remaining MFMAs]: the reads start early in the shadow of the MFMA stream and are the only LDS
    // operations outstanding when the next chunk needs them.  The loop body is branch-free (a branch would split
    // the scheduling region): the two DMAs past the last K-step fetch out-of-range / unused data into a buffer
    // nobody reads, and are drained before the epilogue reuses the LDS.
    constexpr int NM = 4 * TI * NJ, ND = TI + NJ, NV = AROWS + BROWS;
    for (int kk = 0; kk < nk; ++kk) {
        const int buf = kk & 1;
        unsigned voffN[AROWS], kbytesN;                // offsets of step kk+2, computed under the MFMAs of this one
        tile_offsets(kk + 2, voffN, kbytesN);
        if constexpr (NORM) {
            // A of step kk+2 and its coefficients: issued first (in the shadow of the MFMAs still executing), in flight
            // for the whole K-step (past the last step: reads of unused data inside the allocations)
            load_a_regs(voffN);
            load_coefs(kk + 2);
            __builtin_amdgcn_sched_barrier(0);
        }
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
        __builtin_amdgcn_sched_barrier(0);            // nothing moves across: the MFMAs are not ordered by the fence
        __builtin_amdgcn_s_waitcnt(kWaitVm0);         // tile kk+1 (issued one K-step ago) has landed
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        // last chunk: MFMAs first, then the DMA issue and the cross-step fragment prefetch in their shadow
        // (ALU may move across the fences, MFMA / LDS / VMEM instructions may not)
        multiply_e(1, 0);
        __builtin_amdgcn_sched_barrier(0x6);
        if constexpr (NORM) store_a_regs(buf, 0, AROWS / 2);
        else issue_dma_a(voffN, buf);
        __builtin_amdgcn_sched_barrier(0x6);
        multiply_e(1, 1);
        __builtin_amdgcn_sched_barrier(0x6);
        issue_dma_b(kbytesN, buf);
        read_frags(0, buf ^ 1, 0);
        __builtin_amdgcn_sched_barrier(0x6);
        multiply_e(1, 2);
        if constexpr (NORM) {
            __builtin_amdgcn_sched_barrier(0x6);
            store_a_regs(buf, AROWS / 2, AROWS);
            __builtin_amdgcn_sched_barrier(0x6);
        }
        multiply_e(1, 3);
    }
    __builtin_amdgcn_s_waitcnt(kWaitVm0);             // drain the trailing DMAs before the epilogue reuses the LDS
    __syncthreads();

    if (a.clk) tc2 = clock64();
    // ---- epilogue.  Branch-free stores: out-of-range rows / columns get an out-of-range buffer offset (stores dropped,
    // loads return 0); with branches the compiler must assume a load pending at every block entry and emits vmcnt(0)
    // before each store.  The accumulate switch is a compile-time tag for the same reason.
    const __amdgpu_buffer_rsrc_t srdO = __builtin_amdgcn_make_buffer_rsrc((void *)a.out, 0, (int)a.outBytes, 0x00020000);
    unsigned pixOff[TI];
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        const int m = m0 + wm * (BM / 2) + i * 32 + (lane & 31);
        int pix = m;
        if constexpr (MODE == 2) {
            const int nn = m / HoWo;
            const int rem = m - nn * HoWo;
            const int jy = rem / a.Wj, jx = rem - jy * a.Wj;
            pix = (nn * a.Ho + 2 * jy + a.py) * a.Wo + 2 * jx + a.px;
        }
        pixOff[i] = (m < a.M) ? (unsigned)(pix * a.ldOut) * 4u : OOB;
    }
    auto store_swapped = [&](auto accTag) {
        constexpr bool ACC = decltype(accTag)::value;
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                unsigned off[4];
                f32x4 old[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int n = nLane + j * 32 + 8 * q;
                    off[q] = (n < a.Cout && pixOff[i] != OOB) ? pixOff[i] + (unsigned)n * 4u : OOB;
                    if constexpr (ACC) old[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdO, (int)off[q], 0, 0));
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f32x4 v = f32x4{ acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3] };
                    if constexpr (ACC) v += old[q];
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), srdO, (int)off[q], 0, 0);
                }
            }
    };
    if (a.accumulate) store_swapped(std::true_type{});
    else store_swapped(std::false_type{});

    // Fused GroupNorm statistics of the OUTPUT (forward only).  A BM-row tile touches at most two images (HW >= BM):
    // slot 0 = rows before `split`, slot 1 = the rest.  Three fixed-order stages, one writer per (image, tile, group):
    //   1. per lane, fp32: sum and sum of squares of each PG-channel piece of its TI pixels, per slot -> LDS
    //      (a lane holds 16 channels per 32-wide block as 4 quads; PG = 4, or 2 when a group has only 2 channels);
    //   2. per (piece, slot), fp64: over the 2 waves and 32 pixel lanes that hold the piece, in index order;
    //   3. per (group, slot), fp64: over the pieces of the group, in channel order.
    if constexpr (MODE == 0 && ZB == 0) {
        if (a.stats != nullptr) {
            const int nLo = m0 / a.HW;
            const int split = (nLo + 1) * a.HW - m0;
            float *sP = smem;                                      // [256 threads][2 slots][NP][2], tiles are dead now
            auto stage1 = [&](auto pgTag) {
                constexpr int PG = decltype(pgTag)::value;         // channels per piece
                constexpr int PQ = 4 / PG;                         // pieces per register quad
                constexpr int NP = NJ * 4 * PQ;                    // pieces per lane
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int h = 0; h < PQ; ++h) {
                            float s[2] = { 0.f, 0.f }, ss[2] = { 0.f, 0.f };
#pragma unroll
                            for (int i = 0; i < TI; ++i) {
                                const int row = wm * (BM / 2) + i * 32 + (lane & 31);
                                float t = 0.f, tt = 0.f;
#pragma unroll
                                for (int e = 0; e < PG; ++e) {
                                    const float v = acc[i][j][4 * q + h * PG + e];
                                    t += v;
                                    tt = fmaf(v, v, tt);
                                }
                                const bool live = m0 + row < a.M, hi = row >= split;
                                s[0] += (live && !hi) ? t : 0.f; ss[0] += (live && !hi) ? tt : 0.f;
                                s[1] += (live && hi) ? t : 0.f;  ss[1] += (live && hi) ? tt : 0.f;
                            }
#pragma unroll
                            for (int sl = 0; sl < 2; ++sl) {
                                float *o = sP + ((tid * 2 + sl) * NP + (j * 4 + q) * PQ + h) * 2;
                                o[0] = s[sl]; o[1] = ss[sl];
                            }
                        }
            };
            const int PGr = (a.cpg >= 4) ? 4 : 2;                  // launch_igemm admits cpg = 2 or a multiple of 4
            if (PGr == 4) stage1(std::integral_constant<int, 4>{});
            else stage1(std::integral_constant<int, 2>{});
            __syncthreads();
            const int PQr = 4 / PGr, NPr = NJ * 4 * PQr;
            const int pieces = BN / PGr;                           // pieces of the tile's BN channels
            double *sC = reinterpret_cast<double *>(smem + 256 * 2 * NPr * 2);      // [pieces][2 slots][2]
            for (int w = tid; w < pieces * 2; w += 256) {
                const int pc = w >> 1, sl = w & 1;
                const int c = pc * PGr;                            // first channel of the piece within the tile
                const int wnP = c / (BN / 2), l = c - wnP * (BN / 2);
                const int j = l >> 5, q = (l & 31) >> 3, half = ((l & 31) & 7) >> 2, h = ((l & 3) / PGr);
                double s1 = 0.0, s2 = 0.0;
                for (int wmP = 0; wmP < 2; ++wmP)
                    for (int pl = 0; pl < 32; ++pl) {
                        const int t = (wmP * 2 + wnP) * 64 + half * 32 + pl;
                        const float *o = sP + ((t * 2 + sl) * NPr + (j * 4 + q) * PQr + h) * 2;
                        s1 += (double)o[0]; s2 += (double)o[1];
                    }
                sC[w * 2] = s1; sC[w * 2 + 1] = s2;
            }
            __syncthreads();
            const int groupsInTile = BN / a.cpg;
            if (tid < groupsInTile * 2) {
                const int gi = tid >> 1, sl = tid & 1;
                const int n = nLo + sl;
                const int firstRow = sl ? split : 0;
                if (n < a.B && m0 + firstRow < a.M && (sl == 0 || split < BM)) {
                    double s1 = 0.0, s2 = 0.0;
                    const int ppg = a.cpg / PGr;                   // pieces per group
                    for (int pc = gi * ppg; pc < (gi + 1) * ppg; ++pc) { s1 += sC[(pc * 2 + sl) * 2]; s2 += sC[(pc * 2 + sl) * 2 + 1]; }
                    const int g = (n0 + gi * a.cpg) / a.cpg;
                    if (g < a.G) {
                        const int k = mt - (int)(((long long)n * a.HW) / BM);       // tile index within the image
                        double *o = a.stats + (((long long)n * a.nchunks + k) * a.G + g) * 2;
                        o[0] = s1; o[1] = s2;
                    }
                }
            }
        }
    }
    if (a.clk && tid == 0) {
        long long *c = a.clk + (long long)blockIdx.x * 8;
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        c[0] = tc0; c[1] = tw0; c[2] = tc1; c[3] = tc2; c[4] = clock64(); c[5] = wall_clock64(); c[6] = hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(hw));
        c[7] = hw;
    }
}

// XL_CONV_CLK=1: waits for the launch and prints what its workgroups recorded (8 values each: shader and wall clock at the
// start, shader clock behind the prologue and the K loop, both clocks at the end, HW_ID, XCC_ID); frees `clk`
int igemm_clk_report(long long *clk, int nwg, int nk, hipStream_t st)
{
    std::vector<long long> h(8 * (size_t)nwg);
    const bool copied = hipStreamSynchronize(st) == hipSuccess &&
                        hipMemcpy(h.data(), clk, sizeof(long long) * 8 * nwg, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(clk);
    if (!copied) return XL_ERR_HIP;
    double pro = 0, loop = 0, epi = 0, tot = 0, wall = 0;
    long long wmin = h[1], wmax = h[5];
    std::map<long long, int> perCu;
    for (int i = 0; i < nwg; ++i) {
        const long long *c = &h[8 * (size_t)i];
        pro += c[2] - c[0]; loop += c[3] - c[2]; epi += c[4] - c[3]; tot += c[4] - c[0]; wall += c[5] - c[1];
        if (c[1] < wmin) wmin = c[1];
        if (c[5] > wmax) wmax = c[5];
        // HW_ID: cu_id bits 8-11, sh 12, se 13-15 ; XCC id low bits
        perCu[((c[7] & 15) << 16) | ((c[6] >> 8) & 0xff)]++;
    }
    int cmin = 1 << 30, cmax = 0;
    for (auto &kv : perCu) { if (kv.second < cmin) cmin = kv.second; if (kv.second > cmax) cmax = kv.second; }
    // residency: workgroup-lifetime per CU over that CU's active span (2.0 = both slots always occupied)
    std::map<long long, std::array<double, 3>> occ;               // busy, first start, last end (100 MHz wall ticks)
    for (int i = 0; i < nwg; ++i) {
        const long long *c = &h[8 * (size_t)i];
        auto &o = occ[((c[7] & 15) << 16) | ((c[6] >> 8) & 0xff)];
        if (o[0] == 0.0) { o[1] = (double)c[1]; o[2] = (double)c[5]; }
        o[0] += (double)(c[5] - c[1]);
        if ((double)c[1] < o[1]) o[1] = (double)c[1];
        if ((double)c[5] > o[2]) o[2] = (double)c[5];
    }
    double resid = 0.0;
    for (auto &kv : occ) resid += kv.second[0] / (kv.second[2] - kv.second[1]);
    fprintf(stderr, "[clk] mean resident workgroups per CU %.3f, mean lifetime %.2f us\n", resid / occ.size(), wall / nwg / 100.0);
    fprintf(stderr, "[clk] wgs %d nk %d: prologue %.0f loop %.0f (%.1f/step) epilogue %.0f total %.0f ticks; clock %.1f MHz; kernel span %.3f ms; CUs seen %zu, tiles per CU %d..%d\n",
            nwg, nk, pro / nwg, loop / nwg, loop / nwg / (nk), epi / nwg, tot / nwg, tot / wall * 100.0,
            (wmax - wmin) / 1e5, perCu.size(), cmin, cmax);
    return XL_OK;
}

template <int KS, int STRIDE, int BN, int CIN, int MODE = 0, int BM = 128, int ZB = 0, int NORM = 0>
int launch_igemm(const xl_op &op, hipStream_t st, int py = 0, int px = 0)
{
    ConvArgs a;
    a.coef = nullptr; a.normLo = 0.f;
    if (NORM) {
        if (!op.aux2 || op.Ho * op.Wo < BM) return XL_ERR_ARG;
        a.coef = (const float *)op.aux2;
        a.normLo = (op.flags & XL_CONV_NORM_RELU) ? 0.f : -__builtin_huge_valf();
    }
    a.in = (const float *)op.in; a.w = (const float *)op.w; a.bias = (const float *)op.bias; a.out = (float *)op.out;
    a.B = op.B; a.Hi = op.Hi; a.Wi = op.Wi; a.Cin = op.Cin; a.Ho = op.Ho; a.Wo = op.Wo; a.Cout = op.Cout;
    a.ldIn = op.ld_in; a.ldOut = op.ld_out;
    a.M = op.B * op.Ho * op.Wo; a.K = op.ksize * op.ksize * op.Cin;
    a.py = py; a.px = px; a.Hj = 0; a.Wj = 0; a.ntaps = 0; a.tapList = 0;
    a.stats = nullptr; a.HW = op.Ho * op.Wo; a.G = 0; a.cpg = 1; a.nchunks = 0;
    a.zCount = 1; a.zIn = 0; a.zW = 0; a.zOut = 0;
    if (ZB) {                                        // batched GEMMs over consecutive blocks of in / w / out
        if (op.stats || op.nchunks2 < 1) return XL_ERR_ARG;
        a.zCount = op.nchunks2;
        a.zIn = (long long)a.M * op.ld_in; a.zW = (long long)op.Cout * a.K; a.zOut = (long long)a.M * op.ld_out;
    }
    if (MODE == 0 && op.stats && op.groups > 0) {
        a.G = op.groups; a.cpg = op.Cout / op.groups; a.nchunks = op.nchunks;
        if (a.HW < BM || op.Cout % op.groups != 0 || BN % a.cpg != 0 || a.nchunks < (a.HW + BM - 1) / BM + 1) return XL_ERR_ARG;
        if (a.cpg != 2 && a.cpg % 4 != 0) return XL_ERR_ARG;         // the statistics epilogue sums 2- or 4-channel pieces
        a.stats = (double *)op.stats;
    }
    if (MODE == 2) {
        // result pixel (iy,ix) = (2jy+py, 2jx+px); source row (iy+1-ky)/2 needs ky of parity (py+1)&1
        a.Hj = (op.Ho - py + 1) / 2; a.Wj = (op.Wo - px + 1) / 2;
        a.M = op.B * a.Hj * a.Wj;
        for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx)
                if (((py + 1 - ky) & 1) == 0 && ((px + 1 - kx) & 1) == 0) { a.tapList |= (unsigned)(ky * 3 + kx) << (4 * a.ntaps); ++a.ntaps; }
        if (a.M == 0) return XL_OK;
    }
    a.nbm = (a.M + BM - 1) / BM; a.nbn = (op.Cout + BN - 1) / BN;   // weight rows past Cout read as zero (bounds check)
    const long long inBytes = (((long long)op.B * op.Hi * op.Wi - 1) * op.ld_in + op.Cin) * 4;
    const long long wBytes = (long long)op.Cout * a.K * 4;
    const long long outBytes = (((long long)op.B * op.Ho * op.Wo - 1) * op.ld_out + op.Cout) * 4;
    if (wBytes >= 0x7fffffffLL) { xl_set_error("conv weights of %lld bytes", wBytes); return XL_ERR_ARG; }
    if (inBytes >= 0x7fffffffLL || outBytes >= 0x7fffffffLL) {
        // The kernel addresses a tensor with 32-bit byte offsets through one buffer descriptor (2 GiB).  Larger batches
        // run as several launches over image ranges, each with its own base pointers.  A range starts on a tile
        // boundary of the un-split launch (b0 * Ho*Wo divisible by BM), so every output tile - and every
        // (image, tile) slot of the fused GroupNorm statistics - is the same as in one launch.
        const long long perIn = (long long)op.Hi * op.Wi * op.ld_in * 4, perOut = (long long)op.Ho * op.Wo * op.ld_out * 4;
        const long long perMax = perIn > perOut ? perIn : perOut;
        int g = op.Ho * op.Wo;                                    // gcd(Ho*Wo, BM)
        for (int y = BM; y; ) { const int t = g % y; g = y; y = t; }
        const int align = BM / g;
        long long seg = (0x7ffffff0LL - 4LL * (op.Cin > op.Cout ? op.Cin : op.Cout)) / perMax;
        seg -= seg % align;
        if (ZB || MODE == 2 || seg < 1 || seg >= op.B) {
            xl_set_error("conv tensors of %lld / %lld bytes exceed 32-bit buffer addressing", inBytes, outBytes);
            return XL_ERR_ARG;
        }
        for (int b0 = 0; b0 < op.B; b0 += (int)seg) {
            xl_op part = op;
            part.B = (op.B - b0 < (int)seg) ? op.B - b0 : (int)seg;
            part.in = (const char *)op.in + (long long)b0 * perIn;
            part.out = (char *)op.out + (long long)b0 * perOut;
            if (op.stats) part.stats = (char *)op.stats + (long long)b0 * op.nchunks * op.groups * 2 * sizeof(double);
            if (NORM) part.aux2 = (const char *)op.aux2 + (long long)b0 * op.Cin * 2 * sizeof(float);
            const int rc = launch_igemm<KS, STRIDE, BN, CIN, MODE, BM, ZB, NORM>(part, st, py, px);
            if (rc != XL_OK) return rc;
        }
        return XL_OK;
    }
    a.inBytes = (unsigned)inBytes; a.wBytes = (unsigned)wBytes; a.outBytes = (unsigned)outBytes;
    a.accumulate = (op.flags & XL_CONV_ACCUMULATE) ? 1 : 0;
    if (op.ld_out % 4 != 0) return XL_ERR_ARG;                    // dwordx4 stores of 4 consecutive channels
    if ((ZB || MODE != 0) && (a.bias || a.stats)) return XL_ERR_ARG;
    if (a.accumulate && a.stats) return XL_ERR_ARG;
    size_t lds = sizeof(float) * 2 * (BM + BN) * kBK;
    if (NORM) lds += sizeof(float) * (4 * (size_t)op.Cin + 256);   // {scale, shift} of two images (+ slack for the unused tail stage)
    if (a.stats) {                                   // the statistics epilogue reuses the tile storage: make sure it fits
        const int pg = a.cpg >= 4 ? 4 : 2, np = (BN / 64) * 4 * (4 / pg);
        const size_t need = sizeof(float) * 256 * 2 * np * 2 + sizeof(double) * (BN / pg) * 2 * 2;
        if (need > lds) lds = need;
    }
    static XlLdsLimit configured;                    // one per template instantiation, tracked per device
    hipError_t e;
    if (configured.configure(reinterpret_cast<const void *>(igemm_conv_kernel<KS, STRIDE, BN, CIN, MODE, BM, ZB, NORM>), lds, &e) != XL_OK) {
        xl_set_error("hipFuncSetAttribute: %s", hipGetErrorString(e));
        return XL_ERR_HIP;
    }
    static const bool clkDbg = getenv("XL_CONV_CLK") != nullptr;
    a.clk = nullptr;
    const int nwg = a.nbm * a.nbn * a.zCount;
    if (clkDbg && hipMalloc(&a.clk, sizeof(long long) * 8 * nwg) != hipSuccess) return XL_ERR_HIP;
    hipLaunchKernelGGL((igemm_conv_kernel<KS, STRIDE, BN, CIN, MODE, BM, ZB, NORM>), dim3(nwg), dim3(256), lds, st, a);
    if (clkDbg) return igemm_clk_report(a.clk, nwg, a.K / kBK, st);
    return XL_OK;
}

}  // namespace

int xl_run_conv(const xl_op &op, hipStream_t st)
{
    if (op.Cin % 32 != 0 || op.Cout % 32 != 0 || op.ld_in % 4 != 0) return XL_ERR_ARG;
    const bool wide = (op.Cout % 128 == 0);
    if (op.flags & XL_CONV_DGRAD) {
        if (op.ksize == 3 && op.stride == 1) return wide ? launch_igemm<3, 1, 128, 0, 1>(op, st) : launch_igemm<3, 1, 64, 0, 1>(op, st);
        if (op.ksize == 3 && op.stride == 2) {
            // four parity classes of result pixels, each with only the taps that reach it
            for (int py = 0; py < 2; ++py)
                for (int px = 0; px < 2; ++px) {
                    const int rc = wide ? launch_igemm<3, 2, 128, 0, 2>(op, st, py, px) : launch_igemm<3, 2, 64, 0, 2>(op, st, py, px);
                    if (rc != XL_OK) return rc;
                }
            return XL_OK;
        }
        if (op.ksize == 1 && op.stride == 1) return wide ? launch_igemm<1, 1, 128, 0, 1>(op, st) : launch_igemm<1, 1, 64, 0, 1>(op, st);
        return XL_ERR_UNSUPPORTED;
    }
    const bool small = (op.reserved_i == 64);          // 64-row tiles: the host asks for them when 128-row tiles
                                                        // would leave most of the 256 CUs idle (small batches)
#define XL_FWD(KS, S, BN, CIN, BM) launch_igemm<KS, S, BN, CIN, 0, BM>(op, st)
    if (op.ksize == 3 && op.stride == 1) {
        if (small) {
            if (wide && op.Cin == 512) return XL_FWD(3, 1, 128, 512, 64);
            return wide ? XL_FWD(3, 1, 128, 0, 64) : XL_FWD(3, 1, 64, 0, 64);
        }
        if (wide && op.Cin == 512) return XL_FWD(3, 1, 128, 512, 128);      // 78 % of the forward FLOPs
        return wide ? XL_FWD(3, 1, 128, 0, 128) : XL_FWD(3, 1, 64, 0, 128);
    }
    if (op.ksize == 3 && op.stride == 2) {
        if (op.flags & XL_CONV_PAIR_F16) return xl_run_pair_stem(op, st);
        if (op.flags & XL_CONV_SPLIT_BF16) return xl_run_split_stem(op, st);
        if (small) return wide ? XL_FWD(3, 2, 128, 0, 64) : XL_FWD(3, 2, 64, 0, 64);
        return wide ? XL_FWD(3, 2, 128, 0, 128) : XL_FWD(3, 2, 64, 0, 128);
    }
    if (op.flags & XL_CONV_SPLIT_BF16) return xl_run_split_gemm(op, st);
    if (op.ksize == 1 && op.stride == 1 && op.nchunks2 > 1) {         // Winograd: nchunks2 GEMMs in one launch
        if (!wide) return XL_ERR_UNSUPPORTED;
        if (small) return op.Cin == 512 ? launch_igemm<1, 1, 128, 512, 0, 64, 1>(op, st) : launch_igemm<1, 1, 128, 0, 0, 64, 1>(op, st);
        return op.Cin == 512 ? launch_igemm<1, 1, 128, 512, 0, 128, 1>(op, st) : launch_igemm<1, 1, 128, 0, 0, 128, 1>(op, st);
    }
    if (op.ksize == 1 && op.stride == 1 && (op.flags & XL_CONV_NORM_IN)) {   // producer's GroupNorm applied on load
        if (!wide || small) return XL_ERR_UNSUPPORTED;
        return op.Cin == 512 ? launch_igemm<1, 1, 128, 512, 0, 128, 0, 1>(op, st) : launch_igemm<1, 1, 128, 0, 0, 128, 0, 1>(op, st);
    }
    if (op.ksize == 1 && op.stride == 1) {
        if (small) {
            if (wide && op.Cin == 512) return XL_FWD(1, 1, 128, 512, 64);
            return wide ? XL_FWD(1, 1, 128, 0, 64) : XL_FWD(1, 1, 64, 0, 64);
        }
        if (wide && op.Cin == 512) return XL_FWD(1, 1, 128, 512, 128);
        return wide ? XL_FWD(1, 1, 128, 0, 128) : XL_FWD(1, 1, 64, 0, 128);
    }
#undef XL_FWD
    return XL_ERR_UNSUPPORTED;
}
