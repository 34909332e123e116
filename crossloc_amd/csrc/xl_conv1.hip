// xl_conv1.hip — XL_OP_CONV1, the first layer: 3x3 s1 on the 3-channel NCHW image -> NHWC.  Three forms: the direct kernel
// (raw output), and the two-pass inference form (statistics only / conv + GroupNorm + ReLU) on the VALU and on the bf16 matrix pipe.
// Behind them XL_OP_CONV1_WGRAD, the layer's weight / bias gradient.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xl_launch.h"
#include "xl_operand_math.h"

namespace {

// ---------------------------------------------------------------------------------------------- conv1

// in NCHW [B,Cin,H,W]; w [(ky*3+kx)*Cin + c][Cout]; out NHWC.  Thread = (pixel, 8 output channels).
__global__ __launch_bounds__(256)
void conv1_direct_kernel(const float *__restrict__ in, const float *__restrict__ w, const float *__restrict__ bias,
                         float *__restrict__ out, int B, int Cin, int H, int W, int Cout, int ldOut)
{
    extern __shared__ __attribute__((aligned(16))) float sW[];      // [9*Cin][Cout] + bias[Cout]
    const int nW = 9 * Cin * Cout;
    for (int i = threadIdx.x; i < nW; i += 256) sW[i] = w[i];
    for (int i = threadIdx.x; i < Cout; i += 256) sW[nW + i] = bias[i];
    __syncthreads();
    const int tpp = Cout >> 3;                                       // threads per pixel
    const int pixPerBlock = 256 / tpp;
    const long long HW = (long long)H * W;
    const long long total = (long long)B * HW;
    const int cg = threadIdx.x % tpp;
    for (long long p = (long long)blockIdx.x * pixPerBlock + threadIdx.x / tpp; p < total;
         p += (long long)gridDim.x * pixPerBlock) {
        const int n = (int)(p / HW);
        const int rem = (int)(p - (long long)n * HW);
        const int y = rem / W, x = rem - y * W;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = sW[nW + cg * 8 + j];
        const float *img = in + (long long)n * Cin * HW;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = y + ky - 1;
            if ((unsigned)iy >= (unsigned)H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = x + kx - 1;
                if ((unsigned)ix >= (unsigned)W) continue;
                for (int c = 0; c < Cin; ++c) {
                    const float v = img[(long long)c * HW + (long long)iy * W + ix];
                    const float *wr = sW + ((ky * 3 + kx) * Cin + c) * Cout + cg * 8;
                    const f32x4 w0 = *reinterpret_cast<const f32x4 *>(wr);
                    const f32x4 w1 = *reinterpret_cast<const f32x4 *>(wr + 4);
                    acc[0] = fmaf(v, w0.x, acc[0]); acc[1] = fmaf(v, w0.y, acc[1]);
                    acc[2] = fmaf(v, w0.z, acc[2]); acc[3] = fmaf(v, w0.w, acc[3]);
                    acc[4] = fmaf(v, w1.x, acc[4]); acc[5] = fmaf(v, w1.y, acc[5]);
                    acc[6] = fmaf(v, w1.z, acc[6]); acc[7] = fmaf(v, w1.w, acc[7]);
                }
            }
        }
        float *o = out + p * ldOut + cg * 8;
        *reinterpret_cast<f32x4 *>(o) = f32x4{ acc[0], acc[1], acc[2], acc[3] };
        *reinterpret_cast<f32x4 *>(o + 4) = f32x4{ acc[4], acc[5], acc[6], acc[7] };
    }
}

// Inference form of the first layer.  conv1 costs 27 MACs per output while its 32-channel full-resolution output is the
// largest tensor of the network: evaluating it twice is cheaper than writing it raw, re-reading it for the GroupNorm
// statistics and re-reading / re-writing it for the apply.  PASS 0 evaluates the convolution and keeps only the
// per-(image, channel) partial sums (32 groups of 1 channel); PASS 1 evaluates it again and writes
// relu(conv * scale + shift) once.  Thread = pixel x all 32 channels: the weights are wave-uniform, so they stream
// through scalar loads and feed v_fmac as SGPR operands (no LDS traffic, no per-lane weight registers).
// in NCHW [B,3,H,W]; w [(ky*3+kx)*3 + c][32]; out NHWC; grid (chunks, B), a workgroup covers ppt*256 pixels of one image.
constexpr int kC1Pitch = 36;                       // LDS row pitch (floats) of the output transpose: 32 channels + 4 pad
template <int PASS>
__global__ __launch_bounds__(256)
void conv1_fused_kernel(const float *__restrict__ in, const float *__restrict__ w, const float *__restrict__ bias,
                        const float *__restrict__ coeff, float *__restrict__ out, double *__restrict__ stats,
                        int H, int W, int ldOut, int ppt, int relu)
{
    constexpr int CO = 32, CI = 3, NT = 9 * CI;
    __shared__ __attribute__((aligned(16))) float sRed[PASS == 0 ? CO * 256 : 256 * kC1Pitch];
    const int n = blockIdx.y, tid = threadIdx.x;
    const int HW = H * W;
    const float *img = in + (long long)n * CI * HW;
    float s[CO], q[CO];
#pragma unroll
    for (int j = 0; j < CO; ++j) { s[j] = 0.f; q[j] = 0.f; }
    for (int k = 0; k < ppt; ++k) {
        const int p = (blockIdx.x * ppt + k) * 256 + tid;
        const bool live = p < HW;
        const int pc = live ? p : HW - 1;
        const int y = pc / W, x = pc - y * W;
        float v[NT];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = y + ky - 1, ix = x + kx - 1;
                const bool inb = ((unsigned)iy < (unsigned)H) & ((unsigned)ix < (unsigned)W);
                const int off = min(max(iy, 0), H - 1) * W + min(max(ix, 0), W - 1);
#pragma unroll
                for (int c = 0; c < CI; ++c) {
                    const float t = img[(long long)c * HW + off];
                    v[(ky * 3 + kx) * CI + c] = inb ? t : 0.f;          // a zero tap leaves the fma chain unchanged
                }
            }
        }
        // the weight offset is laundered per pixel: otherwise all 864 scalar loads are hoisted out of the loop and
        // spilled into VGPR lanes (one v_readlane per weight per pixel - more VALU work than the convolution itself)
        int zero = 0;
        asm volatile("" : "+s"(zero));
        const float *wk = w + zero;
        float acc[CO];
#pragma unroll
        for (int j = 0; j < CO; ++j) acc[j] = bias[j];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int j = 0; j < CO; ++j) acc[j] = fmaf(v[t], wk[t * CO + j], acc[j]);
        }
        if (PASS == 0) {
#pragma unroll
            for (int j = 0; j < CO; ++j) {
                const float a = live ? acc[j] : 0.f;
                s[j] += a;
                q[j] = fmaf(a, a, q[j]);
            }
        } else {
            // a wave owns 64 consecutive pixels = one contiguous 8 KB span of the NHWC output (ldOut == 32): transpose
            // through LDS so that every store instruction writes 1 KB of consecutive addresses instead of 64 scattered
            // 16-byte pieces
            const float *cf = coeff + (long long)n * CO * 2;
            const int lane = tid & 63;
            float *row = sRed + (tid >> 6) * (64 * kC1Pitch);
#pragma unroll
            for (int j = 0; j < CO; j += 4) {
                f32x4 r;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = acc[j + e] * cf[(j + e) * 2] + cf[(j + e) * 2 + 1];
                    if (relu) t = fmaxf(t, 0.f);
                    r[e] = t;
                }
                *reinterpret_cast<f32x4 *>(row + lane * kC1Pitch + j) = r;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int p0 = (blockIdx.x * ppt + k) * 256 + (tid & ~63);     // first pixel of the wave
            float *o = out + ((long long)n * HW + p0) * CO;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int qd = c * 64 + lane;                               // 16-byte piece of the span
                const int px = qd >> 3, part = qd & 7;
                const f32x4 r = *reinterpret_cast<const f32x4 *>(row + px * kC1Pitch + part * 4);
                if (p0 + px < HW) *reinterpret_cast<f32x4 *>(o + (long long)qd * 4) = r;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (PASS == 0) {
        // per-thread fp32 partials -> fp64 across the workgroup: value-major transpose through LDS, 4 threads per value
        const int vsel = tid >> 2, part = tid & 3;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            __syncthreads();
#pragma unroll
            for (int j = 0; j < CO; ++j) sRed[j * 256 + tid] = half ? q[j] : s[j];
            __syncthreads();
            if (vsel < CO) {
                double a = 0.0;
                for (int i = 0; i < 64; ++i) a += (double)sRed[vsel * 256 + part * 64 + ((i + vsel + 16 * part) & 63)];
                a += __shfl_xor(a, 1);
                a += __shfl_xor(a, 2);
                if (part == 0) stats[(((long long)n * gridDim.x + blockIdx.x) * CO + vsel) * 2 + half] = a;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- conv1 on the matrix pipe
//
// The same two evaluations (statistics only / normalise + ReLU + write) with the multiplies on the bf16 matrix pipe instead
// of 432 packed VALU FMAs per pixel: every fp32 value - image and weights - is an exact sum of three bf16 terms, six term
// pairs per product, fp32 accumulation (as csrc/xl_gemm_split.hip).  A workgroup owns 16 x 64 output pixels: the 18 x 66
// halo of the image is split ONCE while it is staged into LDS (each value is used by nine patches), one 8-byte word
// {R, G, B, 0} per pixel and plane.  The K dimension is laid out so that a K-step of v_mfma_f32_32x32x16_bf16 is one row of
// the 3 x 3 window: 16 slots = 4 pixels (x-1, x, x+1 and a fourth with zero weights) x {R, G, B, 0}; a lane's 8 values are
// two neighbouring pixel words = one ds_read2_b64, no gather.  32 pixels of a row x 32 channels = 3 K-steps x 6 term
// pairs = 18 MFMAs; the weight fragments (9 x 4 registers) are built once per wave.
constexpr int kC1TH = 16, kC1TW = 64, kC1HH = kC1TH + 2, kC1HW = kC1TW + 4;   // 66 halo columns + 2 of zeros (slot dx = 3 of the last pixels)
constexpr int kC1Halo = 3 * kC1HH * kC1HW * 8;                 // bytes: [plane][row][col] of 8-byte pixel words

template <int PASS>
__global__ __launch_bounds__(256)
void conv1_mfma_kernel(const float *__restrict__ in, const u32x4 *__restrict__ wfrag, const float *__restrict__ bias,
                       const float *__restrict__ coeff, float *__restrict__ out, double *__restrict__ stats,
                       int H, int W, int tilesX, int relu)
{
    constexpr int CO = 32;
    // PASS 0: statistics only; 1: conv * scale + shift (+ReLU) written; 2 (round 3): the RAW convolution written AND its
    // statistics, one evaluation - the consumer (conv2 on the split pipe) applies the GroupNorm while it loads its operand
    constexpr bool kStats = PASS != 1, kWrite = PASS != 0;
    constexpr int kSmW = kC1Halo + 4 * 32 * kC1Pitch * 4, kSmS = kC1Halo > 256 * 32 * 4 ? kC1Halo : 256 * 32 * 4;
    constexpr int kSm = !kWrite ? kSmS : (kStats && kSmS > kSmW ? kSmS : kSmW);
    __shared__ __attribute__((aligned(16))) unsigned char smem[kSm];
    const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ty = blockIdx.x / tilesX, tx = blockIdx.x - ty * tilesX;
    const int y0 = ty * kC1TH, x0 = tx * kC1TW;
    const long long HW = (long long)H * W;
    const float *img = in + (long long)n * 3 * HW;

    // ---- halo -> LDS, split
    u32x2 *sH = reinterpret_cast<u32x2 *>(smem);
    for (int i = tid; i < kC1HH * kC1HW; i += 256) {
        const int r = i / kC1HW, c = i - r * kC1HW;
        const int y = y0 - 1 + r, x = x0 - 1 + c;
        const bool inb = ((unsigned)y < (unsigned)H) & ((unsigned)x < (unsigned)W) & (c < kC1TW + 2);
        const long long off = (long long)(inb ? y : 0) * W + (inb ? x : 0);
        unsigned h[3][3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float v = inb ? img[ch * HW + off] : 0.f;
            xl_bf16_split3(v, h[0][ch], h[1][ch], h[2][ch]);
        }
#pragma unroll
        for (int p = 0; p < 3; ++p) sH[p * (kC1HH * kC1HW) + i] = u32x2{ h[p][0] | (h[p][1] << 16), h[p][2] };
    }
    // ---- weight fragments: lane -> (channel lane & 31, K half lane >> 5); slot j of a K-step = (dx = j >> 2, c = j & 3),
    // zero for c = 3 and dx = 3.  Split and packed once per plan on the host side: wfrag[plane][dy][lane], 16 bytes each.
    const int kh = lane >> 5;
    bf16x8 wf[3][3];                                                 // [plane][dy]
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) wf[p][dy] = __builtin_bit_cast(bf16x8, wfrag[(p * 3 + dy) * 64 + lane]);
    // accumulator element r of a lane: pixel lane & 31, channel 8 (r >> 2) + 4 kh + (r & 3)
    float b16[16], sc[16], sh[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int c = 8 * (r >> 2) + 4 * kh + (r & 3);
        b16[r] = bias[c];
        if (PASS == 1) { sc[r] = coeff[((long long)n * CO + c) * 2]; sh[r] = coeff[((long long)n * CO + c) * 2 + 1]; }
    }
    float s[16], q[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = 0.f; q[r] = 0.f; }
    __syncthreads();

    const int px = lane & 31;
#pragma unroll 1
    for (int blk = 0; blk < 8; ++blk) {
        const int ly = wv * 4 + (blk >> 1), lx = (blk & 1) * 32 + px;   // pixel of this lane inside the tile
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = b16[r];
        bf16x8 pf[3][3];                                             // [plane][dy]
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const u32x2 *src = sH + p * (kC1HH * kC1HW) + (ly + dy) * kC1HW + lx + 2 * kh;
                const u32x2 a = src[0], b = src[1];
                pf[p][dy] = __builtin_bit_cast(bf16x8, u32x4{ a[0], a[1], b[0], b[1] });
            }
        constexpr int PW[6] = { 2, 1, 0, 1, 0, 0 }, PP[6] = { 0, 1, 2, 0, 1, 0 };   // smallest terms first
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[PW[t]][dy], pf[PP[t]][dy], acc, 0, 0, 0);
        const int y = y0 + ly, xb = x0 + (blk & 1) * 32;               // first pixel of the block
        if (kStats) {
            const bool live = (y < H) & (xb + px < W);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float a = live ? acc[r] : 0.f;
                s[r] += a;
                q[r] = fmaf(a, a, q[r]);
            }
        }
        if (kWrite) {
            // the block is one contiguous 4 KB span of the NHWC output: transposed through a wave-private LDS area so that
            // every store instruction writes 1 KB of consecutive addresses
            float *row = reinterpret_cast<float *>(smem + kC1Halo) + wv * (32 * kC1Pitch);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = acc[4 * g + e];
                    if (PASS == 1) {
                        t = t * sc[4 * g + e] + sh[4 * g + e];
                        if (relu) t = fmaxf(t, 0.f);
                    }
                    v[e] = t;
                }
                *reinterpret_cast<f32x4 *>(row + px * kC1Pitch + 8 * g + 4 * kh) = v;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (y < H) {
                float *o = out + (((long long)n * H + y) * W + xb) * CO;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int qd = c * 64 + lane;                       // 16-byte piece of the span
                    const int pp = qd >> 3, part = qd & 7;
                    const f32x4 v = *reinterpret_cast<const f32x4 *>(row + pp * kC1Pitch + part * 4);
                    if (xb + pp < W) *reinterpret_cast<f32x4 *>(o + (long long)qd * 4) = v;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (kStats) {
        // per-lane fp32 partials (8 pixels each) -> fp64 over the 128 lanes that hold a channel, fixed order.
        // Staging layout [value][thread] (round 6): with [thread][32 values] every lane of a ds_write_b32 hit the same bank - 32 writes
        // of 64 LDS cycles each per wave, four times the LDS time of the whole convolution loop, and the kernel was bound by it
        // (0.40 of its LDS cycles were conflict cycles).  The readers start at different lanes (l + c) so that they, too, spread
        // over the banks; an fp64 sum of 128 fp32 values of one sign-mixed magnitude range is exact, the order is fixed anyway.
        float *sRed = reinterpret_cast<float *>(smem);
        __syncthreads();                                             // every wave is done with the halo
#pragma unroll
        for (int r = 0; r < 16; ++r) { sRed[r * 256 + tid] = s[r]; sRed[(16 + r) * 256 + tid] = q[r]; }
        __syncthreads();
        if (tid < 64) {
            const int c = tid & 31, half = tid >> 5;
            const int khc = (c >> 2) & 1, r = ((c >> 3) << 2) | (c & 3);
            const float *src = sRed + (half * 16 + r) * 256 + khc * 32;
            double a = 0.0;
            for (int wq = 0; wq < 4; ++wq)
                for (int l = 0; l < 32; ++l) a += (double)src[wq * 64 + ((l + c) & 31)];
            stats[(((long long)n * gridDim.x + blockIdx.x) * CO + c) * 2 + half] = a;
        }
    }
}

}  // namespace

int xl_run_conv1(const xl_op &op, hipStream_t st)
{
    if (op.stats || op.aux2) {
        // inference form: statistics-only pass (stats, nchunks workgroups per image, reserved_i pixels/256 each)
        // or conv + deferred GroupNorm (aux2 = {scale, shift} pairs) + ReLU (flags & XL_GN_RELU_IN)
        const float *coeff = op.stats ? nullptr : (const float *)op.aux2;
        const int relu = (!op.stats && (op.flags & XL_GN_RELU_IN)) ? 1 : 0;
        if (op.Cin == 3 && op.Cout == 32 && op.ld_out == 32 && op.reserved_i == 0) {
            // matrix-pipe form: one workgroup per 16 x 64 output tile, nchunks = tiles per image; `w` = the weight
            // fragments [3 planes][3 rows of the window][64 lanes][8] bf16 (crossloc_amd/networks.py, pack_conv1_split)
            const int tilesX = (op.Wi + kC1TW - 1) / kC1TW, tilesY = (op.Hi + kC1TH - 1) / kC1TH;
            if (op.nchunks != tilesX * tilesY || (op.stats && op.groups != 32)) return XL_ERR_ARG;
            auto kernel = !op.stats ? conv1_mfma_kernel<1> : op.out ? conv1_mfma_kernel<2> : conv1_mfma_kernel<0>;
            hipLaunchKernelGGL(kernel, dim3(op.nchunks, op.B), dim3(256), 0, st, (const float *)op.in, (const u32x4 *)op.w,
                               (const float *)op.bias, coeff, (float *)op.out, (double *)op.stats, op.Hi, op.Wi, tilesX, relu);
            return XL_OK;
        }
        if (op.Cin != 3 || op.Cout != 32 || op.ld_out != 32 || op.reserved_i < 1 ||
            (long long)op.nchunks * op.reserved_i * 256 < (long long)op.Hi * op.Wi || (op.stats && op.groups != 32))
            return XL_ERR_ARG;
        hipLaunchKernelGGL(op.stats ? conv1_fused_kernel<0> : conv1_fused_kernel<1>, dim3(op.nchunks, op.B), dim3(256), 0, st,
                           (const float *)op.in, (const float *)op.w, (const float *)op.bias, coeff, op.stats ? nullptr : (float *)op.out,
                           (double *)op.stats, op.Hi, op.Wi, op.ld_out, op.reserved_i, relu);
        return XL_OK;
    }
    if (op.Cout % 8 != 0 || op.Cout > 64 || 256 % (op.Cout / 8) != 0 || op.ld_out % 4 != 0) return XL_ERR_ARG;
    const size_t lds = sizeof(float) * (size_t)(9 * op.Cin * op.Cout + op.Cout);
    const long long pix = (long long)op.B * op.Hi * op.Wi;
    const int ppb = 256 / (op.Cout / 8);
    hipLaunchKernelGGL(conv1_direct_kernel, dim3(xl_grid(pix, ppb, 65536)), dim3(256), lds, st,
                       (const float *)op.in, (const float *)op.w, (const float *)op.bias, (float *)op.out,
                       op.B, op.Cin, op.Hi, op.Wi, op.Cout, op.ld_out);
    return XL_OK;
}

// ---------------------------------------------------------------------------------------------- XL_OP_CONV1_WGRAD

namespace {

// dW[o][c][ky][kx] = sum dY[n,y,x,o] * img[n,c,y+ky-1,x+kx-1]; db[o] = sum dY.  Cout = 32.
// Thread = (4 consecutive output channels og, pixel lane pl of 32): per pixel one 16-byte dY load (the 8 threads of a
// pixel read its 128 contiguous bytes) and 9 ds_read_b128 of the image taps feed 108 FMAs - 12 per LDS read; with one
// output channel per thread (3 per read) the kernel sat on the LDS pipe at 6x its HBM time.
// A block walks `rowsPerBlock` output rows of one image two at a time; the 4 image rows (with halo, channels padded
// to a float4) they touch are staged in LDS.  partial [gridDim.y * gridDim.x][28][32]
// FOLD (round 5): `dy` is the gradient w.r.t. the GroupNorm(+ReLU) OUTPUT of conv1 and `x` conv1's raw output: the apply pass of
// the GroupNorm backward (dx = k1 dv - k2 - xhat k3, the arithmetic of gnb_apply_kernel - same operations, same order, same bits)
// runs on load, from the forward table `fco` and the coefficients `bco` XL_OP_GNB_FINAL left.  conv1 has no data gradient: its dx
// had this kernel as only reader, and the apply pass read and wrote 2.1 GB for it at batch 16.
template <bool FOLD>
__global__ __launch_bounds__(256)
void conv1_wgrad_kernel(const float *__restrict__ img, const float *__restrict__ dy, float *__restrict__ partial,
                        int B, int Cin, int H, int W, int ldY, int rowsPerBlock,
                        const float *__restrict__ x, int ldX, const float *__restrict__ fco, const float *__restrict__ bco, int reluIn)
{
    constexpr int R = 2, CO = 32;
    extern __shared__ __attribute__((aligned(16))) float sDyn[];
    f32x4 *sImg = reinterpret_cast<f32x4 *>(sDyn);                 // [(R+2)][W+2]
    float *sRed = sDyn;                                            // [4 waves][32][28], reuses the tile after the loop
    const int og = threadIdx.x & 7, pl = threadIdx.x >> 3;
    const int n = blockIdx.y;
    const long long HW = (long long)H * W;
    const int yBeg = blockIdx.x * rowsPerBlock;
    int yEnd = yBeg + rowsPerBlock; if (yEnd > H) yEnd = H;
    f32x4 acc[28];                                                 // [tap*3 + c] (27: bias) x 4 output channels
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = f32x4{ 0.f, 0.f, 0.f, 0.f };
    f32x4 kMu, kRs, kSc, kSh, k1, k2, k3;                          // FOLD: this thread's four channels of image n
    if constexpr (FOLD) {
        const float *scsh = fco + ((long long)n * CO + 4 * og) * 2, *murs = fco + (((long long)B + n) * CO + 4 * og) * 2;
        const float *bo = bco + ((long long)n * CO + 4 * og) * 3;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            kSc[j] = scsh[2 * j]; kSh[j] = scsh[2 * j + 1]; kMu[j] = murs[2 * j]; kRs[j] = murs[2 * j + 1];
            k1[j] = bo[3 * j]; k2[j] = bo[3 * j + 1]; k3[j] = bo[3 * j + 2];
        }
    }
    auto grad_of = [&](const f32x4 &d4, const f32x4 &xv) {
        if constexpr (!FOLD) return d4;
        f32x4 dx;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = xv[j] * kSc[j] + kSh[j];
            const float xh = (xv[j] - kMu[j]) * kRs[j];
            const float dv = (reluIn && !(v > 0.f)) ? 0.f : d4[j];
            dx[j] = k1[j] * dv - k2[j] - xh * k3[j];
        }
        return dx;
    };
    const int W2 = W + 2;
    for (int y0 = yBeg; y0 < yEnd; y0 += R) {
        __syncthreads();
        // staging in batches of 4 entries per thread: all loads of a batch are in flight before the first LDS write
        // (clamped addresses + a select instead of a branch around the loads)
        for (int base = threadIdx.x; base < (R + 2) * W2; base += 4 * 256) {
            f32x4 v[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * 256;
                const int r = idx / W2, xx = idx - r * W2 - 1;
                const int iy = y0 - 1 + r;
                ok[u] = (idx < (R + 2) * W2) & ((unsigned)iy < (unsigned)H) & ((unsigned)xx < (unsigned)W);
                const int iyc = min(max(iy, 0), H - 1), xc = min(max(xx, 0), W - 1);
                const float *q = img + (long long)n * Cin * HW + (long long)iyc * W + xc;
                v[u] = f32x4{ q[0], Cin > 1 ? q[HW] : 0.f, Cin > 1 ? q[2 * HW] : 0.f, 0.f };
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * 256;
                if (idx < (R + 2) * W2) sImg[idx] = ok[u] ? v[u] : f32x4{ 0.f, 0.f, 0.f, 0.f };
            }
        }
        __syncthreads();
        const int rows = (yEnd - y0 < R) ? (yEnd - y0) : R;
        // rows y0.. are consecutive in memory: pixel p of the step is dyRow + p*ldY.  The load of the next pixel is
        // issued before the FMAs of the current one (one HBM round trip per iteration otherwise).
        const float *dyRow = dy + ((long long)n * H + y0) * W * ldY + 4 * og;
        const float *xRow = FOLD ? x + ((long long)n * H + y0) * W * ldX + 4 * og : nullptr;
        const int np = rows * W;
        f32x4 gNext = f32x4{ 0.f, 0.f, 0.f, 0.f }, xNext = f32x4{ 0.f, 0.f, 0.f, 0.f };
        if (pl < np) {
            gNext = *reinterpret_cast<const f32x4 *>(dyRow + (long long)pl * ldY);
            if constexpr (FOLD) xNext = *reinterpret_cast<const f32x4 *>(xRow + (long long)pl * ldX);
        }
        for (int p = pl; p < np; p += 32) {
            const int ry = p / W, xcol = p - ry * W;
            const f32x4 g = grad_of(gNext, xNext);
            if (p + 32 < np) {
                gNext = *reinterpret_cast<const f32x4 *>(dyRow + (long long)(p + 32) * ldY);
                if constexpr (FOLD) xNext = *reinterpret_cast<const f32x4 *>(xRow + (long long)(p + 32) * ldX);
            }
            acc[27] += g;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const f32x4 *row = sImg + (ry + ky) * W2 + xcol;
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const f32x4 v = row[kx];
                    acc[(ky * 3 + kx) * 3 + 0] += g * v.x;
                    acc[(ky * 3 + kx) * 3 + 1] += g * v.y;
                    acc[(ky * 3 + kx) * 3 + 2] += g * v.z;
                }
            }
        }
    }
    // fixed-order reduction: the 8 pixel lanes of a wave (lane bits 3..5), then the 4 waves through LDS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 28; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = acc[k][e];
            v += __shfl_xor(v, 8);
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            acc[k][e] = v;
        }
    __syncthreads();
    if (lane < 8) {
#pragma unroll
        for (int k = 0; k < 28; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) sRed[(wave * CO + 4 * og + e) * 28 + k] = acc[k][e];
    }
    __syncthreads();
    const long long blk = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    for (int i = threadIdx.x; i < 28 * CO; i += 256) {
        const int k = i / CO, o = i - k * CO;
        float s = 0.f;
        for (int w = 0; w < 4; ++w) s += sRed[(w * CO + o) * 28 + k];
        partial[(blk * 28 + k) * CO + o] = s;
    }
}

// out: dW OIHW [Cout][Cin][3][3] and db[Cout] from the block partials.  grid (28): one tap/channel slot k per block;
// 256 threads = 32 output channels x 8 parts, each part sums a contiguous eighth of the blocks (4 loads in flight), the
// eighths are added in order.  (One thread per output walking all partials serially was a 0.5 ms chain of loads.)
__global__ __launch_bounds__(256)
void conv1_wgrad_reduce_kernel(const float *__restrict__ partial, float *__restrict__ dw, float *__restrict__ db,
                               int blocks, int Cin)
{
    constexpr int CO = 32;
    __shared__ double sP[8 * CO];
    const int k = blockIdx.x, o = threadIdx.x & 31, part = threadIdx.x >> 5;
    const int per = (blocks + 7) >> 3;
    const int b0 = part * per;
    int b1 = b0 + per; if (b1 > blocks) b1 = blocks;
    double s = 0.0;
#pragma unroll 4
    for (int b = b0; b < b1; ++b) s += (double)partial[((long long)b * 28 + k) * CO + o];
    sP[part * CO + o] = s;
    __syncthreads();
    if (part != 0) return;
    double t = 0.0;
    for (int q = 0; q < 8; ++q) t += sP[q * CO + o];
    if (k == 27) { db[o] = (float)t; return; }
    const int tap = k / 3, c = k - tap * 3;
    if (c < Cin) dw[((long long)o * Cin + c) * 9 + tap] = (float)t;
}

}  // namespace

int xl_run_conv1_wgrad(const xl_op &op, hipStream_t st)
{
    if (op.Cout != 32 || op.Cin > 3) return XL_ERR_UNSUPPORTED;
    const int rowsPerBlock = op.reserved_i > 0 ? op.reserved_i : 16;     // scratch: B*ceil(Hi/rows)*28*Cout floats
    if (op.ld_aux % 4 != 0) return XL_ERR_ARG;
    const int rb = (op.Hi + rowsPerBlock - 1) / rowsPerBlock;
    const int blocks = rb * op.B;
    size_t lds = sizeof(float) * (size_t)4 * (op.Wi + 2) * 4;
    if (lds < sizeof(float) * (size_t)4 * op.Cout * 28) lds = sizeof(float) * (size_t)4 * op.Cout * 28;
    // the staged rows take 64 * (Wi + 2) bytes: up to the 160 KiB of a CU (frames up to 2558 pixels wide; the training
    // augmentation's largest scale, 3/2 of a 720-wide frame, needs 68 KiB)
    if (lds > 160 * 1024) return XL_ERR_UNSUPPORTED;
    // fold: GroupNorm-backward apply on load: aux2 = conv1's raw output (ld_in), w = the layer's forward table (XL_OP_GN_FINAL with
    // out2), bias = the coefficients [B][Cout][3] of XL_OP_GNB_FINAL, flags = the GroupNorm's XL_GN_RELU_IN; the plain form gets zeros
    const bool fold = op.aux2 != nullptr;
    const auto kernel = fold ? conv1_wgrad_kernel<true> : conv1_wgrad_kernel<false>;
    if (lds > 64 * 1024) {
        static XlLdsLimit configured[2];     // per instantiation, tracked per device
        if (configured[fold].configure(reinterpret_cast<const void *>(kernel), lds) != XL_OK) return XL_ERR_HIP;
    }
    if (fold && (!op.w || !op.bias || op.ld_in % 4 != 0)) return XL_ERR_ARG;
    hipLaunchKernelGGL(kernel, dim3(rb, op.B), dim3(256), lds, st, (const float *)op.in, (const float *)op.aux, (float *)op.stats2, op.B, op.Cin,
                       op.Hi, op.Wi, op.ld_aux, rowsPerBlock, (const float *)op.aux2, fold ? op.ld_in : 0, (const float *)(fold ? op.w : nullptr),
                       (const float *)(fold ? op.bias : nullptr), (fold && (op.flags & XL_GN_RELU_IN)) ? 1 : 0);
    hipLaunchKernelGGL(conv1_wgrad_reduce_kernel, dim3(28), dim3(256), 0, st,
                       (const float *)op.stats2, (float *)op.out, (float *)op.out2, blocks, op.Cin);
    return XL_OK;
}

