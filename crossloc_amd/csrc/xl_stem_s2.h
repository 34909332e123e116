// crossloc_hip: the stride-2 3x3 stem convolutions (conv2 32->64, conv3 64->128, conv4 128->256; networks.py:191-201 of
// the reference) of inference plans on the matrix pipe, fp32-accurate - the loop, once, for both operand forms.
//
//   out[m][n] = bias[n] + sum_{tap, c} f(in[pix(m, tap)][c]) * W[n][tap][c]        m = output pixel (B*Ho*Wo of them, NHWC)
//
// f = the producer's deferred GroupNorm + ReLU (per-(image, channel) {scale, shift}, applied to in-image pixels only: the
// zero padding of the convolution stays zero) or the identity.  The loop is split_conv1x1_kernel's: persistent workgroups
// walk tiles of 256 (128) output pixels x all Cout channels; the weights - converted once per plan, interleaved planes, K
// ordered tap-major - stream by LDS-DMA through a ring of three stages, two K-steps ahead of the multiplies; the activations arrive as fp32: every thread gathers 8 channels of ONE source pixel of its row
// (row = tid >> 1; the pixel moves with the tap: (2 oy + dy - 1, 2 ox + dx - 1), out of the image -> an out-of-range buffer
// offset, which reads as zero), two K-steps ahead, and normalises, converts and writes them into the activation stage of the
// next K-step under the MFMAs of the current one.  A K-step = 16 channels of one tap = one k-depth of
// v_mfma_f32_32x32x16_bf16 / _f16.  Workgroups: Cout 256: 8 waves (2 x 4 of 128 x 64) on tiles of 256 pixels, one per CU;
// Cout 128: 4 waves (2 x 2 of 64 x 64) on tiles of 128 pixels, two per CU; Cout 64: 4 waves (4 x 1 of 32 x 64) on tiles of 128
// pixels, three per CU - a K-step of the narrow layers has few MFMAs per wave (24 / 12 in the six-pass form) under the same
// fixed costs (conversion, LDS traffic, the barrier), so several independent workgroups per CU fill each other's gaps.
// Everything the buffer instructions take as scalars (descriptor, scalar offsets, the LDS base in M0) is passed through readfirstlane where the compiler would otherwise
// carry it in vector registers across the loop and wrap each load in a readfirstlane loop.
// The GroupNorm statistics of the output come from the epilogue (round 4; until then XL_OP_GN_STATS re-read the output).
//
// The two operand forms (PAIR = false / true; csrc/xl_stem_split.hip and csrc/xl_stem_pair.hip) differ in the places marked
// `if constexpr (PAIR)` of csrc/xl_stem_s2_body.h and nowhere else:
//   * six passes on three bf16 terms (operands as exact sums of three bf16 terms, six term pairs, fp32 accumulation -
//     csrc/xl_gemm_split.hip explains the arithmetic).  Weights [Cout][9 Cin / 16][3][16] bf16; LDS rows of 96 bytes = 6 slots
//     of 16, the slots of row r rotated by (r >> 3) & 1.  The weight stage of a K-step is Cout x 96 bytes = 24 / 12 / 6 DMA
//     instructions: every wave issues three per K-step (so that the K-step is straight-line code and the counted vmcnt waits
//     are the same in all waves); with Cout 64 the instructions of waves 2 and 3 read out of range and write their zeros into
//     a scratch KB of LDS.
//   * three passes on fp16 PAIRS (round 5), the arithmetic of csrc/xl_gemm_pair.hip: an activation (times the plan's
//     power-of-two scale) is {hi, lo' = (a - hi) 2^11}, a weight (times its matrix's own power of two) {hi, lo} with
//     hs = hi 2^-11 derived in registers; products hs x lo', lo x hi, hi x hi on v_mfma_f32_32x32x16_f16, fp32 accumulation,
//     exact un-scaling in the epilogue.  Weights: [Cout][9 Cin / 16][2][16] fp16, K ordered tap-major, + 2 floats
//     (xl_cnn_pair_weight with taps = 9).  Both operands: 64-byte LDS rows, slot s of row r at s ^ swz(r).  A weight stage is
//     Cout x 64 bytes = 16 / 8 / 4 DMA instructions: every wave issues two per K-step (straight-line code, the same counted
//     waits in all waves; with Cout 64 those of waves 2 and 3 land in a scratch KB).
// What a form supplies: row pitch and plane count, the slot of a 16-byte piece in its row, the DMA instructions per wave and
// K-step with their source addressing, the conversion (with the {scale, shift} * s table and the bias in the scaled domain of
// the pairs), the fragment type and MFMA, its K-step - term order, scheduling groups and counted waits are one schedule and
// stay one piece of text per form - and the un-scaling at the head of the pair epilogue.
//
// The kernel's statements are csrc/xl_stem_s2_body.h, which each form's __global__ function includes between its braces.  They
// are not a __device__ function that the two kernels call: the compiler optimises such a function on its own before it
// inlines it, and the assembly of all 24 instantiations then differs from what the same statements give inside the kernel
// (tried: e.g. split_conv3x3s2_kernel<256, false, 8> grows from 34616 to 36448 bytes of code).  These kernels have no
// registers to spare and their waits are counted by hand, so the text is shared and the compiler's view of it is left as it
// was; tools/kernel_asm_diff.py holds a change here to the assembly.
//
// The argument struct (StemArgs / PairStemArgs, defined beside their __global__ wrappers) carries, for both forms:
//    const float *in; u (the weights); const float *bias; float *out;
//    const float *coef; float normLo;                 NORM: [B][Cin][2] {scale, shift}; lower clamp (0 = ReLU, -inf = none)
//    int B, Hi, Wi, Cin, Ho, Wo, ldIn, ldOut, M, nbm;
//    int nbn;                                         column tiles of NT channels (1, or 2 when Cout = 256 runs on 128-wide tiles)
//    double *stats; int G, nchunks;
// GroupNorm partial sums of the output (stats == nullptr: none), G = Cout / 2 (Cout 64), / 4 (128), / 8 (256) groups:
// [B][nchunks][G][2] fp64 {sum, sum of squares}; chunk = (tile index within the image) * WM + (the wave's row block wm): one
// writer per entry, every entry of a tile that overlaps the image is written.  nchunks >= (ceil(Ho*Wo / BM) + 1) * WM.
// PAIR adds uInv (the inverse weight scale, one float) and aScale ({s, 1 / s} of the activations).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>

#include "xl_launch.h"
#include "xl_operand_math.h"

// ---- the host side.  Form (csrc/xl_stem_split.hip, csrc/xl_stem_pair.hip) names the operand form's argument struct and kernel:
//    static constexpr bool PAIR;  using Args = ...;
//    template <int NT, bool NORM, int NW, int WPS, int CPT> static constexpr auto kernel = the __global__ wrapper;
template <class Form, int NT, int NW, int PER_CU, int CPT = 8>
int xl_stem_s2_launch(typename Form::Args a, bool norm, hipStream_t st)
{
    constexpr int kUnit = Form::PAIR ? 64 : 96;
    constexpr int BM = 4 * NW * CPT;
    const size_t lds = 3 * NT * kUnit + 2 * BM * kUnit + 4096 + 1024 + 1024;
    static XlLdsLimit configured[2];
    constexpr int WPS = NW * PER_CU / 4 < 2 ? 2 : NW * PER_CU / 4;
    constexpr auto kNorm = Form::template kernel<NT, true, NW, WPS, CPT>, kPlain = Form::template kernel<NT, false, NW, WPS, CPT>;
    if (configured[norm].configure(reinterpret_cast<const void *>(norm ? kNorm : kPlain), lds) != XL_OK) return XL_ERR_HIP;
    a.nbm = (a.M + BM - 1) / BM;
    constexpr int WM = NW / (NT / 64);
    if (a.stats && (a.nchunks < ((a.Ho * a.Wo + BM - 1) / BM + 1) * WM || a.G * (NT == 64 ? 2 : NT == 256 || a.nbn == 2 ? 8 : 4) != a.nbn * NT)) return XL_ERR_ARG;
    int grid = 256 * PER_CU;                                          // persistent: PER_CU workgroups per CU (LDS- and register-bound)
    if (grid > ((a.nbm * a.nbn + 7) & ~7)) grid = (a.nbm * a.nbn + 7) & ~7;
    hipLaunchKernelGGL((norm ? kNorm : kPlain), dim3(grid), dim3(64 * NW), lds, st, a);
    return XL_OK;
}

// XL_OP_CONV with ksize 3, stride 2 and XL_CONV_SPLIT_BF16 | XL_CONV_SPLIT_IL (| XL_CONV_PAIR_F16): in fp32 NHWC [B,Hi,Wi,Cin]
// (ld_in), out fp32 NHWC [B,Ho,Wo,Cout] (ld_out), w = the form's weights (K = tap * Cin + c, tap = 3 ky + kx), bias (, scale);
// optionally XL_CONV_NORM_IN (aux2 = [B][Cin][2] coefficients, XL_CONV_NORM_RELU).  Cin in {32, 64, 128}, Cout in {64, 128, 256},
// Ho*Wo >= 256.  stats (optional, groups = 32, nchunks): GroupNorm partial sums of the output, see the argument struct - chunk =
// tile * WM + wm with (rows per tile, WM) = (128, 4) for Cout 64, (128, 2) for Cout 128, (256, 2) for Cout 256 and (128, 2)
// for its latency form; XL_OP_GN_FINAL sums them with reserved_i = rows per tile, stride = WM.
template <class Form>
int xl_stem_s2_run(const xl_op &op, hipStream_t st)
{
    const long long M = (long long)op.B * op.Ho * op.Wo;
    const bool norm = (op.flags & XL_CONV_NORM_IN) != 0;
    if (op.ksize != 3 || op.stride != 2 || (op.Cin != 32 && op.Cin != 64 && op.Cin != 128) ||
        (op.Cout != 64 && op.Cout != 128 && op.Cout != 256) || op.Ho != (op.Hi - 1) / 2 + 1 || op.Wo != (op.Wi - 1) / 2 + 1 ||
        op.Ho * op.Wo < 256 || op.ld_in < op.Cin || op.ld_out < op.Cout || (op.ld_in & 3) || (op.ld_out & 3) || !op.bias ||
        (op.flags & (XL_CONV_ACCUMULATE | XL_CONV_DGRAD)) || !op.in || !op.w || !op.out || (op.stats && ((uintptr_t)op.stats & 15)) ||
        (((uintptr_t)op.in | (uintptr_t)op.out | (uintptr_t)op.w) & 15) || M >= 0x7fffffffLL - 256 || (Form::PAIR && !op.scale) ||
        2LL * op.Hi * op.Wi * op.ld_in * 4 >= 0x7fffffffLL || 256LL * op.ld_out * 4 >= 0x7fffffffLL || (norm && !op.aux2))
        return XL_ERR_ARG;
    typename Form::Args a;
    if constexpr (Form::PAIR) {                                       // (the two floats behind the weights: {scale, 1 / scale})
        a.uInv = reinterpret_cast<const float *>((const unsigned char *)op.w + (long long)op.Cout * 9 * op.Cin * 4) + 1;
        a.aScale = (const float *)op.scale;
    }
    a.in = (const float *)op.in; a.u = (decltype(a.u))op.w; a.bias = (const float *)op.bias; a.out = (float *)op.out;
    a.coef = (const float *)op.aux2;
    a.normLo = (op.flags & XL_CONV_NORM_RELU) ? 0.f : -__builtin_inff();
    a.B = op.B; a.Hi = op.Hi; a.Wi = op.Wi; a.Cin = op.Cin; a.Ho = op.Ho; a.Wo = op.Wo;
    a.ldIn = op.ld_in; a.ldOut = op.ld_out; a.M = (int)M; a.nbm = 0; a.nbn = 1;
    a.stats = (double *)op.stats; a.G = op.groups; a.nchunks = op.nchunks;
    static const char *form = getenv("XL_STEM_FORM");                // measurement switch: "8x2" = 8-wave workgroups, two per CU
    if (op.Cout == 64) return form && !strcmp(form, "8x2") ? xl_stem_s2_launch<Form, 64, 8, 2>(a, norm, st)
                            : form && !strcmp(form, "c16") ? xl_stem_s2_launch<Form, 64, 4, 2, 16>(a, norm, st) : xl_stem_s2_launch<Form, 64, 4, 3>(a, norm, st);
    if (op.Cout == 128) return form && !strcmp(form, "8x2") ? xl_stem_s2_launch<Form, 128, 8, 1>(a, norm, st) : xl_stem_s2_launch<Form, 128, 4, 2>(a, norm, st);
    if (op.reserved_i == 128) {                                       // latency form (the host asks when 256-row tiles cannot fill
        a.nbn = 2;                                                    // the chip): 128 x 128 tiles, two column tiles per row tile
        return xl_stem_s2_launch<Form, 128, 4, 2>(a, norm, st);
    }
    return xl_stem_s2_launch<Form, 256, 8, 1>(a, norm, st);
}
