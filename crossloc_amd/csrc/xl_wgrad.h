// crossloc_hip: weight gradients of training plans on the matrix pipe, fp32-accurate - the loop, once, for both operand forms.
//
//   P_z,s[o][c] = sum_{t in split s} dY_z[t][o] * X_z[t][c]            ("pixels as the GEMM K dimension")
//
// for a 1x1 layer (Z = 1, t = the B*H*W pixels, split-K over `splits` workgroups per tile) and for the batched products of a
// Winograd layer (Z = (m+2)^2 frequencies, t = the tiles, dY = dM = A dY A^T, X = V = B^T x B); the fixed-order reduce over the
// splits and the layout / transform of the result stay with wgrad_reduce_kernel / XL_OP_WINO_WFINAL (csrc/xl_wgrad_f32.hip).
//
// Both operands arrive as fp32 with the K dimension (t) OUTERMOST in memory - rows of channels.  The MFMA wants 8
// consecutive k per lane and row, so a thread owns ONE channel (row of the operand tile) and 8 consecutive t: 8 dword loads
// whose lanes run along the channels (256 contiguous bytes per wave-load), converted to the form's planes in registers
// and written as 16-byte pieces into the same LDS rows as the form's other kernels - the transpose costs
// nothing.  Tile 256 (o) x 256 (c), 8 waves of 128 x 64, K-step = 16 t; one register set per operand, loaded a step ahead,
// converted under the MFMAs of the step; two LDS stages, one barrier per step.
//
// The two operand forms (PAIR = false / true; csrc/xl_wgrad_split.hip and csrc/xl_wgrad_pair.hip) differ in the places marked
// `if constexpr (PAIR)` of csrc/xl_wgrad_body.h and nowhere else:
//   * six passes on three bf16 terms (operands as exact sums of three bf16 terms, six term pairs, fp32 accumulation -
//     csrc/xl_gemm_split.hip explains the arithmetic): 3 x 16 bytes per thread and operand into rotated 96-byte LDS rows, two
//     stages of 2 x 24 KB; the conversion runs under the MFMAs of terms 4 and 5.
//   * three passes on fp16 PAIRS (round 5), the arithmetic of csrc/xl_gemm_pair.hip; 64-byte rows, slot s of row r at s ^ swz(r),
//     two stages of 2 x 16 KB.  Neither operand is packed ahead of time here, and both are converted in the kernel, but they are
//     not symmetric:
//       - X - the layer's (normalised) input, or V = B^T x B for a Winograd layer - is a GroupNorm output: it takes the PLAN's
//         power-of-two scale (a bound, loose by construction) and the form that does not mind: {hi, lo' = (x - hi) 2^11};
//       - dY - a gradient (or dM = A dY A^T) - has no static bound: its scale comes from the DATA, the maximum magnitude the pass that
//         wrote it recorded (xl_wave_max_commit in csrc/xl_gn_bwd.hip, csrc/xl_wgrad_f32.hip; max |dY| 2^e in [2^14, 2^15)), which makes it tight - so dY takes
//         the weight-like form {hi, lo = dY - hi} and its hs = hi 2^-11 is derived in registers.
//     Products hs x lo', lo x hi, hi x hi on v_mfma_f32_32x32x16_f16, fp32 accumulation, exact un-scaling of the partial tile.
// A form's K-step - fragment reads, term order, scheduling groups - is one schedule and stays one piece of text per form.
//
// The kernel's statements are csrc/xl_wgrad_body.h, which each form's __global__ function includes between its braces.  They are
// not a __device__ function that the two kernels call: the compiler optimises such a function on its own before it inlines it,
// and the assembly of all four kernels then differs from what the same statements give inside the kernel (tried: 1594 -> 1499
// and 1816 -> 1828 lines for wgrad_split_kernel<false> / <true>).  tools/kernel_asm_diff.py holds a change here to the assembly.
//
// The argument struct (WgSplitArgs / WgPairArgs, beside their kernels) carries, for both forms:
//    const float *x, *dy; float *partial;
//    int M, Cin, Cout, ldX, ldY, splits, mPerSplit, zCount, nbo, nbc;  long long zX, zY;  unsigned xBytes, dyBytes;
//    const float *coef; int HW; float normLo;
// NORM: `x` is the RAW output of the producing convolution; its GroupNorm (+ReLU) is applied while the operand is loaded
// (round 4, training plans whose GroupNorm applies are left to the consumers): coef = [B][Cin][2] {scale, shift}, HW pixels
// per image (a multiple of 8: the 8 consecutive t of a thread belong to one image), normLo = 0 (ReLU) or -inf.
// PAIR adds xScale ({s, 1 / s} of X: the plan's activation scale; its Winograd pair for V) and dyAmax (max |dY| (or |dM|) of the
// launch's dY operand, as float bits).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "xl_launch.h"
#include "xl_operand_math.h"

// XL_OP_WGRAD with ksize 1 and XL_CONV_SPLIT_BF16 (| XL_CONV_PAIR_F16): the same operands and scratch layout as the fp32 kernel -
// in = x [M][Cin] (ld_in), aux = dY [M][Cout] (ld_aux), stats2 = partial [z][splits][Cout][Cin], groups = Z batched GEMMs (dense
// operands), nchunks2 = splits.  Cin % 4 == 0.  The caller runs wgrad_reduce_kernel afterwards.  XL_CONV_NORM_IN (1x1 layers,
// Z = 1): `in` is the raw output of the producing convolution, aux2 = its {scale, shift} pairs [B][Cin][2], XL_CONV_NORM_RELU;
// Ho*Wo % 8 == 0.  PAIR: scale = {s, 1 / s} of `in` (the plan's activation scale), out2 = the slot holding max |aux| as float bits
// (written by the pass that produced `aux`).
// Form names the operand form's argument struct and kernel:
//    static constexpr bool PAIR;  using Args = ...;  template <bool NORM> static constexpr auto kernel = the __global__ function;
template <class Form>
int xl_wgrad_run(const xl_op &op, hipStream_t st)
{
    if (op.ksize != 1 || op.stride != 1 || op.nchunks2 < 1 || op.ld_in % 4 != 0 || op.ld_aux % 4 != 0 || op.Cin % 4 != 0 ||
        !op.in || !op.aux || !op.stats2 || (Form::PAIR && (!op.scale || !op.out2))) return XL_ERR_ARG;
    const bool norm = (op.flags & XL_CONV_NORM_IN) != 0;
    if (norm && (!op.aux2 || op.groups > 1 || (op.Ho * op.Wo) % 8 != 0)) return XL_ERR_ARG;
    typename Form::Args a;
    if constexpr (Form::PAIR) { a.xScale = (const float *)op.scale; a.dyAmax = (const unsigned *)op.out2; }
    a.x = (const float *)op.in; a.dy = (const float *)op.aux; a.partial = (float *)op.stats2;
    a.M = op.B * op.Ho * op.Wo; a.Cin = op.Cin; a.Cout = op.Cout; a.ldX = op.ld_in; a.ldY = op.ld_aux;
    a.splits = op.nchunks2;
    a.mPerSplit = ((a.M + a.splits - 1) / a.splits + 15) / 16 * 16;
    a.nbo = (op.Cout + 255) / 256; a.nbc = (op.Cin + 255) / 256;
    a.zCount = op.groups > 1 ? op.groups : 1;
    if (a.zCount > 1 && (op.ld_in != op.Cin || op.ld_aux != op.Cout)) return XL_ERR_ARG;
    a.zX = (long long)a.M * op.Cin; a.zY = (long long)a.M * op.Cout;
    const long long xb = (((long long)a.M - 1) * op.ld_in + op.Cin) * 4, yb = (((long long)a.M - 1) * op.ld_aux + op.Cout) * 4;
    if (xb >= 0x7fffffffLL || yb >= 0x7fffffffLL) return XL_ERR_ARG;
    a.xBytes = (unsigned)xb; a.dyBytes = (unsigned)yb;
    a.coef = (const float *)op.aux2; a.HW = op.Ho * op.Wo;
    a.normLo = (op.flags & XL_CONV_NORM_RELU) ? 0.f : -__builtin_inff();
    const size_t lds = 4 * 256 * (size_t)(Form::PAIR ? 64 : 96);      // two stages of two operands of 256 rows: 64 KB / 96 KB
    static XlLdsLimit configured[2];
    constexpr auto kNorm = Form::template kernel<true>, kPlain = Form::template kernel<false>;
    if (configured[norm].configure(reinterpret_cast<const void *>(norm ? kNorm : kPlain), lds) != XL_OK) return XL_ERR_HIP;
    hipLaunchKernelGGL((norm ? kNorm : kPlain), dim3(a.zCount * a.nbo * a.nbc * a.splits), dim3(512), lds, st, a);
    return XL_OK;
}
