// crossloc_hip: the launcher of the 1x1 convolutions and XL_CONV_SPLIT_ACT products on the matrix pipe - once, for both operand
// forms (csrc/xl_gemm_split.hip: six passes on three bf16 terms; csrc/xl_gemm_pair.hip: three passes on fp16 pairs).  The kernels
// stay with their forms (term count, ring depth, epilogue order differ); the checks of the op, the argument fill, the tile forms
// and their launches are the same for both and are here.
//
// XL_OP_CONV with XL_CONV_SPLIT_BF16 | XL_CONV_SPLIT_IL (| XL_CONV_PAIR_F16) and nchunks2 <= 1: a 1x1 stride-1 convolution, fp32 NHWC
// in / out (ld_in / ld_out), w = the form's weight layout ([Cout][Cin/16][3][16] bf16; [Cout][Cin/16][2][16] fp16 + the scales),
// bias, optionally XL_CONV_NORM_IN (aux2 = [B][Cin][2] coefficients) and the statistics epilogue (stats / groups / nchunks with
// 256-row tiles: nchunks >= ceil(HW / 256) + 1, 16 channels per group).  With XL_CONV_SPLIT_ACT and nchunks2 = Z > 1: the Z batched
// products of a Winograd layer, in = V fp32 [Z][rows][Cin], out = M fp32 [Z][rows][Cout] (XL_CONV_M_TILE_MAJOR: [row][Z][Cout]).
//
// reserved_i selects the tile form: +-256 (or 0 / 64, what the fp32 path passes): 256 x 256 tiles; 192: 256 rows x 128 columns;
// 384: 256 x 256 tiles for the full rounds of the 256 CUs and 256 x 128 tiles for a last partial round (same statistics rows);
// +-128: 128 x 128 tiles (the statistics epilogue then writes one entry per 128-row tile: nchunks >= ceil(HW / 128) + 1,
// GN_FINAL / GN_APPLY take 128); negative: tiles start at image boundaries.
//
// Form (SplitConv1x1 / PairConv1x1, beside their kernels) names what differs: Args, the kernels' argument struct (= their kernarg
// layout); kWeightBytes per weight element (6 / 4); kScale: op.scale is required; lds_bytes<NW, BN>(); fill_extra(op, a, Z) for
// the fields only this form has; kernel<NORM, ACC, NW, ZB, BN> and res_kernel<NW, BN>; kClk with clk_wanted() and launch_clk(...)
// for the form's measurement launch (XL_PAIR_CLK).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xl_launch.h"

// One launch of the tile form NW x BN (8 x 256: 256 x 256 tiles, 8 x 128: 256 x 128, 4 x 128: 128 x 128).
// tileFrom / tileCount: this launch covers the tiles [tileFrom, tileFrom + tileCount) of the form's own (z, m-tile, n-tile)
// numbering (tileCount < 0: all of them).  A 256 x 256 tile t is the 256 x 128 tiles 2t and 2t + 1.
template <class Form, int NW, int BN>
int xl_conv1x1_launch(const xl_op &op, typename Form::Args a, bool norm, int Z, hipStream_t st, int tileFrom = 0, int tileCount = -1)
{
    using Args = typename Form::Args;
    constexpr int BM = 32 * NW;
    const bool perImage = op.reserved_i < 0;         // tiles start at image boundaries (reserved_i = -256 / -128)
    a.tpi = perImage ? (a.HW + BM - 1) / BM : 0;
    a.nbm = perImage ? op.B * a.tpi : (int)(((long long)a.M + BM - 1) / BM);
    a.nbn = (op.Cout + BN - 1) / BN;
    const size_t lds = Form::template lds_bytes<NW, BN>();
    const bool accumulate = (op.flags & XL_CONV_ACCUMULATE) != 0;
    const bool resid = norm && a.res != nullptr;
    const bool dominant = Z > 1 && op.Cin == 512 && op.Cout == 512 && !accumulate && !norm;     // the 512 -> 512 Winograd layers
    // the six kernels of a tile form, in the order of their slots: plain, NORM, accumulate, batched, batched 512 -> 512, residual
    static void (*const kernels[6])(Args) = { Form::template kernel<false, false, NW, 0, BN>, Form::template kernel<true, false, NW, 0, BN>,
                                              Form::template kernel<false, true, NW, 0, BN>, Form::template kernel<false, false, NW, 1, BN>,
                                              Form::template kernel<false, false, NW, 2, BN>, Form::template res_kernel<NW, BN> };
    static XlLdsLimit configured[6];
    const int slot = accumulate ? 2 : (resid ? 5 : (norm ? 1 : (dominant ? 4 : (Z > 1 ? 3 : 0))));
    void (*const kernel)(Args) = kernels[slot];
    if (configured[slot].configure(reinterpret_cast<const void *>(kernel), lds) != XL_OK) return XL_ERR_HIP;
    const int nwg = tileCount < 0 ? a.nbm * a.nbn * Z : tileCount;
    a.tile0 = tileFrom; a.ntiles = nwg;
    const int grid = xl_persistent_grid(nwg);
    if constexpr (Form::kClk && NW == 8 && BN == 256) {
        if (Form::clk_wanted() && !accumulate && Z == 1) return Form::launch_clk(op, a, norm, resid, lds, grid, st);
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * NW), lds, st, a);
    return XL_OK;
}

template <class Form>
int xl_conv1x1_run(const xl_op &op, hipStream_t st)
{
    const long long M = (long long)op.B * op.Ho * op.Wo;
    const int HW = op.Ho * op.Wo;
    const bool norm = (op.flags & XL_CONV_NORM_IN) != 0;
    const bool small = op.reserved_i == 128 || op.reserved_i == -128;
    const int BM = small ? 128 : 256;
    const int Z = op.nchunks2 > 1 ? op.nchunks2 : 1;            // Z > 1: XL_CONV_SPLIT_ACT, the batched GEMMs of a Winograd layer
    if (Z > 1 && (op.bias || op.stats || norm || op.reserved_i < 0 || op.ld_in != op.Cin || op.ld_out != op.Cout)) return XL_ERR_ARG;
    if (op.ksize != 1 || op.stride != 1 || op.Cin % 32 != 0 || op.Cout % 256 != 0 || op.Cout > 1024 || op.ld_in < op.Cin ||
        op.ld_out < op.Cout || (op.ld_in & 3) || (op.ld_out & 3) || ((op.flags & XL_CONV_ACCUMULATE) && (norm || Z > 1 || op.stats)) || !op.in ||
        !op.w || !op.out || (Form::kScale && !op.scale) || (((uintptr_t)op.in | (uintptr_t)op.out | (uintptr_t)op.w) & 15) || M >= 0x7fffffffLL ||
        (long long)op.Cout * op.Cin * Form::kWeightBytes >= 0x7fffffffLL || 256LL * op.ld_in * 4 >= 0x7fffffffLL || 256LL * op.ld_out * 4 >= 0x7fffffffLL)
        return XL_ERR_ARG;
    if (norm && (!op.aux2 || op.Cin > 512 || HW < BM)) return XL_ERR_ARG;
    if (op.stats && (op.groups <= 0 || op.Cout != 16 * op.groups || HW < BM || op.nchunks < (HW + BM - 1) / BM + 1)) return XL_ERR_ARG;
    if (op.reserved_i < 0 && HW < BM) return XL_ERR_ARG;
    typename Form::Args a;
    a.in = (const float *)op.in; a.u = (decltype(a.u))op.w; a.bias = (const float *)op.bias; a.out = (float *)op.out;
    a.coef = (const float *)op.aux2;
    a.normLo = (op.flags & XL_CONV_NORM_RELU) ? 0.f : -__builtin_inff();
    a.stats = (double *)op.stats; a.HW = HW; a.G = op.groups; a.nchunks = op.nchunks; a.B = op.B;
    a.M = (int)M; a.C = op.Cin; a.N = op.Cout; a.ldIn = op.ld_in; a.ldOut = op.ld_out;
    a.Z = Z; a.zIn = M * op.ld_in; a.zOut = M * op.ld_out;
    a.res = nullptr; a.ldRes = 0;
    Form::fill_extra(op, a, Z);
    if (op.flags & XL_CONV_NORM_ADD) {                // the producer's GroupNorm + ReLU + residual (aux, ld_aux) + ReLU applied on load
        if (!norm || !(op.flags & XL_CONV_NORM_RELU) || !op.aux || op.ld_aux < op.Cin || (op.ld_aux & 3) || ((uintptr_t)op.aux & 15) || Z > 1 ||
            256LL * op.ld_aux * 4 >= 0x7fffffffLL) return XL_ERR_ARG;
        a.res = (const float *)op.aux; a.ldRes = op.ld_aux;
    }
    if (op.flags & XL_CONV_M_TILE_MAJOR) {            // result [row][Z][Cout]: a row of product z starts Z*Cout floats after the one before
        if (Z < 2 || op.ld_out != op.Cout || 256LL * Z * op.Cout * 4 >= 0x7fffffffLL) return XL_ERR_ARG;
        a.zOut = op.Cout; a.ldOut = Z * op.Cout;
    }
    if (small) return xl_conv1x1_launch<Form, 4, 128>(op, a, norm, Z, st);
    if (op.reserved_i == 192) return xl_conv1x1_launch<Form, 8, 128>(op, a, norm, Z, st);
    if (op.reserved_i == 384) {
        // full rounds of 256 x 256 tiles on the 256 CUs, then the rest as 256 x 128 tiles when those fit in ONE round (0.65 of
        // the time of a round of large tiles): two launches over disjoint tile ranges of the same output
        const int nbig = (int)((M + 255) / 256) * (op.Cout / 256) * Z, full = nbig / 256 * 256, rem = nbig - full;
        if (full > 0 && rem > 0 && 2 * rem <= 256) {
            const int rc = xl_conv1x1_launch<Form, 8, 256>(op, a, norm, Z, st, 0, full);
            return rc != XL_OK ? rc : xl_conv1x1_launch<Form, 8, 128>(op, a, norm, Z, st, 2 * full, 2 * rem);
        }
        if (full == 0 && 2 * rem <= 256) return xl_conv1x1_launch<Form, 8, 128>(op, a, norm, Z, st);
    }
    return xl_conv1x1_launch<Form, 8, 256>(op, a, norm, Z, st);
}
