/*
 * xl_operand_math.h — the operand arithmetic of the split (bf16, six passes) and pair (fp16, three passes) GEMM pipes, once.
 *
 *   bf16 split   x = t1 + t2 + t3 exactly: t1 = bf16(x), t2 = bf16(x - t1), t3 = bf16(x - t1 - t2), round to nearest even,
 *                residuals exact in fp32.  The integer form rounds one value on the float's bits; the packed form takes two
 *                through the packed convert, one 32-bit word {bf16(v[0]) low, bf16(v[1]) high} per term.  They compile to
 *                different instructions and every caller chose one deliberately, so they stay separate functions; on finite
 *                inputs they give the same bits (NaN and infinity: not defined by the integer form, fed by no caller).
 *   fp16 pair    x, times a power-of-two scale, = hi + lo with hi = fp16(x), lo = fp16(x - hi): the form of weights and
 *                gradients, whose consumer derives hs = hi 2^-11 in registers.  Activations carry lo' = fp16((x - hi) 2^11),
 *                so that hs x lo' + lo x hi + hi x hi is the product.
 *
 * Contract: expression order and rounding points are the interface - a kernel agrees with the pack kernel that feeds it
 * because both call these functions - and both sides compile with -ffp-contract=off.  Included by the CNN's .hip files
 * (which also take the vector typedefs from here) and by tests/operand_math_ref.cpp, the CPU build that
 * tests/test_operand_math_cpu.py pins bit for bit.  Under hipcc the functions are __host__ __device__; any other C++ compiler
 * that knows ext_vector_type, __bf16 and _Float16 (clang) gets static inline functions and nothing from HIP.
 */
#ifndef XL_OPERAND_MATH_H
#define XL_OPERAND_MATH_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define XL_OPERAND_FN __host__ __device__ __forceinline__
#else
#define XL_OPERAND_FN static inline
#endif
#include <stdint.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr float kXlPairLoScale = 2048.f;                 /* 2^11: lo' = (x - hi) 2^11 */
constexpr float kXlPairHsScale = 0.00048828125f;         /* 2^-11: hs = hi 2^-11 */

/* ---- bf16 split, integer form: fp32 -> bf16 bits (round to nearest even) and back; a = h1 + h2 + h3 */
XL_OPERAND_FN unsigned xl_bf16_rn(float x)
{
    unsigned u = __builtin_bit_cast(unsigned, x);
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}
XL_OPERAND_FN float xl_bf16_f(unsigned h) { return __builtin_bit_cast(float, h << 16); }
XL_OPERAND_FN void xl_bf16_split3(float a, unsigned &h1, unsigned &h2, unsigned &h3)
{
    h1 = xl_bf16_rn(a);
    const float r1 = a - xl_bf16_f(h1);
    h2 = xl_bf16_rn(r1);
    h3 = xl_bf16_rn(r1 - xl_bf16_f(h2));
}

/* ---- bf16 split, packed form: {bf16(x), bf16(y)} (v_cvt_pk_bf16_f32) and the two halves of such a word as floats */
XL_OPERAND_FN unsigned xl_bf16_pk(float x, float y)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{ x, y }, bf16x2));
}
XL_OPERAND_FN float xl_bf16_hi_f(unsigned w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
XL_OPERAND_FN float xl_bf16_lo_f(unsigned w) { return __builtin_bit_cast(float, w << 16); }
/* two values at a time as a float pair (v_pk_add_f32 for the residuals) */
XL_OPERAND_FN void xl_bf16_split3_pk(f32x2 v, unsigned &w1, unsigned &w2, unsigned &w3)
{
    w1 = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    const f32x2 r = v - f32x2{ xl_bf16_lo_f(w1), xl_bf16_hi_f(w1) };
    w2 = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
    const f32x2 r2 = r - f32x2{ xl_bf16_lo_f(w2), xl_bf16_hi_f(w2) };
    w3 = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, bf16x2));
}
/* the same from two scalars with scalar residuals (v_sub_f32): xl_wgrad_split.hip, whose values lie in separate registers */
XL_OPERAND_FN void xl_bf16_split3_pk(float x, float y, unsigned &w1, unsigned &w2, unsigned &w3)
{
    w1 = xl_bf16_pk(x, y);
    const float rx = x - xl_bf16_lo_f(w1), ry = y - xl_bf16_hi_f(w1);
    w2 = xl_bf16_pk(rx, ry);
    w3 = xl_bf16_pk(rx - xl_bf16_lo_f(w2), ry - xl_bf16_hi_f(w2));
}

/* ---- fp16 pair: {hi, lo = x - hi} (weights, gradients) and {hi, lo' = (x - hi) 2^11} (activations) */
XL_OPERAND_FN void xl_f16_pair_pk(f32x2 v, f16x2 &hi, f16x2 &lo)
{
    hi = __builtin_convertvector(v, f16x2);
    lo = __builtin_convertvector(v - __builtin_convertvector(hi, f32x2), f16x2);
}
XL_OPERAND_FN void xl_f16_pair_scaled_pk(f32x2 v, f16x2 &hi, f16x2 &lo)
{
    hi = __builtin_convertvector(v, f16x2);
    lo = __builtin_convertvector((v - __builtin_convertvector(hi, f32x2)) * kXlPairLoScale, f16x2);
}
/* one value at a time, as fp16 bits (the pack kernels) */
XL_OPERAND_FN void xl_f16_pair(float x, uint16_t &hi, uint16_t &lo)
{
    const _Float16 h = (_Float16)x;
    const _Float16 l = (_Float16)(x - (float)h);
    hi = __builtin_bit_cast(uint16_t, h); lo = __builtin_bit_cast(uint16_t, l);
}
XL_OPERAND_FN void xl_f16_pair_scaled(float x, uint16_t &hi, uint16_t &lo)
{
    const _Float16 h = (_Float16)x;
    const _Float16 l = (_Float16)((x - (float)h) * kXlPairLoScale);
    hi = __builtin_bit_cast(uint16_t, h); lo = __builtin_bit_cast(uint16_t, l);
}
XL_OPERAND_FN f16x8 xl_f16_hs(f16x8 hi) { return hi * (_Float16)kXlPairHsScale; }      /* hi 2^-11: 4 x v_pk_mul_f16 */

/* The power of two that brings a matrix whose largest magnitude has the float bits maxBits into [2^14, 2^15): the scale every
 * pair consumer assumes of its weights.  All zero, or a subnormal maximum: no scaling. */
XL_OPERAND_FN float xl_pair_scale_of_max(unsigned maxBits)
{
    if (maxBits == 0u || (maxBits >> 23) == 0u) return 1.f;
    const int E = (int)(maxBits >> 23) - 127;                                    /* floor(log2(max)) */
    int e = 14 - E;
    if (e > 100) e = 100;
    if (e < -100) e = -100;
    return __builtin_bit_cast(float, (unsigned)(e + 127) << 23);
}

#endif
