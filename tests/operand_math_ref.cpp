// TEST INFRASTRUCTURE ONLY: the functions of crossloc_amd/csrc/xl_operand_math.h applied to arrays, for the CPU.
// tests/test_operand_math_cpu.py builds this file with clang++ (-x c++ -O2 -ffp-contract=off, nothing from HIP), loads it with
// ctypes and compares every output bit for bit with numpy.  bf16 / fp16 values travel as their 16 bits; n is a multiple of 8.
#include "xl_operand_math.h"

static inline uint16_t bits16(_Float16 h) { return __builtin_bit_cast(uint16_t, h); }

extern "C" {

// planes [3][n]; form 0: xl_bf16_split3, 1: xl_bf16_split3_pk(f32x2), 2: xl_bf16_split3_pk(float, float)
void xo_bf16_split3(const float *x, int n, int form, uint16_t *planes)
{
    for (int i = 0; i < n; i += 2) {
        unsigned w[3], b[3];
        if (form == 1) xl_bf16_split3_pk(f32x2{ x[i], x[i + 1] }, w[0], w[1], w[2]);
        else if (form == 2) xl_bf16_split3_pk(x[i], x[i + 1], w[0], w[1], w[2]);
        else {
            xl_bf16_split3(x[i], w[0], w[1], w[2]);
            xl_bf16_split3(x[i + 1], b[0], b[1], b[2]);
            for (int p = 0; p < 3; ++p) w[p] |= b[p] << 16;
        }
        for (int p = 0; p < 3; ++p) { planes[p * n + i] = (uint16_t)w[p]; planes[p * n + i + 1] = (uint16_t)(w[p] >> 16); }
    }
}

// form bit 0: the scaled pair {hi, lo'}; bit 1: the f32x2 variants
void xo_f16_pair(const float *x, int n, int form, uint16_t *hi, uint16_t *lo)
{
    for (int i = 0; i < n; i += 2) {
        f16x2 h, l;
        if (form == 3) xl_f16_pair_scaled_pk(f32x2{ x[i], x[i + 1] }, h, l);
        else if (form == 2) xl_f16_pair_pk(f32x2{ x[i], x[i + 1] }, h, l);
        if (form >= 2) { hi[i] = bits16(h[0]); hi[i + 1] = bits16(h[1]); lo[i] = bits16(l[0]); lo[i + 1] = bits16(l[1]); }
        else for (int e = i; e < i + 2; ++e) form ? xl_f16_pair_scaled(x[e], hi[e], lo[e]) : xl_f16_pair(x[e], hi[e], lo[e]);
    }
}

void xo_f16_hs(const uint16_t *hi, int n, uint16_t *hs)
{
    for (int i = 0; i < n; i += 8) {
        f16x8 h;
        for (int e = 0; e < 8; ++e) h[e] = __builtin_bit_cast(_Float16, hi[i + e]);
        const f16x8 s = xl_f16_hs(h);
        for (int e = 0; e < 8; ++e) hs[i + e] = bits16(s[e]);
    }
}

void xo_pair_scale_of_max(const uint32_t *maxBits, int n, float *scale)
{
    for (int i = 0; i < n; ++i) scale[i] = xl_pair_scale_of_max(maxBits[i]);
}

}  // extern "C"
