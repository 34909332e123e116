// crossloc_hip: the stride-2 3x3 stem convolutions of inference plans in the six-pass form on three bf16 terms.  The loop is that
// of csrc/xl_stem_s2.h, which explains it; here are the form's argument struct, its kernel and its entry point.
#include "xl_stem_s2.h"

namespace {

struct StemArgs {
    const float *in; const uint16_t *u; const float *bias; float *out;
    const float *coef; float normLo;                 // NORM: [B][Cin][2] {scale, shift}; lower clamp (0 = ReLU, -inf = none)
    int B, Hi, Wi, Cin, Ho, Wo, ldIn, ldOut, M, nbm;
    int nbn;                                         // column tiles of NT channels (1, or 2 when Cout = 256 runs on 128-wide tiles)
    double *stats; int G, nchunks;                   // GroupNorm partial sums of the output (csrc/xl_stem_s2.h)
};

template <int NT, bool NORM, int NW, int WPS = (NT == 64 ? 3 : 2), int CPT = 8>    // Cout; normalise on load; waves per workgroup; per SIMD
__global__ __launch_bounds__(64 * NW, WPS)                          // waves per SIMD: 3 workgroups of 4 waves per CU / 2 of 4 / 1 of 8
void split_conv3x3s2_kernel(StemArgs a)
{
    constexpr bool PAIR = xl_dependent<NT, false>;
    const float *const aScale = nullptr, *const uInv = nullptr;      // (the pair form's scales)
#include "xl_stem_s2_body.h"
}

struct SplitStem {
    static constexpr bool PAIR = false;
    using Args = StemArgs;
    template <int NT, bool NORM, int NW, int WPS, int CPT> static constexpr auto kernel = split_conv3x3s2_kernel<NT, NORM, NW, WPS, CPT>;
};

}  // namespace

// w = [Cout][9 Cin / 16][3][16] bf16; everything else as csrc/xl_stem_s2.h says at xl_stem_s2_run
int xl_run_split_stem(const xl_op &op, hipStream_t st) { return xl_stem_s2_run<SplitStem>(op, st); }
