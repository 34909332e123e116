// crossloc_hip: the stride-2 3x3 stem convolutions of inference plans as fp16 PAIRS, three matrix-pipe passes (round 5).  The loop
// is that of csrc/xl_stem_s2.h, which explains it; here are the form's argument struct, its kernel and its entry point.
#include "xl_stem_s2.h"

namespace {

struct PairStemArgs {
    const float *in; const unsigned char *u; const float *bias; float *out;
    const float *uInv; const float *aScale;          // inverse weight scale (one float); {s, 1 / s} of the activations
    const float *coef; float normLo;                 // NORM: [B][Cin][2] {scale, shift}; lower clamp (0 = ReLU, -inf = none)
    int B, Hi, Wi, Cin, Ho, Wo, ldIn, ldOut, M, nbm;
    int nbn;                                         // column tiles of NT channels (1, or 2 when Cout = 256 runs on 128-wide tiles)
    double *stats; int G, nchunks;                   // GroupNorm partial sums of the output (csrc/xl_stem_s2.h)
};

template <int NT, bool NORM, int NW, int WPS = (NT == 64 ? 3 : 2), int CPT = 8>    // Cout; normalise on load; waves per workgroup; per SIMD
__global__ __launch_bounds__(64 * NW, WPS)                          // waves per SIMD: 3 workgroups of 4 waves per CU / 2 of 4 / 1 of 8
void pair_conv3x3s2_kernel(PairStemArgs a)
{
    constexpr bool PAIR = xl_dependent<NT, true>;
    const float *const aScale = a.aScale, *const uInv = a.uInv;
#include "xl_stem_s2_body.h"
}

struct PairStem {
    static constexpr bool PAIR = true;
    using Args = PairStemArgs;
    template <int NT, bool NORM, int NW, int WPS, int CPT> static constexpr auto kernel = pair_conv3x3s2_kernel<NT, NORM, NW, WPS, CPT>;
};

}  // namespace

// w = [Cout][9 Cin / 16][2][16] fp16 + 2 floats, scale = {s, 1 / s} of the activations; everything else as csrc/xl_stem_s2.h says
// at xl_stem_s2_run
int xl_run_pair_stem(const xl_op &op, hipStream_t st) { return xl_stem_s2_run<PairStem>(op, st); }
