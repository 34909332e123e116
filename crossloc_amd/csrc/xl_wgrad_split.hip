// crossloc_hip: weight gradients of training plans in the six-pass form on three bf16 terms.  The loop is that of csrc/xl_wgrad.h,
// which explains it; here are the form's argument struct, its kernel and its entry point.
#include "xl_wgrad.h"

namespace {

struct WgSplitArgs {
    const float *x, *dy; float *partial;
    int M, Cin, Cout, ldX, ldY, splits, mPerSplit, zCount, nbo, nbc;
    long long zX, zY;
    unsigned xBytes, dyBytes;
    const float *coef; int HW; float normLo;         // NORM: the GroupNorm of `x`, applied on load (csrc/xl_wgrad.h)
};

template <bool NORM>
__global__ __launch_bounds__(512)
void wgrad_split_kernel(WgSplitArgs a)
{
    constexpr bool PAIR = xl_dependent<NORM, false>;
    const float *const xScale = nullptr; const unsigned *const dyAmax = nullptr;   // (the pair form's scales)
#include "xl_wgrad_body.h"
}

struct WgSplit {
    static constexpr bool PAIR = false;
    using Args = WgSplitArgs;
    template <bool NORM> static constexpr auto kernel = wgrad_split_kernel<NORM>;
};

}  // namespace

int xl_run_wgrad_split(const xl_op &op, hipStream_t st) { return xl_wgrad_run<WgSplit>(op, st); }
