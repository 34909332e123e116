// crossloc_hip: weight gradients of training plans as fp16 PAIRS, three matrix-pipe passes (round 5).  The loop is that of
// csrc/xl_wgrad.h, which explains it; here are the form's argument struct, its kernel and its entry point.
#include "xl_wgrad.h"

namespace {

struct WgPairArgs {
    const float *x, *dy; float *partial;
    int M, Cin, Cout, ldX, ldY, splits, mPerSplit, zCount, nbo, nbc;
    long long zX, zY;
    unsigned xBytes, dyBytes;
    const float *coef; int HW; float normLo;         // NORM: the GroupNorm of `x`, applied on load (csrc/xl_wgrad.h)
    const float *xScale;             // {s, 1 / s} of X (the plan's activation scale; its Winograd pair for V)
    const unsigned *dyAmax;          // max |dY| (or |dM|) of the launch's dY operand, as float bits
};

template <bool NORM>
__global__ __launch_bounds__(512)
void wgrad_pair_kernel(WgPairArgs a)
{
    constexpr bool PAIR = xl_dependent<NORM, true>;
    const float *const xScale = a.xScale; const unsigned *const dyAmax = a.dyAmax;
#include "xl_wgrad_body.h"
}

struct WgPair {
    static constexpr bool PAIR = true;
    using Args = WgPairArgs;
    template <bool NORM> static constexpr auto kernel = wgrad_pair_kernel<NORM>;
};

}  // namespace

int xl_run_wgrad_pair(const xl_op &op, hipStream_t st) { return xl_wgrad_run<WgPair>(op, st); }
