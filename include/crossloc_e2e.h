/*
 * crossloc_e2e.h — C ABI of the end-to-end training step's own op (libcrossloc_hip.so): per-image finishing of the DSAC*
 * pose gradient, between the solver's backward pass (crossloc_dsac.h) and prediction.backward(grad).
 *
 *   xl_e2e_pose_gradient    g [B,3,Ho,Wo] (d expected pose loss / d scene coordinates, any strides) and loss [B] (the
 *                           solver's expected losses) -> out [B,C,Ho,Wo], the gradient w.r.t. the network's C-channel
 *                           output, and stats [B+1,4].
 *
 * For image b:
 *   n_b         sqrt(sum g^2) over its 3*Ho*Wo elements: float64 squares of the float32 values, summed in a fixed order
 *               (thread t of 1024 owns cells t, t + 1024, ... in ascending order, channels 0, 1, 2 within a cell, then the
 *               block sum of xl_dsac_reduce.h); no floating-point atomics.
 *   accepted_b  loss[b] and every element of g[b] are finite.  (The float64 sum of squares is finite exactly then: a square
 *               is at most 1.2e77.)
 *   s_b         accepted_b ? (float)((double)weight / B * (clip_norm > 0 && n_b > clip_norm ? clip_norm / n_b : 1.0)) : 0.
 *               The divisor is B whatever was rejected: a rejected frame contributes zero, so the gradient of one rank
 *               does not depend on what another rank rejected.
 *   out         beta == 0:  out[b,c<3] = s_b * g[b,c] (one float32 multiply), out[b,c>=3] = 0; `out` is not read.
 *               beta != 0:  out[b,c<3] = beta * out[b,c<3] + s_b * g[b,c], out[b,c>=3] = beta * out[b,c>=3]
 *               (float32, no contraction: two multiplies and one add).
 *               A rejected image contributes exact zeros in place of s_b * g, never 0 * NaN.
 *   stats[b]    { loss[b], n_b, s_b, accepted_b }          (n_b is not finite where g[b] holds a non-finite element)
 *   stats[B]    { mean loss over the accepted frames (0 if none), number accepted, max n_b over the accepted frames
 *                 (0 if none), number of accepted frames that were clipped }, summed in ascending b.
 *
 * One launch of B workgroups, no allocation, no host synchronisation; asynchronous on `stream` (a hipStream_t; NULL = the
 * default stream).  The workgroup that finishes last writes stats[B]; it is found with one integer counter of the library,
 * so calls on ONE device must be ordered against each other (one stream, or events) - calls on different devices are
 * independent.  `out` must not overlap g.
 *
 * Returns 0 or a negative xl status (crossloc_dsac.h), checked before any HIP call: XL_ERR_ARG for a null g / loss / out /
 * stats, B, Ho or Wo not positive, or C < 3; XL_ERR_GRID where Ho * Wo does not fit the int cell index.
 */
#ifndef CROSSLOC_E2E_H
#define CROSSLOC_E2E_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XL_E2E_STATS 4                     /* doubles per row of `stats` */

int xl_e2e_pose_gradient(const float *g, int64_t gb, int64_t gc, int64_t gy, int64_t gx,   /* [B,3,Ho,Wo], any strides */
                         const double *loss,            /* [B] expected pose losses of the solver */
                         int B, int Ho, int Wo, int C,  /* C >= 3: channels of the network output */
                         float weight, float clip_norm, /* clip_norm <= 0: no clipping */
                         float beta,                    /* 0: `out` is not read */
                         float *out,                    /* [B,C,Ho,Wo] contiguous, written whole */
                         double *stats,                 /* [B+1, 4] */
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif
