/*
 * xl_dsac_reduce.h — the canonical block sum of the DSAC* solver family, written once.
 *
 * THE ORDER.  A workgroup is 256 threads: 4 wavefronts of 64 lanes; thread t is lane t % 64 of wave t / 64.  A value per
 * thread is summed in two steps.  (1) Per wave, an xor butterfly: for off = 32, 16, 8, 4, 2, 1 every lane replaces its value
 * v by v + (the value of lane ^ off); after the six steps all 64 lanes hold the same bits.  (2) The four wave sums are added
 * in the order ((w0 + w1) + w2) + w3.  Every bit-exactness claim of xl_dsac.hip, xl_dsac_quality.hip, xl_dsac_rgbd*.hip and
 * of their CPU restatements rests on this order; it is stated here and nowhere else.
 *
 * Device half (hipcc): included inside the consumer's anonymous namespace after xl_common.h (wave_butterfly), xl_dsac_math.h
 * (Pose) and the consumer's kWaves.  Plain-C half (gcc): the serial model for oracle/ and tests/, which compile with
 * -I crossloc_amd/csrc.
 */
#ifndef XL_DSAC_REDUCE_H
#define XL_DSAC_REDUCE_H

#if defined(__HIPCC__)

// Sums a[k] over the workgroup in place, K values at once; every thread gets the totals.  `red` is LDS the caller does not
// touch until its next barrier (the callers alternate two buffers); exactly one barrier per call.
template <int K, int CAP>
__device__ __forceinline__ void block_sum(double (&a)[K], double (&red)[CAP], int wave, int lane)
{
    static_assert(kWaves * K <= CAP, "the LDS buffer holds K sums of every wave");
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double v = wave_butterfly(a[k]);
        if (lane == 0) red[wave * K + k] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double tot = red[k];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) tot = tot + red[w * K + k];
        a[k] = tot;
    }
}

// lane `src`'s pose in every lane of the wave
__device__ __forceinline__ Pose wave_bcast_pose(const Pose &p, int src)
{
    Pose o;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.R[i] = __shfl(p.R[i], src);
#pragma unroll
    for (int i = 0; i < 3; ++i) o.t[i] = __shfl(p.t[i], src);
    return o;
}

#else

#include <string.h>

#define XL_BLOCK_THREADS 256          /* 4 waves of 64 */

/* step (1) on the 64 values of one wave; p is overwritten, every element ends as the wave's sum, which is returned */
static double butterfly64(double p[64])
{
    double q[64];
    for (int off = 32; off >= 1; off >>= 1) {
        for (int l = 0; l < 64; ++l) q[l] = p[l] + p[l ^ off];
        memcpy(p, q, sizeof(q));
    }
    return p[0];
}

/* steps (1) and (2) on K values per virtual thread: part is [XL_BLOCK_THREADS][K], out [K] */
static void block_sum(const double *part, int K, double *out)
{
    for (int k = 0; k < K; ++k) {
        double tot = 0.0;
        for (int w = 0; w < XL_BLOCK_THREADS / 64; ++w) {
            double p[64];
            for (int l = 0; l < 64; ++l) p[l] = part[(w * 64 + l) * K + k];
            const double ws = butterfly64(p);
            tot = (w == 0) ? ws : tot + ws;
        }
        out[k] = tot;
    }
}

#endif
#endif  /* XL_DSAC_REDUCE_H */
