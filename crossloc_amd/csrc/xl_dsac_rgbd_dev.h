// xl_dsac_rgbd_dev.h — the pieces of the RGB-D DSAC* solver that the forward kernel (xl_dsac_rgbd.hip), the backward kernels
// (xl_dsac_rgbd_bwd.hip) and the quality pass (xl_dsac_rgbd_quality.hip) share: the input record and its checks (RgbdIn, rgbd_input),
// the LDS view, staging of an image into LDS, the sampling of one hypothesis by a wave, its scoring walk and score constants, and
// the refinement loop of the workgroup.  The order of a block sum is stated in xl_dsac_reduce.h.  Written once; included inside the consumer's anonymous
// namespace after <hip/hip_runtime.h>, crossloc_dsac.h and xl_common.h.  One 256-thread workgroup (4 wavefronts); arithmetic
// contract as in xl_dsac_rgbd_math.h (-ffp-contract=off, fixed reduction order).
#pragma once

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxCells = XL_DSAC_RGBD_MAX_CELLS;
constexpr size_t kMaxLds = 160 * 1024;

#include "xl_dsac_rgbd_bwd_math.h"
#include "xl_dsac_reduce.h"             // block_sum (the canonical order is stated there), wave_bcast_pose

// where an image comes from: scene coordinates, and camera coordinates or depth
struct RgbdIn {
    const float *coords; int64_t sb, sc, sy, sx;
    const float *cam; int64_t mb, mc, my, mx;
    const float *depth; int64_t db, dy, dx;
    const float *focals;
    int Ho, Wo, sub, Npad;
    float focal, ppx, ppy;
};

// RgbdIn from the flat arguments of the C ABI, with the checks every entry point shares.  Npad stays 0: a pass that stages
// sets it once its own grid check has passed.
inline int rgbd_input(RgbdIn &in, const float *coords, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                      const float *cam, int64_t mb, int64_t mc, int64_t my, int64_t mx,
                      const float *depth, int64_t db, int64_t dy, int64_t dx, int B, int Ho, int Wo,
                      float focal, float ppx, float ppy, int sub, const float *focals)
{
    if (!coords || (cam == nullptr) == (depth == nullptr) || B <= 0 || Ho <= 0 || Wo <= 0 || (depth && sub <= 0)) return XL_ERR_ARG;
    in = RgbdIn{ coords, sb, sc, sy, sx, cam, mb, mc, my, mx, depth, db, dy, dx, focals, Ho, Wo, sub, 0, focal, ppx, ppy };
    return XL_OK;
}

struct Smem {
    double red[2][kWaves * XLR_SUMS_COV];
    double bestPose[kWaves][12];
    double pose0[12];
    double bestScore[kWaves];
    int bestIdx[kWaves];
    int anyNan[kWaves];
    unsigned cnt[2][kWaves];
};

constexpr size_t kSmemBytes = (sizeof(Smem) + 15) & ~size_t(15);
static_assert(kSmemBytes + (size_t)26 * kMaxCells <= kMaxLds, "the largest grid fits the LDS of a CU");
static_assert(kMaxCells <= 65536 && kMaxCells <= 64 * kThreads, "16-bit cell indices, 64-bit per-thread inlier masks");

__host__ __device__ inline size_t rgbd_lds_bytes(int Npad) { return kSmemBytes + (size_t)26 * Npad; }

// raises the dynamic LDS limit of `kernels` to `lds` bytes, once per device (`configured`: a static of the entry point)
template <size_t NK>
inline bool rgbd_raise_lds_limit(XlLdsLimit &configured, const void *const (&kernels)[NK], size_t lds)
{
    int dev;
    if (!configured.needs(lds, &dev)) return true;
    for (const void *k : kernels)
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return false;
    configured.done(lds, dev);
    return true;
}

// the staged image: planes in valid-list order
struct Cells {
    const float *px, *py, *pz, *X, *Y, *Z;
    __device__ __forceinline__ float err(const Pose &p, int k, float maxDist) const
    {
        return rgbd_cell_err(&p, (double)X[k], (double)Y[k], (double)Z[k], (double)px[k], (double)py[k], (double)pz[k], maxDist);
    }
};

// the dynamic LDS of a staging kernel: Smem, then the six planes of Npad floats, then the 16-bit cell indices.  A kernel forms
// its Cells from sF itself, after rgbd_stage, and hands rgbd_stage the three pieces: with a helper for the Cells (member,
// constructor, free function) or the view passed whole, hipcc allocated the scalar registers of K0, K1, K3 and of the forward
// kernel differently, and K1 ran 5 % slower
struct Lds { Smem &S; float *sF; unsigned short *sCell; };

__device__ __forceinline__ Lds rgbd_lds_view(unsigned char *smem_raw, int Npad)
{
    float *sF = reinterpret_cast<float *>(smem_raw + kSmemBytes);
    return Lds{ *reinterpret_cast<Smem *>(smem_raw), sF, reinterpret_cast<unsigned short *>(sF + 6 * (size_t)Npad) };
}

// the constants of the soft-inlier score; the term of an invalid cell (error maxDist) is formed by the two kernels that score
struct ScoreConst {
    float beta, fac;
    __device__ __forceinline__ ScoreConst(float thr, float alpha, int Ho, int Wo) : beta(5.0f / thr), fac(alpha / (float)Wo / (float)Ho) {}
    __device__ __forceinline__ double invalid_term(float maxDist, float thr) const { return rgbd_soft_term(maxDist, beta, thr); }
};

// camera coordinate of cell (y, x) of image b, from the camera tensor or from depth
__device__ __forceinline__ void rgbd_load_cam(const RgbdIn &P, int b, float f, int y, int x, float &cx, float &cy, float &cz)
{
    if (P.cam) {
        const float *q = P.cam + (int64_t)b * P.mb + (int64_t)y * P.my + (int64_t)x * P.mx;
        cx = q[0]; cy = q[P.mc]; cz = q[2 * P.mc];
    } else {
        const float d = P.depth[(int64_t)b * P.db + (int64_t)y * P.dy + (int64_t)x * P.dx];
        rgbd_cam_from_depth(d, y, x, f, P.ppx, P.ppy, P.sub, &cx, &cy, &cz);
    }
}

// stage: the valid list (x-major) and the valid cells' six floats as SoA planes in LDS, the cell index beside them.  Returns
// nValid; ends in a barrier.  placeOf (optional, global, [Ho*Wo] of this image): the place of every cell in the valid list, -1
// for an invalid cell.
__device__ __forceinline__ int rgbd_stage(const RgbdIn &P, int b, Smem &S, float *sF, unsigned short *sCell, int &cntSel,
                                          int tid, int lane, int wave, int32_t *placeOf)
{
    const int N = P.Ho * P.Wo;
    int nValid = 0;
    const float f = P.focals ? P.focals[b] : P.focal;
    const float *gCo = P.coords + (int64_t)b * P.sb;
    // (x-major: neighbouring threads read addresses a row apart, so these loads do not coalesce - once per image and cell)
    for (int j0 = 0; j0 < N; j0 += kThreads) {
        const int j = j0 + tid;
        bool valid = false;
        float cx = 0.0f, cy = 0.0f, cz = 0.0f;
        int x = 0, y = 0;
        if (j < N) {
            x = j / P.Ho; y = j - x * P.Ho;
            rgbd_load_cam(P, b, f, y, x, cx, cy, cz);
            valid = cz != 0.0f;
        }
        const unsigned long long m = __ballot(valid);
        if (lane == 0) S.cnt[cntSel][wave] = (unsigned)__popcll(m);
        __syncthreads();
        const unsigned c0 = S.cnt[cntSel][0], c1 = S.cnt[cntSel][1], c2 = S.cnt[cntSel][2], c3 = S.cnt[cntSel][3];
        cntSel ^= 1;
        if (valid) {
            const unsigned before = (wave > 0 ? c0 : 0u) + (wave > 1 ? c1 : 0u) + (wave > 2 ? c2 : 0u);
            const int k = nValid + (int)before + __popcll(m & ((1ull << lane) - 1ull));      // k < nValid + c0..c3 <= N
            const float *q = gCo + (int64_t)y * P.sy + (int64_t)x * P.sx;
            sF[k] = cx;
            sF[P.Npad + k] = cy;
            sF[2 * P.Npad + k] = cz;
            sF[3 * P.Npad + k] = q[0];
            sF[4 * P.Npad + k] = q[P.sc];
            sF[5 * P.Npad + k] = q[2 * P.sc];
            sCell[k] = (unsigned short)(y * P.Wo + x);
            if (placeOf) placeOf[y * P.Wo + x] = k;
        } else if (placeOf && j < N) {
            placeOf[y * P.Wo + x] = -1;
        }
        nValid += (int)(c0 + c1 + c2 + c3);
    }
    __syncthreads();
    return nValid;
}

// one sampling try: returns the accept flag, pose = the fit, ks = the three draws (places in the valid list)
__device__ bool rgbd_sample_try(const Cells &ce, int nValid, float thr, uint64_t imageKey, uint32_t hyp, uint32_t t,
                                Pose &pose, int (&ks)[3])
{
    const uint64_t st = try_state(imageKey, hyp, t);
    double pc[9], Xw[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int k = draw(st, j, nValid);
        ks[j] = k;
        pc[3 * j] = (double)ce.px[k]; pc[3 * j + 1] = (double)ce.py[k]; pc[3 * j + 2] = (double)ce.pz[k];
        Xw[3 * j] = (double)ce.X[k];  Xw[3 * j + 1] = (double)ce.Y[k];  Xw[3 * j + 2] = (double)ce.Z[k];
    }
    return rgbd_try_fit(pc, Xw, thr, &pose);
}

// sampling of hypothesis h by one wave: the 64 lanes evaluate 64 consecutive tries, __ballot picks the lowest accepted one.
// Returns the tries used (negative: budget exhausted, the last try's fit is kept; 0: nothing sampled, identity pose, k3 = -1).
__device__ __forceinline__ int rgbd_sample_hyp(const Cells &ce, int nValid, float thr, uint64_t imageKey, int h, uint32_t maxTries,
                                               int lane, Pose &pose, int (&k3)[3])
{
    pose_identity(&pose);
    k3[0] = -1; k3[1] = -1; k3[2] = -1;
    int triesUsed = 0;
    if (nValid > 0)
    for (uint32_t t0 = 0; t0 < maxTries; t0 += 64) {
        const uint32_t t = t0 + (uint32_t)lane;
        Pose p;
        int kk[3] = { -1, -1, -1 };
        bool ok = false;
        if (t < maxTries) ok = rgbd_sample_try(ce, nValid, thr, imageKey, (uint32_t)h, t, p, kk);
        else pose_identity(&p);
        const unsigned long long m = __ballot(ok);
        int src;
        if (m != 0ull) { src = __ffsll((long long)m) - 1; triesUsed = (int)t0 + src + 1; }
        else if (t0 + 64u >= maxTries) { src = (int)(maxTries - 1u - t0); triesUsed = -(int)maxTries; }
        else continue;
        pose = wave_bcast_pose(p, src);
#pragma unroll
        for (int j = 0; j < 3; ++j) k3[j] = __shfl(kk[j], src);
        break;
    }
    return triesUsed;
}

// soft-inlier score of a pose by one wave (lanes stride the valid list, xor butterfly; the invalid cells enter as one product)
__device__ __forceinline__ double rgbd_score_hyp(const Cells &ce, int nValid, int N, const Pose &pose, float maxDist, float thr,
                                                 const ScoreConst &sc, double invalidTerm, int lane)
{
    const float beta = sc.beta;
    // four cells per lane and trip, added in the order of the one-cell loop: the same bits, four dependent chains (distance,
    // sqrt, exp, divide) in flight - the kernel runs at one wave per SIMD and is bound by their latency
    double acc = 0.0;
    int k = lane;
    for (; k + 192 < nValid; k += 256) {
        const float e0 = ce.err(pose, k, maxDist), e1 = ce.err(pose, k + 64, maxDist);
        const float e2 = ce.err(pose, k + 128, maxDist), e3 = ce.err(pose, k + 192, maxDist);
        const double s0 = rgbd_soft_term(e0, beta, thr), s1 = rgbd_soft_term(e1, beta, thr);
        const double s2 = rgbd_soft_term(e2, beta, thr), s3 = rgbd_soft_term(e3, beta, thr);
        acc += s0;
        acc += s1;
        acc += s2;
        acc += s3;
    }
    for (; k < nValid; k += 64) acc += rgbd_soft_term(ce.err(pose, k, maxDist), beta, thr);
    double total = wave_butterfly(acc);
    total = total + (double)(N - nValid) * invalidTerm;
    return total * (double)sc.fac;
}

// what the refinement leaves behind besides the pose.  inl, cp, cX, a: the inlier set of the last FITTED round (bit j of `inl`
// <-> place tid + 256 j of the valid list), its centroids and centred cross-covariance - the inputs of the fit that gave the pose
struct RefineOut {
    unsigned long long inl;
    unsigned finalInl;
    int rounds;
    double cp[3], cX[3], a[XLR_SUMS_COV];
};

// refine: all 256 threads: inlier set, two block reductions (centroids, centred cross-covariance), Kabsch redundantly in every
// thread so control flow stays uniform, while the inlier count grows (refineHypRGBD, dsacstar_util.h:611-677)
__device__ __forceinline__ void rgbd_refine(const Cells &ce, int nValid, float thr, float maxDist, Smem &S, int &cntSel, int &redSel,
                                            int tid, int wave, int lane, Pose &pose, RefineOut &ro)
{
    unsigned best = 3;
    ro.inl = 0ull; ro.finalInl = 0; ro.rounds = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) { ro.cp[i] = 0.0; ro.cX[i] = 0.0; }
#pragma unroll
    for (int i = 0; i < XLR_SUMS_COV; ++i) ro.a[i] = 0.0;
    for (int step = 0; step < XL_DSAC_MAX_REF_STEPS; ++step) {
        unsigned long long inl = 0ull;
        {
            int j = 0;
            for (int k = tid; k < nValid; k += kThreads, ++j)
                if (ce.err(pose, k, maxDist) < thr) inl |= (1ull << j);
        }
        unsigned cnt = (unsigned)__popcll(inl);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cnt += (unsigned)__shfl_xor((int)cnt, off);
        if (lane == 0) S.cnt[cntSel][wave] = cnt;
        __syncthreads();
        cnt = S.cnt[cntSel][0] + S.cnt[cntSel][1] + S.cnt[cntSel][2] + S.cnt[cntSel][3];
        cntSel ^= 1;
        if (cnt <= best) break;
        best = cnt;

        double s[XLR_SUMS_CENTROID], a[XLR_SUMS_COV], cp[3], cX[3];
#pragma unroll
        for (int i = 0; i < XLR_SUMS_CENTROID; ++i) s[i] = 0.0;
        {
            int j = 0;
            for (int k = tid; k < nValid; k += kThreads, ++j)
                if ((inl >> j) & 1ull)
                    rgbd_acc_centroid(s, (double)ce.px[k], (double)ce.py[k], (double)ce.pz[k],
                                      (double)ce.X[k], (double)ce.Y[k], (double)ce.Z[k]);
        }
        block_sum(s, S.red[redSel], wave, lane); redSel ^= 1;
        rgbd_centroids(s, cp, cX);
#pragma unroll
        for (int i = 0; i < XLR_SUMS_COV; ++i) a[i] = 0.0;
        {
            int j = 0;
            for (int k = tid; k < nValid; k += kThreads, ++j)
                if ((inl >> j) & 1ull)
                    rgbd_acc_cov(a, cp, cX, (double)ce.px[k], (double)ce.py[k], (double)ce.pz[k],
                                 (double)ce.X[k], (double)ce.Y[k], (double)ce.Z[k]);
        }
        block_sum(a, S.red[redSel], wave, lane); redSel ^= 1;
        rgbd_kabsch_fit(cp, cX, a, &pose);
        ro.finalInl = cnt;
        ++ro.rounds;
        ro.inl = inl;
#pragma unroll
        for (int i = 0; i < 3; ++i) { ro.cp[i] = cp[i]; ro.cX[i] = cX[i]; }
#pragma unroll
        for (int i = 0; i < XLR_SUMS_COV; ++i) ro.a[i] = a[i];
    }
}
