// xl_dsac_rgbd.hip — the RGB-D DSAC* pose solver on MI355X (gfx950): Kabsch hypotheses from camera coordinates (depth),
// batched.  Replaces the forward pass of dsacstar_rgbd_forward (dsacstar/dsacstar.cpp:495-612 of the reference project)
// behind xl_dsac_forward_rgbd_batch (include/crossloc_dsac.h, semantics and debug layout there).  The RGB kernels of
// xl_dsac.hip are not involved.  One 256-thread workgroup (4 wavefronts) per image, one launch per batch:
//
//   stage      the cells are walked x-major (x outer, y inner, the order of the reference's validPts) in chunks of 256; a
//              cell is valid iff its camera z is nonzero; ballot + popcount give every valid cell its place in the valid
//              list, and its six floats (camera x y z, scene X Y Z) go to LDS as SoA planes in that order, with the cell
//              index beside them.  In depth form the camera coordinate is formed here (rgbd_cam_from_depth)
//   sample     wavefront w owns hypotheses w, w+4, ...; the 64 lanes evaluate 64 consecutive tries of one hypothesis (three
//              draws from the valid list, Kabsch, three residuals); __ballot picks the lowest accepted try
//              (sampleHypothesesRGBD, dsacstar_util.h:236-307)
//   score      the same wavefront walks the valid list (lanes stride it), distance error, soft-inlier term, xor butterfly;
//              the invalid cells all have the error maxDist and enter as one product (get3DDistErrs + getHypScores,
//              dsacstar_util.h:457-507, 316-343); error maps never leave registers
//   select     first maximum wins, across the 4 wavefronts through LDS
//   refine     all 256 threads: inlier set, two block reductions (centroids, centred cross-covariance), Kabsch redundantly
//              in every thread so control flow stays uniform, while the inlier count grows (refineHypRGBD,
//              dsacstar_util.h:611-677)
//   write      inverse rigid transform as float 4x4 (pose2trans)
//
// LDS: 26 bytes per cell (6 floats + a 16-bit cell index) behind the 1152 bytes of Smem: 141 552 bytes (138 KiB of the CU's
// 160 KiB) at 60 x 90, one workgroup per CU.  Arithmetic contract as in xl_dsac.hip: -ffp-contract=off, fixed reduction order.  What one lane computes
// on its own is in xl_dsac_rgbd_math.h; tests/dsac_rgbd_ref.c compiles the same header with gcc and restates this file's
// orchestration serially, and tests/test_dsac_rgbd_gpu.py compares every output bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>                    // memcpy in the host half of xl_dsac_math.h (bits_f64), as that header asks

#include "../../include/crossloc_dsac.h"
#include "xl_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxCells = XL_DSAC_RGBD_MAX_CELLS;
constexpr size_t kMaxLds = 160 * 1024;

#include "xl_dsac_rgbd_math.h"

struct RgbdParams {
    const float *coords; int64_t sb, sc, sy, sx;
    const float *cam; int64_t mb, mc, my, mx;
    const float *depth; int64_t db, dy, dx;
    float *outPoses;
    const float *focals;
    int32_t *cells; int32_t *tries; double *scores; double *dbg;
    uint64_t seed, image0, imageStride;
    uint32_t maxTries;
    int nHyp, Ho, Wo, sub, Npad;
    float thr, alpha, maxDist, focal, ppx, ppy;
};

struct Smem {
    double red[2][kWaves * XLR_SUMS_COV];
    double bestPose[kWaves][12];
    double pose0[12];
    double bestScore[kWaves];
    int bestIdx[kWaves];
    int anyNan[kWaves];
    unsigned cnt[2][kWaves];
};

static_assert(((sizeof(Smem) + 15) & ~size_t(15)) + (size_t)26 * kMaxCells <= kMaxLds, "the largest grid fits the LDS of a CU");
static_assert(kMaxCells <= 65536 && kMaxCells <= 64 * kThreads, "16-bit cell indices, 64-bit per-thread inlier masks");

// the staged image: planes in valid-list order
struct Cells {
    const float *px, *py, *pz, *X, *Y, *Z;
    __device__ __forceinline__ float err(const Pose &p, int k, float maxDist) const
    {
        return rgbd_cell_err(&p, (double)X[k], (double)Y[k], (double)Z[k], (double)px[k], (double)py[k], (double)pz[k], maxDist);
    }
};

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

__device__ __forceinline__ Pose wave_bcast_pose(const Pose &p, int src)
{
    Pose o;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.R[i] = __shfl(p.R[i], src);
#pragma unroll
    for (int i = 0; i < 3; ++i) o.t[i] = __shfl(p.t[i], src);
    return o;
}

// canonical block sum of K per-thread values: butterfly per wave, waves added in order.  `red` is one of the two LDS buffers
// the caller alternates; one barrier per call.
template <int K>
__device__ __forceinline__ void block_reduce(double (&a)[K], double *red, int wave, int lane)
{
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

__global__ __launch_bounds__(kThreads)
void xl_dsac_rgbd_forward_kernel(RgbdParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Smem &S = *reinterpret_cast<Smem *>(smem_raw);
    float *sF = reinterpret_cast<float *>(smem_raw + ((sizeof(Smem) + 15) & ~size_t(15)));
    unsigned short *sCell = reinterpret_cast<unsigned short *>(sF + 6 * (size_t)P.Npad);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const int N = P.Ho * P.Wo;
    int cntSel = 0;

    // ---- stage: valid list (x-major) and the valid cells' six floats
    int nValid = 0;
    {
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
                if (P.cam) {
                    const float *q = P.cam + (int64_t)b * P.mb + (int64_t)y * P.my + (int64_t)x * P.mx;
                    cx = q[0]; cy = q[P.mc]; cz = q[2 * P.mc];
                } else {
                    const float d = P.depth[(int64_t)b * P.db + (int64_t)y * P.dy + (int64_t)x * P.dx];
                    rgbd_cam_from_depth(d, y, x, f, P.ppx, P.ppy, P.sub, &cx, &cy, &cz);
                }
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
            }
            nValid += (int)(c0 + c1 + c2 + c3);
        }
    }
    __syncthreads();
    const Cells ce{ sF, sF + P.Npad, sF + 2 * P.Npad, sF + 3 * P.Npad, sF + 4 * P.Npad, sF + 5 * P.Npad };

    const uint64_t imageIdx = P.image0 + (uint64_t)b * P.imageStride;
    const uint64_t imageKey = image_key(P.seed, imageIdx);
    const float thr = P.thr, maxDist = P.maxDist;
    const float beta = 5.0f / thr;
    const float fac = P.alpha / (float)P.Wo / (float)P.Ho;
    const double invalidTerm = rgbd_soft_term(maxDist, beta, thr);

    // ---- sample + score: this wave's hypotheses
    double bestScore = 0.0;
    int bestIdx = -1;
    int anyNan = 0;
    for (int h = wave; h < P.nHyp; h += kWaves) {
        Pose pose;
        pose_identity(&pose);
        int k3[3] = { -1, -1, -1 };
        int triesUsed = 0;
        if (nValid > 0)
        for (uint32_t t0 = 0; t0 < P.maxTries; t0 += 64) {
            const uint32_t t = t0 + (uint32_t)lane;
            Pose p;
            int kk[3] = { -1, -1, -1 };
            bool ok = false;
            if (t < P.maxTries) ok = rgbd_sample_try(ce, nValid, thr, imageKey, (uint32_t)h, t, p, kk);
            else pose_identity(&p);
            const unsigned long long m = __ballot(ok);
            int src;
            if (m != 0ull) { src = __ffsll((long long)m) - 1; triesUsed = (int)t0 + src + 1; }
            else if (t0 + 64u >= P.maxTries) { src = (int)(P.maxTries - 1u - t0); triesUsed = -(int)P.maxTries; }
            else continue;
            pose = wave_bcast_pose(p, src);
#pragma unroll
            for (int j = 0; j < 3; ++j) k3[j] = __shfl(kk[j], src);
            break;
        }

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
        const double score = total * (double)fac;

        if (lane == 0) {
            if (P.cells) {
                int32_t *o = P.cells + ((int64_t)b * P.nHyp + h) * 3;
#pragma unroll
                for (int j = 0; j < 3; ++j) o[j] = (k3[j] >= 0) ? (int32_t)sCell[k3[j]] : -1;
            }
            if (P.tries) P.tries[(int64_t)b * P.nHyp + h] = triesUsed;
            if (P.scores) P.scores[(int64_t)b * P.nHyp + h] = score;
        }
        if (score != score) anyNan = 1;
        const bool better = (bestIdx < 0) || (score > bestScore);
        if (h == 0 && lane == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) S.pose0[i] = pose.R[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) S.pose0[9 + i] = pose.t[i];
        }
        if (better) {
            bestScore = score; bestIdx = h;
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 9; ++i) S.bestPose[wave][i] = pose.R[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) S.bestPose[wave][9 + i] = pose.t[i];
            }
        }
    }
    if (lane == 0) { S.bestScore[wave] = bestScore; S.bestIdx[wave] = bestIdx; S.anyNan[wave] = anyNan; }
    __syncthreads();

    // ---- select: first maximum wins; any NaN score makes every soft-max probability NaN and draw() return 0
    int win = -1, winWave = 0, nanAny = 0;
    {
        double ws = 0.0;
        for (int w = 0; w < kWaves; ++w) {
            const double sc = S.bestScore[w];
            const int idx = S.bestIdx[w];
            nanAny |= S.anyNan[w];
            if (idx < 0) continue;
            if (win < 0 || sc > ws || (sc == ws && idx < win)) { win = idx; ws = sc; winWave = w; }
        }
        if (nanAny) win = 0;
    }
    Pose pose;
    {
        const double *src = nanAny ? S.pose0 : S.bestPose[winWave];
#pragma unroll
        for (int i = 0; i < 9; ++i) pose.R[i] = src[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) pose.t[i] = src[9 + i];
    }

    // ---- refine: bit j of `inl` <-> place tid + 256 j of the valid list
    unsigned best = 3, finalInl = 0;
    int rounds = 0, redSel = 0;
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
        block_reduce<XLR_SUMS_CENTROID>(s, S.red[redSel], wave, lane); redSel ^= 1;
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
        block_reduce<XLR_SUMS_COV>(a, S.red[redSel], wave, lane); redSel ^= 1;
        rgbd_kabsch_fit(cp, cX, a, &pose);
        finalInl = cnt;
        ++rounds;
    }

    // ---- write (pose2trans): inverse rigid transform, float row-major
    if (tid == 0) {
        float *o = P.outPoses + (int64_t)b * 16;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) o[4 * i + j] = (float)pose.R[3 * j + i];
            o[4 * i + 3] = (float)(-(pose.R[i] * pose.t[0] + pose.R[3 + i] * pose.t[1] + pose.R[6 + i] * pose.t[2]));
        }
        o[12] = 0.0f; o[13] = 0.0f; o[14] = 0.0f; o[15] = 1.0f;
        if (P.dbg) {
            double *q = P.dbg + (int64_t)b * XL_DSAC_RGBD_DBG_DOUBLES;
            q[0] = (double)win; q[1] = (double)nValid; q[2] = (double)rounds; q[3] = (double)finalInl;
            for (int i = 0; i < 9; ++i) q[4 + i] = pose.R[i];
            for (int i = 0; i < 3; ++i) q[13 + i] = pose.t[i];
        }
    }
}

}  // namespace

extern "C" int xl_dsac_forward_rgbd_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                          const float *cam_dev, int64_t mb, int64_t mc, int64_t my, int64_t mx,
                                          const float *depth_dev, int64_t db, int64_t dy, int64_t dx,
                                          int B, int Ho, int Wo, float *out_poses_dev,
                                          int n_hyp, float thr, float alpha, float max_dist,
                                          float focal, float ppx, float ppy, int sub, const float *focals_dev,
                                          uint64_t seed, uint64_t image0, uint64_t image_stride, uint32_t max_tries,
                                          void *stream,
                                          int32_t *cells_dev, int32_t *tries_dev, double *scores_dev, double *dbg_dev)
{
    if (!coords_dev || !out_poses_dev || (cam_dev == nullptr) == (depth_dev == nullptr) || B <= 0 || Ho <= 0 || Wo <= 0 ||
        n_hyp <= 0 || max_tries == 0 || max_tries > XL_DSAC_RGBD_MAX_TRIES)
        return XL_ERR_ARG;
    if (depth_dev && sub <= 0) return XL_ERR_ARG;
    if ((int64_t)Ho * (int64_t)Wo > (int64_t)kMaxCells) return XL_ERR_GRID;
    const int N = Ho * Wo;
    RgbdParams P;
    P.coords = coords_dev; P.sb = sb; P.sc = sc; P.sy = sy; P.sx = sx;
    P.cam = cam_dev; P.mb = mb; P.mc = mc; P.my = my; P.mx = mx;
    P.depth = depth_dev; P.db = db; P.dy = dy; P.dx = dx;
    P.outPoses = out_poses_dev; P.focals = focals_dev;
    P.cells = cells_dev; P.tries = tries_dev; P.scores = scores_dev; P.dbg = dbg_dev;
    P.seed = seed; P.image0 = image0; P.imageStride = image_stride; P.maxTries = max_tries;
    P.nHyp = n_hyp; P.Ho = Ho; P.Wo = Wo; P.sub = sub; P.Npad = (N + 3) & ~3;
    P.thr = thr; P.alpha = alpha; P.maxDist = max_dist; P.focal = focal; P.ppx = ppx; P.ppy = ppy;

    const size_t lds = ((sizeof(Smem) + 15) & ~size_t(15)) + (size_t)26 * P.Npad;
    if (lds > kMaxLds) return XL_ERR_GRID;
    static XlLdsLimit configured;
    int cfgDev;
    if (configured.needs(lds, &cfgDev)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(xl_dsac_rgbd_forward_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return XL_ERR_HIP;
        configured.done(lds, cfgDev);
    }
    hipLaunchKernelGGL(xl_dsac_rgbd_forward_kernel, dim3(B), dim3(kThreads), lds, (hipStream_t)stream, P);
    return hipGetLastError() == hipSuccess ? XL_OK : XL_ERR_HIP;
}
