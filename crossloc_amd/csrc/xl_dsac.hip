// xl_dsac.hip — MI355X (gfx950) kernel bundle for CrossLoc's DSAC* pose solver.
//
// Replaces dsacstar_rgb_forward (/root/reference/dsacstar/dsacstar.cpp:63-178) behind the C ABI of
// include/crossloc_dsac.h.  One 256-thread workgroup (4 wavefronts) per image, everything in one launch (large
// batches), or — when the batch alone cannot fill 256 CUs — the sample/score phase spread over S workgroups per
// image followed by a select/refine launch (xl_dsac_forward_kernel<1>, <2>); both forms give identical bits:
//
//   stage      scene coordinates -> LDS as SoA planes (64.8 KB for 60x90), read by every later phase
//   sample     wavefront w owns hypotheses w, w+4, ...; the 64 lanes evaluate 64 consecutive tries of
//              one hypothesis in parallel (counter-based RNG keyed by try index, one P3P per lane);
//              __ballot picks the lowest accepted try = the reference's "first accepted try"
//              (sampleHypotheses, dsacstar_util.h:135-221)
//   score      the same wavefront projects all cells through the accepted pose (lanes stride the
//              cells), soft-inlier sigmoid, xor-butterfly reduction (getReproErrs + getHypScores,
//              dsacstar_util.h:316-343, 356-446); error maps never leave registers
//   select     argmax with first-maximum-wins across the 4 wavefronts through LDS (softMax/draw,
//              dsacstar_util.h:684-752)
//   refine     all 256 threads: inlier set, Levenberg-Marquardt PnP on the inliers (28 wave-reduced
//              sums per evaluation, 6x6 Cholesky redundantly in every thread so control flow stays
//              uniform without broadcasts), repeat while the inlier count grows (refineHyp,
//              dsacstar_util.h:522-597)
//   write      inverse rigid transform as float 4x4 (pose2trans, dsacstar_util.h:759-770)
//
// Arithmetic contract: compiled with -ffp-contract=off; every transcendental is a fixed polynomial in
// + - * / sqrt; reductions use a fixed order.  What one lane computes on its own lives in xl_dsac_math.h, which the CPU oracle
// compiles too: the polynomials, the RNG, the camera record (cam_make) and the pixel centre of a cell (cell_px), projection, cell
// error and the soft-inlier sigmoid (soft_inlier_st), quartic, P3P, the per-cell normal equations (XL_PNP_CELL_ROWS, pnp_cell_normal_eq), the
// Cholesky step, the LM stop rule and its constants (lm_step_small, XLM_LM_MAX_ITER), the not-NaN test of an LM result
// (pose_not_nan), the pose forms (pose_load12 / pose_store12, pose_to_c2w16) and the backward pass's derivatives.  This file
// keeps what is parallel: LDS staging (stage_coords), ballots, wave and block reductions, the LM state machine, the kernels and
// the host entry points.  The order of a block sum is stated in xl_dsac_reduce.h (block_sum).  tests/test_dsac_gpu.py checks
// sampled cells, tries, scores, winner and refined pose against oracle/dsac_oracle.c bit for bit - a check of that parallel part
// and of gcc == hipcc, not of the shared formulas (those: tests/indep_dsac.py and tests/test_oracle_dsac_pin.py).  The oracle
// includes the header; nothing here includes the oracle.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/crossloc_dsac.h"
#include "xl_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxCellsPerThread = 64;
constexpr int kMaxCells = kThreads * kMaxCellsPerThread;     // 16384

// Pose, Cam, V3 and every function one lane evaluates on its own (listed at the top): shared with the CPU oracle, written once
#include "xl_dsac_math.h"
#include "xl_dsac_reduce.h"             // the canonical block sum (block_sum: the order is stated there) and wave_bcast_pose

// scene coordinates of the image: SoA planes in LDS (cell i = y * Wo + x)
struct Coords {
    const float *sx, *sy, *sz;
    __device__ __forceinline__ void fetch(int i, double &X, double &Y, double &Z) const
    {
        X = (double)sx[i]; Y = (double)sy[i]; Z = (double)sz[i];
    }
    // clamped reprojection error of cell i, whose row / column the caller divides out or carries along (CellWalk)
    __device__ __forceinline__ float err(const Pose &p, int i, int y, int x, const Cam &cam) const
    {
        double X, Y, Z;
        fetch(i, X, Y, Z);
        return cell_err(&p, X, Y, Z, y, x, &cam);
    }
    __device__ __forceinline__ float err(const Pose &p, int i, const Cam &cam) const
    {
        int y = i / cam.Wo, x = i - y * cam.Wo;
        return err(p, i, y, x, cam);
    }
};

// validity mask of the image (masked solver): a bit plane in LDS beside the coordinate planes, bit i & 31 of word i >> 5 <-> cell i
struct MaskBits {
    const uint32_t *w;
    __device__ __forceinline__ bool usable(int i) const { return (w[i >> 5] >> (i & 31)) & 1u; }
    // thread tid's slice of the mask in the layout of an inlier word (RefineOut::inlAcc): bit j <-> cell tid + 256 j
    __device__ __forceinline__ unsigned long long slice(int tid, int N) const
    {
        unsigned long long u = 0ull;
        int j = 0;
        for (int i = tid; i < N; i += kThreads, ++j) if (usable(i)) u |= (1ull << j);
        return u;
    }
};

// row / column of a cell index that advances by a constant stride: one division at the start, then adds and compares (an integer
// division by the run-time grid width is ~25 of a cell's ~160 instructions in the scoring loop)
struct CellWalk {
    int y, x, sy, sx, Wo;
    __device__ __forceinline__ CellWalk(int i0, int stride, int wo) : y(i0 / wo), x(i0 - (i0 / wo) * wo), sy(stride / wo), sx(stride - (stride / wo) * wo), Wo(wo) {}
    __device__ __forceinline__ void step() { y += sy; x += sx; if (x >= Wo) { x -= Wo; ++y; } }
};

// scene coordinates of one image (g: its first element; sc, sy, sx: the caller's strides) -> LDS as three planes of Npad floats;
// serves the forward kernel and the backward kernels, whose parameter records differ
__device__ __forceinline__ void stage_coords(const float *g, int64_t sc, int64_t sy, int64_t sx, int Wo, int N, int Npad, float *sCo, int tid)
{
    for (int i = tid; i < N; i += kThreads) {
        int y = i / Wo, x = i - y * Wo;
        const float *q = g + (int64_t)y * sy + (int64_t)x * sx;
        sCo[i] = q[0];
        sCo[Npad + i] = q[sc];
        sCo[2 * Npad + i] = q[2 * sc];
    }
}

// validity mask of one image (gm: its N bytes, nonzero = usable) -> LDS as a bit plane of ceil(N / 32) words: each wave ballots 64
// consecutive cells into two words.  Returns the usable cells this wave counted (the same in all of its lanes); the caller adds
// the four up after its barrier.  Serves the forward kernel and the backward kernels K1 and K3.
__device__ __forceinline__ int stage_mask(const uint8_t *gm, int N, uint32_t *sMask, int wave, int lane)
{
    const int nWords = (N + 31) >> 5;
    int cnt = 0;
    for (int base = wave * 64; base < N; base += kThreads) {
        const int i = base + lane;
        const bool u = (i < N) && gm[i] != 0;
        const unsigned long long m = __ballot(u);
        cnt += __popcll(m);
        if (lane == 0) {
            sMask[base >> 5] = (uint32_t)m;
            if ((base >> 5) + 1 < nWords) sMask[(base >> 5) + 1] = (uint32_t)(m >> 32);
        }
    }
    return cnt;
}

// the mask mode of the forward kernel: the unmasked solver, and the masked solver behind either sampler (XL_DSAC_SAMPLER_*)
constexpr int kMaskNone = 0, kMaskReject = 1, kMaskCompact = 2;

// rank plane of the mask (compact sampler): nWords + 1 words in LDS behind the bit plane, rank[w] = usable cells in words
// 0 .. w-1 (mask_rank_plane of xl_dsac_math.h).  Thread t owns words 2t and 2t+1, so a wave owns 128 consecutive words: it sums
// the words of the waves before it (at most three pairs per lane and one butterfly) and scans its own, which needs no exchange
// between waves and one barrier after the writes.  nUsable is the workgroup's count from stage_mask (= rank[nWords]).  Call after
// the barrier that follows stage_mask.
__device__ __forceinline__ void build_rank_plane(const uint32_t *sMask, uint32_t *sRank, int nWords, int nUsable, int wave, int lane)
{
    auto pair = [&](int w2, int &c0, int &c1) {
        c0 = (w2 < nWords) ? __popc(sMask[w2]) : 0;
        c1 = (w2 + 1 < nWords) ? __popc(sMask[w2 + 1]) : 0;
    };
    int before = 0;
    for (int v = 0; v < wave; ++v) {
        int c0, c1;
        pair(2 * (v * 64 + lane), c0, c1);
        before += c0 + c1;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) before += __shfl_xor(before, off);
    const int w2 = 2 * (wave * 64 + lane);
    int c0, c1;
    pair(w2, c0, c1);
    int incl = c0 + c1;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    const int excl = before + incl - (c0 + c1);
    if (w2 < nWords) sRank[w2] = (uint32_t)excl;
    if (w2 + 1 < nWords) sRank[w2 + 1] = (uint32_t)(excl + c0);
    if (wave == 0 && lane == 0) sRank[nWords] = (uint32_t)nUsable;     // (512 words at the largest grid: past the last pair)
}

// one sampling try (dsacstar_util.h:159-219); returns accept flag, pose = try result (identity if P3P failed)
// kMaskReject: the same four draws; a try that drew a masked-out cell is rejected before P3P (identity pose, like a failed P3P)
// and the coordinates of such a cell are never read
// kMaskCompact: four draws of a rank among the usable cells (compact_try_cells: LDS reads only); no try is rejected by the mask
template <int MASK>
__device__ bool sample_try(const Coords &co, const MaskBits &mb, const Cam &cam, uint64_t imageKey, uint32_t hyp, uint32_t t,
                           Pose &pose, int (&cells)[4])
{
    constexpr bool REJECT = MASK == kMaskReject;
    uint64_t st = try_state(imageKey, hyp, t);
    V3 P[4];
    double uv[4][2];
    float px[4], py[4];
    if constexpr (MASK == kMaskCompact) compact_try_cells(st, mb.w, mb.w + ((cam.N + 31) >> 5), (cam.N + 31) >> 5, cells);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int x, y;
        if constexpr (MASK == kMaskCompact) {
            y = cells[j] / cam.Wo; x = cells[j] - y * cam.Wo;
        } else {
            x = draw(st, 2 * j, cam.Wo);
            y = draw(st, 2 * j + 1, cam.Ho);
            cells[j] = y * cam.Wo + x;
        }
        px[j] = cell_px(&cam, x);
        py[j] = cell_px(&cam, y);
        uv[j][0] = (double)px[j]; uv[j][1] = (double)py[j];
        if constexpr (!REJECT) co.fetch(cells[j], P[j].x, P[j].y, P[j].z);
    }
    if constexpr (REJECT) {
        if (!(mb.usable(cells[0]) && mb.usable(cells[1]) && mb.usable(cells[2]) && mb.usable(cells[3]))) {
            pose_identity(&pose);
            return false;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) co.fetch(cells[j], P[j].x, P[j].y, P[j].z);
    }
    if (!p3p(P[0], P[1], P[2], P[3], uv, &cam, &pose)) {
        pose_identity(&pose);
        return false;
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float u, v;
        project(&pose, P[j].x, P[j].y, P[j].z, &cam, &u, &v);
        float dx = px[j] - u, dy = py[j] - v;
        double n = sqrt((double)dx * (double)dx + (double)dy * (double)dy);
        if (ok && !(n < (double)cam.thr)) ok = false;
    }
    return ok;
}

// ------------------------------------------------------------------------------ LM pieces

// per-thread accumulation of the normal equations over this thread's inlier cells.  The rows are the shared statement
// (XL_PNP_CELL_ROWS of xl_dsac_math.h); the six lines that add them up restate pnp_cell_normal_eq here instead of calling it: with the
// call (force-inlined) hipcc schedules refine_pose differently at equal register figures and the single-frame solve ran 0.2562-0.2565 ms
// against the parent's 0.2532-0.2540 (+1.25 %, 95 frames +0.15 %: both outside the run-to-run range); expanded here it is at the
// hand-written loop's time (profiles/rgb_solver_shared_math.txt)
__device__ __forceinline__ void normal_eq_thread(const Coords &co, const Cam &camRef, const Pose &pose,
                                                 unsigned long long inl, int tid, double (&a)[28])
{
    const Cam *cam = &camRef;
    const Pose *p = &pose;
#pragma unroll
    for (int k = 0; k < 28; ++k) a[k] = 0.0;
    int j = 0;
    for (int i = tid; i < cam->N; i += kThreads, ++j) {
        if (!((inl >> j) & 1ull)) continue;
        int y = i / cam->Wo, x = i - y * cam->Wo;
        double X, Y, Z;
        co.fetch(i, X, Y, Z);
        XL_PNP_CELL_ROWS
        int k = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) { a[k] += Ju[r] * Ju[c] + Jv[r] * Jv[c]; ++k; }
#pragma unroll
        for (int r = 0; r < 6; ++r) a[21 + r] += Ju[r] * ru + Jv[r] * rv;
        a[27] += ru * ru + rv * rv;
    }
}

struct Params {
    const float *coords; int64_t sb, sc, sy, sx;
    float *outPoses;
    const float *focals;
    int32_t *cells; int32_t *tries; double *scores; double *dbg;
    double *hypPoses;             // optional [B][nHyp][12]: every hypothesis' pose (backward_rgb)
    uint64_t seed, image0, imageStride;
    uint32_t maxTries;
    int nHyp, Ho, Wo, sub, Npad;
    double *part;                 // split launch: [B][S*4][16] per-wave bests + [B][12] pose of hypothesis 0
    int S;                        // sub-blocks per image in the split launch
    float thr, focal, ppx, ppy, alpha, maxReproj;
    int pairCells;                // scoring loop: two cells per lane and trip (same bits, more instruction-level parallelism)
    int cellWalk;                 // scoring loop: row / column carried along instead of divided out (XL_DSAC_CELL_WALK=0: divide)
    const uint8_t *mask;          // masked solver: [B][Ho*Wo], nonzero = usable cell
    int32_t *status;              // masked solver, optional: [B], 1 = fewer than four usable cells (identity pose written)
};

// LDS carve (all dynamic, 16-byte aligned pieces)
struct Smem {
    double red[2][kWaves * 28];
    double bestPose[kWaves][12];
    double pose0[12];
    double bestScore[kWaves];
    int bestIdx[kWaves];
    int anyNan[kWaves];
    unsigned cnt[2][kWaves];
    int pad[4];                   // masked solver: the usable cells each wave counted while staging the mask
};

// refineHyp (dsacstar_util.h:522-597), cooperative over the 256 threads of the workgroup: the pose is refined in
// place; o.inlAcc is this thread's slice (bit j <-> cell tid + 256 j) of the inlier map of the last successful
// re-fit, o.finalInl its size.  redSel / cntSel select the double-buffered LDS reduction scratch.
// MASKED: `usable` is this thread's slice of the validity mask in the layout of inlAcc; a cell is an inlier iff it is usable and
// its error is below the threshold.
struct RefineOut { unsigned long long inlAcc; unsigned finalInl; int rounds, evals; };

template <bool MASKED = false>
__device__ __forceinline__ void refine_pose(const Coords &co, const Cam &cam, Smem &S, int tid, int wave, int lane,
                                            Pose &pose, RefineOut &o, int &redSel, int &cntSel, unsigned long long usable = ~0ull)
{
    const int N = cam.N;
    unsigned long long inlAcc = 0ull;
    unsigned best = 4;
    int rounds = 0, evals = 0;
    unsigned finalInl = 0;
    for (int step = 0; step < XL_DSAC_MAX_REF_STEPS; ++step) {
        unsigned long long inl = 0ull;
        {
            int j = 0;
            for (int i = tid; i < N; i += kThreads, ++j) {
                float e = co.err(pose, i, cam);
                if (e < cam.thr) inl |= (1ull << j);
            }
        }
        if constexpr (MASKED) inl &= usable;
        unsigned cnt = (unsigned)__popcll(inl);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cnt += (unsigned)__shfl_xor((int)cnt, off);
        if (lane == 0) S.cnt[cntSel][wave] = cnt;
        __syncthreads();
        cnt = S.cnt[cntSel][0] + S.cnt[cntSel][1] + S.cnt[cntSel][2] + S.cnt[cntSel][3];
        cntSel ^= 1;
        if (cnt <= best) break;
        best = cnt;

        // Levenberg-Marquardt on the inliers (cv::solvePnP ITERATIVE + extrinsic guess)
        Pose cur = pose, prev;
        double ne[28], neNew[28];
        int lg = -3, iters = 0;
        bool failed = false;
        normal_eq_thread(co, cam, cur, inl, tid, ne);
        block_sum(ne, S.red[redSel], wave, lane); redSel ^= 1; ++evals;
        for (;;) {
            double d[6];
            prev = cur;
            if (!solve6(ne, lambda_of(lg), d)) { failed = true; break; }
            apply_step(&prev, d, &cur);
            double prevErr = ne[27];
            normal_eq_thread(co, cam, cur, inl, tid, neNew);
            block_sum(neNew, S.red[redSel], wave, lane); redSel ^= 1; ++evals;
            while (neNew[27] > prevErr) {
                if (++lg <= 16) {
                    if (!solve6(ne, lambda_of(lg), d)) { failed = true; break; }
                    apply_step(&prev, d, &cur);
                    normal_eq_thread(co, cam, cur, inl, tid, neNew);
                    block_sum(neNew, S.red[redSel], wave, lane); redSel ^= 1; ++evals;
                } else break;
            }
            if (failed) break;
            lg = (lg - 1 > -16) ? lg - 1 : -16;
            ++iters;
            if (iters >= XLM_LM_MAX_ITER || lm_step_small(d, &prev)) break;
#pragma unroll
            for (int k = 0; k < 28; ++k) ne[k] = neNew[k];
        }
        if (failed || !pose_not_nan(&cur)) break;              // the solver's test is x == x: an infinite entry passes
        pose = cur;
        finalInl = cnt;
        inlAcc = inl;
        ++rounds;
    }

    o.inlAcc = inlAcc; o.finalInl = finalInl; o.rounds = rounds; o.evals = evals;
}

// PHASE 0: whole pipeline, one workgroup per image (enough images to fill the chip).
// PHASE 1: sample + score only, S workgroups per image (grid S x B); per-wave bests go to P.part.
// PHASE 2: select over the S*4 per-wave bests + refine + write, one workgroup per image.
// The split (1 then 2) exists for small batches: with B < ~100 images the fused kernel leaves most CUs idle and
// its latency is the 64 hypotheses each wavefront walks through.  Results are identical in both forms.
// MASKED (xl_dsac_forward_rgb_masked_batch): the same pipeline over the cells P.mask admits.  The mask is staged as a bit plane
// behind the coordinate planes and its usable cells are counted; a try that drew a masked-out cell is rejected before P3P; the
// score sums the usable cells only (a masked cell's term is selected away, so whatever is stored there reaches neither the sum
// nor the NaN flag); an inlier is a usable cell below the threshold.  An image with fewer than four usable cells is dead: the
// try loop is not entered, the identity pose and status 1 are written (the branch is uniform over the workgroup, and over the
// workgroups of an image in the split form: each of them counts the same mask).  With an all-ones mask every output is the
// unmasked kernel's, bit for bit.  That is MASK = kMaskReject.
// MASK = kMaskCompact (xl_dsac_forward_rgb_masked_sampled_batch, XL_DSAC_SAMPLER_COMPACT): the same, except that a try draws four
// ranks among the usable cells and selects their cells through a rank plane kept behind the bit plane (build_rank_plane, one
// more barrier; each workgroup of an image builds the same plane), so the mask rejects no try.  Score, select, refine, the dead
// image and the NaN rule are the masked solver's.  An all-ones mask does not reproduce the unmasked kernel's draws.
template <int PHASE, int MASK = kMaskNone>
__global__ __launch_bounds__(kThreads, PHASE == 1 ? 2 : 1)     // (sample + score: LDS allows two workgroups per CU, 256 registers per wave)
void xl_dsac_forward_kernel(Params P)
{
    constexpr bool MASKED = MASK != kMaskNone;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Smem &S = *reinterpret_cast<Smem *>(smem_raw);
    float *sCo = reinterpret_cast<float *>(smem_raw + ((sizeof(Smem) + 15) & ~size_t(15)));

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = (PHASE == 1) ? blockIdx.y : blockIdx.x;
    const int sub = (PHASE == 1) ? blockIdx.x : 0;
    const int nSub = (PHASE == 1) ? P.S : 1;
    const int N = P.Ho * P.Wo;

    const Cam cam = cam_make(P.Ho, P.Wo, P.thr, P.focals ? P.focals[b] : P.focal, P.ppx, P.ppy, P.alpha, P.maxReproj, P.sub);

    stage_coords(P.coords + (int64_t)b * P.sb, P.sc, P.sy, P.sx, P.Wo, N, P.Npad, sCo, tid);
    // ---- masked: the mask as a bit plane (each wave ballots 64 consecutive cells into two words), usable cells counted per wave
    uint32_t *sMask = reinterpret_cast<uint32_t *>(sCo + 3 * P.Npad);
    if constexpr (MASKED) {
        const int cnt = stage_mask(P.mask + (int64_t)b * N, N, sMask, wave, lane);
        if (lane == 0) S.pad[wave] = cnt;
    }
    __syncthreads();
    Coords co{ sCo, sCo + P.Npad, sCo + 2 * P.Npad };
    MaskBits mb{ sMask };
    unsigned long long usable = ~0ull;                              // this thread's slice of the mask: bit j <-> cell tid + 256 j
    if constexpr (MASKED) {
        const int nUsable = S.pad[0] + S.pad[1] + S.pad[2] + S.pad[3];
        if (nUsable < 4) {
            // dead image (the same decision in every thread of every workgroup of this image): nothing is sampled
            if (PHASE != 2 && sub == 0)
                for (int h = tid; h < P.nHyp; h += kThreads) {
                    if (P.cells) {
                        int32_t *o = P.cells + ((int64_t)b * P.nHyp + h) * 4;
                        o[0] = -1; o[1] = -1; o[2] = -1; o[3] = -1;
                    }
                    if (P.tries) P.tries[(int64_t)b * P.nHyp + h] = 0;
                    if (P.scores) P.scores[(int64_t)b * P.nHyp + h] = 0.0;
                }
            if (PHASE != 1 && tid == 0) {
                float *o = P.outPoses + (int64_t)b * 16;
#pragma unroll
                for (int i = 0; i < 16; ++i) o[i] = (i % 5 == 0) ? 1.0f : 0.0f;     // not pose_to_c2w16 of the identity: its translation column is -0.0f
                if (P.status) P.status[b] = 1;
                if (P.dbg) {
                    double *q = P.dbg + (int64_t)b * XL_DSAC_DBG_DOUBLES;
                    q[0] = -1.0; q[1] = 0.0; q[2] = 0.0; q[3] = 0.0;
                    Pose id;
                    pose_identity(&id);
                    pose_store12(&id, q + 4);
                    pose_store12(&id, q + 16);
                }
            }
            return;
        }
        if constexpr (MASK == kMaskCompact) {
            // the rank plane behind the bit plane (every workgroup of the image builds the same one); PHASE 2 samples nothing
            if (PHASE != 2) {
                const int nWords = (N + 31) >> 5;
                build_rank_plane(sMask, sMask + nWords, nWords, nUsable, wave, lane);
                __syncthreads();
            }
        }
        usable = mb.slice(tid, N);
    }

    const uint64_t imageIdx = P.image0 + (uint64_t)b * P.imageStride;
    const uint64_t imageKey = image_key(P.seed, imageIdx);

    // ---- sample + score: this wave's hypotheses
    double bestScore = 0.0;
    int bestIdx = -1;
    int anyNan = 0;
    const float beta = 5.0f / cam.thr;
    const float fac = cam.alpha / (float)cam.Wo / (float)cam.Ho;

    if (PHASE != 2)
    for (int h = sub * kWaves + wave; h < P.nHyp; h += kWaves * nSub) {
        Pose pose;
        int c4[4] = { 0, 0, 0, 0 };
        int triesUsed = 0;
        for (uint32_t t0 = 0; t0 < P.maxTries; t0 += 64) {
            uint32_t t = t0 + (uint32_t)lane;
            Pose p;
            int cc[4] = { 0, 0, 0, 0 };
            bool ok = false;
            if (t < P.maxTries) ok = sample_try<MASK>(co, mb, cam, imageKey, (uint32_t)h, t, p, cc);
            else pose_identity(&p);
            unsigned long long m = __ballot(ok);
            int src;
            if (m != 0ull) { src = __ffsll((long long)m) - 1; triesUsed = (int)t0 + src + 1; }
            else if (t0 + 64u >= P.maxTries) { src = (int)(P.maxTries - 1u - t0); triesUsed = -(int)P.maxTries; }
            else continue;
            pose = wave_bcast_pose(p, src);
#pragma unroll
            for (int j = 0; j < 4; ++j) c4[j] = __shfl(cc[j], src);
            break;
        }

        // two cells per lane and trip: two independent chains of ~200 dependent fp64 instructions each (projection, divide, sqrt,
        // exp, divide) in flight - the kernel runs at 1-2 waves per SIMD and was bound by that latency.  Same operations per
        // cell, same order of the additions into `acc`: the bits do not change (XL_DSAC_PAIR_CELLS=0: one cell per trip)
        double acc = 0.0;
        // compact sampler: the lane as the compiler cannot see through it, so that the walk's start (row, column, mask word of
        // the first cells) is worked out per hypothesis - two integer divisions - instead of being hoisted out of the hypothesis
        // loop, where at 256 registers it is spilled (16 bytes of scratch per lane without this; the other modes keep their code)
        int lane0 = lane;
        if constexpr (MASK == kMaskCompact) asm volatile("" : "+v"(lane0));
        int i = lane0;
        CellWalk w0(lane0, 128, cam.Wo), w1(lane0 + 64, 128, cam.Wo);
        if (P.pairCells)
        for (; i + 64 < N; i += 128) {
            float e0, e1;
            if (P.cellWalk) {
                e0 = co.err(pose, i, w0.y, w0.x, cam); e1 = co.err(pose, i + 64, w1.y, w1.x, cam);
                w0.step(); w1.step();
            } else {
                e0 = co.err(pose, i, cam); e1 = co.err(pose, i + 64, cam);
            }
            const double st0 = soft_inlier_st(e0, cam.thr, beta), st1 = soft_inlier_st(e1, cam.thr, beta);
            if constexpr (MASKED) {
                acc += mb.usable(i) ? 1.0 - st0 : 0.0;
                acc += mb.usable(i + 64) ? 1.0 - st1 : 0.0;
            } else {
                acc += 1.0 - st0;
                acc += 1.0 - st1;
            }
        }
        for (; i < N; i += 64) {
            const double st = soft_inlier_st(co.err(pose, i, cam), cam.thr, beta);
            if constexpr (MASKED) acc += mb.usable(i) ? 1.0 - st : 0.0;
            else acc += 1.0 - st;
        }
        double total = wave_butterfly(acc);
        double score = total * (double)fac;

        if (lane == 0) {
            if (P.cells) {
                int32_t *o = P.cells + ((int64_t)b * P.nHyp + h) * 4;
                o[0] = c4[0]; o[1] = c4[1]; o[2] = c4[2]; o[3] = c4[3];
            }
            if (P.tries) P.tries[(int64_t)b * P.nHyp + h] = triesUsed;
            if (P.scores) P.scores[(int64_t)b * P.nHyp + h] = score;
            if (P.hypPoses) pose_store12(&pose, P.hypPoses + ((int64_t)b * P.nHyp + h) * 12);
        }
        if (score != score) anyNan = 1;
        bool better = (bestIdx < 0) || (score > bestScore);
        if (h == 0 && lane == 0) pose_store12(&pose, S.pose0);
        if (better) {
            bestScore = score; bestIdx = h;
            if (lane == 0) pose_store12(&pose, S.bestPose[wave]);
        }
    }
    if (PHASE == 1) {
        // publish this wave's best to global memory for the PHASE 2 launch (stream order makes it visible)
        __syncthreads();                                            // S.bestPose / S.pose0 written by lane 0s
        if (lane == 0) {
            double *o = P.part + ((int64_t)b * (P.S * kWaves) + sub * kWaves + wave) * 16;
            o[0] = bestScore; o[1] = (double)bestIdx; o[2] = (double)anyNan;
            for (int i = 0; i < 12; ++i) o[3 + i] = S.bestPose[wave][i];
            if (sub == 0 && wave == 0) {
                double *q = P.part + (int64_t)gridDim.y * (P.S * kWaves) * 16 + (int64_t)b * 12;
                for (int i = 0; i < 12; ++i) q[i] = S.pose0[i];
            }
        }
        return;
    }
    if (PHASE == 0) {
        if (lane == 0) { S.bestScore[wave] = bestScore; S.bestIdx[wave] = bestIdx; S.anyNan[wave] = anyNan; }
        __syncthreads();
    }

    // ---- select: first maximum wins (draw(probs,false), dsacstar_util.h:727-752)
    int win = -1, winWave = 0, nanAny = 0;
    const int nPart = (PHASE == 2) ? P.S * kWaves : kWaves;
    const double *gPart = (PHASE == 2) ? P.part + (int64_t)b * nPart * 16 : nullptr;
    {
        double ws = 0.0;
        for (int w = 0; w < nPart; ++w) {
            const double sc = (PHASE == 2) ? gPart[w * 16] : S.bestScore[w];
            const int idx = (PHASE == 2) ? (int)gPart[w * 16 + 1] : S.bestIdx[w];
            nanAny |= (PHASE == 2) ? (int)gPart[w * 16 + 2] : S.anyNan[w];
            if (idx < 0) continue;
            if (win < 0 || sc > ws || (sc == ws && idx < win)) { win = idx; ws = sc; winWave = w; }
        }
        if (nanAny) win = 0;        // any NaN score makes every softmax prob NaN -> draw() returns 0
    }
    Pose pose;
    {
        const double *src;
        if (PHASE == 2) src = nanAny ? P.part + (int64_t)gridDim.x * nPart * 16 + (int64_t)b * 12 : gPart + winWave * 16 + 3;
        else src = nanAny ? S.pose0 : S.bestPose[winWave];
        pose_load12(src, &pose);
    }
    if (tid == 0 && P.dbg) {
        double *o = P.dbg + (int64_t)b * XL_DSAC_DBG_DOUBLES;
        o[0] = (double)win;
        pose_store12(&pose, o + 4);
    }

    // ---- refine (refineHyp, dsacstar_util.h:522-597)
    RefineOut ro;
    int redSel = 0, cntSel = 0;
    refine_pose<MASKED>(co, cam, S, tid, wave, lane, pose, ro, redSel, cntSel, usable);
    const int rounds = ro.rounds, evals = ro.evals;
    const unsigned finalInl = ro.finalInl;

    // ---- write (pose2trans): inverse rigid transform, float row-major
    if (tid == 0) {
        pose_to_c2w16(&pose, P.outPoses + (int64_t)b * 16);
        if constexpr (MASKED) if (P.status) P.status[b] = 0;
        if (P.dbg) {
            double *q = P.dbg + (int64_t)b * XL_DSAC_DBG_DOUBLES;
            q[1] = (double)rounds; q[2] = (double)finalInl; q[3] = (double)evals;
            pose_store12(&pose, q + 16);
        }
    }
}

// ============================================================================== backward_rgb
// dsacstar_rgb_backward (dsacstar.cpp:200-483): expected pose loss over the soft-max distribution of the hypotheses
// and its gradient w.r.t. the scene coordinates (path I through the refined poses, path II through the scores).
// The per-cell and per-hypothesis derivatives are in xl_dsac_math.h (reference line numbers there); the kernels below
// keep the order of oracle/dsac_bwd_oracle.c's reductions, so the two produce identical bits.

// per-hypothesis record in global memory (doubles); the first 53 entries are the oracle's debug record
constexpr int kRec = XL_DSAC_BWD_REC;
constexpr int kRecDRinit = 64, kRecDRref = 91;             // 27 doubles each
constexpr int kRecInit = 118;                              // unused tail up to kRec

struct BwdParams {
    const float *coords; int64_t sb, sc, sy, sx;
    float *grad; int64_t gsb, gsc, gsy, gsx;
    const float *gt; const float *focals;
    const double *hypPoses; const double *scores; const int32_t *cells;
    double *rec; unsigned long long *masks; double *outLoss;
    int nHyp, Ho, Wo, sub, Npad;
    float thr, focal, ppx, ppy, alpha, maxReproj, wRot, wTrans, softClamp;
    const uint8_t *mask;          // masked backward: [B][Ho*Wo], nonzero = usable cell
    int32_t *status;              // masked backward: [B], 1 = dead image (fewer than four usable cells), else 0; never null there.
                                  // Written by the h == 0 workgroup of K1, read by K2, K3 and K4 (later launches on the same stream)
};

// MASKED (xl_dsac_backward_rgb_masked_batch), the forward's rules carried over.  K1 and K3 stage the mask as the forward kernel's bit
// plane behind the coordinate planes.  K1 refines over the usable cells (refine_pose<true>), so the inlier words it leaves in
// P.masks hold usable cells only and the two inlier walks need nothing more.  K3 sums path II over the usable cells (a masked-out
// cell's term is selected away, never multiplied by zero) and gives a hypothesis that carries a masked-out cell - tries exhausted
// on a mask-rejected try: identity pose, the last draws - the zero dPNP of a failed solve without reading that cell.  K4 leaves
// the gradient of a masked-out cell as it came in, without reading its coordinates.  A dead image (fewer than four usable cells;
// xl_dsac_forward_kernel<1, true> has then written neither poses nor cells) gets loss 0, status 1, zero records and an untouched
// gradient: K1 decides that on its own count before it reads a score and publishes it in P.status, on which K2, K3 and K4 return
// before they read anything of that image's workspace.
// Under the compact sampler (backward_rgb_launch<kMaskCompact>: the sample + score launch is xl_dsac_forward_kernel<1, kMaskCompact>,
// K1 - K4 are these MASKED instantiations) every hypothesis carries four usable cells, so K3's skip never fires and a hypothesis
// whose tries ran out is differentiated as the unmasked pass differentiates one.

// K1 (grid nHyp x B): soft-max probability of the hypothesis, refinement if it matters, loss, path-I quantities
template <bool MASKED = false>
__global__ __launch_bounds__(kThreads)
void xl_dsac_bwd_hyp_kernel(BwdParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Smem &S = *reinterpret_cast<Smem *>(smem_raw);
    float *sCo = reinterpret_cast<float *>(smem_raw + ((sizeof(Smem) + 15) & ~size_t(15)));
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.x, b = blockIdx.y;
    const Cam cam = cam_make(P.Ho, P.Wo, P.thr, P.focals ? P.focals[b] : P.focal, P.ppx, P.ppy, P.alpha, P.maxReproj, P.sub);
    const int N = cam.N;
    MaskBits mb{ reinterpret_cast<const uint32_t *>(sCo + 3 * P.Npad) };
    if constexpr (MASKED) {
        const int cnt = stage_mask(P.mask + (int64_t)b * N, N, reinterpret_cast<uint32_t *>(sCo + 3 * P.Npad), wave, lane);
        if (lane == 0) S.pad[wave] = cnt;
        __syncthreads();
        const bool dead = S.pad[0] + S.pad[1] + S.pad[2] + S.pad[3] < 4;          // uniform over the workgroups of the image
        if (h == 0 && tid == 0) P.status[b] = dead ? 1 : 0;
        if (dead) {
            // nothing of this image was sampled: the record is all zero, and neither a score nor a pose is read
            double *rec = P.rec + ((int64_t)b * P.nHyp + h) * kRec;
            for (int i = tid; i < kRec; i += kThreads) rec[i] = 0.0;
            return;
        }
    }

    // softMax (dsacstar_util.h:684-704), every thread in the same order
    const double *sc = P.scores + (int64_t)b * P.nHyp;
    double maxScore = 0.0, sum = 0.0;
    for (int i = 0; i < P.nHyp; ++i) if (i == 0 || sc[i] > maxScore) maxScore = sc[i];
    for (int i = 0; i < P.nHyp; ++i) sum += det_exp(sc[i] - maxScore);
    const double prob = det_exp(sc[h] - maxScore) / sum;
    const bool active = !(prob < XLM_PROB_THRESH);

    Pose init, pose;
    pose_load12(P.hypPoses + ((int64_t)b * P.nHyp + h) * 12, &init);
    pose = init;
    RefineOut ro;
    ro.inlAcc = 0ull; ro.finalInl = 0; ro.rounds = 0; ro.evals = 0;
    int redSel = 0, cntSel = 0;
    Coords co{ sCo, sCo + P.Npad, sCo + 2 * P.Npad };
    if (active) {
        stage_coords(P.coords + (int64_t)b * P.sb, P.sc, P.sy, P.sx, P.Wo, N, P.Npad, sCo, tid);
        __syncthreads();
        if constexpr (MASKED) refine_pose<true>(co, cam, S, tid, wave, lane, pose, ro, redSel, cntSel, mb.slice(tid, N));
        else refine_pose(co, cam, S, tid, wave, lane, pose, ro, redSel, cntSel);
    }
    Gt gt;
    gt_from_pose16(P.gt + (int64_t)b * 16, &gt);
    const double loss = pose_loss(&pose, &gt, (double)P.wRot, (double)P.wTrans, (double)P.softClamp);

    double *rec = P.rec + ((int64_t)b * P.nHyp + h) * kRec;
    double dLossH[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, wv[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    double maxJR = 0.0, rv[3] = { 0.0, 0.0, 0.0 };
    int clampI = 0;
    if (active) {
        double r0[3], dRi[27], dRr[27];
        log_so3(init.R, r0);
        rodrigues_jac(r0, dRi);
        log_so3(pose.R, rv);
        rodrigues_jac(rv, dRr);
        dloss(&pose, dRr, &gt, (double)P.wRot, (double)P.wTrans, (double)P.softClamp, dLossH);
        if (tid == 0)
            for (int i = 0; i < 27; ++i) { rec[kRecDRinit + i] = dRi[i]; rec[kRecDRref + i] = dRr[i]; }
        if (ro.finalInl >= 4) {
            double a[28];
#pragma unroll
            for (int k = 0; k < 28; ++k) a[k] = 0.0;
            int j = 0;
            for (int i = tid; i < N; i += kThreads, ++j) {
                if (!((ro.inlAcc >> j) & 1ull)) continue;
                int y = i / cam.Wo, x = i - y * cam.Wo;
                double X, Y, Z, J6[6];
                co.fetch(i, X, Y, Z);
                resid_row(&pose, dRr, X, Y, Z, cell_px(&cam, x), cell_px(&cam, y), &cam, J6);
                int k = 0;
#pragma unroll
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = r; c < 6; ++c) { a[k] += J6[r] * J6[c]; ++k; }
            }
            block_sum(a, S.red[redSel], wave, lane); redSel ^= 1;
            double A[36], Ainv[36];
            {
                int k = 0;
                for (int r = 0; r < 6; ++r)
                    for (int c = r; c < 6; ++c) { A[6 * r + c] = a[k]; A[6 * c + r] = a[k]; ++k; }
            }
            pinv6(A, Ainv);
            // max |jacobeanR| over this thread's inliers, then over the workgroup (order-free)
            j = 0;
            for (int i = tid; i < N; i += kThreads, ++j) {
                if (!((ro.inlAcc >> j) & 1ull)) continue;
                int y = i / cam.Wo, x = i - y * cam.Wo;
                double X, Y, Z, J6[6];
                co.fetch(i, X, Y, Z);
                resid_row(&pose, dRr, X, Y, Z, cell_px(&cam, x), cell_px(&cam, y), &cam, J6);
                for (int r = 0; r < 6; ++r) {
                    double u = 0.0;
                    for (int c = 0; c < 6; ++c) u += Ainv[6 * r + c] * J6[c];
                    u = fabs(u);
                    if (u > maxJR) maxJR = u;
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) { double o = __shfl_xor(maxJR, off); if (o > maxJR) maxJR = o; }
            __syncthreads();                                    // S.bestScore is free: the reduction above has completed
            if (lane == 0) S.bestScore[wave] = maxJR;
            __syncthreads();
            maxJR = S.bestScore[0];
            for (int w = 1; w < kWaves; ++w) if (S.bestScore[w] > maxJR) maxJR = S.bestScore[w];
            clampI = (maxJR > 10.0) ? 1 : 0;                    // dsacstar.cpp:411-412
            for (int r = 0; r < 6; ++r) {
                double v = 0.0;
                for (int c = 0; c < 6; ++c) v += Ainv[6 * r + c] * dLossH[c];
                wv[r] = v;
            }
        }
    }
    P.masks[((int64_t)b * P.nHyp + h) * kThreads + tid] = ro.inlAcc;
    if (tid == 0) {
        rec[0] = prob; rec[1] = loss; rec[2] = active ? 1.0 : 0.0; rec[3] = (double)ro.finalInl; rec[4] = (double)clampI;
        rec[5] = 0.0;
        pose_store12(&pose, rec + 6);
        for (int i = 0; i < 6; ++i) { rec[18 + i] = dLossH[i]; rec[24 + i] = wv[i]; }
        for (int i = 0; i < 12; ++i) rec[30 + i] = 0.0;
        rec[42] = maxJR; rec[43] = 0.0;
        for (int i = 0; i < 6; ++i) rec[44 + i] = 0.0;
        for (int i = 0; i < 3; ++i) rec[50 + i] = rv[i];
    }
}

// K2 (grid B): expected loss and the gradient of the soft-max selection (dsacstar_derivative.h:345-356)
template <bool MASKED = false>
__global__ __launch_bounds__(kThreads)
void xl_dsac_bwd_expect_kernel(BwdParams P)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    if constexpr (MASKED)
        if (P.status[b]) {                                      // dead image (K1 wrote the flag): loss 0, no record walk
            if (tid == 0) P.outLoss[b] = 0.0;
            return;
        }
    double *rec = P.rec + (int64_t)b * P.nHyp * kRec;
    if (tid == 0) {
        double e = 0.0;
        for (int h = 0; h < P.nHyp; ++h) e += rec[(int64_t)h * kRec] * rec[(int64_t)h * kRec + 1];
        P.outLoss[b] = e;
    }
    for (int i = tid; i < P.nHyp; i += kThreads) {
        const double pi = rec[(int64_t)i * kRec];
        if (pi < XLM_PROB_THRESH) continue;
        double g = pi * rec[(int64_t)i * kRec + 1];
        for (int j = 0; j < P.nHyp; ++j) g -= pi * rec[(int64_t)j * kRec] * rec[(int64_t)j * kRec + 1];
        rec[(int64_t)i * kRec + 5] = g;
    }
}

// K3 (grid nHyp x B): path II per hypothesis — g6 = sum_c dRepro(c) J_init(c), dPNP by central differences,
// support-point gradients (dsacstar_derivative.h:209-320)
template <bool MASKED = false>
__global__ __launch_bounds__(kThreads)
void xl_dsac_bwd_score_kernel(BwdParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Smem &S = *reinterpret_cast<Smem *>(smem_raw);
    float *sCo = reinterpret_cast<float *>(smem_raw + ((sizeof(Smem) + 15) & ~size_t(15)));
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.x, b = blockIdx.y;
    // dead image: K1 has counted the mask and written the flag; nothing of the image's workspace is read, rec[0] included (an
    // inactive hypothesis of a live image then leaves as early as in the unmasked kernel, without staging anything)
    if constexpr (MASKED) if (P.status[b]) return;
    double *rec = P.rec + ((int64_t)b * P.nHyp + h) * kRec;
    if (rec[0] < XLM_PROB_THRESH) return;
    const Cam cam = cam_make(P.Ho, P.Wo, P.thr, P.focals ? P.focals[b] : P.focal, P.ppx, P.ppy, P.alpha, P.maxReproj, P.sub);
    const int N = cam.N;
    stage_coords(P.coords + (int64_t)b * P.sb, P.sc, P.sy, P.sx, P.Wo, N, P.Npad, sCo, tid);
    MaskBits mb{ reinterpret_cast<const uint32_t *>(sCo + 3 * P.Npad) };
    if constexpr (MASKED) (void)stage_mask(P.mask + (int64_t)b * N, N, reinterpret_cast<uint32_t *>(sCo + 3 * P.Npad), wave, lane);
    __syncthreads();
    Coords co{ sCo, sCo + P.Npad, sCo + 2 * P.Npad };
    Pose init;
    pose_load12(P.hypPoses + ((int64_t)b * P.nHyp + h) * 12, &init);
    double dRi[27];
    for (int i = 0; i < 27; ++i) dRi[i] = rec[kRecDRinit + i];
    const double sog = rec[5];
    const float beta = 5.0f / cam.thr;
    const float facf = cam.alpha / (float)cam.Wo / (float)cam.Ho;

    double a[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) a[k] = 0.0;
    for (int i = tid; i < N; i += kThreads) {
        int y = i / cam.Wo, x = i - y * cam.Wo;
        double X, Y, Z, J6[6];
        co.fetch(i, X, Y, Z);
        double st = soft_inlier_st(co.err(init, i, y, x, cam), cam.thr, beta);
        double dRep = -st * (1.0 - st) * (double)beta * sog;
        dRep *= (double)facf;
        resid_row(&init, dRi, X, Y, Z, cell_px(&cam, x), cell_px(&cam, y), &cam, J6);
        if constexpr (MASKED) {
            // whatever a masked-out cell holds was fetched and differentiated above; none of it reaches a[]
            const bool u = mb.usable(i);
#pragma unroll
            for (int k = 0; k < 6; ++k) a[k] += u ? dRep * J6[k] : 0.0;
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) a[k] += dRep * J6[k];
        }
    }
    block_sum(a, S.red[0], wave, lane);

    // dPNP (dsacstar_derivative.h:131-190): lanes 0..17 each solve one perturbed P3P; the float += eps / -= 2 eps /
    // += eps sequence of the earlier columns is replayed so every solve sees the points the serial code would
    double *sol = S.red[1];                                  // [18][7]: rvec, tvec, ok
    const int32_t *cells = P.cells + ((int64_t)b * P.nHyp + h) * 4;
    // masked: a hypothesis whose tries ran out on a mask-rejected try carries masked-out cells; their coordinates are not read,
    // the 18 solves are skipped and J is the zero of a failed solve (the same decision in every thread: it is read off the plane)
    bool skip = false;
    if constexpr (MASKED) skip = !(mb.usable(cells[0]) && mb.usable(cells[1]) && mb.usable(cells[2]) && mb.usable(cells[3]));
    if (!skip && tid < 18) {
        const float eps = 0.001f;
        float pts[4][3];
        double uv[4][2];
        for (int q = 0; q < 4; ++q) {
            const int ci = cells[q];
            const int y = ci / cam.Wo, x = ci - y * cam.Wo;
            pts[q][0] = sCo[ci]; pts[q][1] = sCo[P.Npad + ci]; pts[q][2] = sCo[2 * P.Npad + ci];
            uv[q][0] = (double)cell_px(&cam, x);
            uv[q][1] = (double)cell_px(&cam, y);
        }
        const int col = tid >> 1, back = tid & 1;
        for (int c = 0; c <= col; ++c) {
            float &v = pts[c / 3][c % 3];
            v += eps;
            if (c < col || back) v -= 2 * eps;
            if (c < col) v += eps;
        }
        Pose sp;
        V3 Q[4];
        for (int q = 0; q < 4; ++q) { Q[q].x = (double)pts[q][0]; Q[q].y = (double)pts[q][1]; Q[q].z = (double)pts[q][2]; }
        const bool ok = p3p(Q[0], Q[1], Q[2], Q[3], uv, &cam, &sp);
        double r[3] = { 0.0, 0.0, 0.0 };
        if (ok) log_so3(sp.R, r);
        double *o = sol + tid * 7;
        o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
        o[3] = ok ? sp.t[0] : 0.0; o[4] = ok ? sp.t[1] : 0.0; o[5] = ok ? sp.t[2] : 0.0;
        o[6] = ok ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double J[72];
        for (int k = 0; k < 72; ++k) J[k] = 0.0;
        const double den = (double)(2 * 0.001f);
        bool fail = skip;
        for (int col = 0; col < 9 && !fail; ++col) {
            const double *f = sol + (2 * col) * 7, *bk = sol + (2 * col + 1) * 7;
            if (f[6] == 0.0 || bk[6] == 0.0) { fail = true; break; }
            for (int k = 0; k < 3; ++k) {
                double av = (f[k] - bk[k]) / den, bv = (f[3 + k] - bk[3 + k]) / den;
                J[k * 12 + col] = av;
                J[(3 + k) * 12 + col] = bv;
                if (!(av == av) || !(bv == bv)) fail = true;
            }
        }
        if (fail) for (int k = 0; k < 72; ++k) J[k] = 0.0;
        double maxH = 0.0;
        for (int k = 0; k < 72; ++k) { double v = fabs(J[k]); if (v > maxH) maxH = v; }
        if (maxH > 10.0) for (int k = 0; k < 72; ++k) J[k] = 0.0;
        for (int c = 0; c < 12; ++c) {
            double v = 0.0;
            for (int r = 0; r < 6; ++r) v += a[r] * J[r * 12 + c];
            rec[30 + c] = v;
        }
        rec[43] = maxH;
        for (int k = 0; k < 6; ++k) rec[44 + k] = a[k];
    }
}

// K4 (grid ceil(N/256) x B): assemble the gradient per cell, hypotheses in ascending order, float accumulation
// like the reference's tensor += (dsacstar.cpp:462-480)
template <bool MASKED = false>
__global__ __launch_bounds__(kThreads)
void xl_dsac_bwd_assemble_kernel(BwdParams P)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const Cam cam = cam_make(P.Ho, P.Wo, P.thr, P.focals ? P.focals[b] : P.focal, P.ppx, P.ppy, P.alpha, P.maxReproj, P.sub);
    if (i >= cam.N) return;
    // masked: a dead image (K1's flag) and a masked-out cell (its byte in global memory: this kernel uses no LDS) keep the incoming
    // gradient bit for bit - it is neither read nor written - and their coordinates are not read
    if constexpr (MASKED) if (P.status[b] || P.mask[(int64_t)b * cam.N + i] == 0) return;
    const int y = i / cam.Wo, x = i - y * cam.Wo;
    const float *q = P.coords + (int64_t)b * P.sb + (int64_t)y * P.sy + (int64_t)x * P.sx;
    const double X = (double)q[0], Y = (double)q[P.sc], Z = (double)q[2 * P.sc];
    const float px = cell_px(&cam, x), py = cell_px(&cam, y);
    float *g = P.grad + (int64_t)b * P.gsb + (int64_t)y * P.gsy + (int64_t)x * P.gsx;
    float acc[3] = { g[0], g[P.gsc], g[2 * P.gsc] };
    const float beta = 5.0f / cam.thr;
    const float facf = cam.alpha / (float)cam.Wo / (float)cam.Ho;
    const int mt = i % kThreads, mj = i / kThreads;
    for (int h = 0; h < P.nHyp; ++h) {
        const double *rec = P.rec + ((int64_t)b * P.nHyp + h) * kRec;
        const double prob = rec[0];
        if (prob < XLM_PROB_THRESH) continue;
        Pose init, ref;
        pose_load12(P.hypPoses + ((int64_t)b * P.nHyp + h) * 12, &init);
        pose_load12(rec + 6, &ref);
        double gI[3] = { 0.0, 0.0, 0.0 };
        const unsigned long long m = P.masks[((int64_t)b * P.nHyp + h) * kThreads + mt];
        if (rec[3] >= 4.0 && rec[4] == 0.0 && ((m >> mj) & 1ull)) {
            double J6[6], dNdO[3];
            resid_row(&ref, rec + kRecDRref, X, Y, Z, px, py, &cam, J6);
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s += J6[k] * rec[24 + k];
            s = -s;
            dproject_dobj(&ref, X, Y, Z, px, py, &cam, dNdO);
            for (int k = 0; k < 3; ++k) gI[k] = s * dNdO[k];
        }
        double st = soft_inlier_st(cell_err(&init, X, Y, Z, y, x, &cam), cam.thr, beta);   // at the clamped float error under the unrefined hypothesis
        double dRep = -st * (1.0 - st) * (double)beta * rec[5];
        dRep *= (double)facf;
        double dPdO[3];
        dproject_dobj(&init, X, Y, Z, px, py, &cam, dPdO);
        double jac[3] = { dPdO[0] * dRep, dPdO[1] * dRep, dPdO[2] * dRep };
        const int32_t *cells = P.cells + ((int64_t)b * P.nHyp + h) * 4;
        for (int j = 0; j < 4; ++j)
            if (cells[j] == i)
                for (int k = 0; k < 3; ++k) jac[k] += rec[30 + 3 * j + k];
        for (int k = 0; k < 3; ++k) acc[k] = (float)((double)acc[k] + (prob * gI[k] + jac[k]));
    }
    g[0] = acc[0]; g[P.gsc] = acc[1]; g[2 * P.gsc] = acc[2];
}

thread_local char g_hipErr[256] = "";

int hip_fail(hipError_t e, const char *what)
{
    snprintf(g_hipErr, sizeof(g_hipErr), "%s: %s", what, hipGetErrorString(e));
    return XL_ERR_HIP;
}

#define XL_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hip_fail(e_, #call); } while (0)

}  // namespace

extern "C" {

int xl_dsac_forward_sub_blocks(int B, int n_hyp)
{
    if (B <= 0 || n_hyp <= 0) return 0;
    // sub-blocks per image: fill ~2 workgroups per CU, at least one hypothesis per wavefront
    int S = 1;
    while (S * 2 <= n_hyp / kWaves && (long long)B * S * 2 <= 512) S *= 2;
    static const char *noSplit = getenv("XL_DSAC_NO_SPLIT");
    if (noSplit) S = 1;
    static const int forceS = getenv("XL_DSAC_SPLIT") ? atoi(getenv("XL_DSAC_SPLIT")) : 0;      // experiments: sub-blocks per image
    if (forceS >= 1 && forceS * kWaves <= n_hyp) S = forceS;
    return S;
}

}  // extern "C"

namespace {

// the forward launch of the solvers: a mask mode other than kMaskNone adds the mask and the status vector and the bit plane to the
// LDS carve, kMaskCompact the rank plane behind it; each mode launches its own instantiations (which keep an LDS limit of their own)
template <int MASK>
int forward_rgb_launch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                       int B, int Ho, int Wo, const uint8_t *mask_dev, float *out_poses_dev, int32_t *status_dev,
                       int n_hyp, float thr, float focal, float ppx, float ppy,
                       float alpha, float max_reproj, int sub, const float *focals_dev,
                       uint64_t seed, uint64_t image0, uint64_t image_stride, uint32_t max_tries,
                       void *stream,
                       int32_t *cells_dev, int32_t *tries_dev, double *scores_dev, double *dbg_dev)
{
    if (!coords_dev || !out_poses_dev || B <= 0 || Ho <= 0 || Wo <= 0 || n_hyp <= 0 || sub <= 0 || max_tries == 0)
        return XL_ERR_ARG;
    constexpr bool MASKED = MASK != kMaskNone;
    if (MASKED && !mask_dev) return XL_ERR_ARG;
    const int N = Ho * Wo;
    if (N > kMaxCells) return XL_ERR_GRID;
    Params P;
    P.mask = mask_dev; P.status = status_dev;
    P.coords = coords_dev; P.sb = sb; P.sc = sc; P.sy = sy; P.sx = sx;
    P.outPoses = out_poses_dev; P.focals = focals_dev;
    P.cells = cells_dev; P.tries = tries_dev; P.scores = scores_dev; P.dbg = dbg_dev; P.hypPoses = nullptr;
    P.seed = seed; P.image0 = image0; P.imageStride = image_stride; P.maxTries = max_tries;
    P.nHyp = n_hyp; P.Ho = Ho; P.Wo = Wo; P.sub = sub; P.Npad = (N + 3) & ~3;
    P.thr = thr; P.focal = focal; P.ppx = ppx; P.ppy = ppy; P.alpha = alpha; P.maxReproj = max_reproj;

    size_t lds = ((sizeof(Smem) + 15) & ~size_t(15)) + (size_t)3 * P.Npad * sizeof(float);
    if (MASKED) lds += sizeof(uint32_t) * (size_t)((N + 31) / 32);          // the bit plane: 676 B at 60x90
    if (MASK == kMaskCompact) lds += sizeof(uint32_t) * (size_t)((N + 31) / 32 + 1);     // the rank plane: 680 B at 60x90
    if (lds > 160 * 1024) return XL_ERR_GRID;
    static XlLdsLimit configured;
    int cfgDev;
    if (configured.needs(lds, &cfgDev)) {
        XL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(xl_dsac_forward_kernel<0, MASK>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        XL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(xl_dsac_forward_kernel<1, MASK>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        XL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(xl_dsac_forward_kernel<2, MASK>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        configured.done(lds, cfgDev);
    }
    hipStream_t st = (hipStream_t)stream;
    const int S = xl_dsac_forward_sub_blocks(B, n_hyp);
    P.part = nullptr; P.S = S;
    static const int pairCells = getenv("XL_DSAC_PAIR_CELLS") ? atoi(getenv("XL_DSAC_PAIR_CELLS")) : 1;
    P.pairCells = pairCells;
    static const int cellWalk = getenv("XL_DSAC_CELL_WALK") ? atoi(getenv("XL_DSAC_CELL_WALK")) : 1;
    P.cellWalk = cellWalk;
    if (S == 1) {
        hipLaunchKernelGGL((xl_dsac_forward_kernel<0, MASK>), dim3(B), dim3(kThreads), lds, st, P);
    } else {
        const size_t bytes = sizeof(double) * ((size_t)B * S * kWaves * 16 + (size_t)B * 12);
        XL_HIP(hipMallocAsync((void **)&P.part, bytes, st));
        hipLaunchKernelGGL((xl_dsac_forward_kernel<1, MASK>), dim3(S, B), dim3(kThreads), lds, st, P);
        hipLaunchKernelGGL((xl_dsac_forward_kernel<2, MASK>), dim3(B), dim3(kThreads), lds, st, P);
        XL_HIP(hipFreeAsync(P.part, st));
    }
    XL_HIP(hipGetLastError());
    return XL_OK;
}

// sub-blocks per image of the backward pass's sample + score launch (it fills the chip further than the forward's: ~4 workgroups per CU)
int backward_sub_blocks(int B, int n_hyp)
{
    int S = 1;
    while (S * 2 * kWaves <= n_hyp && (long long)B * S * 2 <= 1024) S *= 2;
    return S;
}

// the LDS limit of the backward kernels K1 and K3, one per instantiation: the masked pair serves both samplers
template <bool MASKED>
XlLdsLimit &backward_kernels_lds()
{
    static XlLdsLimit limit;
    return limit;
}

// the launch sequence of the backward passes: a mask mode other than kMaskNone adds the mask and the status vector, the bit plane
// to the LDS carve, and launches the masked instantiations of K1 - K4; the sample + score launch is the mode's own (kMaskCompact:
// with the rank plane behind the bit plane), so the hypotheses differentiated are the ones that mode's forward produced.
// Everything is validated before the first HIP call.
template <int MASK>
int backward_rgb_launch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                        int B, int Ho, int Wo, const uint8_t *mask_dev,
                        float *grad_dev, int64_t gsb, int64_t gsc, int64_t gsy, int64_t gsx,
                        const float *gt_poses_dev, double *out_loss_dev, int32_t *status_dev,
                        int n_hyp, float thr, float focal, float ppx, float ppy,
                        float w_rot, float w_trans, float soft_clamp, float alpha, float max_reproj, int sub,
                        const float *focals_dev, uint64_t seed, uint64_t image0, uint64_t image_stride,
                        uint32_t max_tries, void *stream, double *rec_dev)
{
    if (!coords_dev || !grad_dev || !gt_poses_dev || !out_loss_dev || B <= 0 || Ho <= 0 || Wo <= 0 || n_hyp <= 0 ||
        sub <= 0 || max_tries == 0)
        return XL_ERR_ARG;
    constexpr bool MASKED = MASK != kMaskNone;
    if (MASKED && !mask_dev) return XL_ERR_ARG;
    const int N = Ho * Wo;
    if (N > kMaxCells) return XL_ERR_GRID;
    const int Npad = (N + 3) & ~3;
    size_t lds = ((sizeof(Smem) + 15) & ~size_t(15)) + (size_t)3 * Npad * sizeof(float);
    if (MASKED) lds += sizeof(uint32_t) * (size_t)((N + 31) / 32);          // the bit plane: 676 B at 60x90
    const size_t ldsSample = lds + (MASK == kMaskCompact ? sizeof(uint32_t) * (size_t)((N + 31) / 32 + 1) : 0);     // + the rank plane
    if (ldsSample > 160 * 1024) return XL_ERR_GRID;
    hipStream_t st = (hipStream_t)stream;
    const size_t nh = (size_t)B * n_hyp;

    // workspace: every hypothesis' pose, score and sampled cells; per-hypothesis records and inlier masks; masked, without a
    // status vector of the caller's: the dead-image flags
    const int S = backward_sub_blocks(B, n_hyp);
    const size_t bPoses = sizeof(double) * nh * 12, bScores = sizeof(double) * nh, bCells = sizeof(int32_t) * nh * 4;
    const size_t bRec = rec_dev ? 0 : sizeof(double) * nh * kRec, bMasks = sizeof(unsigned long long) * nh * kThreads;
    const size_t bPart = sizeof(double) * ((size_t)B * S * kWaves * 16 + (size_t)B * 12);
    const size_t bFlags = (MASKED && !status_dev) ? sizeof(int32_t) * (size_t)B : 0;
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    unsigned char *ws = nullptr;
    XL_HIP(hipMallocAsync((void **)&ws, up(bPoses) + up(bScores) + up(bCells) + up(bRec) + up(bMasks) + up(bPart) + up(bFlags), st));
    unsigned char *cur = ws;
    double *hypPoses = (double *)cur; cur += up(bPoses);
    double *scores = (double *)cur; cur += up(bScores);
    int32_t *cells = (int32_t *)cur; cur += up(bCells);
    double *rec = rec_dev ? rec_dev : (double *)cur; cur += up(bRec);
    unsigned long long *masks = (unsigned long long *)cur; cur += up(bMasks);
    double *part = (double *)cur; cur += up(bPart);
    int32_t *flags = status_dev ? status_dev : (int32_t *)cur;

    Params P;
    P.coords = coords_dev; P.sb = sb; P.sc = sc; P.sy = sy; P.sx = sx;
    P.outPoses = nullptr; P.focals = focals_dev;
    P.cells = cells; P.tries = nullptr; P.scores = scores; P.dbg = nullptr; P.hypPoses = hypPoses;
    P.seed = seed; P.image0 = image0; P.imageStride = image_stride; P.maxTries = max_tries;
    P.nHyp = n_hyp; P.Ho = Ho; P.Wo = Wo; P.sub = sub; P.Npad = Npad;
    P.thr = thr; P.focal = focal; P.ppx = ppx; P.ppy = ppy; P.alpha = alpha; P.maxReproj = max_reproj;
    P.part = part; P.S = S;
    P.pairCells = 1; P.cellWalk = 1;
    P.mask = mask_dev; P.status = nullptr;                     // (the sample + score phase writes no status: K1 does)
    BwdParams Q;
    Q.coords = coords_dev; Q.sb = sb; Q.sc = sc; Q.sy = sy; Q.sx = sx;
    Q.grad = grad_dev; Q.gsb = gsb; Q.gsc = gsc; Q.gsy = gsy; Q.gsx = gsx;
    Q.gt = gt_poses_dev; Q.focals = focals_dev;
    Q.hypPoses = hypPoses; Q.scores = scores; Q.cells = cells; Q.rec = rec; Q.masks = masks; Q.outLoss = out_loss_dev;
    Q.nHyp = n_hyp; Q.Ho = Ho; Q.Wo = Wo; Q.sub = sub; Q.Npad = P.Npad;
    Q.thr = thr; Q.focal = focal; Q.ppx = ppx; Q.ppy = ppy; Q.alpha = alpha; Q.maxReproj = max_reproj;
    Q.wRot = w_rot; Q.wTrans = w_trans; Q.softClamp = soft_clamp;
    Q.mask = mask_dev; Q.status = MASKED ? flags : nullptr;

    static XlLdsLimit configured;
    int cfgDev;
    if (configured.needs(ldsSample, &cfgDev)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(xl_dsac_forward_kernel<1, MASK>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsSample);
        if (e != hipSuccess) { (void)hipFreeAsync(ws, st); return hip_fail(e, "hipFuncSetAttribute(backward_rgb)"); }
        configured.done(ldsSample, cfgDev);
    }
    XlLdsLimit &configuredBwd = backward_kernels_lds<MASKED>();
    if (configuredBwd.needs(lds, &cfgDev)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(xl_dsac_bwd_hyp_kernel<MASKED>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void *>(xl_dsac_bwd_score_kernel<MASKED>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { (void)hipFreeAsync(ws, st); return hip_fail(e, "hipFuncSetAttribute(backward_rgb)"); }
        configuredBwd.done(lds, cfgDev);
    }
    hipLaunchKernelGGL((xl_dsac_forward_kernel<1, MASK>), dim3(S, B), dim3(kThreads), ldsSample, st, P);
    hipLaunchKernelGGL((xl_dsac_bwd_hyp_kernel<MASKED>), dim3(n_hyp, B), dim3(kThreads), lds, st, Q);
    hipLaunchKernelGGL((xl_dsac_bwd_expect_kernel<MASKED>), dim3(B), dim3(kThreads), 0, st, Q);
    hipLaunchKernelGGL((xl_dsac_bwd_score_kernel<MASKED>), dim3(n_hyp, B), dim3(kThreads), lds, st, Q);
    hipLaunchKernelGGL((xl_dsac_bwd_assemble_kernel<MASKED>), dim3((N + kThreads - 1) / kThreads, B), dim3(kThreads), 0, st, Q);
    XL_HIP(hipFreeAsync(ws, st));
    XL_HIP(hipGetLastError());
    return XL_OK;
}

}  // namespace

extern "C" {

int xl_dsac_forward_rgb_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                              int B, int Ho, int Wo, float *out_poses_dev,
                              int n_hyp, float thr, float focal, float ppx, float ppy,
                              float alpha, float max_reproj, int sub, const float *focals_dev,
                              uint64_t seed, uint64_t image0, uint64_t image_stride, uint32_t max_tries,
                              void *stream,
                              int32_t *cells_dev, int32_t *tries_dev, double *scores_dev, double *dbg_dev)
{
    return forward_rgb_launch<kMaskNone>(coords_dev, sb, sc, sy, sx, B, Ho, Wo, nullptr, out_poses_dev, nullptr, n_hyp, thr, focal,
                                     ppx, ppy, alpha, max_reproj, sub, focals_dev, seed, image0, image_stride, max_tries, stream,
                                     cells_dev, tries_dev, scores_dev, dbg_dev);
}

int xl_dsac_forward_rgb_masked_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                     int B, int Ho, int Wo, const uint8_t *mask_dev, float *out_poses_dev, int32_t *status_dev,
                                     int n_hyp, float thr, float focal, float ppx, float ppy,
                                     float alpha, float max_reproj, int sub, const float *focals_dev,
                                     uint64_t seed, uint64_t image0, uint64_t image_stride, uint32_t max_tries,
                                     void *stream,
                                     int32_t *cells_dev, int32_t *tries_dev, double *scores_dev, double *dbg_dev)
{
    return xl_dsac_forward_rgb_masked_sampled_batch(coords_dev, sb, sc, sy, sx, B, Ho, Wo, mask_dev, XL_DSAC_SAMPLER_REJECT,
                                                    out_poses_dev, status_dev, n_hyp, thr, focal, ppx, ppy, alpha, max_reproj, sub,
                                                    focals_dev, seed, image0, image_stride, max_tries, stream,
                                                    cells_dev, tries_dev, scores_dev, dbg_dev);
}

int xl_dsac_forward_rgb_masked_sampled_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                             int B, int Ho, int Wo, const uint8_t *mask_dev, int sampler,
                                             float *out_poses_dev, int32_t *status_dev,
                                             int n_hyp, float thr, float focal, float ppx, float ppy,
                                             float alpha, float max_reproj, int sub, const float *focals_dev,
                                             uint64_t seed, uint64_t image0, uint64_t image_stride, uint32_t max_tries,
                                             void *stream,
                                             int32_t *cells_dev, int32_t *tries_dev, double *scores_dev, double *dbg_dev)
{
    if (sampler == XL_DSAC_SAMPLER_REJECT)
        return forward_rgb_launch<kMaskReject>(coords_dev, sb, sc, sy, sx, B, Ho, Wo, mask_dev, out_poses_dev, status_dev, n_hyp, thr,
                                               focal, ppx, ppy, alpha, max_reproj, sub, focals_dev, seed, image0, image_stride,
                                               max_tries, stream, cells_dev, tries_dev, scores_dev, dbg_dev);
    if (sampler == XL_DSAC_SAMPLER_COMPACT)
        return forward_rgb_launch<kMaskCompact>(coords_dev, sb, sc, sy, sx, B, Ho, Wo, mask_dev, out_poses_dev, status_dev, n_hyp, thr,
                                                focal, ppx, ppy, alpha, max_reproj, sub, focals_dev, seed, image0, image_stride,
                                                max_tries, stream, cells_dev, tries_dev, scores_dev, dbg_dev);
    return XL_ERR_ARG;                                           // unknown sampler: before any device work
}

// The reference's call shape (utils/evaluation.py:160-172): ONE frame, host tensors in, host pose out, blocking.  Round 6: the device
// and pinned staging buffers and the stream of a calling thread are kept between calls (the loop of test_single_task.py:347-363
// calls this once per frame: six hipMalloc / hipFree pairs - each hipFree a device-wide synchronisation - and a pageable H2D
// copy per call were a tenth of the 2.3 ms a frame took end to end); everything runs on that private stream and the call
// returns after ONE hipStreamSynchronize.  Buffers grow on demand and live as long as the process (no destructor: the HIP
// runtime may be gone when a thread-local dies).  The debug outputs (tests only) are allocated per call as before.
namespace {
struct HostWorkspace {
    int dev = -1;
    hipStream_t st = nullptr;
    float *dCo = nullptr, *hCo = nullptr; size_t cap = 0;      // device / pinned host staging of the [3,Ho,Wo] coordinates (floats)
    float *dPose = nullptr, *hPose = nullptr;                  // 16 floats each
};
thread_local HostWorkspace g_hostWs;
}  // namespace

int xl_dsac_forward_rgb_host(const float *coords_host, int64_t sc, int64_t sy, int64_t sx, int Ho, int Wo,
                             float *out_pose_host, int n_hyp, float thr, float focal, float ppx, float ppy,
                             float alpha, float max_reproj, int sub,
                             uint64_t seed, uint64_t image, uint32_t max_tries,
                             int32_t *cells_host, int32_t *tries_host, double *scores_host, double *dbg_host)
{
    if (!coords_host || !out_pose_host || Ho <= 0 || Wo <= 0 || n_hyp <= 0) return XL_ERR_ARG;
    const int N = Ho * Wo;
    if (N > kMaxCells) return XL_ERR_GRID;
    int32_t *dCells = nullptr, *dTries = nullptr;
    double *dScores = nullptr, *dDbg = nullptr;
    int rc = XL_OK;
    hipError_t e;
#define XL_TRY(call) do { e = (call); if (e != hipSuccess) { rc = hip_fail(e, #call); goto done; } } while (0)
    {
        HostWorkspace &w = g_hostWs;
        int dev = 0;
        XL_TRY(hipGetDevice(&dev));
        if (w.dev != dev) {                                  // first call of this thread, or the thread switched devices: start over
            w = HostWorkspace();                             // (buffers of another device are left to that device's context)
            XL_TRY(hipStreamCreateWithFlags(&w.st, hipStreamNonBlocking));
            XL_TRY(hipMalloc(&w.dPose, sizeof(float) * 16));
            XL_TRY(hipHostMalloc((void **)&w.hPose, sizeof(float) * 16, hipHostMallocDefault));
            w.dev = dev;
        }
        if (w.cap < (size_t)3 * N) {
            if (w.dCo) { (void)hipFree(w.dCo); w.dCo = nullptr; }
            if (w.hCo) { (void)hipHostFree(w.hCo); w.hCo = nullptr; }
            w.cap = 0;
            XL_TRY(hipMalloc(&w.dCo, sizeof(float) * 3 * (size_t)N));
            XL_TRY(hipHostMalloc((void **)&w.hCo, sizeof(float) * 3 * (size_t)N, hipHostMallocDefault));
            w.cap = (size_t)3 * N;
        }
        // pack to the contiguous [3,Ho,Wo] pinned staging buffer (honours arbitrary host strides)
        if (sx == 1 && sy == Wo && sc == (int64_t)N) memcpy(w.hCo, coords_host, sizeof(float) * 3 * (size_t)N);
        else
            for (int c = 0; c < 3; ++c)
                for (int y = 0; y < Ho; ++y)
                    for (int x = 0; x < Wo; ++x)
                        w.hCo[((size_t)c * Ho + y) * Wo + x] = coords_host[c * sc + y * sy + x * sx];
        XL_TRY(hipMemcpyAsync(w.dCo, w.hCo, sizeof(float) * 3 * (size_t)N, hipMemcpyHostToDevice, w.st));
        if (cells_host) XL_TRY(hipMalloc(&dCells, sizeof(int32_t) * 4 * (size_t)n_hyp));
        if (tries_host) XL_TRY(hipMalloc(&dTries, sizeof(int32_t) * (size_t)n_hyp));
        if (scores_host) XL_TRY(hipMalloc(&dScores, sizeof(double) * (size_t)n_hyp));
        if (dbg_host) XL_TRY(hipMalloc(&dDbg, sizeof(double) * XL_DSAC_DBG_DOUBLES));
        rc = xl_dsac_forward_rgb_batch(w.dCo, (int64_t)3 * N, N, Wo, 1, 1, Ho, Wo, w.dPose, n_hyp, thr, focal, ppx, ppy,
                                       alpha, max_reproj, sub, nullptr, seed, image, 1, max_tries, (void *)w.st,
                                       dCells, dTries, dScores, dDbg);
        if (rc != XL_OK) goto done;
        XL_TRY(hipMemcpyAsync(w.hPose, w.dPose, sizeof(float) * 16, hipMemcpyDeviceToHost, w.st));
        XL_TRY(hipStreamSynchronize(w.st));
        memcpy(out_pose_host, w.hPose, sizeof(float) * 16);
        if (cells_host) XL_TRY(hipMemcpy(cells_host, dCells, sizeof(int32_t) * 4 * (size_t)n_hyp, hipMemcpyDeviceToHost));
        if (tries_host) XL_TRY(hipMemcpy(tries_host, dTries, sizeof(int32_t) * (size_t)n_hyp, hipMemcpyDeviceToHost));
        if (scores_host) XL_TRY(hipMemcpy(scores_host, dScores, sizeof(double) * (size_t)n_hyp, hipMemcpyDeviceToHost));
        if (dbg_host) XL_TRY(hipMemcpy(dbg_host, dDbg, sizeof(double) * XL_DSAC_DBG_DOUBLES, hipMemcpyDeviceToHost));
    }
done:
#undef XL_TRY
    if (rc != XL_OK && g_hostWs.st) (void)hipStreamSynchronize(g_hostWs.st);     // nothing of a failed call stays in flight on the buffers
    if (dCells) (void)hipFree(dCells);
    if (dTries) (void)hipFree(dTries);
    if (dScores) (void)hipFree(dScores);
    if (dDbg) (void)hipFree(dDbg);
    return rc;
}

int xl_dsac_backward_sub_blocks(int B, int n_hyp)
{
    return (B <= 0 || n_hyp <= 0) ? 0 : backward_sub_blocks(B, n_hyp);
}

int xl_dsac_backward_rgb_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                               int B, int Ho, int Wo,
                               float *grad_dev, int64_t gsb, int64_t gsc, int64_t gsy, int64_t gsx,
                               const float *gt_poses_dev, double *out_loss_dev,
                               int n_hyp, float thr, float focal, float ppx, float ppy,
                               float w_rot, float w_trans, float soft_clamp, float alpha, float max_reproj, int sub,
                               const float *focals_dev, uint64_t seed, uint64_t image0, uint64_t image_stride,
                               uint32_t max_tries, void *stream, double *rec_dev)
{
    return backward_rgb_launch<kMaskNone>(coords_dev, sb, sc, sy, sx, B, Ho, Wo, nullptr, grad_dev, gsb, gsc, gsy, gsx, gt_poses_dev,
                                      out_loss_dev, nullptr, n_hyp, thr, focal, ppx, ppy, w_rot, w_trans, soft_clamp, alpha,
                                      max_reproj, sub, focals_dev, seed, image0, image_stride, max_tries, stream, rec_dev);
}

int xl_dsac_backward_rgb_masked_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                      int B, int Ho, int Wo, const uint8_t *mask_dev,
                                      float *grad_dev, int64_t gsb, int64_t gsc, int64_t gsy, int64_t gsx,
                                      const float *gt_poses_dev, double *out_loss_dev, int32_t *status_dev,
                                      int n_hyp, float thr, float focal, float ppx, float ppy,
                                      float w_rot, float w_trans, float soft_clamp, float alpha, float max_reproj, int sub,
                                      const float *focals_dev, uint64_t seed, uint64_t image0, uint64_t image_stride,
                                      uint32_t max_tries, void *stream, double *rec_dev)
{
    return xl_dsac_backward_rgb_masked_sampled_batch(coords_dev, sb, sc, sy, sx, B, Ho, Wo, mask_dev, XL_DSAC_SAMPLER_REJECT,
                                                     grad_dev, gsb, gsc, gsy, gsx, gt_poses_dev, out_loss_dev, status_dev, n_hyp, thr,
                                                     focal, ppx, ppy, w_rot, w_trans, soft_clamp, alpha, max_reproj, sub, focals_dev,
                                                     seed, image0, image_stride, max_tries, stream, rec_dev);
}

int xl_dsac_backward_rgb_masked_sampled_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                              int B, int Ho, int Wo, const uint8_t *mask_dev, int sampler,
                                              float *grad_dev, int64_t gsb, int64_t gsc, int64_t gsy, int64_t gsx,
                                              const float *gt_poses_dev, double *out_loss_dev, int32_t *status_dev,
                                              int n_hyp, float thr, float focal, float ppx, float ppy,
                                              float w_rot, float w_trans, float soft_clamp, float alpha, float max_reproj, int sub,
                                              const float *focals_dev, uint64_t seed, uint64_t image0, uint64_t image_stride,
                                              uint32_t max_tries, void *stream, double *rec_dev)
{
    if (sampler == XL_DSAC_SAMPLER_REJECT)
        return backward_rgb_launch<kMaskReject>(coords_dev, sb, sc, sy, sx, B, Ho, Wo, mask_dev, grad_dev, gsb, gsc, gsy, gsx,
                                                gt_poses_dev, out_loss_dev, status_dev, n_hyp, thr, focal, ppx, ppy, w_rot, w_trans,
                                                soft_clamp, alpha, max_reproj, sub, focals_dev, seed, image0, image_stride,
                                                max_tries, stream, rec_dev);
    if (sampler == XL_DSAC_SAMPLER_COMPACT)
        return backward_rgb_launch<kMaskCompact>(coords_dev, sb, sc, sy, sx, B, Ho, Wo, mask_dev, grad_dev, gsb, gsc, gsy, gsx,
                                                 gt_poses_dev, out_loss_dev, status_dev, n_hyp, thr, focal, ppx, ppy, w_rot, w_trans,
                                                 soft_clamp, alpha, max_reproj, sub, focals_dev, seed, image0, image_stride,
                                                 max_tries, stream, rec_dev);
    return XL_ERR_ARG;                                           // unknown sampler: before any device work
}

int xl_dsac_forward_rgbd(void) { return XL_ERR_UNSUPPORTED; }
int xl_dsac_backward_rgbd(void) { return XL_ERR_UNSUPPORTED; }

const char *xl_status_string(int status)
{
    switch (status) {
        case XL_OK: return "ok";
        case XL_ERR_ARG: return "invalid argument (null pointer or non-positive size)";
        case XL_ERR_GRID: return "coordinate grid too large for the kernel (Ho*Wo > 16384 or LDS exceeded)";
        case XL_ERR_HIP: return "HIP runtime error (see xl_last_hip_error)";
        case XL_ERR_UNSUPPORTED: return "entry point exported for interface parity but not implemented";
        default: return "unknown status";
    }
}

const char *xl_last_hip_error(void) { return g_hipErr; }

}  // extern "C"
