/*
 * crossloc_dsac.h — C ABI of the MI355X-native DSAC* pose solver (libcrossloc_hip.so).
 *
 * Drop-in boundary for the reference's `dsacstar` extension module
 * (/root/reference/dsacstar/dsacstar.cpp:887-892, PYBIND11_MODULE exporting forward_rgb,
 * backward_rgb, forward_rgbd, backward_rgbd).  The reference binds at a pybind11/ATen level;
 * here the compute core sits behind plain C entry points (pointers + sizes, no torch types) and
 * `dsacstar.py` is the thin Python shim a maintainer would keep in place of the extension.
 *
 * All pointers named *_dev are device (HIP) pointers; *_host are host pointers.
 * Strides are in ELEMENTS (floats), exactly what at::TensorAccessor would honour
 * (dsacstar.cpp:78-79).  Poses are cam->world 4x4, float32, row-major (dsacstar.cpp:172-177).
 * Every function returns 0 on success or a negative xl status (see xl_status_string).
 */
#ifndef CROSSLOC_DSAC_H
#define CROSSLOC_DSAC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XL_OK 0
#define XL_ERR_ARG (-1)        /* null pointer / non-positive size */
#define XL_ERR_GRID (-2)       /* Ho*Wo larger than the kernel supports (16384 cells) */
#define XL_ERR_HIP (-3)        /* a HIP runtime call failed; see xl_last_hip_error() */
#define XL_ERR_UNSUPPORTED (-4)

#define XL_DSAC_MAX_REF_STEPS 100          /* dsacstar.cpp:47 */
#define XL_DSAC_MAX_HYP_TRIES 1000000u     /* dsacstar.cpp:48 */
#define XL_DSAC_DBG_DOUBLES 28             /* per-image debug record, layout below */

/* The launch form xl_dsac_forward_rgb_batch selects for a batch of B images and n_hyp hypotheses: 1 = one fused launch (a
 * workgroup per image: sample, score, select, refine), S > 1 = the split form (S sub-blocks per image sample and score, a second
 * launch selects and refines).  Results are bit-identical across forms; parity tests assert which one they exercised.
 * No reference counterpart (the reference loops over hypotheses with OpenMP, dsacstar.cpp:112-130). */
int xl_dsac_forward_sub_blocks(int B, int n_hyp);

/*
 * Batched forward_rgb: replaces dsacstar_rgb_forward (dsacstar.cpp:63-178) for B independent
 * images in one launch (the reference supports batch 1 only, dsacstar_util.h:161).
 *
 *   coords_dev     [B,3,Ho,Wo] float32 scene coordinates, strides (sb, sc, sy, sx) in elements
 *   out_poses_dev  [B,16] float32, written in place (caller-owned, like outPoseSrc)
 *   n_hyp, thr, focal, ppx, ppy, alpha, max_reproj, sub
 *                  ransacHypotheses, inlierThreshold, focalLength, ppointX, ppointY,
 *                  inlierAlpha, maxReproj, subSampling of dsacstar.cpp:63-73
 *   focals_dev     optional [B] per-image focal lengths (NULL -> `focal` for every image)
 *   seed           RANSAC seed (reference: ThreadRand seed 1305, thread_rand.h:101)
 *   image0, image_stride   global index of image b is image0 + b*image_stride; the sampler is
 *                  keyed on it so results do not depend on batch composition or rank count
 *   max_tries      MAX_HYPOTHESES_TRIES (dsacstar.cpp:48); pass XL_DSAC_MAX_HYP_TRIES to mirror
 *   stream         hipStream_t to launch on (NULL = default stream); asynchronous
 *   cells_dev      optional [B,n_hyp,4] int32: sampled cells (y*Wo + x) of the accepted try
 *   tries_dev      optional [B,n_hyp] int32: tries used (negative: budget exhausted)
 *   scores_dev     optional [B,n_hyp] float64 soft-inlier scores
 *   dbg_dev        optional [B,28] float64: [0] winner, [1] refinement rounds, [2] inliers,
 *                  [3] LM evaluations, [4..15] winner pose before refinement (R row-major, t),
 *                  [16..27] refined pose (world->camera)
 */
int xl_dsac_forward_rgb_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                              int B, int Ho, int Wo, float *out_poses_dev,
                              int n_hyp, float thr, float focal, float ppx, float ppy,
                              float alpha, float max_reproj, int sub, const float *focals_dev,
                              uint64_t seed, uint64_t image0, uint64_t image_stride, uint32_t max_tries,
                              void *stream,
                              int32_t *cells_dev, int32_t *tries_dev, double *scores_dev, double *dbg_dev);

/*
 * The RGB solver over a per-cell validity mask (no reference counterpart): xl_dsac_forward_rgb_batch with the cells the
 * caller rules out taken away from every stage that chooses the hypothesis.  Same kernels (a template instantiation of
 * their own), same launch forms (xl_dsac_forward_sub_blocks), same arguments, plus
 *
 *   mask_dev       [B,Ho,Wo] uint8, contiguous: nonzero = the cell is usable
 *   status_dev     optional [B] int32: 0, or 1 for an image with fewer than four usable cells
 *
 * stage   the mask is kept in LDS as a bit plane of ceil(Ho*Wo / 32) words beside the coordinate planes (676 B at 60x90);
 *         the workgroup counts the usable cells.  A grid whose planes fit in 160 KB only without it returns XL_ERR_GRID.
 * sample  the four cells of a try are drawn exactly as in the unmasked solver (same generator state, same draws).  A try
 *         that drew a masked-out cell is rejected before P3P: its pose is the identity, like a failed P3P, and it counts as
 *         a try.  The first accepted try still wins; the expected number of tries grows as (usable fraction)^-4
 *         (xl_dsac_forward_rgb_masked_sampled_batch offers a sampler that draws from the usable cells only).  After
 *         max_tries the hypothesis is the last try's result - the identity pose if the mask rejected that try.
 * score   the sum runs over the usable cells; the term of a masked-out cell is selected away, never multiplied by zero, so
 *         whatever is stored there (NaN, Inf) reaches neither the sum nor the NaN flag.  The factor stays alpha / Wo / Ho.
 * select  unchanged.
 * refine  a cell is an inlier iff it is usable and its error is below thr; the rest of the refinement is unchanged.
 *
 * With fewer than four usable cells nothing is sampled: the 4x4 identity is written, status 1, and with debug outputs
 * tries 0, scores 0, cells -1, dbg [0] -1, [1..3] 0 and the identity pose in [4..15] and [16..27].
 *
 * Identity A: with an all-ones mask every output equals xl_dsac_forward_rgb_batch's bit for bit.
 * Identity B: the values stored at masked-out cells influence no output bit.
 *
 * XL_ERR_ARG for a null mask and for everything xl_dsac_forward_rgb_batch refuses, before any HIP call.  The backward pass
 * and the two passes behind the solver take the same mask (xl_dsac_backward_rgb_masked_batch, xl_dsac_pose_quality_masked_batch,
 * xl_dsac_refine_pose_masked_batch).  Not covered: the RGB-D solver and its passes and the single-image host entry point.
 */
int xl_dsac_forward_rgb_masked_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                     int B, int Ho, int Wo, const uint8_t *mask_dev, float *out_poses_dev, int32_t *status_dev,
                                     int n_hyp, float thr, float focal, float ppx, float ppy,
                                     float alpha, float max_reproj, int sub, const float *focals_dev,
                                     uint64_t seed, uint64_t image0, uint64_t image_stride, uint32_t max_tries,
                                     void *stream,
                                     int32_t *cells_dev, int32_t *tries_dev, double *scores_dev, double *dbg_dev);

/*
 * The masked RGB solver with a choice of sampler: xl_dsac_forward_rgb_masked_batch plus `sampler` after the mask.
 *
 *   XL_DSAC_SAMPLER_REJECT    the sampler described above; xl_dsac_forward_rgb_masked_batch is this call, bit for bit.
 *   XL_DSAC_SAMPLER_COMPACT   draws the four cells of a try from the usable cells only.  stage: behind the bit plane the kernel
 *                             keeps a rank plane of ceil(Ho*Wo / 32) + 1 words (680 B at 60x90): rank[w] = usable cells in
 *                             mask words 0 .. w-1 (xl_dsac_math.h: mask_rank_plane).  sample: with st the try's generator
 *                             state as before, cell j is the usable cell of rank draw(st, j, nUsable) in row-major order
 *                             (mask_select: a binary search over the rank plane, then a select within the word; integers
 *                             only); the four draws are independent and with replacement.  No try is rejected by the mask,
 *                             so the number of tries stays at the unmasked solver's level whatever the usable fraction, and
 *                             a hypothesis whose tries ran out carries four usable cells and its last P3P result.
 *                             Everything behind the cells (P3P, the four-cell check, tries, score, select, refine, the dead
 *                             image) is the masked solver's.  Conditional on acceptance the reject sampler is uniform over
 *                             usable quadruples, so both samplers draw hypotheses from the same distribution; they do not
 *                             draw the same ones, and Identity A does not hold for this sampler (the unmasked solver draws
 *                             x and y separately).  Identity B holds.  No weights: every usable cell is equally likely.
 *
 * XL_ERR_ARG for any other sampler value and for everything xl_dsac_forward_rgb_masked_batch refuses, XL_ERR_GRID for a grid
 * whose planes fit in 160 KB only without the planes of the chosen sampler; all before any HIP call.  The passes behind the
 * solver take a pose, not a sampler.  Not covered: the RGB-D solver, the single-image host entry point and any weighted draw.
 */
#define XL_DSAC_SAMPLER_REJECT 0
#define XL_DSAC_SAMPLER_COMPACT 1
int xl_dsac_forward_rgb_masked_sampled_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                             int B, int Ho, int Wo, const uint8_t *mask_dev, int sampler,
                                             float *out_poses_dev, int32_t *status_dev,
                                             int n_hyp, float thr, float focal, float ppx, float ppy,
                                             float alpha, float max_reproj, int sub, const float *focals_dev,
                                             uint64_t seed, uint64_t image0, uint64_t image_stride, uint32_t max_tries,
                                             void *stream,
                                             int32_t *cells_dev, int32_t *tries_dev, double *scores_dev, double *dbg_dev);

/*
 * Reference-shaped single-image call on HOST memory: same argument meaning as
 * dsacstar.forward_rgb(sceneCoordinates[1,3,Ho,Wo] CPU, outPose[4,4] CPU, ...)
 * (utils/evaluation.py:162-172).  Copies in, runs the batch kernel with B=1 on `stream`,
 * copies the pose out and synchronises.  Debug outputs are host pointers (nullable).
 */
int xl_dsac_forward_rgb_host(const float *coords_host, int64_t sc, int64_t sy, int64_t sx, int Ho, int Wo,
                             float *out_pose_host, int n_hyp, float thr, float focal, float ppx, float ppy,
                             float alpha, float max_reproj, int sub,
                             uint64_t seed, uint64_t image, uint32_t max_tries,
                             int32_t *cells_host, int32_t *tries_host, double *scores_host, double *dbg_host);

/*
 * Batched backward_rgb: replaces dsacstar_rgb_backward (dsacstar.cpp:200-215, 215-483) for B independent images.
 * Computes the DSAC* expectation of the pose loss over the soft-max distribution of n_hyp hypotheses and ACCUMULATES
 * (+=, like the reference) its gradient w.r.t. the scene coordinates.
 *
 *   coords_dev     [B,3,Ho,Wo] float32, strides (sb, sc, sy, sx) in elements
 *   grad_dev       [B,3,Ho,Wo] float32 gradient, strides (gsb, gsc, gsy, gsx); accumulated in place
 *   gt_poses_dev   [B,16] float32 ground-truth cam->world poses (gtPoseSrc)
 *   out_loss_dev   [B] float64: the expected loss the reference returns
 *   w_rot, w_trans, soft_clamp   wLossRot, wLossTrans, softClamp of dsacstar.cpp:210-212
 *   seed           randomSeed of dsacstar.cpp:215 (keys the counter-based sampler together with the image index)
 *   rec_dev        optional [B,n_hyp,XL_DSAC_BWD_REC] float64 per-hypothesis records for parity tests:
 *                  [0] prob [1] loss [2] active (prob >= 1e-3) [3] accepted inliers [4] path I clamped [5] soft-max
 *                  gradient [6..17] refined pose (R row-major, t) [18..23] dLoss/d(rvec,tvec) [24..29] pinv(JtJ) dLoss^T
 *                  [30..41] support-point gradients [42] max|jacobeanR| [43] max|dPNP| [44..49] sum_c dRepro J
 *                  [50..52] rvec of the refined pose; the rest is workspace
 *   other arguments as in xl_dsac_forward_rgb_batch.  Asynchronous on `stream`.
 */
#define XL_DSAC_BWD_REC 128
int xl_dsac_backward_rgb_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                               int B, int Ho, int Wo,
                               float *grad_dev, int64_t gsb, int64_t gsc, int64_t gsy, int64_t gsx,
                               const float *gt_poses_dev, double *out_loss_dev,
                               int n_hyp, float thr, float focal, float ppx, float ppy,
                               float w_rot, float w_trans, float soft_clamp, float alpha, float max_reproj, int sub,
                               const float *focals_dev, uint64_t seed, uint64_t image0, uint64_t image_stride,
                               uint32_t max_tries, void *stream, double *rec_dev);

/* sub-blocks per image of the backward passes' sample + score launch (0 for a non-positive argument); the results do not depend on it */
int xl_dsac_backward_sub_blocks(int B, int n_hyp);

/*
 * xl_dsac_backward_rgb_batch over the per-cell validity mask of xl_dsac_forward_rgb_masked_batch: the same five launches in
 * template instantiations of their own, the same arguments, plus
 *
 *   mask_dev       [B,Ho,Wo] uint8, contiguous: nonzero = the cell is usable
 *   status_dev     optional [B] int32: 0, or 1 for an image with fewer than four usable cells
 *
 * sample, score   the masked forward solver's (above): the hypotheses, their scores and so the soft-max distribution are the
 *                 ones xl_dsac_forward_rgb_masked_batch chooses from.
 * refine (K1)     a cell is an inlier iff it is usable and below thr, so path I runs over usable cells only.
 * path II (K3)    g6 = sum_c dRepro(c) J_init(c) runs over the usable cells; a masked-out cell's term is selected away, never
 *                 multiplied by zero.  A hypothesis whose tries ran out on a mask-rejected try (identity pose, the last
 *                 draws) carries masked-out cells: their coordinates are not read, the perturbed P3P solves are skipped and
 *                 its dPNP is the zero of a failed solve (rec [30..41] and [43] are 0).
 * assemble (K4)   the gradient of a masked-out cell is neither read nor written; its coordinates are not read.
 * dead image      fewer than four usable cells: out_loss 0, status 1, grad untouched, and with rec_dev the image's records
 *                 all zero.
 *
 * Identity A: with an all-ones mask loss, records and gradient equal xl_dsac_backward_rgb_batch's bit for bit.
 * Identity B: the values stored at masked-out cells influence no bit of loss, record or gradient.
 * Identity C: the gradient at a masked-out cell is the caller's incoming value, bit for bit.
 *
 * XL_ERR_ARG for a null mask and for everything xl_dsac_backward_rgb_batch refuses, XL_ERR_GRID for a grid whose planes fit
 * in 160 KB only without the bit plane; both before any HIP call.  Not covered: the RGB-D backward pass takes no mask.
 */
int xl_dsac_backward_rgb_masked_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                      int B, int Ho, int Wo, const uint8_t *mask_dev,
                                      float *grad_dev, int64_t gsb, int64_t gsc, int64_t gsy, int64_t gsx,
                                      const float *gt_poses_dev, double *out_loss_dev, int32_t *status_dev,
                                      int n_hyp, float thr, float focal, float ppx, float ppy,
                                      float w_rot, float w_trans, float soft_clamp, float alpha, float max_reproj, int sub,
                                      const float *focals_dev, uint64_t seed, uint64_t image0, uint64_t image_stride,
                                      uint32_t max_tries, void *stream, double *rec_dev);

/*
 * xl_dsac_backward_rgb_masked_batch plus `sampler` after the mask (XL_DSAC_SAMPLER_*, as in
 * xl_dsac_forward_rgb_masked_sampled_batch): the sample + score launch runs that sampler, so the pass differentiates the
 * hypotheses the forward call with the same sampler, seed and image keys produced.  Under XL_DSAC_SAMPLER_COMPACT no hypothesis
 * carries a masked-out cell, so K3 never skips the perturbed solves; a hypothesis whose tries ran out is treated as
 * xl_dsac_backward_rgb_batch treats one.  Identities B and C hold for both samplers, Identity A for XL_DSAC_SAMPLER_REJECT only.
 * XL_ERR_ARG for any other sampler value, before any HIP call.
 */
int xl_dsac_backward_rgb_masked_sampled_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                              int B, int Ho, int Wo, const uint8_t *mask_dev, int sampler,
                                              float *grad_dev, int64_t gsb, int64_t gsc, int64_t gsy, int64_t gsx,
                                              const float *gt_poses_dev, double *out_loss_dev, int32_t *status_dev,
                                              int n_hyp, float thr, float focal, float ppx, float ppy,
                                              float w_rot, float w_trans, float soft_clamp, float alpha, float max_reproj, int sub,
                                              const float *focals_dev, uint64_t seed, uint64_t image0, uint64_t image_stride,
                                              uint32_t max_tries, void *stream, double *rec_dev);

/*
 * Per-frame pose quality (no reference counterpart): how far the pose of an image can be trusted.  A stand-alone pass over
 * the scene coordinates at ONE given pose per image - usually the one xl_dsac_forward_rgb_batch wrote, enqueued behind it
 * on the same stream.  One workgroup per image; coordinates are read in place through the strides, so any grid size is
 * accepted (also those the solver refuses with XL_ERR_GRID).  Asynchronous on `stream`: no host synchronisation, no
 * allocation.  A null pointer or a non-positive size returns XL_ERR_ARG before any HIP call.
 *
 *   coords_dev     [B,3,Ho,Wo] float32, strides (sb, sc, sy, sx) in elements
 *   poses_dev      [B,16] float32 cam->world 4x4, row-major; read as the backward pass reads its ground truth (rotation
 *                  made exactly orthonormal, then inverted to world->camera {R, t})
 *   thr, focal, ppx, ppy, alpha, max_reproj, sub, focals_dev   as in xl_dsac_forward_rgb_batch
 *   rows_dev       [B,XL_DSAC_QUALITY_DOUBLES] float64, one row per image:
 *
 *     [0]      n_cells = Ho*Wo
 *     [1]      n_inliers: cells whose clamped float reprojection error e is < thr (the refinement's comparison)
 *     [2]      soft-inlier score at this pose: (alpha / Wo / Ho in float) * sum over all cells of 1 - sigmoid(5/thr (e - thr))
 *     [3],[4]  sum e, sum e^2 over the inliers
 *     [5]      SSE = sum (ru^2 + rv^2) over the inliers, double residuals in pixels
 *     [6]      status: 0 ok; 1 fewer than 4 inliers; 2 JtJ not positive definite; 3 a pose entry (rows 0..2) is not finite
 *     [7]      sigma_px = sqrt(SSE / (2 n_inliers - 6))
 *     [8]      sigma_pos_m = sqrt(trace Sigma_C)
 *     [9]      sigma_rot_deg = sqrt(Sigma_00 + Sigma_11 + Sigma_22) * 180/pi
 *     [10..30] JtJ over the inliers, upper triangle row-major
 *     [31..51] Sigma = sigma_px^2 (JtJ)^-1, upper triangle row-major
 *     [52..57] Sigma_C = A Sigma A^T, upper triangle: covariance of the camera centre C = -R^T t in world coordinates,
 *              A = [ -R^T [t]x , -R^T ] (3x6)
 *     [58]     n_masked: 0.0; xl_dsac_pose_quality_masked_batch: the cells its mask rules out
 *     [59..63] 0.0 (reserved)
 *
 *   Parameters of JtJ and Sigma: (wx, wy, wz, tx, ty, tz) with R' = Exp(w) R, t' = t + d on the world->camera pose, the
 *   increment of the Levenberg-Marquardt refinement.  With status 1 or 2, [7..9] and [31..57] are NaN and the rest is valid;
 *   with status 3 every field except [0] and [6] is NaN.
 *
 * xl_dsac_pose_quality_masked_batch is the same pass over the per-cell validity mask of xl_dsac_forward_rgb_masked_batch
 * (mask_dev [B,Ho,Wo] uint8 contiguous, nonzero = usable; usually the mask the solver read): the mask byte of a cell is read
 * before anything else of it, and a masked-out cell is skipped - its coordinate is not loaded, it is no inlier and adds to no
 * sum.  [0] stays Ho*Wo, [1] and [3..57] run over usable cells only, [2] sums the usable cells with the same factor
 * alpha / Wo / Ho (the masked solver's score), [58] counts the masked-out cells (NaN with status 3, like its neighbours).
 * With an all-ones mask every output equals xl_dsac_pose_quality_batch's bit for bit; the values stored at masked-out cells
 * influence no output bit.  A null mask is XL_ERR_ARG, before any HIP call.
 */
#define XL_DSAC_QUALITY_DOUBLES 64
int xl_dsac_pose_quality_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                               int B, int Ho, int Wo, const float *poses_dev /* [B,16] cam->world */,
                               float thr, float focal, float ppx, float ppy, float alpha, float max_reproj, int sub,
                               const float *focals_dev, double *rows_dev /* [B,64] */, void *stream);
int xl_dsac_pose_quality_masked_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                      int B, int Ho, int Wo, const uint8_t *mask_dev, const float *poses_dev /* [B,16] cam->world */,
                                      float thr, float focal, float ppx, float ppy, float alpha, float max_reproj, int sub,
                                      const float *focals_dev, double *rows_dev /* [B,64] */, void *stream);

/*
 * Batched RGB-D forward pass: the solver of dsacstar_rgbd_forward (dsacstar.cpp:495-612) for B independent images in one
 * launch, one 256-thread workgroup per image.  Every cell has a scene coordinate X (world, metres) and a camera coordinate
 * p (camera frame, metres); a pose hypothesis is the closed-form rigid (Kabsch) fit p = R X + t of three sampled cells.
 *
 *   coords_dev     [B,3,Ho,Wo] float32 scene coordinates, strides (sb, sc, sy, sx) in elements
 *   cam_dev        [B,3,Ho,Wo] float32 camera coordinates, strides (mb, mc, my, mx), or NULL
 *   depth_dev      [B,Ho,Wo] float32 depth along the optical axis, strides (db, dy, dx), or NULL.  EXACTLY ONE of cam_dev and
 *                  depth_dev is non-null (otherwise XL_ERR_ARG).  In depth form the kernel forms the camera coordinate of cell
 *                  (y, x) itself, in float32 without contraction:  px = x*sub + sub/2, py = y*sub + sub/2 (integers),
 *                  p = ( ((float)px - ppx) / f * d,  ((float)py - ppy) / f * d,  d )  with f = focals_dev[b] or `focal`;
 *                  a camera tensor built by the same formula gives the same bits.  focal, ppx, ppy, sub and focals_dev are
 *                  read in depth form only.
 *   thr, max_dist  inlierThreshold and maxDistError in CENTIMETRES: distances (metres) are multiplied by 100 before they are
 *                  compared or clamped (dsacstar_util.h:296, 502)
 *   alpha          inlierAlpha
 *   other arguments as in xl_dsac_forward_rgb_batch.  Asynchronous on `stream`.
 *
 * Valid cells: a cell is valid iff its camera z is nonzero (zero depth = no measurement).  DEVIATION: the reference tests
 * channel 0 three times (dsacstar.cpp:522-524), which drops the column x_cam == 0 of an odd-width grid.  The valid list is
 * ordered x-major (x outer, y inner) like the reference's validPts; draw k of the sampler means its k-th entry.
 * Sampling: try t of hypothesis h draws three entries draw(try_state(imageKey, h, t), j, nValid), j = 0..2 (repeats allowed),
 * fits Kabsch on the three pairs and accepts iff all three residuals |p - (R X + t)| * 100 are < thr; the first accepted try
 * wins; a hypothesis that exhausts max_tries keeps its last fit and is still scored.  With nValid == 0 nothing is sampled
 * and the identity pose is written.
 * Kabsch: centroids, centred cross-covariance A = sum (p - c_p)(X - c_X)^T, R = U diag(1, 1, det(U V^T)) V^T, t = c_p - R c_X,
 * in double (Horn's quaternion form; rank-deficient A gives one of the optimal proper rotations, A = 0 the identity).
 * Score: err = min((float)(|p - (R X + t)| * 100), max_dist) for valid cells and max_dist for invalid ones, which DO enter the
 * sum; score = (alpha / Wo / Ho in float) * sum over all Ho*Wo cells of 1 - sigmoid(5/thr (err - thr)); first maximum wins.
 * Refinement (dsacstar_util.h:611-677): inliers err < thr (float compare); stop when their number is <= the best so far
 * (initially 3); else re-fit Kabsch on all inliers; at most XL_DSAC_MAX_REF_STEPS rounds.
 * out_poses_dev: the inverse rigid transform, float32 cam->world 4x4, as xl_dsac_forward_rgb_batch writes it.
 *
 * max_tries <= XL_DSAC_RGBD_MAX_TRIES (the try counter is 32 bits wide and advances in steps of 64; tries_dev reports the
 * exhausted budget as a negative int), otherwise XL_ERR_ARG.
 * Limit: Ho*Wo <= XL_DSAC_RGBD_MAX_CELLS (the image is staged in the 160 KB LDS of one CU at 26 bytes per cell); larger grids
 * return XL_ERR_GRID before any launch.  Argument errors are detected before any HIP call.
 *
 *   cells_dev      optional [B,n_hyp,3] int32: cells (y*Wo + x) of the accepted try (-1 when nothing was sampled)
 *   tries_dev      optional [B,n_hyp] int32: tries used (negative: budget exhausted; 0: nothing sampled)
 *   scores_dev     optional [B,n_hyp] float64 soft-inlier scores
 *   dbg_dev        optional [B,XL_DSAC_RGBD_DBG_DOUBLES] float64: [0] winner, [1] nValid, [2] refinement rounds, [3] inliers of
 *                  the last fitted round, [4..12] refined R row-major, [13..15] refined t (world->camera)
 */
#define XL_DSAC_RGBD_MAX_CELLS 6144
#define XL_DSAC_RGBD_DBG_DOUBLES 16
#define XL_DSAC_RGBD_MAX_TRIES 2147483584u          /* 2^31 - 64 */
int xl_dsac_forward_rgbd_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                               const float *cam_dev, int64_t mb, int64_t mc, int64_t my, int64_t mx,
                               const float *depth_dev, int64_t db, int64_t dy, int64_t dx,
                               int B, int Ho, int Wo, float *out_poses_dev,
                               int n_hyp, float thr, float alpha, float max_dist,
                               float focal, float ppx, float ppy, int sub, const float *focals_dev,
                               uint64_t seed, uint64_t image0, uint64_t image_stride, uint32_t max_tries,
                               void *stream,
                               int32_t *cells_dev, int32_t *tries_dev, double *scores_dev, double *dbg_dev);

/*
 * Batched RGB-D backward pass: dsacstar_rgbd_backward (dsacstar.cpp:631-885) for B independent images: the DSAC* expectation
 * of the pose loss over the hypothesis distribution, written to out_loss_dev [B] (float64), and its gradient w.r.t. the scene
 * coordinates, ACCUMULATED (+=) into grad_dev ([B,3,Ho,Wo] float32, strides (gsb, gsc, gsy, gsx) in elements).  Five launches
 * on `stream`, no host synchronisation; the workspace comes from hipMallocAsync / hipFreeAsync on `stream`.
 *
 *   coords / cam / depth, thr, alpha, max_dist, focal, ppx, ppy, sub, focals_dev, seed, image0, image_stride, max_tries
 *                  as in xl_dsac_forward_rgbd_batch; the same limits (XL_ERR_ARG, XL_ERR_GRID) are checked before any HIP call
 *   gt_poses_dev   [B,16] float32 cam->world 4x4, row-major
 *   w_rot, w_trans, soft_clamp   weights of the pose loss and its soft clamp, as in xl_dsac_backward_rgb_batch
 *   rec_dev        optional [B,n_hyp,XL_DSAC_RGBD_BWD_REC] float64 per-hypothesis records (layout below)
 *
 * Sampling, scores and the selection distribution are the forward pass's: the same sampler keys with `seed`, the same score
 * bits.  p = softmax(scores); a hypothesis with p < 1e-3 is inactive: it enters the expectation with the loss of its unrefined
 * pose and gets no gradient.  An active hypothesis is refined with the forward pass's refinement loop; its loss is the pose
 * loss (dsacstar_loss.h:47-88) of the refined pose.  Expected loss E = sum_h p_h loss_h; soft-max gradient
 * dE/dscore_h = p_h (loss_h - E).
 *
 * Gradient of E w.r.t. the scene coordinate X of a valid cell (an invalid cell gets nothing), hypotheses added in ascending
 * order in float:  acc = (float)((double)acc + (p_h * gI + gII)).
 *   Path I  (through the refined pose): the closed-form adjoint of the Horn/Kabsch fit of the last fitted refinement round:
 *           gI = H^T (p - c_p) - v for the cells of that round's inlier set, H = dloss/dA, v = R^T g_t / n.  dloss/dR and g_t =
 *           dloss/dt are taken from dLoss (dsacstar_loss.h:99-212) with all its quirks.  None when no round was fitted.
 *   Path II (through the score): w = -s (1 - s) (5 / thr) dE/dscore_h (alpha / Wo / Ho) per valid cell, s the sigmoid of the
 *           score term, d^ = d / (|d| + 1e-8) of the metre residual d = p - (R X + t) under the UNREFINED pose; a cell whose
 *           unclamped float error exceeds max_dist has w = 0.  Direct term gII = w (-100 R^T d^); the three drawn cells also get
 *           the adjoint of the minimal fit for G_R = sum w (-100 d^ X^T), g_t = sum w (-100 d^) (a repeated draw: every one of
 *           its columns).
 * DEVIATIONS from the reference, beside those of the forward pass:
 *   - the factor 100: the reference differentiates the metre error while its score uses centimetres
 *     (dsacstar_derivative.h:443-458 against dsacstar_util.h:502); here the gradient is the derivative of the score computed.
 *   - the Kabsch derivative is analytic everywhere (the reference: SVD backward, central differences for a zero singular
 *     value, i.e. for every three-point set).
 *   - eigen-gap guard: a fit whose (lambda_top - lambda_second) / max |lambda| of Horn's 4x4 is <= 1e-8 is not unique
 *     (collinear or repeated points): the hypothesis contributes nothing through that fit (path I: gI = 0; path II: the
 *     support-point gradients are 0, the direct term stays) and the record flags it.
 *   - path-II guard: the same when the largest entry of the 3x9 rotation Jacobian d omega / d X of the support points
 *     (delta R = [delta omega]x R) exceeds 10 rad/m.  The reference's clamp max |d(rvec, tvec)/dX| > 10
 *     (dsacstar_derivative.h:638) is NOT taken over: its tvec rows scale with the distance of the scene from the origin.
 *
 * Record of hypothesis h (XL_DSAC_RGBD_BWD_REC = 64 doubles); an inactive hypothesis has [0], [1] and zeros:
 *     [0] prob   [1] loss   [2] active   [3] inliers of the last fitted round (0 if none)   [4] path-I guard flag
 *     [5] soft-max gradient dE/dscore    [6..17] refined pose: R row-major, t (world->camera)
 *     [18..26] H row-major   [27..29] v   [30..32] c_p of the final inlier set
 *     [33..41] support-point gradients [draw j][xyz]   [42] max |d omega / d X| over the support points
 *     [43] path-II guard flag (eigen-gap of the minimal fit, the rotation Jacobian, or nothing sampled)
 *     [44..52] G_R row-major and [53..55] g_t: the twelve score sums
 *     [56] relative eigen-gap of the refined fit   [57] of the minimal fit   [58..63] 0
 */
#define XL_DSAC_RGBD_BWD_REC 64
int xl_dsac_backward_rgbd_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                const float *cam_dev, int64_t mb, int64_t mc, int64_t my, int64_t mx,
                                const float *depth_dev, int64_t db, int64_t dy, int64_t dx,
                                int B, int Ho, int Wo,
                                float *grad_dev, int64_t gsb, int64_t gsc, int64_t gsy, int64_t gsx,
                                const float *gt_poses_dev, double *out_loss_dev,
                                int n_hyp, float thr, float alpha, float max_dist,
                                float w_rot, float w_trans, float soft_clamp,
                                float focal, float ppx, float ppy, int sub, const float *focals_dev,
                                uint64_t seed, uint64_t image0, uint64_t image_stride, uint32_t max_tries,
                                void *stream, double *rec_dev);

/*
 * Per-frame pose quality of the RGB-D solver: how far ONE given pose per image can be trusted, rated by its metric 3-D
 * residuals.  A stand-alone pass (one 256-thread workgroup per image, two walks over the cells, nothing staged in LDS: any grid
 * size, XL_DSAC_RGBD_MAX_CELLS does not apply), the sibling of xl_dsac_pose_quality_batch; usually enqueued on the stream of
 * xl_dsac_forward_rgbd_batch directly behind it, on the poses that call wrote.
 *
 *   coords / cam / depth with their strides, thr, alpha, max_dist (centimetres), focal, ppx, ppy, sub, focals_dev
 *                  as in xl_dsac_forward_rgbd_batch: EXACTLY ONE of cam_dev and depth_dev is non-null, the depth form builds the
 *                  camera coordinate with the same float formula and bits
 *   poses_dev      [B,16] float32 cam->world 4x4, row-major; read as the world->camera pose {R, t} the backward passes derive
 *   rows_dev       [B,XL_DSAC_QUALITY_DOUBLES] float64, one row per image, all 64 written
 *
 * Model.  m = R X + t is the predicted camera point of a cell (X its scene coordinate), r = p - m its residual in metres (p
 * its camera coordinate).  A cell is valid iff its camera z != 0; a valid cell is an inlier iff
 * e = min((float)(|r| * 100), max_dist) < thr, the float comparison of the solver's refinement.  The covariance is that of the
 * unweighted rigid least-squares fit the refinement performs on the n inliers, with isotropic noise of sigma metres per axis:
 * sigma^2 = SSE / (3 n - 6).  Everything is accumulated about the inlier centroid c of m in the camera frame (scene coordinates
 * lie up to 1200 m from the world origin; the uncentred normal matrix has a condition number of 1e6 to 1e9): with u = m - c and
 * C = sum u u^T the fit decouples into a rotation about c with information M = tr(C) I - C (3x3) and the centroid translation
 * tau with information n I.  JtJ and Sigma are reported in the parameters of the RGB row, (wx, wy, wz, tx, ty, tz) with
 * R' = Exp(w) R, t' = t + d, through d = tau - [t - c]x w:  G = [[I, 0], [-[t - c]x, I]],
 * Sigma = G diag(sigma^2 M^-1, sigma^2 / n I) G^T,  JtJ = G^-T diag(M, n I) G^-1  (= sum J^T J, J = [[R X]x, -I]).
 * Degenerate: inliers on one line or at one point leave M singular; M is factored by Cholesky and a pivot that is not above
 * 1e-12 times its diagonal entry (or is not finite) is a breakdown (rounding leaves about 3e-16, three neighbouring cells of a
 * grid row 3e-6 or more on the test scenes).
 *
 * Row of image b (doubles; the RGB row's positions wherever the meaning is the same):
 *     [0]      n_cells = Ho * Wo
 *     [1]      n_inliers
 *     [2]      soft score of the pose over ALL cells, invalid ones at the error max_dist: the solver's score at this pose
 *     [3]      sum of e over the inliers (centimetres)        [4]  sum of e^2 over the inliers
 *     [5]      SSE = sum |r|^2 over the inliers, m^2
 *     [6]      status: 0 ok; 1 fewer than 3 inliers (no valid cell included); 2 degenerate (see above); 3 a pose entry is not finite
 *     [7]      sigma_m = sqrt(SSE / (3 n - 6)), metres per axis
 *     [8]      sigma_pos_m = sqrt(trace Sigma_C)
 *     [9]      sigma_rot_deg = sqrt(Sigma_00 + Sigma_11 + Sigma_22) * 180/pi
 *     [10..30] JtJ over the inliers, upper triangle row-major
 *     [31..51] Sigma, upper triangle row-major
 *     [52..57] Sigma_C = A Sigma A^T, upper triangle: covariance of the camera centre, as in the RGB row
 *     [58]     n_valid
 *     [59..63] 0.0 (reserved)
 *   With status 1 or 2, [7..9] and [31..57] are NaN and the rest is valid; with status 3 every field except [0] and [6] is NaN.
 *
 * XL_ERR_ARG (before any HIP call): a null coords / poses / rows pointer, neither or both of cam_dev and depth_dev, B, Ho, Wo or
 * sub not positive.  XL_ERR_GRID: Ho * Wo does not fit the int cell index.
 */
int xl_dsac_pose_quality_rgbd_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                    const float *cam_dev, int64_t mb, int64_t mc, int64_t my, int64_t mx,
                                    const float *depth_dev, int64_t db, int64_t dy, int64_t dx,
                                    int B, int Ho, int Wo, const float *poses_dev /* [B,16] cam->world */,
                                    float thr, float alpha, float max_dist,
                                    float focal, float ppx, float ppy, int sub, const float *focals_dev,
                                    double *rows_dev /* [B,64] */, void *stream);

/*
 * Uncertainty-weighted pose refinement (no reference counterpart): ONE given pose per image - usually the one
 * xl_dsac_forward_rgb_batch wrote, enqueued behind it on the same stream - is re-fitted over its inliers by iteratively
 * re-weighted Levenberg-Marquardt, every cell weighted by the standard deviation the network predicts for it.  A stand-alone
 * pass, one 256-thread workgroup per image; the solver's kernels are not involved.  Asynchronous on `stream`: no host
 * synchronisation, no allocation.
 *
 *   coords_dev     [B,3,Ho,Wo] float32, strides (sb, sc, sy, sx) in elements
 *   sigma_dev      [B,Ho,Wo] float32 standard deviation of each cell's scene coordinate in metres, strides (gb, gy, gx) - the
 *                  fourth channel of a network trained with the MLE coordinate loss, which models the error of a cell as an
 *                  isotropic 3-D Gaussian of that sigma - or NULL: every weight is 1, a plain re-fit over the inliers
 *   poses_dev      [B,16] float32 cam->world 4x4, read as xl_dsac_pose_quality_batch reads it
 *   out_poses_dev  [B,16] float32 cam->world, the refined pose, formed from the double pose as the solver forms its output;
 *                  the input's 16 floats bit for bit when no round completed (status != 0).  May be poses_dev itself.
 *   rows_dev       [B,XL_DSAC_REFINE_DOUBLES] float64, one row per image, all 64 written
 *   w2c_dev        optional [B,12] float64: the refined world->camera pose, R row-major then t (the pose read from poses_dev
 *                  when no round completed; NaN with status 3)
 *   thr, focal, ppx, ppy, max_reproj, sub, focals_dev   as in xl_dsac_forward_rgb_batch
 *   s0             floor of the residual's standard deviation in pixels (the pixel noise of a perfectly known cell), > 0
 *   max_rounds     1 .. XL_DSAC_REFINE_MAX_ROUNDS
 *
 * Model.  A round starts at pose P_k.  Its inlier set is { i : e_i(P_k) < thr } with e the solver's clamped float reprojection
 * error and float comparison; with z_i the camera depth of cell i at P_k (z_i == 0 read as 1) its weight is
 * w_i = 1 / (s0^2 + (f sigma_i / z_i)^2).  A cell whose sigma is not finite or is negative is left out of every set and
 * counted in [5].  Set and weights stay fixed for the whole round (weights that followed the moving pose would favour large
 * depths and bias the estimating equation sum w_i J_i^T r_i = 0) while the solver's Levenberg-Marquardt (damping from 1e-3,
 * accept test on the weighted cost, 20 iterations at most, the same step-size stop) minimises sum w_i |r_i|^2 over the
 * increment R' = Exp(w) R, t' = t + d of the world->camera pose.  The rounds stop when a round's set equals the previous
 * round's (converged), after max_rounds, when the set has fewer than 4 cells, or when a solve breaks down or the pose stops
 * being finite; the pose of the last completed round is the result.  With sigma_dev == NULL the weights are 1; a map of zeros
 * with s0 == 1 gives the bits of the NULL form.
 *
 * Row of image b (doubles; the pose-quality row's positions wherever the meaning is the same):
 *     [0]      n_cells = Ho * Wo
 *     [1]      inliers of the last completed round
 *     [2]      inliers at the input pose
 *     [3]      weighted cost sum w |r|^2 at the input pose (the first evaluation)
 *     [4]      weighted cost at the output pose, over the last completed round's set and weights
 *     [5]      cells left out for an unusable sigma
 *     [6]      status: 0 ok; 1 fewer than 4 inliers at the input pose; 2 the first round failed (normal matrix not positive
 *              definite, LM breakdown or a pose that is not finite); 3 an input pose entry (rows 0..2) is not finite
 *     [7]      chi = sqrt([4] / (2 [1] - 6)): 1 when sigma is calibrated, > 1 when the network is over-confident
 *     [8]      sigma_pos_m = sqrt(trace Sigma_C)
 *     [9]      sigma_rot_deg = sqrt(Sigma_00 + Sigma_11 + Sigma_22) * 180/pi
 *     [10..30] J^T W J at the output pose, upper triangle row-major
 *     [31..51] Sigma = chi^2 (J^T W J)^-1, upper triangle row-major
 *     [52..57] Sigma_C, covariance of the camera centre as in the pose-quality row
 *     [58]     rounds completed       [59] normal-equation evaluations       [60] converged (1 / 0)
 *     [61]     rotation between input and output pose, degrees               [62] distance of their camera centres, metres
 *     [63]     n_masked: 0.0; xl_dsac_refine_pose_masked_batch: the cells its mask rules out
 *   NaN pattern as in the pose-quality row.  With status 1 or 2 no round completed: [1] = [2], [4] = [3] and [10..30] come from
 *   the first evaluation at the input pose, [7..9] and [31..57] are NaN, [58] and [60..62] are 0.  With status 3 every field
 *   except [0] and [6] is NaN.  With status 0, [8], [9] and [31..57] are NaN if J^T W J at the output pose has no Cholesky factor.
 *   The hard gate at thr truncates the residuals of cells whose sigma in pixels approaches thr, so chi reads below 1 on honest
 *   sigma there, and an s0 above the true pixel noise makes Sigma conservative.
 *
 * The image is staged in the LDS of one CU as four float planes: Ho * Wo <= XL_DSAC_REFINE_MAX_CELLS, else XL_ERR_GRID.
 * XL_ERR_ARG: a null coords / poses / out_poses / rows pointer, B, Ho, Wo or sub not positive, s0 not above 0, max_rounds out
 * of range.  Both are returned before any HIP call.
 *
 * xl_dsac_refine_pose_masked_batch is the same pass over the per-cell validity mask of xl_dsac_forward_rgb_masked_batch
 * (mask_dev [B,Ho,Wo] uint8 contiguous, nonzero = usable; usually the mask the solver read).  No plane is added to the LDS, so
 * the cell limit is the same: every thread keeps the mask bytes of its own cells as a 64-bit word.  A masked-out cell is not
 * staged and is passed by in every round before its sigma is checked and before its error is formed: it is in no inlier set
 * and neither its coordinate nor its sigma enters any arithmetic.  [5] counts usable cells only, [63] the masked-out cells
 * (NaN with status 3); everything else keeps its meaning.  An image with fewer than four usable cells has status 1 and its
 * input pose comes back bit for bit (behind the masked solver: the identity it wrote).  With an all-ones mask every output
 * equals xl_dsac_refine_pose_batch's bit for bit; the values stored at masked-out cells influence no output bit.  A null mask
 * is XL_ERR_ARG, before any HIP call.
 */
#define XL_DSAC_REFINE_DOUBLES 64
#define XL_DSAC_REFINE_MAX_CELLS 10128      /* (160 KiB - reduction scratch) / 16 bytes per cell */
#define XL_DSAC_REFINE_MAX_ROUNDS 16
int xl_dsac_refine_pose_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                              const float *sigma_dev, int64_t gb, int64_t gy, int64_t gx,
                              int B, int Ho, int Wo, const float *poses_dev /* [B,16] cam->world */,
                              float *out_poses_dev /* [B,16] */, double *rows_dev /* [B,64] */, double *w2c_dev /* [B,12] or NULL */,
                              float thr, float focal, float ppx, float ppy, float max_reproj, int sub,
                              const float *focals_dev, float s0, int max_rounds, void *stream);
int xl_dsac_refine_pose_masked_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                     const float *sigma_dev, int64_t gb, int64_t gy, int64_t gx,
                                     int B, int Ho, int Wo, const uint8_t *mask_dev, const float *poses_dev /* [B,16] cam->world */,
                                     float *out_poses_dev /* [B,16] */, double *rows_dev /* [B,64] */, double *w2c_dev /* [B,12] or NULL */,
                                     float thr, float focal, float ppx, float ppy, float max_reproj, int sub,
                                     const float *focals_dev, float s0, int max_rounds, void *stream);

/*
 * Ray-aware uncertainty-weighted pose refinement behind the RGB-D solver (no reference counterpart): ONE given pose per image -
 * usually the one xl_dsac_forward_rgbd_batch wrote, enqueued behind it on the same stream - is re-fitted over its inliers by
 * Levenberg-Marquardt under a 3x3 information matrix per cell.  The sibling of xl_dsac_refine_pose_batch and of
 * xl_dsac_pose_quality_rgbd_batch: a stand-alone pass, one 256-thread workgroup per image, nothing staged in LDS (any grid size,
 * XL_DSAC_RGBD_MAX_CELLS does not apply); the solver's kernels are not involved.  Asynchronous on `stream`: no host
 * synchronisation, no allocation.
 *
 *   coords / cam / depth with their strides, thr, max_dist (centimetres), focal, ppx, ppy, sub, focals_dev
 *                  as in xl_dsac_forward_rgbd_batch: EXACTLY ONE of cam_dev and depth_dev is non-null, the depth form builds the
 *                  camera coordinate with the same float formula and bits
 *   sigma_dev      [B,Ho,Wo] float32 standard deviation of each cell's scene coordinate in metres, strides (gb, gy, gx) - the
 *                  uncertainty channel of the coordinate network - or NULL: sigma = 0
 *   depth_sigma_dev  [B,Ho,Wo] float32 standard deviation of each cell's depth (camera z) in metres, strides (zb, zy, zx) - the
 *                  uncertainty channel of a depth network - or NULL: sigma_z = 0
 *   poses_dev      [B,16] float32 cam->world 4x4, read as xl_dsac_pose_quality_rgbd_batch reads it
 *   out_poses_dev  [B,16] float32 cam->world, the refined pose, formed from the double pose as the solver forms its output;
 *                  the input's 16 floats bit for bit when no round completed (status != 0).  May be poses_dev itself.
 *   rows_dev       [B,XL_DSAC_REFINE_DOUBLES] float64, one row per image, all 64 written
 *   w2c_dev        optional [B,12] float64: the refined world->camera pose, R row-major then t (the pose read from poses_dev
 *                  when no round completed; NaN with status 3)
 *   s0             floor of the scene coordinate's standard deviation in metres, > 0
 *   depth_rel      k: relative depth noise (0.01: one per cent of the depth), >= 0 and finite
 *   max_rounds     1 .. XL_DSAC_REFINE_MAX_ROUNDS
 *
 * Model.  m = R X + t is the predicted camera point of a cell (X its scene coordinate), r = p - m its residual in metres (p its
 * camera coordinate).  A cell is valid iff its camera z != 0.  A valid cell is an inlier at pose P_k iff
 * e = min((float)(|r| * 100), max_dist) < thr, the solver's clamp and float comparison.  Noise of cell i: the scene coordinate
 * has isotropic noise a_i = s0^2 + sigma_i^2; the depth noise acts along the unit ray rho_i = p_i / |p_i| with variance
 * b_i = (sigma_z,i^2 + (k z_i)^2) |p_i|^2 / z_i^2 (an error dz of the depth moves p = z (x/z, y/z, 1) by dz |p| / z along the
 * ray).  The covariance of r_i is a_i I + b_i rho_i rho_i^T and, by Sherman-Morrison, its information matrix is
 * W_i = (I - b_i / (a_i + b_i) rho_i rho_i^T) / a_i.  rho, a and b belong to the measurement: they do not depend on the pose and
 * are fixed for the whole call.  A valid cell whose sigma or sigma_z is negative or not finite is left out of every inlier set and
 * counted in [5].  Plain form: with sigma_dev == NULL, depth_sigma_dev == NULL and depth_rel == 0 every W_i is the identity and
 * s0 is not used - a plain re-fit over the inliers, and chi is the residual standard deviation in metres per axis, the RGB-D
 * quality row's sigma_m.  Maps of zeros with s0 == 1 and depth_rel == 0 give the bits of the plain form.
 *
 * Rounds.  The inlier set is fixed per round and taken at the round's start pose P_k.  Within a round the solver's
 * Levenberg-Marquardt (damping from 1e-3, accept test on the cost, 20 iterations at most, the same step-size stop) minimises
 * sum r^T W r over the 6-parameter increment.  The rounds stop when a round's set equals the previous round's (converged), after
 * max_rounds, when fewer than 3 inliers remain, when the normal matrix has no sound Cholesky factor (a pivot not above 1e-12
 * times its diagonal entry: inliers on one line) or LM breaks down, or on a pose that is not finite.  The result is the pose of
 * the last completed round.  The row rates the pose the caller receives: after the last round the normal equations are
 * evaluated once more, over that round's set, at the float32 matrix written to out_poses_dev read back as every pass reads a
 * pose (counted in [59]); [4], [7..57], [61] and [62] refer to that pose, so a xl_dsac_pose_quality_rgbd_batch call behind this
 * one rates the same pose.  w2c_dev keeps the unrounded double pose.
 *
 * Conditioning.  Scene coordinates lie up to 1200 m from the world origin; the uncentred normal matrix has a condition number of
 * 1e7 to 1e9.  Every normal equation is accumulated about the round's inlier centroid c of m, and the step is solved in
 * (rotation w about c, centroid translation tau): m' = Exp(w) (m - c) + c + tau, J = [[m - c]x, -I].  JtJ and Sigma are reported
 * in the parameters of the other rows, (wx, wy, wz, tx, ty, tz) with R' = Exp(w) R, t' = t + d, through d = tau - [t - c]x w, the
 * G of the RGB-D quality row: G = [[I, 0], [-[t - c]x, I]], JtJ = G^-T (J^T W J) G^-1 (= sum J^T W J with J = [[R X]x, -I]: the
 * lever arm of the rotation is R X, not m), Sigma = G (chi^2 (J^T W J)^-1) G^T.
 *
 * Row of image b (doubles; the positions of the xl_dsac_refine_pose_batch row):
 *     [0]      n_cells = Ho * Wo
 *     [1]      inliers of the last completed round
 *     [2]      inliers at the input pose
 *     [3]      cost sum r^T W r at the input pose (the first evaluation)
 *     [4]      cost at the output pose, over the last completed round's set
 *     [5]      valid cells left out for an unusable sigma or sigma_z
 *     [6]      status: 0 ok; 1 fewer than 3 inliers at the input pose; 2 the first round failed (normal matrix degenerate, LM
 *              breakdown or a pose that is not finite); 3 an input pose entry (rows 0..2) is not finite
 *     [7]      chi = sqrt([4] / (3 [1] - 6)): 1 when sigma, sigma_z and k are calibrated; metres per axis in the plain form
 *     [8]      sigma_pos_m = sqrt(trace Sigma_C)
 *     [9]      sigma_rot_deg = sqrt(Sigma_00 + Sigma_11 + Sigma_22) * 180/pi
 *     [10..30] J^T W J at the output pose, upper triangle row-major
 *     [31..51] Sigma = chi^2 (J^T W J)^-1, upper triangle row-major
 *     [52..57] Sigma_C, covariance of the camera centre as in the pose-quality row
 *     [58]     rounds completed       [59] normal-equation evaluations       [60] converged (1 / 0)
 *     [61]     rotation between input and output pose, degrees               [62] distance of their camera centres, metres
 *     [63]     n_valid
 *   NaN pattern as in the sibling.  With status 1 or 2 no round completed: [1] = [2], [4] = [3] and [10..30] come from the first
 *   evaluation at the input pose, [7..9] and [31..57] are NaN, [58] and [60..62] are 0.  With status 3 every field except [0] and
 *   [6] is NaN.  With status 0, [8], [9] and [31..57] are NaN if J^T W J at the output pose has no Cholesky factor.
 *   The gate stays the solver's Euclidean one: it truncates the residuals of cells whose noise approaches thr, so chi reads
 *   below 1 on honest sigma there, and an s0 above the true floor makes Sigma conservative.
 *
 * XL_ERR_ARG (before any HIP call): a null coords / poses / out_poses / rows pointer, neither or both of cam_dev and depth_dev, B,
 * Ho, Wo or sub not positive, s0 not above 0, depth_rel negative or not finite, max_rounds out of range.  XL_ERR_GRID: Ho * Wo does
 * not fit the int cell index.
 */
int xl_dsac_refine_pose_rgbd_batch(const float *coords_dev, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                                   const float *cam_dev, int64_t mb, int64_t mc, int64_t my, int64_t mx,
                                   const float *depth_dev, int64_t db, int64_t dy, int64_t dx,
                                   const float *sigma_dev, int64_t gb, int64_t gy, int64_t gx,
                                   const float *depth_sigma_dev, int64_t zb, int64_t zy, int64_t zx,
                                   int B, int Ho, int Wo, const float *poses_dev /* [B,16] cam->world */,
                                   float *out_poses_dev /* [B,16] */, double *rows_dev /* [B,64] */, double *w2c_dev /* [B,12] or NULL */,
                                   float thr, float max_dist, float focal, float ppx, float ppy, int sub,
                                   const float *focals_dev, float s0, float depth_rel, int max_rounds, void *stream);

/* The reference-shaped single-image RGB-D entries (dsacstar.cpp:889-891) are not wired to the solver above yet: they
 * return XL_ERR_UNSUPPORTED. */
int xl_dsac_forward_rgbd(void);
int xl_dsac_backward_rgbd(void);

const char *xl_status_string(int status);
const char *xl_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif
