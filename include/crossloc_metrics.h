/*
 * crossloc_metrics.h — C ABI of the fused per-image evaluation metrics (libcrossloc_hip.so).
 *
 * Replaces the PyTorch-eager bodies of the reference's evaluation metrics
 *   depth_eval      utils/evaluation.py:247-267
 *   normal_eval     utils/evaluation.py:294-316 (+ utils/learning.py:417-440 angle helpers)
 *   semantic_eval   utils/evaluation.py:339-414 (arg-max + SemanticsEvaluator._generate_matrix)
 * with one streaming launch over [B, C, n_cells] plus one small finalisation launch each.  The result is one ROW PER IMAGE
 * on the device; the reference's per-batch (depth, normal) and per-image (semantics) figures are sums / ratios of rows, so
 * any grouping of frames can be reproduced on the host whatever batch size or rank count produced the rows.
 *
 *   depth      rows double[B,3]  = { sum |d-g|*m/g, sum (|d-g|*m)^2, sum m }            m = (g != nodata)
 *   normal     rows double[B,2]  = { sum angle_deg*m, sum m }                          m = no label channel == nodata
 *   semantics  counts int64[B,36]: 6x6 confusion matrix, rows = ground truth, over cells with 0 <= label < 6 (tested on the
 *              float label, which is truncated to int afterwards); class = FIRST arg-max of the 6 logits (ties take the lowest
 *              index); class_map (optional, may be NULL) uint8[B,n_cells] receives the class of every cell.
 *
 * Predictions: float32 device pointer with an image stride and a channel stride in ELEMENTS; cells of a channel are contiguous.
 * The `pred[:, :nt]` view of the network's [B, nt+1, H, W] output is passed as it is (sb = (nt+1)*n_cells, sc = n_cells).
 * Labels: contiguous float32 [B,1,n] (depth, semantics) / [B,3,n] (normal).  Any n_cells >= 1 and any 4-byte aligned base.
 *
 * Arithmetic: per-cell arithmetic of depth and normal is float64 from the float32 inputs, in the reference's operation order
 * and with its clamp constants; sums are float64.  Like the reference the terms are MULTIPLIED by the mask (not skipped), so a
 * non-finite prediction on a nodata cell propagates exactly as it does there.
 *
 * Determinism: image b is cut into chunks of XL_METRICS_CHUNK cells, one workgroup each; within a chunk lane t owns the cells
 * 4*(t + 256*k) .. +3.  This mapping depends on n_cells only - not on B, not on the slot of the image and not on the alignment of
 * its planes: a plane whose chunk base is 16-byte aligned is read with 16-byte loads, any other plane (odd n_cells, a shifted
 * base) and the ragged last group with 4-byte loads of the SAME cells.  Sums run wave butterfly -> LDS -> per-chunk partial ->
 * sequential finalise in chunk order.  A frame's row is therefore bitwise the same alone or in any slot of any batch.
 *
 * No global atomics, no memset: partials go to `workspace`, xl_metrics_workspace_bytes(B, n_cells) bytes of device scratch
 * (8-byte aligned), fully overwritten before it is read.  All calls are asynchronous on `stream` (a hipStream_t; NULL = the
 * default stream), never synchronise with the host, and return 0 or a negative xl status (crossloc_dsac.h); arguments are
 * validated before any HIP call.
 */
#ifndef CROSSLOC_METRICS_H
#define CROSSLOC_METRICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XL_METRICS_CHUNK 4096              /* cells per workgroup */
#define XL_METRICS_CLASSES 6               /* semantics classes of CrossLoc (evaluation.py:402) */
#define XL_METRICS_MAX_BATCH 65535         /* images per call (the grid's y extent); more -> XL_ERR_ARG, split the batch */

/* B * ceil(n_cells / XL_METRICS_CHUNK) * 144 bytes (36 int32 per chunk: the largest of the three tasks); <= 0 arguments -> 0 */
int64_t xl_metrics_workspace_bytes(int B, int n_cells);

int xl_metrics_depth(const float *pred, int64_t pred_sb, int64_t pred_sc, const float *gt_depth, int B, int n_cells,
                     float nodata, void *workspace, double *rows, void *stream);

int xl_metrics_normal(const float *logits, int64_t pred_sb, int64_t pred_sc, const float *gt_normals, int B, int n_cells,
                      float nodata, void *workspace, double *rows, void *stream);

/* C must be XL_METRICS_CLASSES */
int xl_metrics_semantics(const float *logits, int64_t pred_sb, int64_t pred_sc, int C, const float *labels, int B,
                         int n_cells, void *workspace, int64_t *counts, uint8_t *class_map, void *stream);

#ifdef __cplusplus
}
#endif
#endif
