/*
 * crossloc_data.h — C ABI of the GPU-side frame / label preparation (libcrossloc_hip.so), SURVEY.md §8(f3).
 *
 * Replaces the CPU-worker bodies of /root/reference/dataloader/dataloader.py:
 *   image_transform / cur_image_transform   :189-232, :349-393   ToPILImage -> Resize(image_height) -> [ColorJitter
 *                                                                 (brightness, contrast)] -> ToTensor -> [Normalize]
 *   batch_resize (collate_fn)               :512-563             one common scale + rotation per mini-batch
 * Decoding the PNG and reading the text files stays on the host (file formats, crossloc_amd/dataset.py); everything
 * after the decoded uint8 frame runs here, so a training batch is uploaded once as bytes.
 *
 * Arithmetic contracts (checked bit for bit against oracle/data_oracle.py, which is pinned against Pillow itself):
 *   resize      Pillow's two-pass bilinear resampler on uint8, 22-bit fixed-point coefficients, horizontal pass first
 *               (what torchvision's Resize does on a PIL image); a pass whose size does not change is skipped
 *   jitter      PIL.ImageEnhance.Brightness / Contrast on uint8 (Image.blend against black / against the rounded mean
 *               of the 'L' conversion), in the order torchvision drew; `jitter` = host array [B][3] of
 *               {brightness factor, contrast factor, 1.0f if contrast is applied first else 0.0f}, NULL = none
 *   to tensor   uint8 / 255 in float32, then (x - mean[c]) / std[c] when mean/std are given (host float[3]); NCHW out
 *   batch aug   images: bilinear resize (align_corners = false, like F.interpolate) to (oh, ow) composed with the
 *               nearest-neighbour rotation of torchvision's tensor `rotate` about the image centre, `fill` outside;
 *               labels: nearest resize (F.interpolate 'nearest') composed with the same rotation
 *   canvas      a scale and a rotation per frame at a fixed size (xl_data_canvas_augment, below): no reference counterpart;
 *               checked bit for bit against the float32 restatement tests/canvas_ref.py
 * All pointers are device pointers unless stated; calls are asynchronous on `stream` (the per-frame jitter records
 * travel as kernel arguments: the host arrays may be freed when a call returns) and return 0 or a negative xl
 * status (crossloc_dsac.h).  Frames of one call share their size (the reference's collate stacks them, :563).
 */
#ifndef CROSSLOC_DATA_H
#define CROSSLOC_DATA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Output size of Resize(image_height) for a stored Hs x Ws frame (smaller edge -> image_height, torchvision rule). */
int xl_data_resized_shape(int Hs, int Ws, int image_height, int *H, int *W);

/* Bytes of device scratch xl_data_prepare_images needs for B frames of Hs x Ws resized to H x W. */
long long xl_data_prepare_workspace_bytes(int B, int Hs, int Ws, int H, int W);

/* src: uint8 [B][Hs][Ws][Cs] (Cs = 3, or 4 with the alpha channel ignored: dataloader.py:305-307);
 * out: float32 [B][3][H][W] with (H, W) = xl_data_resized_shape(Hs, Ws, image_height). */
int xl_data_prepare_images(const uint8_t *src, int B, int Hs, int Ws, int Cs, int image_height,
                           const float *jitter_host, const float *mean_host, const float *std_host,
                           float *out, void *workspace, void *stream);

/* The grayscale pipeline (dataloader.py:171-187, 359-373: ... Resize -> Grayscale -> [ColorJitter] -> ToTensor ->
 * Normalize(mean[1], std[1])): Pillow's 'L' conversion (R*19595 + G*38470 + B*7471 + 0x8000) >> 16 of the resized frame,
 * the jitter on that one channel; out: float32 [B][1][H][W]; mean_host / std_host: one float each (or NULL). */
int xl_data_prepare_images_gray(const uint8_t *src, int B, int Hs, int Ws, int Cs, int image_height,
                                const float *jitter_host, const float *mean_host, const float *std_host,
                                float *out, void *workspace, void *stream);

/* in: float32 [B][C][H][W] -> out [B][C][oh][ow]: resize (bilinear = 1: images; 0: nearest, labels) + rotation by
 * angle_deg (counter-clockwise, nearest, `fill` outside the rotated frame). */
int xl_data_batch_augment(const float *in, float *out, int B, int C, int H, int W, int oh, int ow,
                          double angle_deg, float fill, int bilinear, void *stream);

/* xl_data_batch_augment with one angle per frame, the whole batch in one launch (64 frames per launch: the rotation
 * records travel as kernel arguments, like the jitter records).  angles_deg_host: host array of B doubles, free to
 * release when the call returns.  Frame b equals xl_data_batch_augment of that frame alone with angles_deg_host[b],
 * bit for bit: the same per-pixel device code under the same four float32 rotation entries. */
int xl_data_batch_augment_frames(const float *in, float *out, int B, int C, int H, int W, int oh, int ow,
                                 const double *angles_deg_host, float fill, int bilinear, void *stream);

/* Fixed-size augmentation: frame b is zoomed by scales_host[b] and rotated by angles_deg_host[b] (counter-clockwise, the
 * sense of xl_data_batch_augment) about the image centre onto a canvas of its own size.  in / out: float32 [B][C][H][W],
 * distinct buffers.  The principal point stays at the centre, the focal length of frame b becomes f_b * scale_b and its
 * pose P_b * Rz(theta_b) (xl_data_rotate_poses).  Output pixel (i, j), X = j + 0.5 - W/2, Y = i + 0.5 - H/2, takes its
 * value from the source position
 *     sx = (c X - s Y) / scale + W/2 - 0.5,   sy = (s X + c Y) / scale + H/2 - 0.5,   c = cos(theta), s = sin(theta)
 * computed in float32 as the rotation kernels compute theirs: the record (r00, r10, r01, r11) of xl_data_batch_augment for
 * an H x W frame, each entry multiplied by (float)(1 / scale); gx = X r00 + Y r10, gy = X r01 + Y r11;
 * sx = ((gx + 1) W - 1) / 2, sy = ((gy + 1) H - 1) / 2.  (ix, iy) = (rintf(sx), rintf(sy)) is the nearest source cell;
 * where it lies outside the frame the pixel is `fill`, in both modes.  Otherwise
 *   bilinear = 0 (label maps)  the value of cell (ix, iy): the nearest path of xl_data_batch_augment_frames under the scaled
 *                record, so a frame with scale 1 is bitwise what that entry returns for it at (oh, ow) = (H, W);
 *   bilinear = 1 (images)      ONE bilinear sample at (sx, sy) itself: x0 = floor(sx), lx = sx - x0, hx = 1 - lx (y alike), the
 *                taps x0, x0 + 1, y0, y0 + 1 clamped to the frame, and in float32, in this order, no contraction,
 *                    hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11).
 *                This is not the "nearest rotation of a bilinearly resized frame" of xl_data_batch_augment: a rotated image is
 *                not bitwise that kernel's output.  Minification (scale < 1) takes the one sample without an anti-alias
 *                filter, as F.interpolate does.
 * A frame with scale == 1.0 and angle == 0.0 is copied through bit for bit.  The records travel as kernel arguments, 64 frames
 * per launch; both host arrays (B doubles each) are free to release when the call returns.  Refused (-1) before any HIP call:
 * null pointers, in == out, non-positive sizes, a scale that is not finite or not positive, an angle that is not finite. */
int xl_data_canvas_augment(const float *in, float *out, int B, int C, int H, int W,
                           const double *scales_host, const double *angles_deg_host, float fill, int bilinear, void *stream);

/* The ground-truth poses of frames rotated by xl_data_batch_augment[_frames].  poses_in / poses_out: float32
 * [B][4][4] row-major cam->world matrices; poses_out may alias poses_in.  The rotation above is counter-clockwise
 * about the image centre by theta = angle * (pi / 180); the pose of the rotated frame is P * Rz(theta),
 *     Rz(theta) = [[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]],  c = cos(theta), s = sin(theta)
 * (the reference's pose_rot, dataloader.py:430-438), so only columns 0 and 1 change:
 *     col0' = c col0 + s col1,  col1' = -s col0 + c col1
 * with c and s from the host's cos / sin in double, the sums in float64, one rounding to float32.  Angle 0 returns the
 * input bit for bit.  angles_deg_host: host array of B doubles, free to release when the call returns. */
int xl_data_rotate_poses(const float *poses_in, float *poses_out, int B, const double *angles_deg_host, void *stream);

#ifdef __cplusplus
}
#endif
#endif
