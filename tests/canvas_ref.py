"""Host restatements of xl_data_canvas_augment (include/crossloc_data.h), shared by test_canvas_cpu.py and test_canvas_gpu.py.

  canvas_augment(x, scales, angles, fill, bilinear)   numpy float32, the kernel's per-pixel arithmetic: the same record
      construction (the host's cos / sin in double through math, rounded to float32; the divisions and the zoom factor in
      float32), the same operation order for the source position and the blend, the same inside rule.  Every intermediate is
      a float32 array or scalar, so each operation rounds once, as the kernel's does without contraction.
  source_positions(H, W, scale, angle)                float64, written from the geometry alone:
      sx = (c X - s Y) / scale + W/2 - 0.5, sy = (s X + c Y) / scale + H/2 - 0.5 - no records, no normalised grid.
  predicted_inside(H, W, scale, angle, eps)           the set of cells whose nearest source cell is inside, from
      source_positions, and the cells it cannot decide: within eps of a rounding tie (which includes the border, a tie between
      the last cell and the first one outside)."""
import math

import numpy as np

F = np.float32


def records(scale, angle_deg, H, W):
    """(r00, r10, r01, r11) of one frame, float32: rotation_record of csrc/xl_data.hip times (float)(1 / scale)."""
    th = float(angle_deg) * (math.pi / 180.0)
    c, s = F(math.cos(th)), F(math.sin(th))
    hw, hh = F(0.5) * F(W), F(0.5) * F(H)
    zoom = F(1.0 / float(scale))
    return (c / hw) * zoom, (-s / hw) * zoom, (s / hh) * zoom, (c / hh) * zoom


def source_f32(scale, angle_deg, H, W):
    """(sx, sy) float32 [H,W] as the kernel computes them."""
    r00, r10, r01, r11 = records(scale, angle_deg, H, W)
    j, i = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    X = j + F(0.5) - F(W) * F(0.5)
    Y = i + F(0.5) - F(H) * F(0.5)
    gx = X * r00 + Y * r10
    gy = X * r01 + Y * r11
    sx = ((gx + F(1)) * F(W) - F(1)) / F(2)
    sy = ((gy + F(1)) * F(H) - F(1)) / F(2)
    assert sx.dtype == F and sy.dtype == F
    return sx, sy


def canvas_frame(x, scale, angle_deg, fill, bilinear):
    """One frame x float32 [C,H,W] -> (out [C,H,W], inside [H,W])."""
    x = np.ascontiguousarray(x, dtype=F)
    C, H, W = x.shape
    if float(scale) == 1.0 and float(angle_deg) == 0.0:
        return x.copy(), np.ones((H, W), bool)
    sx, sy = source_f32(scale, angle_deg, H, W)
    ix, iy = np.rint(sx).astype(np.int64), np.rint(sy).astype(np.int64)
    inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    cx, cy = np.clip(ix, 0, W - 1), np.clip(iy, 0, H - 1)
    if not bilinear:
        out = x[:, cy, cx]
    else:
        fx, fy = np.floor(sx), np.floor(sy)
        lx, ly = sx - fx, sy - fy
        hx, hy = F(1) - lx, F(1) - ly
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        x0, y0 = np.maximum(x0, 0), np.maximum(y0, 0)
        x0, x1, y0, y1 = (np.clip(v, 0, m) for v, m in ((x0, W - 1), (x1, W - 1), (y0, H - 1), (y1, H - 1)))   # (outside cells)
        out = hy * (hx * x[:, y0, x0] + lx * x[:, y0, x1]) + ly * (hx * x[:, y1, x0] + lx * x[:, y1, x1])
        assert out.dtype == F
    return np.where(inside[None], out, F(fill)).astype(F), inside


def canvas_augment(x, scales, angles_deg, fill, bilinear):
    """x float32 [B,C,H,W] -> the kernel's output, float32 [B,C,H,W]."""
    assert len(scales) == len(angles_deg) == x.shape[0]
    return np.stack([canvas_frame(x[b], scales[b], angles_deg[b], fill, bilinear)[0] for b in range(x.shape[0])])


def source_positions(H, W, scale, angle_deg):
    """(sx, sy) float64 [H,W] from the geometry: the output pixel relative to the centre, rotated by theta, shrunk by the
    scale, relative to the source's first pixel centre."""
    theta = math.radians(float(angle_deg))
    rot = np.array([[math.cos(theta), -math.sin(theta)], [math.sin(theta), math.cos(theta)]])
    centre = np.array([W / 2.0, H / 2.0])
    pix = np.stack(np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5), -1)             # [H,W,2] pixel centres (x, y)
    src = (pix - centre) @ rot.T / float(scale) + centre - 0.5
    return src[..., 0], src[..., 1]


def predicted_inside(H, W, scale, angle_deg, eps=1e-3):
    """(inside [H,W] bool, undecided [H,W] bool): the nearest source cell of a pixel is inside the frame; undecided where a
    source coordinate lies within eps of a half-integer (a rounding tie; -0.5 and size - 0.5 are the border)."""
    sx, sy = source_positions(H, W, scale, angle_deg)
    inside = (sx > -0.5) & (sx < W - 0.5) & (sy > -0.5) & (sy < H - 0.5)
    tie = lambda v: np.abs((v - 0.5) - np.rint(v - 0.5)) < eps                           # noqa: E731
    return inside, tie(sx) | tie(sy)
