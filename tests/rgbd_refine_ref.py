"""ctypes loader of tests/rgbd_refine_ref.c — TEST INFRASTRUCTURE ONLY: the CPU restatement of the ray-aware pose refinement
behind the RGB-D solver.

`load(tmpdir)` compiles the C file (gcc -O2 -ffp-contract=off, a second) against the product's shared header
crossloc_amd/csrc/xl_dsac_rgbd_refine_math.h into `tmpdir` and returns the front-end; the test modules do that in a
module-scoped fixture, so nothing is written into the repository tree."""
import ctypes
import os

import numpy as np

from rgbd_ref_common import HERE, INTR_ARGTYPES, SRC_ARGTYPES, _el_strides, _ptr, compile_lib, source_args

SRC = os.path.join(HERE, "rgbd_refine_ref.c")
ROW = 64


def rt12(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


def _map(a, Ho, Wo):
    if a is None:
        return None, [0, 0]
    a = np.asarray(a)
    assert a.dtype == np.float32 and a.shape == (Ho, Wo)
    return a, _el_strides(a)


class Ref:
    def __init__(self, path):
        L = ctypes.CDLL(path)
        i64, ci, cf, cd, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p
        L.xrr_refine_pose.restype = ci
        L.xrr_refine_pose.argtypes = SRC_ARGTYPES + [vp, i64, i64, vp, i64, i64, vp, cf, cf] + INTR_ARGTYPES + [
            cf, cf, ci, vp, vp, vp, vp]
        L.xrr_test_noise.restype = None
        L.xrr_test_noise.argtypes = [vp, cd, cd, cd, cd, vp]
        L.xrr_test_cell_normal_eq.restype = None
        L.xrr_test_cell_normal_eq.argtypes = [vp, vp, vp, vp, cd, cd, cd, cd, vp]
        L.xrr_test_apply_step.restype = None
        L.xrr_test_apply_step.argtypes = [vp, vp, vp, vp]
        self.L = L

    def refine(self, coords, pose, thr, max_dist, cam=None, depth=None, sigma=None, depth_sigma=None, depth_rel=0.0, s0=0.01,
               max_rounds=8, focal=480.0, ppx=None, ppy=None, sub=8):
        """What the kernel must produce for one image: coords float32 [3,Ho,Wo], cam float32 [3,Ho,Wo] or depth float32 [Ho,Wo],
        sigma / depth_sigma float32 [Ho,Wo] or None (any strides), pose 4x4 cam->world (taken as float32) -> (pose float32 [4,4],
        row [64], w2c [12], mask bool [Ho,Wo]: the inlier set of the last completed round)."""
        prefix, intr, _keep = source_args(coords, cam, depth, focal, ppx, ppy, sub)
        Ho, Wo = prefix[-2:]
        sigma, gs = _map(sigma, Ho, Wo)
        depth_sigma, zs = _map(depth_sigma, Ho, Wo)
        pose = np.ascontiguousarray(pose, np.float32).reshape(16)
        out = np.zeros(16, np.float32)
        row = np.zeros(ROW, np.float64)
        w2c = np.zeros(12, np.float64)
        mask = np.zeros(Ho * Wo, np.uint8)
        rc = self.L.xrr_refine_pose(*prefix, _ptr(sigma), *gs, _ptr(depth_sigma), *zs, _ptr(pose), float(thr), float(max_dist),
                                    *intr, float(s0), float(depth_rel), int(max_rounds), _ptr(out), _ptr(row), _ptr(w2c), _ptr(mask))
        if rc != 0:
            raise RuntimeError("rgbd_refine_ref failed: %d" % rc)
        return out.reshape(4, 4), row, w2c, mask.reshape(Ho, Wo).astype(bool)

    def noise(self, p, sigma, sigma_z, s0sq, k):
        """(a, b, rho [3], W [3,3]) of a cell with camera coordinate p"""
        p = np.ascontiguousarray(p, np.float64)
        out = np.zeros(14, np.float64)
        self.L.xrr_test_noise(_ptr(p), float(sigma), float(sigma_z), float(s0sq), float(k), _ptr(out))
        return out[0], out[1], out[2:5].copy(), out[5:14].reshape(3, 3).copy()

    def cell_normal_eq(self, R, t, xyz, p, c, sigma, sigma_z, s0sq, k):
        """the 28 sums of one cell at the world->camera pose {R, t} about the centre c"""
        xyz, p, c = (np.ascontiguousarray(v, np.float64) for v in (xyz, p, c))
        out = np.zeros(28, np.float64)
        self.L.xrr_test_cell_normal_eq(_ptr(rt12(R, t)), _ptr(xyz), _ptr(p), _ptr(c), float(sigma), float(sigma_z), float(s0sq),
                                       float(k), _ptr(out))
        return out

    def apply_step(self, R, t, c, d):
        """rgbdr_apply_step: R' = Exp(-d[:3]) R, t' = c + Exp(-d[:3]) (t - c) - d[3:]"""
        c, d = np.ascontiguousarray(c, np.float64), np.ascontiguousarray(d, np.float64)
        out = np.zeros(12, np.float64)
        self.L.xrr_test_apply_step(_ptr(rt12(R, t)), _ptr(c), _ptr(d), _ptr(out))
        return out[:9].reshape(3, 3).copy(), out[9:].copy()


def load(tmpdir):
    return Ref(compile_lib(tmpdir, SRC, "rgbd_refine_ref"))
