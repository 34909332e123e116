"""ctypes loader of tests/pose_refine_ref.c — TEST INFRASTRUCTURE ONLY: the CPU restatement of the pose-refinement pass.

`load(tmpdir)` compiles the C file (gcc -O2 -ffp-contract=off, a second) against the product's shared header
crossloc_amd/csrc/xl_dsac_refine_math.h into `tmpdir` and returns the front-end; the test modules do that in a
module-scoped fixture, so nothing is written into the repository tree."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "crossloc_amd", "csrc")
ROW = 64


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def rt12(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


class Ref:
    def __init__(self, path):
        L = ctypes.CDLL(path)
        c_i64, c_int, c_f, c_d, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p
        L.xr_refine_pose.restype = c_int
        L.xr_refine_pose.argtypes = [vp, c_i64, c_i64, c_i64, vp, c_i64, c_i64, c_int, c_int, vp, c_f, c_f, c_f, c_f, c_f, c_int,
                                     c_f, c_int, vp, vp, vp, vp]
        L.xr_test_cell_normal_eq.restype = None
        L.xr_test_cell_normal_eq.argtypes = [vp, vp, c_d, c_int, c_int, c_f, c_f, c_f, c_int, vp, vp]
        L.xr_test_weight.restype = c_d
        L.xr_test_weight.argtypes = [vp, vp, c_d, c_d, c_f]
        L.xr_test_pose_to_c2w16.restype = None
        L.xr_test_pose_to_c2w16.argtypes = [vp, vp]
        self.L = L

    def refine(self, coords, sigma, pose, thr, focal, ppx, ppy, max_reproj, sub, s0=1.0, max_rounds=8):
        """What the kernel must produce for one image: coords float32 [3,Ho,Wo] (any strides), sigma float32 [Ho,Wo] (any
        strides) or None, pose 4x4 cam->world (taken as float32) -> (pose float32 [4,4], row [64], w2c [12], mask bool [Ho,Wo]:
        the inlier set of the last completed round)."""
        coords = np.asarray(coords)
        assert coords.dtype == np.float32 and coords.ndim == 3 and coords.shape[0] == 3
        sc, sy, sx = [s // 4 for s in coords.strides]
        _, Ho, Wo = coords.shape
        gy = gx = 0
        if sigma is not None:
            sigma = np.asarray(sigma)
            assert sigma.dtype == np.float32 and sigma.shape == (Ho, Wo)
            gy, gx = [s // 4 for s in sigma.strides]
        pose = np.ascontiguousarray(pose, np.float32).reshape(16)
        out = np.zeros(16, np.float32)
        row = np.zeros(ROW, np.float64)
        w2c = np.zeros(12, np.float64)
        mask = np.zeros(Ho * Wo, np.uint8)
        rc = self.L.xr_refine_pose(_ptr(coords), sc, sy, sx, _ptr(sigma), gy, gx, Ho, Wo, _ptr(pose), float(thr), float(focal),
                                   float(ppx), float(ppy), float(max_reproj), int(sub), float(s0), int(max_rounds),
                                   _ptr(out), _ptr(row), _ptr(w2c), _ptr(mask))
        if rc != 0:
            raise RuntimeError("pose_refine_ref failed: %d" % rc)
        return out.reshape(4, 4), row, w2c, mask.reshape(Ho, Wo).astype(bool)

    def cell_normal_eq(self, R, t, xyz, w, y, x, focal, ppx, ppy, sub):
        """(the 28 sums of one cell through pnp_cell_normal_eq_w with weight w, the same through pnp_cell_normal_eq)"""
        a, q = np.zeros(28, np.float64), np.zeros(28, np.float64)
        xyz = np.ascontiguousarray(xyz, np.float64)
        self.L.xr_test_cell_normal_eq(_ptr(rt12(R, t)), _ptr(xyz), float(w), int(y), int(x), float(focal), float(ppx), float(ppy),
                                      int(sub), _ptr(a), _ptr(q))
        return a, q

    def weight(self, R, t, xyz, sigma, s0, focal):
        xyz = np.ascontiguousarray(xyz, np.float64)
        return float(self.L.xr_test_weight(_ptr(rt12(R, t)), _ptr(xyz), float(sigma), float(s0), float(focal)))

    def pose_to_c2w16(self, R, t):
        out = np.zeros(16, np.float32)
        self.L.xr_test_pose_to_c2w16(_ptr(rt12(R, t)), _ptr(out))
        return out.reshape(4, 4)


def load(tmpdir):
    out = os.path.join(str(tmpdir), "libpose_refine_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Wno-unused-function",
                           "-I" + CSRC, "-shared", "-o", out, os.path.join(HERE, "pose_refine_ref.c"), "-lm"])
    return Ref(out)
