"""ctypes loader of tests/pose_refine_masked_ref.c — TEST INFRASTRUCTURE ONLY: the CPU restatement of the masked pose-refinement
pass.  `load(tmpdir)` compiles the C file as tests/pose_refine_ref.py compiles its own (gcc -O2 -ffp-contract=off against the
product's shared headers, into `tmpdir`) and returns the front-end."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "crossloc_amd", "csrc")
ROW = 64


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


class Ref:
    def __init__(self, path):
        L = ctypes.CDLL(path)
        c_i64, c_int, c_f, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
        L.xrm_refine_pose.restype = c_int
        L.xrm_refine_pose.argtypes = [vp, c_i64, c_i64, c_i64, vp, c_i64, c_i64, c_int, c_int, vp, vp, c_f, c_f, c_f, c_f, c_f,
                                      c_int, c_f, c_int, vp, vp, vp, vp]
        self.L = L

    def refine(self, coords, mask, sigma, pose, thr, focal, ppx, ppy, max_reproj, sub, s0=1.0, max_rounds=8):
        """What the masked kernel must produce for one image: coords float32 [3,Ho,Wo] (any strides), mask [Ho,Wo] (nonzero =
        usable), sigma float32 [Ho,Wo] (any strides) or None, pose 4x4 cam->world (taken as float32) -> (pose float32 [4,4],
        row [64], w2c [12], inliers bool [Ho,Wo]: the inlier set of the last completed round)."""
        coords = np.asarray(coords)
        assert coords.dtype == np.float32 and coords.ndim == 3 and coords.shape[0] == 3
        sc, sy, sx = [s // 4 for s in coords.strides]
        _, Ho, Wo = coords.shape
        mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        assert mask.shape == (Ho, Wo)
        gy = gx = 0
        if sigma is not None:
            sigma = np.asarray(sigma)
            assert sigma.dtype == np.float32 and sigma.shape == (Ho, Wo)
            gy, gx = [s // 4 for s in sigma.strides]
        pose = np.ascontiguousarray(pose, np.float32).reshape(16)
        out = np.zeros(16, np.float32)
        row = np.zeros(ROW, np.float64)
        w2c = np.zeros(12, np.float64)
        inl = np.zeros(Ho * Wo, np.uint8)
        rc = self.L.xrm_refine_pose(_ptr(coords), sc, sy, sx, _ptr(sigma), gy, gx, Ho, Wo, _ptr(mask), _ptr(pose), float(thr),
                                    float(focal), float(ppx), float(ppy), float(max_reproj), int(sub), float(s0), int(max_rounds),
                                    _ptr(out), _ptr(row), _ptr(w2c), _ptr(inl))
        if rc != 0:
            raise RuntimeError("pose_refine_masked_ref failed: %d" % rc)
        return out.reshape(4, 4), row, w2c, inl.reshape(Ho, Wo).astype(bool)


def load(tmpdir):
    out = os.path.join(str(tmpdir), "libpose_refine_masked_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra",
                           "-Wno-unused-function", "-I" + CSRC, "-shared", "-o", out,
                           os.path.join(HERE, "pose_refine_masked_ref.c"), "-lm"])
    return Ref(out)
