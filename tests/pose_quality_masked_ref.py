"""ctypes loader of tests/pose_quality_masked_ref.c — TEST INFRASTRUCTURE ONLY: the CPU restatement of the masked pose-quality
pass.  `load(tmpdir)` compiles the C file as tests/pose_quality_ref.py compiles its own (gcc -O2 -ffp-contract=off against the
product's shared headers, into `tmpdir`) and returns the front-end."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "crossloc_amd", "csrc")
ROW = 64


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Ref:
    def __init__(self, path):
        L = ctypes.CDLL(path)
        c_i64, c_int, c_f, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
        L.xqm_pose_quality.restype = c_int
        L.xqm_pose_quality.argtypes = [vp, c_i64, c_i64, c_i64, c_int, c_int, vp, vp, c_f, c_f, c_f, c_f, c_f, c_f, c_int, vp]
        self.L = L

    def row(self, coords, mask, pose, thr, focal, ppx, ppy, alpha, max_reproj, sub):
        """The row the masked kernel must produce: coords float32 [3,Ho,Wo] (any strides), mask [Ho,Wo] (nonzero = usable),
        pose 4x4 cam->world (taken as float32)."""
        coords = np.asarray(coords)
        assert coords.dtype == np.float32 and coords.ndim == 3 and coords.shape[0] == 3
        sc, sy, sx = [s // 4 for s in coords.strides]
        _, Ho, Wo = coords.shape
        mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        assert mask.shape == (Ho, Wo)
        pose = np.ascontiguousarray(pose, np.float32).reshape(16)
        row = np.zeros(ROW, np.float64)
        rc = self.L.xqm_pose_quality(_ptr(coords), sc, sy, sx, Ho, Wo, _ptr(mask), _ptr(pose), float(thr), float(focal), float(ppx),
                                     float(ppy), float(alpha), float(max_reproj), int(sub), _ptr(row))
        if rc != 0:
            raise RuntimeError("pose_quality_masked_ref failed: %d" % rc)
        return row


def load(tmpdir):
    out = os.path.join(str(tmpdir), "libpose_quality_masked_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra",
                           "-Wno-unused-function", "-I" + CSRC, "-shared", "-o", out,
                           os.path.join(HERE, "pose_quality_masked_ref.c"), "-lm"])
    return Ref(out)
