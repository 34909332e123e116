"""ctypes loader of tests/pose_quality_ref.c — TEST INFRASTRUCTURE ONLY: the CPU restatement of the pose-quality pass.

`load(tmpdir)` compiles the C file (gcc -O2 -ffp-contract=off, a second) against the product's shared header
crossloc_amd/csrc/xl_dsac_quality_math.h into `tmpdir` and returns the front-end; the test modules do that in a
module-scoped fixture, so nothing is written into the repository tree."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "crossloc_amd", "csrc")
ROW = 64


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _strides(coords):
    coords = np.asarray(coords)
    assert coords.dtype == np.float32 and coords.ndim == 3 and coords.shape[0] == 3
    return coords, [s // coords.itemsize for s in coords.strides]


def rt12(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


class Ref:
    def __init__(self, path):
        L = ctypes.CDLL(path)
        c_i64, c_int, c_f, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
        for name in ("xq_pose_quality", "xq_pose_quality_w2c", "xq_test_sums_w2c"):
            getattr(L, name).restype = c_int
            getattr(L, name).argtypes = [vp, c_i64, c_i64, c_i64, c_int, c_int, vp, c_f, c_f, c_f, c_f, c_f, c_f, c_int, vp]
        L.xq_test_pose_from16.restype = None
        L.xq_test_pose_from16.argtypes = [vp, vp]
        L.xq_test_apply_step.restype = None
        L.xq_test_apply_step.argtypes = [vp, vp, vp]
        L.xq_test_inv6.restype = c_int
        L.xq_test_inv6.argtypes = [vp, vp]
        self.L = L

    def _call(self, fn, coords, pose, thr, focal, ppx, ppy, alpha, max_reproj, sub, width=ROW):
        coords, (sc, sy, sx) = _strides(coords)
        row = np.zeros(width, np.float64)
        rc = fn(_ptr(coords), sc, sy, sx, coords.shape[1], coords.shape[2], _ptr(pose), float(thr), float(focal), float(ppx),
                float(ppy), float(alpha), float(max_reproj), int(sub), _ptr(row))
        if rc != 0:
            raise RuntimeError("pose_quality_ref failed: %d" % rc)
        return row

    def row(self, coords, pose, thr, focal, ppx, ppy, alpha, max_reproj, sub):
        """The row the kernel must produce: coords float32 [3,Ho,Wo] (any strides), pose 4x4 cam->world (taken as float32)."""
        pose = np.ascontiguousarray(pose, np.float32).reshape(16)
        return self._call(self.L.xq_pose_quality, coords, pose, thr, focal, ppx, ppy, alpha, max_reproj, sub)

    def row_w2c(self, coords, R, t, thr, focal, ppx, ppy, alpha, max_reproj, sub):
        """The same at a float64 world->camera pose {R, t} (e.g. the oracle's `pose1`)."""
        return self._call(self.L.xq_pose_quality_w2c, coords, rt12(R, t), thr, focal, ppx, ppy, alpha, max_reproj, sub)

    def sums_w2c(self, coords, R, t, thr, focal, ppx, ppy, alpha, max_reproj, sub):
        """The 32 reduced sums (28 normal-equation sums, count, soft sum, sum e, sum e^2) at a float64 world->camera pose."""
        return self._call(self.L.xq_test_sums_w2c, coords, rt12(R, t), thr, focal, ppx, ppy, alpha, max_reproj, sub, width=32)

    def pose_from16(self, pose):
        """World->camera (R [3,3], t [3]) the kernel derives from a float32 cam->world 4x4."""
        pose = np.ascontiguousarray(pose, np.float32).reshape(16)
        out = np.zeros(12, np.float64)
        self.L.xq_test_pose_from16(_ptr(pose), _ptr(out))
        return out[:9].reshape(3, 3).copy(), out[9:].copy()

    def apply_step(self, R, t, d):
        """xl_dsac_math.h apply_step: R' = Exp(-d[:3]) R, t' = t - d[3:]."""
        src, d = rt12(R, t), np.ascontiguousarray(d, np.float64).reshape(6)
        out = np.zeros(12, np.float64)
        self.L.xq_test_apply_step(_ptr(src), _ptr(d), _ptr(out))
        return out[:9].reshape(3, 3).copy(), out[9:].copy()

    def inv6(self, ut21):
        ut21 = np.ascontiguousarray(ut21, np.float64).reshape(21)
        out = np.zeros(36, np.float64)
        ok = self.L.xq_test_inv6(_ptr(ut21), _ptr(out))
        return bool(ok), out.reshape(6, 6)


def load(tmpdir):
    out = os.path.join(str(tmpdir), "libpose_quality_ref.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Wno-unused-function",
                           "-I" + CSRC, "-shared", "-o", out, os.path.join(HERE, "pose_quality_ref.c"), "-lm"])
    return Ref(out)


class OracleNormalEq:
    """tests/pose_quality_oracle_ne.c: the oracle's own normal equations over the refinement's inlier set at a pose."""

    def __init__(self, path):
        self.L = ctypes.CDLL(path)
        c_i64, c_int, c_f, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
        self.L.xq_oracle_normal_eq.restype = c_int
        self.L.xq_oracle_normal_eq.argtypes = [vp, c_i64, c_i64, c_i64, c_int, c_int, vp, c_f, c_f, c_f, c_f, c_f, c_f, c_int, vp]

    def normal_eq(self, coords, R, t, thr, focal, ppx, ppy, alpha, max_reproj, sub):
        coords, (sc, sy, sx) = _strides(coords)
        out = np.zeros(28, np.float64)
        rc = self.L.xq_oracle_normal_eq(_ptr(coords), sc, sy, sx, coords.shape[1], coords.shape[2], _ptr(rt12(R, t)), float(thr),
                                        float(focal), float(ppx), float(ppy), float(alpha), float(max_reproj), int(sub), _ptr(out))
        assert rc == 0
        return out


def load_oracle_normal_eq(tmpdir):
    out = os.path.join(str(tmpdir), "libpose_quality_oracle_ne.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
                           "-I" + CSRC, "-shared", "-o", out, os.path.join(HERE, "pose_quality_oracle_ne.c"), "-lm"])
    return OracleNormalEq(out)


def sym(ut, n):
    """Full symmetric [n,n] matrix from its row-major upper triangle."""
    M = np.zeros((n, n), np.float64)
    M[np.triu_indices(n)] = np.asarray(ut, np.float64)
    return M + np.triu(M, 1).T
