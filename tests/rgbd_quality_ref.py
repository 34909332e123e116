"""ctypes loader of tests/rgbd_quality_ref.c — TEST INFRASTRUCTURE ONLY: the CPU restatement of the RGB-D pose-quality pass.

`load(tmpdir)` compiles the C file (gcc -O2 -ffp-contract=off, a second) against the product's shared header
crossloc_amd/csrc/xl_dsac_rgbd_quality_math.h into `tmpdir` and returns the front-end; the test modules do that in a
module-scoped fixture, so nothing is written into the repository tree.  `build_program(tmpdir, sanitize=True)` builds the
same file with its own main() as an executable, with AddressSanitizer and UBSan linked statically."""
import ctypes
import os

import numpy as np

from rgbd_ref_common import HERE, INTR_ARGTYPES, SRC_ARGTYPES, _ptr, compile_lib, compile_program, source_args

SRC = os.path.join(HERE, "rgbd_quality_ref.c")
ROW = 64
SUMS = 25


def rt12(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


class Ref:
    def __init__(self, path):
        L = ctypes.CDLL(path)
        ci, cf, vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
        for name in ("xrq_pose_quality", "xrq_pose_quality_w2c", "xrq_test_sums_w2c"):
            getattr(L, name).restype = ci
            getattr(L, name).argtypes = SRC_ARGTYPES + [vp, cf, cf, cf] + INTR_ARGTYPES + [vp]
        L.xrq_test_pose_from16.restype = None
        L.xrq_test_pose_from16.argtypes = [vp, vp]
        L.xrq_test_apply_step.restype = None
        L.xrq_test_apply_step.argtypes = [vp, vp, vp]
        L.xrq_test_inv3.restype = ci
        L.xrq_test_inv3.argtypes = [vp, vp, vp]
        self.L = L

    def _call(self, fn, coords, pose, thr, alpha, max_dist, cam, depth, focal, ppx, ppy, sub, width):
        prefix, intr, _keep = source_args(coords, cam, depth, focal, ppx, ppy, sub)
        out = np.zeros(width, np.float64)
        rc = fn(*prefix, _ptr(pose), float(thr), float(alpha), float(max_dist), *intr, _ptr(out))
        if rc != 0:
            raise RuntimeError("rgbd_quality_ref failed: %d" % rc)
        return out

    def row(self, coords, pose, thr, alpha, max_dist, cam=None, depth=None, focal=480.0, ppx=None, ppy=None, sub=8):
        """The row the kernel must produce: coords float32 [3,Ho,Wo], cam float32 [3,Ho,Wo] or depth float32 [Ho,Wo] (any
        strides), pose 4x4 cam->world (taken as float32)."""
        pose = np.ascontiguousarray(pose, np.float32).reshape(16)
        return self._call(self.L.xrq_pose_quality, coords, pose, thr, alpha, max_dist, cam, depth, focal, ppx, ppy, sub, ROW)

    def row_w2c(self, coords, R, t, thr, alpha, max_dist, cam=None, depth=None, focal=480.0, ppx=None, ppy=None, sub=8):
        """The same at a float64 world->camera pose {R, t} (e.g. dbg[4:16] of the solver restatement)."""
        return self._call(self.L.xrq_pose_quality_w2c, coords, rt12(R, t), thr, alpha, max_dist, cam, depth, focal, ppx, ppy, sub, ROW)

    def sums_w2c(self, coords, R, t, thr, alpha, max_dist, cam=None, depth=None, focal=480.0, ppx=None, ppy=None, sub=8):
        """dict of the reduced sums at a float64 world->camera pose: n_valid, n, sum_m [3], soft (valid cells only), sum_err,
        sum_err2, sse, C [3,3], grad_w = sum u x r [3], grad_t = sum r [3], c [3], pivot_ratio."""
        s = self._call(self.L.xrq_test_sums_w2c, coords, rt12(R, t), thr, alpha, max_dist, cam, depth, focal, ppx, ppy, sub, SUMS)
        C = np.array([[s[9], s[10], s[11]], [s[10], s[12], s[13]], [s[11], s[13], s[14]]])
        return dict(n_valid=s[0], n=s[1], sum_m=s[2:5].copy(), soft=s[5], sum_err=s[6], sum_err2=s[7], sse=s[8], C=C,
                    grad_w=s[15:18].copy(), grad_t=s[18:21].copy(), c=s[21:24].copy(), pivot_ratio=s[24])

    def pose_from16(self, pose):
        """World->camera (R [3,3], t [3]) the kernel derives from a float32 cam->world 4x4."""
        pose = np.ascontiguousarray(pose, np.float32).reshape(16)
        out = np.zeros(12, np.float64)
        self.L.xrq_test_pose_from16(_ptr(pose), _ptr(out))
        return out[:9].reshape(3, 3).copy(), out[9:].copy()

    def apply_step(self, R, t, d):
        """xl_dsac_math.h apply_step: R' = Exp(-d[:3]) R, t' = t - d[3:]."""
        src, d = rt12(R, t), np.ascontiguousarray(d, np.float64).reshape(6)
        out = np.zeros(12, np.float64)
        self.L.xrq_test_apply_step(_ptr(src), _ptr(d), _ptr(out))
        return out[:9].reshape(3, 3).copy(), out[9:].copy()

    def inv3(self, ut6):
        """(ok, inverse [3,3], smallest relative pivot) of the symmetric 3x3 with upper triangle xx xy xz yy yz zz"""
        ut6 = np.ascontiguousarray(ut6, np.float64).reshape(6)
        out, ratio = np.zeros(9, np.float64), np.zeros(1, np.float64)
        ok = self.L.xrq_test_inv3(_ptr(ut6), _ptr(out), _ptr(ratio))
        return bool(ok), out.reshape(3, 3), float(ratio[0])


def load(tmpdir):
    return Ref(compile_lib(tmpdir, SRC, "rgbd_quality_ref"))


def build_program(tmpdir, sanitize=True):
    """The restatement with its own main() as an executable; with `sanitize` under AddressSanitizer and UBSan."""
    return compile_program(tmpdir, SRC, "rgbd_quality_ref", "XRQ_MAIN", sanitize)


def sym(ut, n):
    """Full symmetric [n,n] matrix from its row-major upper triangle."""
    M = np.zeros((n, n), np.float64)
    M[np.triu_indices(n)] = np.asarray(ut, np.float64)
    return M + np.triu(M, 1).T
