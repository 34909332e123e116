"""ctypes loader of tests/dsac_rgbd_ref.c — TEST INFRASTRUCTURE ONLY: the CPU restatement of the RGB-D DSAC* solver.

`load(tmpdir)` compiles the C file (gcc -O2 -ffp-contract=off, a second) against the product's shared header
crossloc_amd/csrc/xl_dsac_rgbd_math.h into `tmpdir` and returns the front-end; the test modules do that in a
module-scoped fixture, so nothing is written into the repository tree.  `build_program(tmpdir, sanitize=True)` builds the
same file with its own main() as an executable, with AddressSanitizer and UBSan."""
import ctypes
import os

import numpy as np

from rgbd_ref_common import HERE, INTR_ARGTYPES, SRC_ARGTYPES, _ptr, compile_lib, compile_program, source_args

SRC = os.path.join(HERE, "dsac_rgbd_ref.c")
DBG = 16
MAX_REF_STEPS = 100


class Ref:
    def __init__(self, path):
        L = ctypes.CDLL(path)
        ci, cf, vp, u64, u32 = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        L.xr_forward_rgbd.restype = ci
        L.xr_forward_rgbd.argtypes = SRC_ARGTYPES + [ci, cf, cf, cf] + INTR_ARGTYPES + [u64, u64, u32] + [vp] * 9
        L.xr_test_kabsch.restype = None
        L.xr_test_kabsch.argtypes = [ci, vp, vp, vp]
        L.xr_test_cam_from_depth.restype = None
        L.xr_test_cam_from_depth.argtypes = [cf, ci, ci, cf, cf, cf, ci, vp]
        self.L = L

    def forward(self, coords, n_hyp, thr, alpha, max_dist, cam=None, depth=None, focal=480.0, ppx=None, ppy=None, sub=8,
                seed=1305, image=0, max_tries=1000000, rounds=False):
        """One image: coords float32 [3,Ho,Wo], and cam float32 [3,Ho,Wo] or depth float32 [Ho,Wo] (any strides).  Returns a dict:
        pose [4,4] float32, cells [nHyp,3], tries [nHyp], scores [nHyp], dbg [16], hyp_poses [nHyp,12]; with rounds=True also
        round_counts (the inlier count of every round entered), round_poses [r,12] and round_masks [r,Ho,Wo] of the r fitted rounds."""
        prefix, intr, (coords, cam, depth) = source_args(coords, cam, depth, focal, ppx, ppy, sub)
        Ho, Wo = coords.shape[1:]
        pose = np.zeros(16, np.float32)
        cells = np.zeros((n_hyp, 3), np.int32)
        tries = np.zeros(n_hyp, np.int32)
        scores = np.zeros(n_hyp, np.float64)
        dbg = np.zeros(DBG, np.float64)
        hyp = np.zeros((n_hyp, 12), np.float64)
        rcnt = rpose = rmask = None
        if rounds:
            rcnt = np.zeros(MAX_REF_STEPS, np.int32)
            rpose = np.zeros((MAX_REF_STEPS, 12), np.float64)
            rmask = np.zeros((MAX_REF_STEPS, Ho, Wo), np.uint8)
        rc = self.L.xr_forward_rgbd(*prefix, int(n_hyp), float(thr), float(alpha), float(max_dist), *intr,
                                    int(seed), int(image), int(max_tries), _ptr(pose), _ptr(cells), _ptr(tries), _ptr(scores),
                                    _ptr(dbg), _ptr(hyp), _ptr(rcnt), _ptr(rpose), _ptr(rmask))
        if rc != 0:
            raise RuntimeError("dsac_rgbd_ref failed: %d" % rc)
        out = dict(pose=pose.reshape(4, 4), cells=cells, tries=tries, scores=scores, dbg=dbg, hyp_poses=hyp)
        if rounds:
            r = int(dbg[2])
            out.update(round_counts=rcnt[rcnt >= 0].copy(), round_poses=rpose[:r].copy(), round_masks=rmask[:r].astype(bool))
        return out

    def kabsch(self, p, X):
        """xl_dsac_rgbd_math.h Kabsch on n pairs (p camera, X scene): world->camera (R [3,3], t [3])."""
        p = np.ascontiguousarray(p, np.float64).reshape(-1, 3)
        X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
        assert p.shape == X.shape
        out = np.zeros(12, np.float64)
        self.L.xr_test_kabsch(p.shape[0], _ptr(p), _ptr(X), _ptr(out))
        return out[:9].reshape(3, 3).copy(), out[9:].copy()

    def cam_from_depth(self, d, y, x, f, ppx, ppy, sub):
        out = np.zeros(3, np.float32)
        self.L.xr_test_cam_from_depth(float(d), int(y), int(x), float(f), float(ppx), float(ppy), int(sub), _ptr(out))
        return out


def load(tmpdir):
    return Ref(compile_lib(tmpdir, SRC, "dsac_rgbd_ref"))


def build_program(tmpdir, sanitize=True):
    """The restatement with its own main() as an executable; with `sanitize` under AddressSanitizer and UBSan."""
    return compile_program(tmpdir, SRC, "dsac_rgbd_ref", "XR_MAIN", sanitize)
