"""ctypes loader of tests/dsac_rgbd_bwd_ref.c — TEST INFRASTRUCTURE ONLY: the CPU restatement of the RGB-D DSAC* backward pass.

`load(tmpdir)` compiles the C file (gcc -O2 -ffp-contract=off) against the product's shared header
crossloc_amd/csrc/xl_dsac_rgbd_bwd_math.h into `tmpdir` and returns the front-end; the test modules do that in a module-scoped
fixture, so nothing is written into the repository tree.  `build_program(tmpdir, sanitize=True)` builds the same file with its
own main() as an executable, with AddressSanitizer and UBSan linked statically."""
import ctypes
import os

import numpy as np

from rgbd_ref_common import HERE, INTR_ARGTYPES, SRC_ARGTYPES, _el_strides, _ptr, compile_lib, compile_program, source_args

SRC = os.path.join(HERE, "dsac_rgbd_bwd_ref.c")
REC = 64
# record columns (include/crossloc_dsac.h)
PROB, LOSS, ACTIVE, INLIERS, GUARD_I, SOG = 0, 1, 2, 3, 4, 5
POSE, H_MAT, V_VEC, C_P, SUPPORT, MAX_DOMEGA, GUARD_II = slice(6, 18), slice(18, 27), slice(27, 30), slice(30, 33), slice(33, 42), 42, 43
SUMS, GAP_REF, GAP_MIN = slice(44, 56), 56, 57


class BwdRef:
    def __init__(self, path):
        L = ctypes.CDLL(path)
        i64, ci, cf, cd, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p
        u64, u32 = ctypes.c_uint64, ctypes.c_uint32
        L.xb_backward_rgbd.restype = ci
        L.xb_backward_rgbd.argtypes = SRC_ARGTYPES + [vp, i64, i64, i64, vp, ci, cf, cf, cf, cf, cf, cf] + INTR_ARGTYPES + [
            u64, u64, u32] + [vp] * 6
        L.xb_test_adjoint.restype = ci
        L.xb_test_adjoint.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp]
        L.xb_test_softmax.restype = None
        L.xb_test_softmax.argtypes = [vp, ci, vp]
        L.xb_test_pose_loss.restype = cd
        L.xb_test_pose_loss.argtypes = [vp, vp, cd, cd, cd]
        self.L = L

    def backward(self, coords, gt_pose, n_hyp, thr, alpha, max_dist, w_rot=1.0, w_trans=100.0, soft_clamp=1e6, cam=None, depth=None,
                 focal=480.0, ppx=None, ppy=None, sub=8, seed=1305, image=0, max_tries=1000000, grad=None):
        """One image: coords float32 [3,Ho,Wo], cam float32 [3,Ho,Wo] or depth float32 [Ho,Wo] (any strides), gt_pose [4,4]
        cam->world.  `grad` (float32 [3,Ho,Wo], any strides) is accumulated in place; without it a zero tensor is made.  Returns a
        dict: loss, grad, rec [nHyp,64], cells [nHyp,3], scores [nHyp], hyp_poses [nHyp,12], masks [nHyp,Ho,Wo] bool."""
        prefix, intr, (coords, cam, depth) = source_args(coords, cam, depth, focal, ppx, ppy, sub)
        Ho, Wo = coords.shape[1:]
        if grad is None:
            grad = np.zeros((3, Ho, Wo), np.float32)
        assert grad.dtype == np.float32 and grad.shape == coords.shape
        gt16 = np.ascontiguousarray(np.asarray(gt_pose, np.float32).reshape(16))
        loss = np.zeros(1, np.float64)
        rec = np.zeros((n_hyp, REC), np.float64)
        cells = np.zeros((n_hyp, 3), np.int32)
        scores = np.zeros(n_hyp, np.float64)
        hyp = np.zeros((n_hyp, 12), np.float64)
        masks = np.zeros((n_hyp, Ho, Wo), np.uint8)
        rc = self.L.xb_backward_rgbd(*prefix, _ptr(grad), *_el_strides(grad), _ptr(gt16), int(n_hyp), float(thr), float(alpha),
                                     float(max_dist), float(w_rot), float(w_trans), float(soft_clamp), *intr, int(seed), int(image),
                                     int(max_tries), _ptr(loss), _ptr(rec), _ptr(cells), _ptr(scores), _ptr(hyp), _ptr(masks))
        if rc != 0:
            raise RuntimeError("dsac_rgbd_bwd_ref failed: %d" % rc)
        return dict(loss=float(loss[0]), grad=grad, rec=rec, cells=cells, scores=scores, hyp_poses=hyp, masks=masks.astype(bool))

    def adjoint(self, p, X, GR, gt):
        """dL/dX_k [n,3] of the header's Kabsch adjoint for G_R [3,3], g_t [3]; also the fit (R, t), the relative gap, the guard"""
        p = np.ascontiguousarray(p, np.float64).reshape(-1, 3)
        X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
        GR = np.ascontiguousarray(GR, np.float64).reshape(9)
        gt = np.ascontiguousarray(gt, np.float64).reshape(3)
        out = np.zeros_like(X)
        fit = np.zeros(12, np.float64)
        gap = np.zeros(1, np.float64)
        guard = self.L.xb_test_adjoint(p.shape[0], _ptr(p), _ptr(X), _ptr(GR), _ptr(gt), _ptr(out), _ptr(fit), _ptr(gap))
        return out, fit[:9].reshape(3, 3).copy(), fit[9:].copy(), float(gap[0]), bool(guard)

    def softmax(self, scores):
        scores = np.ascontiguousarray(scores, np.float64)
        out = np.zeros_like(scores)
        self.L.xb_test_softmax(_ptr(scores), scores.size, _ptr(out))
        return out

    def pose_loss(self, R, t, gt_pose, w_rot, w_trans, cut):
        Rt = np.ascontiguousarray(np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)]))
        gt16 = np.ascontiguousarray(np.asarray(gt_pose, np.float32).reshape(16))
        return float(self.L.xb_test_pose_loss(_ptr(Rt), _ptr(gt16), float(w_rot), float(w_trans), float(cut)))


def load(tmpdir):
    return BwdRef(compile_lib(tmpdir, SRC, "dsac_rgbd_bwd_ref"))


def build_program(tmpdir, sanitize=True):
    """The restatement with its own main() as an executable; with `sanitize` under AddressSanitizer and UBSan."""
    return compile_program(tmpdir, SRC, "dsac_rgbd_bwd_ref", "XB_MAIN", sanitize)
