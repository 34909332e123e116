"""ctypes loader of tests/dsac_compact_ref.c — TEST INFRASTRUCTURE ONLY: the CPU restatement of the masked RGB DSAC* solver and
its backward pass under the compact sampler, and of mask_select on its own.

`load(tmpdir)` compiles the C file (gcc -O2 -ffp-contract=off, a few seconds; it includes tests/dsac_masked_bwd_ref.c and
tests/dsac_masked_ref.c) against the product's shared headers crossloc_amd/csrc/xl_dsac_math.h and xl_dsac_reduce.h into `tmpdir`
and returns the front-end; the test modules do that in a module-scoped fixture, so nothing is written into the repository tree.
`build_program(tmpdir, sanitize=True)` builds the same file with its own main() as an executable, with AddressSanitizer and
UBSan."""
import ctypes
import os

import numpy as np

from rgbd_ref_common import HERE, _ptr, compile_lib, compile_program

SRC = os.path.join(HERE, "dsac_compact_ref.c")
DBG = 28
REC = 64                                  # doubles per hypothesis in the restatement's record
FIELDS = 53                               # of which the documented fields of XL_DSAC_BWD_REC


class Ref:
    def __init__(self, path):
        L = ctypes.CDLL(path)
        ci, cf, vp, i64, u64, u32 = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint32
        L.xc_mask_select.restype = ci
        L.xc_mask_select.argtypes = [vp, ci, ci]
        L.xc_forward_rgb_compact.restype = ci
        L.xc_forward_rgb_compact.argtypes = [vp, i64, i64, i64, ci, ci, vp, vp, vp, ci, cf, cf, cf, cf, cf, cf, ci, u64, u64, u32,
                                             vp, vp, vp, vp]
        L.xc_backward_rgb_compact.restype = ci
        L.xc_backward_rgb_compact.argtypes = [vp, i64, i64, i64, ci, ci, vp, vp, i64, i64, i64, vp, ci, cf, cf, cf, cf, cf, cf, cf,
                                              cf, cf, ci, u64, u64, u32, vp, vp, vp, vp, vp]
        self.L = L

    def mask_select(self, mask, k):
        """The index of the usable cell of rank k of `mask` (flattened in row-major order), or -1 when k is out of range"""
        mask = np.ascontiguousarray(np.asarray(mask).astype(np.uint8).reshape(-1))
        return int(self.L.xc_mask_select(_ptr(mask), int(mask.size), int(k)))

    def forward(self, coords, mask, n_hyp, thr, focal, ppx, ppy, alpha, max_reproj, sub, seed=1305, image=0, max_tries=1000000):
        """One image: coords float32 [3,Ho,Wo] (any strides), mask [Ho,Wo] (nonzero / True = usable).  Returns a dict in the
        names of oracle.forward_rgb(debug=True) plus pose [4,4] float32, status and the raw dbg [28]."""
        coords = np.asarray(coords)
        assert coords.dtype == np.float32 and coords.ndim == 3 and coords.shape[0] == 3
        _, Ho, Wo = coords.shape
        mask = np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
        assert mask.shape == (Ho, Wo)
        sc, sy, sx = (s // coords.itemsize for s in coords.strides)
        pose = np.zeros((4, 4), np.float32)
        status = np.full(1, -1, np.int32)
        cells = np.zeros((n_hyp, 4), np.int32)
        tries = np.zeros(n_hyp, np.int32)
        scores = np.zeros(n_hyp, np.float64)
        dbg = np.zeros(DBG, np.float64)
        rc = self.L.xc_forward_rgb_compact(_ptr(coords), sc, sy, sx, Ho, Wo, _ptr(mask), _ptr(pose), _ptr(status), int(n_hyp),
                                           float(thr), float(focal), float(ppx), float(ppy), float(alpha), float(max_reproj),
                                           int(sub), int(seed), int(image), int(max_tries), _ptr(cells), _ptr(tries),
                                           _ptr(scores), _ptr(dbg))
        if rc != 0:
            raise RuntimeError("dsac_compact_ref forward failed: %d" % rc)
        return dict(pose=pose, status=int(status[0]), cells=cells, tries=tries, scores=scores, dbg=dbg, winner=int(dbg[0]),
                    rounds=int(dbg[1]), inliers=int(dbg[2]), lm_evals=int(dbg[3]), pose0=dbg[4:16].copy(), pose1=dbg[16:28].copy())

    def backward(self, coords, mask, gt_pose, n_hyp, thr, focal, ppx, ppy, w_rot, w_trans, soft_clamp, alpha, max_reproj, sub,
                 seed=1305, image=0, max_tries=1000000, grad=None):
        """One image: coords float32 [3,Ho,Wo] (any strides), mask [Ho,Wo] (nonzero / True = usable), gt_pose [4,4] cam->world;
        grad float32 [3,Ho,Wo] is the incoming gradient (zeros when None) and is not modified: the result is a copy.  Returns a
        dict: loss, status, rec [n_hyp,53], grad, tries [n_hyp], cells [n_hyp,4]."""
        coords = np.asarray(coords)
        assert coords.dtype == np.float32 and coords.ndim == 3 and coords.shape[0] == 3
        _, Ho, Wo = coords.shape
        mask = np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
        assert mask.shape == (Ho, Wo)
        g = np.zeros((3, Ho, Wo), np.float32) if grad is None else np.array(grad, dtype=np.float32, order="C")
        assert g.shape == (3, Ho, Wo)
        gt = np.ascontiguousarray(np.asarray(gt_pose, dtype=np.float32).reshape(16))
        sc, sy, sx = (s // coords.itemsize for s in coords.strides)
        loss = np.full(1, -1.0, np.float64)
        status = np.full(1, -1, np.int32)
        rec = np.zeros((n_hyp, REC), np.float64)
        tries = np.zeros(n_hyp, np.int32)
        cells = np.zeros((n_hyp, 4), np.int32)
        rc = self.L.xc_backward_rgb_compact(_ptr(coords), sc, sy, sx, Ho, Wo, _ptr(mask), _ptr(g), Ho * Wo, Wo, 1, _ptr(gt),
                                            int(n_hyp), float(thr), float(focal), float(ppx), float(ppy), float(w_rot),
                                            float(w_trans), float(soft_clamp), float(alpha), float(max_reproj), int(sub),
                                            int(seed), int(image), int(max_tries), _ptr(loss), _ptr(status), _ptr(rec),
                                            _ptr(tries), _ptr(cells))
        if rc != 0:
            raise RuntimeError("dsac_compact_ref backward failed: %d" % rc)
        return dict(loss=float(loss[0]), status=int(status[0]), rec=np.ascontiguousarray(rec[:, :FIELDS]), grad=g, tries=tries,
                    cells=cells)


def load(tmpdir):
    return Ref(compile_lib(tmpdir, SRC, "dsac_compact_ref"))


def build_program(tmpdir, sanitize=True):
    """The restatement with its own main() as an executable; with `sanitize` under AddressSanitizer and UBSan."""
    return compile_program(tmpdir, SRC, "dsac_compact_ref", "XC_MAIN", sanitize)
