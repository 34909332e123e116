"""Recorder of tests/golden/dsac_oracle_pin.npz: the bits oracle/libxl_oracle.so produced at the commit BEFORE the solver's
lane-local arithmetic moved into crossloc_amd/csrc/xl_dsac_math.h (when the oracle still carried its own copy of every
formula).  The GPU==oracle tests cannot see a reordering made on both sides at once; this fixture pins the oracle, and
through those tests the kernels, to that earlier arithmetic.  The oracle uses only + - * / sqrt floor without contraction, so
the recorded bits do not depend on the compiler.

    python tests/golden/make_dsac_oracle_pin.py          # rewrites the fixture from the oracle of the checked-out tree

Re-record only when the arithmetic is changed on purpose.  tests/test_oracle_dsac_pin.py calls compute() and compares.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from crossloc_amd import synth                   # noqa: E402
from oracle import dsac_oracle as xo             # noqa: E402

PATH = os.path.join(HERE, "dsac_oracle_pin.npz")
FRAMES, FWD_HYP, BWD_HYP = 16, 64, 16
FWD = dict(thr=10.0, focal=synth.FOCAL, ppx=360.0, ppy=240.0, alpha=100.0, max_reproj=100.0, sub=8)
BWD = dict(FWD, w_rot=1.0, w_trans=1.0, soft_clamp=100.0)
CAM = (480.0, 360.0, 240.0)


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def _forward(out, tag, coords, n_hyp, **kw):
    pose, d = xo.forward_rgb(coords, n_hyp, debug=True, **kw)
    out[tag + "pose"] = pose
    out[tag + "cells"], out[tag + "tries"], out[tag + "scores"] = d["cells"].astype(np.int16), d["tries"], d["scores"]
    out[tag + "counts"] = np.array([d["winner"], d["rounds"], d["inliers"], d["lm_evals"]], np.int64)
    out[tag + "pose01"] = np.concatenate([d["pose0"], d["pose1"]])


def _backward(out, tag, coords, gt_pose, n_hyp, **kw):
    grad = np.zeros_like(coords)
    loss = xo.backward_rgb(coords, grad, gt_pose, n_hyp, **kw)
    flat = grad.reshape(-1)
    out[tag + "loss"] = np.float64(loss)
    out[tag + "grad_sha"] = _sha(grad)
    out[tag + "grad_sample"] = flat[::max(1, flat.size // 256)][:256].copy()


def _rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th < 1e-300:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * K


def unit_inputs():
    """Fixed inputs of the xo_test_* entry points (a few dozen each).  They are stored in the fixture next to the results,
    and the test reads them from there, so the pin does not depend on the random generator."""
    rng = np.random.default_rng(20240607)
    u = {}
    u["in_exp"] = np.concatenate([rng.normal(size=24) * 10.0 ** rng.integers(-3, 3, size=24),
                                  [0.0, -0.0, 709.0, 709.5, -708.0, -708.5, 1e-300, np.inf, -np.inf, np.nan, 0.5 * np.log(2.0)]])
    u["in_sincos"] = np.concatenate([rng.normal(size=24) * 10.0 ** rng.integers(-3, 5, size=24),
                                     [0.0, np.pi / 4, -np.pi / 4, np.pi / 2, -np.pi, 1e6, -1e6, 1e-200]])
    u["in_atan2"] = np.concatenate([rng.normal(size=(28, 2)) * 10.0 ** rng.integers(-6, 6, size=(28, 1)),
                                    [[0.0, 0.0], [0.0, -1.0], [0.0, 1.0], [1.0, 0.0], [-1.0, 0.0], [1.0, 1.0], [-1e-300, -1.0]]])
    # quartics: products of real / complex quadratic factors, then biquadratics (the resolvent cubic's positive root
    # is found by an iteration that never returns exactly zero on finite input, so these go through the general branch
    # too), the same shifted, ones without a real root, and non-finite coefficients: what reaches the degenerate branch
    q = [np.polymul([1.0, a, b], [s, c, d]) for a, b, s, c, d in
         zip(rng.normal(size=24) * 3, rng.normal(size=24) * 3, rng.uniform(0.5, 2, size=24), rng.normal(size=24) * 3,
             rng.normal(size=24) * 3)]
    for p, r in [(3.0, -4.0), (5.0, 4.0), (-5.0, 4.0), (0.0, -1.0), (0.0, 0.0), (2.0, 1.0), (7.0, -18.0), (4.0, 3.0),
                 (1.0, -2.0), (6.0, 9.0), (0.0, 1.0), (10.0, 0.0)]:
        q.append(np.array([1.0, 0.0, p, 0.0, r]))
        q.append(np.poly1d([2.0, 0.0, 2.0 * p, 0.0, 2.0 * r])(np.poly1d([1.0, -1.5])).coeffs)      # the same in x - 1.5
    q += [np.array(c) for c in ([1.0, 0.0, np.nan, 0.0, 1.0], [1e-320, 1.0, 1.0, 1.0, 1.0], [1.0, np.inf, 0.0, 0.0, 0.0],
                                [1.0, 0.0, -np.inf, 0.0, 1.0], [1.0, 0.0, 1.0, 0.0, np.nan])]
    u["in_quartic"] = np.array(q)
    u["in_draws"] = np.stack([rng.integers(0, 2 ** 62, size=32), rng.integers(0, 2 ** 40, size=32),
                              rng.integers(0, 1024, size=32), rng.integers(0, 2 ** 31, size=32),
                              rng.integers(1, 200, size=32), rng.integers(1, 200, size=32)], 1).astype(np.uint64)
    # P3P: points in front of a known camera, exact / perturbed pixels (rejected roots occur in most of them), then
    # collinear and coincident points
    P, uv = [], []
    for k in range(32):
        T = np.linalg.inv(synth.random_pose(rng))
        X = rng.uniform(-200, 200, size=(4, 3)) + synth.SCENE_MEAN - [0, 0, 240.0]
        Xc = X @ T[:3, :3].T + T[:3, 3]
        pix = np.stack([CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[1], CAM[0] * Xc[:, 1] / Xc[:, 2] + CAM[2]], 1)
        if k % 2:
            pix += rng.normal(size=pix.shape) * 3.0
        P.append(X); uv.append(pix)
    P.append(np.array([[0, 0, 50.0], [1, 1, 51.0], [2, 2, 52.0], [3, 0, 50.0]])); uv.append(uv[0])
    P.append(np.array([[0, 0, 50.0], [0, 0, 50.0], [2, 5, 52.0], [3, 0, 50.0]])); uv.append(uv[1])
    u["in_p3p_P"], u["in_p3p_uv"] = np.array(P), np.array(uv)
    u["in_dpnp_obj"] = u["in_p3p_P"][:8].astype(np.float32)
    u["in_r3"] = np.concatenate([rng.normal(size=(28, 3)) * rng.uniform(1e-3, 1.8, size=(28, 1)),
                                 [[0.0, 0.0, 0.0], [1e-17, 0.0, 0.0], [np.pi, 0.0, 0.0], [0.0, np.pi, 0.0],
                                  [2.2, -2.2, 0.1], [1e-9, -1e-9, 1e-9]]])
    u["in_t3"] = rng.normal(size=(len(u["in_r3"]), 3)) * 5 + [0.0, 0.0, 60.0]
    u["in_X3"] = rng.normal(size=(len(u["in_r3"]), 3)) * 10
    u["in_X3"][3] = -u["in_t3"][3]                       # a point in the camera centre: the z guard
    u["in_px"] = rng.uniform(0, 720, size=(len(u["in_r3"]), 2)).astype(np.float32)
    u["in_maxrep"] = np.where(np.arange(len(u["in_r3"])) % 4 == 0, 100.0, 1e9).astype(np.float32)
    A = []
    for k in range(16):
        J = rng.normal(size=(40, 6 if k % 3 else 4)) * rng.uniform(0.1, 100, size=(6 if k % 3 else 4))
        if not k % 3:
            J = J @ rng.normal(size=(4, 6))
        A.append(J.T @ J)
    A.append(np.zeros((6, 6))); A.append(np.eye(6))
    u["in_pinv6"] = np.array(A)
    gt = []
    for k in range(len(u["in_r3"])):
        gt.append(synth.random_pose(rng).astype(np.float32))
    u["in_gt"] = np.array(gt)
    u["in_R9"] = np.array([_rodrigues(r).reshape(9) for r in u["in_r3"]])
    return u


def unit_results(u):
    """Raw results of every xo_test_* entry point on the inputs `u`."""
    o = {}
    f, cx, cy = CAM
    o["exp"] = np.array([xo.exp(x) for x in u["in_exp"]])
    o["sincos"] = np.array([xo.sincos(x) for x in u["in_sincos"]])
    o["atan2"] = np.array([xo.atan2(y, x) for y, x in u["in_atan2"]])
    roots = np.full((len(u["in_quartic"]), 5), np.nan)
    for i, A in enumerate(u["in_quartic"]):
        r = xo.quartic(A)
        roots[i, 0] = len(r)
        roots[i, 1:1 + len(r)] = r
    o["quartic"] = roots
    o["draws"] = np.array([xo.draws(*[int(v) for v in row]) for row in u["in_draws"]])
    p3p = np.zeros((len(u["in_p3p_P"]), 13))
    for i, (P, uv) in enumerate(zip(u["in_p3p_P"], u["in_p3p_uv"])):
        got = xo.p3p(P, uv, f, cx, cy)
        if got is not None:
            p3p[i] = np.concatenate([[1.0], got[0].reshape(9), got[1]])
    o["p3p"] = p3p
    o["dpnp"] = np.array([xo.dpnp(obj, uv, f, cx, cy) for obj, uv in zip(u["in_dpnp_obj"], u["in_p3p_uv"])])
    o["log_so3"] = np.array([xo.log_so3(R) for R in u["in_R9"]])
    o["rodrigues_jac"] = np.array([xo.rodrigues_jac(r) for r in u["in_r3"]])
    o["pinv6"] = np.array([xo.pinv6(A) for A in u["in_pinv6"]])
    rows, dobj, loss, dl = [], [], [], []
    for R, t, r, X, px, mr, gt in zip(u["in_R9"], u["in_t3"], u["in_r3"], u["in_X3"], u["in_px"], u["in_maxrep"], u["in_gt"]):
        e, J = xo.resid_row(R, t, r, X, px[0], px[1], f, cx, cy, mr)
        rows.append(np.concatenate([[e], J]))
        dobj.append(xo.dproject_dobj(R, t, X, px[0], px[1], f, cx, cy, mr))
        for cut in (100.0, 0.5):
            loss.append(xo.pose_loss(R, t, gt, 1.0, 100.0, cut))
            dl.append(xo.dloss(R, t, r, gt, 1.0, 100.0, cut))
    # an estimate that equals the ground truth: the guarded branches of the loss derivative
    gt = u["in_gt"][0].astype(np.float64)
    Rw, tw = gt[:3, :3].T, -gt[:3, :3].T @ gt[:3, 3]
    loss.append(xo.pose_loss(Rw, tw, gt, 1.0, 100.0, 100.0))
    dl.append(xo.dloss(Rw, tw, xo.log_so3(Rw), gt, 1.0, 100.0, 100.0))
    o["resid_row"], o["dproject_dobj"], o["pose_loss"], o["dloss"] = np.array(rows), np.array(dobj), np.array(loss), np.array(dl)
    sc = synth.make_scene(77, Ho=9, Wo=11)
    o["score"] = np.array([xo.score(sc["coords"], R.reshape(3, 3), t, 10.0, 100.0, 100.0, f, 44.0, 36.0, 8)
                           for R, t in zip(u["in_R9"][:8], u["in_t3"][:8])]
                          + [xo.score(sc["coords"][:, ::2, ::3], np.eye(3), np.zeros(3), 10.0, 100.0, 100.0, f, 44.0, 36.0, 8)])
    return o


def scene_results():
    o, frames = {}, []
    for b in range(FRAMES):
        sc = synth.make_scene(4100 + b, noise=0.5, outlier_ratio=0.1 * (b % 7))
        fr = dict(in_sha=_sha(sc["coords"]))
        _forward(fr, "f_", sc["coords"], FWD_HYP, image=3 + b, **FWD)
        _backward(fr, "b_", sc["coords"], sc["pose"], BWD_HYP, seed=11 + b, image=b, **BWD)
        frames.append(fr)
    for k in frames[0]:                              # one array per quantity, frames stacked
        o["frames_" + k] = np.stack([fr[k] for fr in frames])
    nodata = np.full((3, 60, 90), -1.0, np.float32)
    _forward(o, "nodata_f_", nodata, 8, max_tries=100, **FWD)
    _backward(o, "nodata_b_", nodata, synth.make_scene(1)["pose"], 8, seed=5, max_tries=100, **BWD)
    sc = synth.make_scene(50, noise=0.2, outlier_ratio=0.2, Ho=7, Wo=5)
    cam = dict(ppx=sc["ppx"], ppy=sc["ppy"])
    o["ragged_in_sha"] = _sha(sc["coords"])
    _forward(o, "ragged_f_", sc["coords"], 16, **dict(FWD, **cam))
    _backward(o, "ragged_b_", sc["coords"], sc["pose"], 16, seed=9, **dict(BWD, **cam))
    return o


def compute(unit_in=None):
    """Everything the fixture holds, computed with the oracle of this tree; `unit_in`: the fixture's own in_* arrays."""
    u = unit_in if unit_in is not None else unit_inputs()
    out = dict(u)
    out.update(unit_results(u))
    out.update(scene_results())
    return out


if __name__ == "__main__":
    np.savez_compressed(PATH, **compute())
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))
