"""Generates tests/golden/eval_metrics.npz by importing the REFERENCE's utils/evaluation.py (/root/reference, available only
in the build container) with stub modules for the packages it imports but these functions never use - the recipe of
make_golden.py.  Run with `python3 -B tests/golden/make_eval_golden.py`.  The fixture holds OUTPUTS only; the inputs are
regenerated from tests/golden/eval_inputs.py on both sides (a checksum of them is stored to catch generator drift).

Reference entry points exercised, each in fp32 (as the evaluation loop runs them) and on `.double()` inputs:
  utils/evaluation.py:247-267  depth_eval      -> <case>_depth32 / _depth64  = [abs_rel, rms] over the whole batch
  utils/evaluation.py:294-316  normal_eval     -> <case>_normal32 / _normal64 = mean angular error (deg) over the whole batch
  utils/evaluation.py:388-415  semantic_eval   -> <case>_sem32 / _sem64 = [3,B] rows miou, fwiou, acc per image
  utils/evaluation.py:373-378  SemanticsEvaluator._generate_matrix -> <case>_cm [B,6,6] per-image confusion matrices
and, for the per-image rows, the same depth / normal functions called on every image alone (<case>_depth64_img [B,2],
<case>_normal64_img [B]; NaN for the image without a valid cell) and on the groups of 4 consecutive frames the reference
loader forms (utils/evaluation.py:69): <case>_depth64_grp [G,2], <case>_normal64_grp [G].
"""
import builtins
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

for n in ['cv2', 'dsacstar', 'matplotlib', 'matplotlib.pyplot', 'dataloader', 'dataloader.dataloader', 'networks',
          'networks.networks', 'tqdm', 'skimage', 'skimage.transform', 'transforms3d', 'transforms3d.quaternions']:
    sys.modules[n] = types.ModuleType(n)
sys.modules['matplotlib'].pyplot = sys.modules['matplotlib.pyplot']
sys.modules['dataloader.dataloader'].CamLocDataset = None
sys.modules['networks.networks'].TransPoseNet = sys.modules['networks.networks'].Network = None
q = sys.modules['transforms3d.quaternions']; q.mat2quat = q.quat2mat = None
t = sys.modules['skimage.transform']; t.rotate = t.resize = None
sys.path.insert(0, '/root/reference')
from utils.evaluation import depth_eval, normal_eval, semantic_eval, SemanticsEvaluator   # noqa: E402

sys.path.insert(0, HERE)
import eval_inputs                                              # noqa: E402

_print = builtins.print


def main():
    out = {}
    T = torch.from_numpy
    for tag, (B, H, W) in eval_inputs.CASES.items():
        o, g = eval_inputs.depth_inputs(tag)
        d, g = T(o[:, :1].copy()), T(g)
        out[tag + "_depth32"] = np.array([float(v) for v in depth_eval(d, g, -1)], np.float64)
        out[tag + "_depth64"] = np.array([float(v) for v in depth_eval(d.double(), g.double(), -1)], np.float64)
        out[tag + "_depth64_img"] = np.array([[float(v) for v in depth_eval(d[b:b + 1].double(), g[b:b + 1].double(), -1)]
                                              for b in range(B)], np.float64)
        out[tag + "_depth64_grp"] = np.array([[float(v) for v in depth_eval(d[s:s + 4].double(), g[s:s + 4].double(), -1)]
                                              for s in range(0, B, 4)], np.float64)
        out[tag + "_depth_checksum"] = np.array(eval_inputs.checksum(o, g.numpy()))

        o, g = eval_inputs.normal_inputs(tag)
        p, g = T(o[:, :2].copy()), T(g)
        out[tag + "_normal32"] = np.array(float(normal_eval(p, g, -1)), np.float64)
        out[tag + "_normal64"] = np.array(float(normal_eval(p.double(), g.double(), -1)), np.float64)
        out[tag + "_normal64_img"] = np.array([float(normal_eval(p[b:b + 1].double(), g[b:b + 1].double(), -1))
                                               for b in range(B)], np.float64)
        out[tag + "_normal64_grp"] = np.array([float(normal_eval(p[s:s + 4].double(), g[s:s + 4].double(), -1))
                                               for s in range(0, B, 4)], np.float64)
        out[tag + "_normal_checksum"] = np.array(eval_inputs.checksum(o, g.numpy()))

    for tag, (B, H, W) in eval_inputs.SEM_CASES.items():
        o, lab = eval_inputs.semantics_inputs(tag)
        lg, lb = T(o[:, :6].copy()), T(lab)
        ev = SemanticsEvaluator(6)
        with np.errstate(divide="ignore", invalid="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                builtins.print = lambda *a, **k: None
                try:
                    cls, miou, fwiou, acc = semantic_eval(lg, lb, mute=True)
                    cls64, miou64, fwiou64, acc64 = semantic_eval(lg.double(), lb.double(), mute=True)
                finally:
                    builtins.print = _print
        assert torch.equal(cls, cls64)
        out[tag + "_sem32"] = np.stack([miou, fwiou, acc]).astype(np.float64)
        out[tag + "_sem64"] = np.stack([miou64, fwiou64, acc64]).astype(np.float64)
        out[tag + "_cm"] = np.stack([ev._generate_matrix(lab[b, 0], cls[b].numpy()) for b in range(B)]).astype(np.int64)
        out[tag + "_sem_checksum"] = np.array(eval_inputs.checksum(o, lab))
    np.savez_compressed(os.path.join(HERE, "eval_metrics.npz"), **out)
    _print("eval_metrics.npz", {k: (v.shape if v.ndim else float(v)) for k, v in out.items()})


if __name__ == "__main__":
    main()
