"""Numpy restatement of the end-to-end step's finishing op (include/crossloc_e2e.h): norms and the scale in float64, the
products and the accumulation in float32 exactly as the rules state them.  Shared by test_e2e_op_gpu.py and
test_e2e_step_gpu.py; independent of the library."""
import numpy as np

F32 = np.float32


def pose_gradient(g, loss, C, weight=1.0, clip_norm=0.0, beta=0.0, out=None):
    """g [B,3,Ho,Wo] float32, loss [B] float64 -> (out [B,C,Ho,Wo] float32, stats [B+1,4] float64)."""
    g = np.asarray(g, F32)
    loss = np.asarray(loss, np.float64)
    B, _, Ho, Wo = g.shape
    weight, clip, beta = F32(weight), F32(clip_norm), F32(beta)           # the ABI passes them as float
    res = np.zeros((B, C, Ho, Wo), F32)
    stats = np.zeros((B + 1, 4), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            g64 = g[b].astype(np.float64)
            n = np.sqrt(np.sum(g64 * g64))
            accepted = bool(np.isfinite(loss[b]) and np.isfinite(g[b]).all())
            clipped = accepted and clip > 0 and n > np.float64(clip)
            s = F32(np.float64(weight) / B * (np.float64(clip) / n if clipped else 1.0)) if accepted else F32(0)
            t = (s * g[b]).astype(F32) if accepted else np.zeros_like(g[b])
            if beta == 0:
                res[b, :3] = t
            else:
                res[b, :3] = (beta * out[b, :3]).astype(F32) + t
                res[b, 3:] = beta * out[b, 3:]
            stats[b] = [loss[b], n, s, float(accepted)]
    acc = stats[:B, 3] == 1.0
    if acc.any():
        total = 0.0
        for b in range(B):                           # ascending b, as the op sums
            total = total + (stats[b, 0] if acc[b] else 0.0)
        stats[B] = [total / acc.sum(), acc.sum(), stats[:B, 1][acc].max(),
                    sum(1 for b in range(B) if acc[b] and clip > 0 and stats[b, 1] > np.float64(clip))]
    return res, stats


def ulp_distance(a, b):
    """Largest distance, in float32 units in the last place, between two finite float32 arrays of one shape."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()

    def ordered(x):                                  # the integers order like the floats
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(ordered(a) - ordered(b)).max()) if a.size else 0
