#!/usr/bin/env python
"""Bit patterns of the 1x1 pair GEMMs (csrc/xl_gemm_pair.hip: pair_conv1x1_kernel, pair_conv1x1_res_kernel) on seeded inputs.

    python tools/pair1x1_golden.py            # record tests/golden/pair1x1_bitwise.npz with the library that is built
    python tools/pair1x1_golden.py --check    # compare the library that is built against the record

A change to these kernels that leaves their arithmetic alone (register allocation, scheduling, where a value is kept) must not
move a bit of the output or of the fp64 GroupNorm partial sums.  The record is made ONCE, from the commit before such a change, and
tests/test_pair_conv1x1_bitwise_gpu.py holds every later build to it.  Per case it keeps
    sha256 of the output tensor's bytes (the comparison), the statistics partials in full,
    and one 64-bit sum of the output's bit patterns per 32 rows (position-weighted): which rows differ when the hash does.
The inputs come from torch's CPU generator (seeded per case), so recording and checking see the same operands.
"""
import ctypes
import hashlib
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "pair1x1_bitwise.npz")

# (name, kind, cin, cout, B, H, W, form)   kind: norm = GroupNorm + ReLU on load, plain, res = norm + residual + ReLU on load (all three
# with bias and the statistics of the output), acc = out += product, z = Z independent products (no bias, no statistics);
# form: the tile form (op.reserved_i; negative: tiles start at image boundaries, "tpi"); for kind z, B is Z and H * W is T.
CASES = [
    # one image of 5400 pixels: 22 row tiles, the last one ends inside the image's last rows (M is no multiple of 256)
    ("norm_512_b1", "norm", 512, 512, 1, 60, 90, 256),
    ("plain_256_b1", "plain", 256, 512, 1, 60, 90, 256),
    ("res_512_b1", "res", 512, 512, 1, 60, 90, 256),
    ("acc_256_b1", "acc", 256, 512, 1, 60, 90, 256),
    # two images of 888 pixels: tile 3 straddles them, both statistics slots are live
    ("norm_256_b2", "norm", 256, 512, 2, 24, 37, 256),
    ("plain_512_b2", "plain", 512, 512, 2, 24, 37, 256),
    ("res_256_b2", "res", 256, 512, 2, 24, 37, 256),
    ("acc_512_b2", "acc", 512, 512, 2, 24, 37, 256),
    # three images, tiles per image
    ("norm_512_b3_tpi", "norm", 512, 512, 3, 24, 37, -256),
    ("plain_256_b3_tpi", "plain", 256, 512, 3, 24, 37, -256),
    ("res_512_b3_tpi", "res", 512, 512, 3, 24, 37, -256),
    # 338 tiles on 256 workgroups: an epilogue with another tile behind it (its stores in flight under the next K-loop)
    ("norm_512_b8", "norm", 512, 512, 8, 60, 90, 256),
    ("plain_512_b8", "plain", 512, 512, 8, 60, 90, 256),
    ("res_512_b8", "res", 512, 512, 8, 60, 90, 256),
    # Z-batched (the kernel's ZB = 1 and ZB = 2 instantiations), 300 rows each: a ragged second row tile
    ("z_256", "z", 256, 512, 3, 1, 300, 256),
    ("z_512", "z", 512, 512, 3, 1, 300, 256),
]


def _scale_for(torch, maxabs, slack):
    e = 14 - math.frexp(max(maxabs, 1e-30))[1] - slack
    s = math.ldexp(1.0, e)
    return torch.tensor([s, 1.0 / s], dtype=torch.float32, device="cuda")


def run_case(case):
    """-> (out [rows, cout] fp32 on the device, statistics partials as a CPU float64 tensor or None)"""
    import torch
    from crossloc_amd import networks
    name, kind, cin, cout, B, H, W, form = case
    L = networks._bind()
    g = torch.Generator().manual_seed(sum(name.encode()) * 7919 + cin)
    PAIR = networks.CONV_SPLIT_BF16 | networks.CONV_SPLIT_IL | networks.CONV_PAIR_F16

    def pair_weight(w2d):
        rows, K = w2d.shape
        dst = torch.zeros(2 * rows * K + 4, dtype=torch.int16, device="cuda")
        networks._check(L.xl_cnn_pair_weight(w2d.contiguous().data_ptr(), dst.data_ptr(), rows, K, 1, None))
        torch.cuda.synchronize()
        return dst

    def run(op):
        arr = (networks.XlOp * 1)(op)
        networks._check(L.xl_cnn_run(arr, 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()

    op = networks.XlOp()
    op.type = networks.XL_OP_CONV
    op.ksize, op.stride, op.flags = 1, 1, PAIR
    if kind == "z":
        Z, T = B, H * W
        V = (torch.randn(Z, T, cin, generator=g) * 2.0).cuda()
        U = (torch.randn(Z, cout, cin, generator=g) * (2.0 / cin) ** 0.5 * torch.logspace(-1, 1, Z)[:, None, None]).cuda()
        Up = torch.zeros(2 * Z * cout * cin + 4 * Z, dtype=torch.int16, device="cuda")
        for z in range(Z):                                           # one scale per matrix: pack one by one, gather the tails
            one = pair_weight(U[z])
            Up[2 * z * cout * cin:2 * (z + 1) * cout * cin] = one[:2 * cout * cin]
            Up[2 * Z * cout * cin:].view(torch.float32)[Z + z] = one[2 * cout * cin:].view(torch.float32)[1]
        scale = _scale_for(torch, V.abs().max().item(), 3)
        out = torch.full((Z * T, cout), float("nan"), device="cuda")
        op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout = 1, T, 1, cin, T, 1, cout
        op.ld_in, op.ld_out, op.nchunks2, op.reserved_i = cin, cout, Z, form
        op.flags |= networks.CONV_SPLIT_ACT
        op.in_, op.w, op.out, op.scale = V.data_ptr(), Up.data_ptr(), out.data_ptr(), scale.data_ptr()
        run(op)
        return out, None

    M = B * H * W
    x = (torch.randn(M, cin, generator=g) * 2.0 + 0.5).cuda()
    w = (torch.randn(cout, cin, generator=g) * (2.0 / cin) ** 0.5).cuda()
    bias = torch.randn(cout, generator=g).cuda()
    coef = torch.stack([torch.rand(B, cin, generator=g) + 0.5, torch.randn(B, cin, generator=g)], 2).contiguous().cuda()
    wp = pair_weight(w)
    op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout = B, H, W, cin, H, W, cout
    op.ld_in, op.ld_out, op.reserved_i = cin, cout, form
    op.in_, op.w, op.bias = x.data_ptr(), wp.data_ptr(), bias.data_ptr()
    bound = 2.0 * 6.0 + 0.5                                         # |x| stays below six sigma
    if kind in ("norm", "res"):
        op.flags |= networks.CONV_NORM_IN | networks.CONV_NORM_RELU
        op.aux2 = coef.data_ptr()
        bound = bound * 1.5 + 6.0
    if kind == "res":
        r = (torch.randn(M, cin, generator=g).clamp(min=0) * 1.5).cuda()
        op.flags |= networks.CONV_NORM_ADD
        op.aux, op.ld_aux = r.data_ptr(), cin
        bound += 9.0
    scale = _scale_for(torch, bound, 2)
    op.scale = scale.data_ptr()
    st = None
    if kind == "acc":
        out = (torch.randn(M, cout, generator=g) * 3.0).cuda()     # what the product is added to
        op.flags |= networks.CONV_ACCUMULATE
    else:
        out = torch.full((M, cout), float("nan"), device="cuda")
        G, nchunks = cout // 16, (H * W + 255) // 256 + 1
        st = torch.zeros(B * nchunks * G * 2, dtype=torch.float64, device="cuda")
        op.stats, op.groups, op.nchunks = st.data_ptr(), G, nchunks
    op.out = out.data_ptr()
    run(op)
    return out, (None if st is None else st.cpu())


def digest(out, st):
    """-> dict of numpy arrays: sha256 of the output's bytes, 64-bit block sums of its bit patterns, the statistics' bit patterns"""
    import numpy as np
    import torch
    assert torch.isfinite(out).all(), "a row of the output was not written"
    rows, cols = out.shape
    bits = out.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    weighted = bits * (1 + torch.arange(cols, device=out.device, dtype=torch.int64))[None, :]
    pad = (-rows) % 32
    if pad:
        weighted = torch.cat([weighted, torch.zeros(pad, cols, dtype=torch.int64, device=out.device)])
    blocks = weighted.view(-1, 32 * cols).sum(1).cpu().numpy()
    sha = np.frombuffer(hashlib.sha256(out.cpu().numpy().tobytes()).digest(), dtype=np.uint8).copy()
    d = {"sha256": sha, "blocks": blocks}
    if st is not None:
        d["stats"] = st.numpy().view(np.int64).copy()
    return d


def main():
    import numpy as np
    check = "--check" in sys.argv
    golden = np.load(GOLDEN) if check else None
    rec, bad = {}, []
    for case in CASES:
        d = digest(*run_case(case))
        for k, v in d.items():
            rec["%s/%s" % (case[0], k)] = v
            if check and not np.array_equal(golden["%s/%s" % (case[0], k)], v):
                bad.append("%s/%s" % (case[0], k))
        print("%-18s sha256 %s%s" % (case[0], bytes(d["sha256"]).hex()[:16], "" if "stats" not in d else "  %d statistics entries" % d["stats"].size))
    if check:
        print("DIFFERS: " + ", ".join(bad) if bad else "all %d cases bit-identical to the record" % len(CASES))
        return 1 if bad else 0
    np.savez_compressed(GOLDEN, **rec)
    print("%s: %d bytes" % (GOLDEN, os.path.getsize(GOLDEN)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
