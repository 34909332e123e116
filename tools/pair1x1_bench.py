"""Timing of the 1x1 layers of the flagship plan on their own (csrc/xl_gemm_pair.hip, 256 x 256 tiles): the NORM form and the residual
form at 512 -> 512 and the plain form at 256 -> 512 and 512 -> 512, each with bias and the GroupNorm partial sums of its output, on
B frames of 60 x 90 pixels (random data).
python tools/pair1x1_bench.py [B=95]        XL_PAIR_CLK=1: shader ticks of the epilogue's phases per wave and tile, one line per form"""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from crossloc_amd import networks

B = int(sys.argv[1]) if len(sys.argv) > 1 else 95
H, W, N = 60, 90, 512
M = B * H * W
L = networks._bind()
g = torch.Generator(device="cuda").manual_seed(1)
x = torch.randn(M, 512, device="cuda", generator=g) * 2.0 + 0.5
r = torch.randn(M, 512, device="cuda", generator=g).clamp(min=0)
out = torch.empty(M, N, device="cuda")
coef = torch.stack([torch.rand(B, 512, device="cuda", generator=g) + 0.5, torch.randn(B, 512, device="cuda", generator=g)], 2).contiguous()
bias = torch.randn(N, device="cuda", generator=g)
scale = torch.tensor([2.0 ** 8, 2.0 ** -8], device="cuda")
G, nchunks = N // 16, (H * W + 255) // 256 + 1
stats = torch.zeros(B * nchunks * G * 2, dtype=torch.float64, device="cuda")
packed = {}
for cin in (256, 512):
    w = torch.randn(N, cin, device="cuda", generator=g) * (2.0 / cin) ** 0.5
    packed[cin] = torch.zeros(2 * N * cin + 4, dtype=torch.int16, device="cuda")
    networks._check(L.xl_cnn_pair_weight(w.data_ptr(), packed[cin].data_ptr(), N, cin, 1, None))


def op(kind, cin):
    o = networks.XlOp()
    o.type = networks.XL_OP_CONV
    o.B, o.Hi, o.Wi, o.Cin, o.Ho, o.Wo, o.Cout = B, H, W, cin, H, W, N
    o.ksize, o.stride, o.ld_in, o.ld_out, o.reserved_i = 1, 1, 512, N, 256        # (256 -> 512: the first 256 channels of x)
    o.flags = networks.CONV_SPLIT_BF16 | networks.CONV_SPLIT_IL | networks.CONV_PAIR_F16
    if kind != "plain":
        o.flags |= networks.CONV_NORM_IN | networks.CONV_NORM_RELU
        o.aux2 = coef.data_ptr()
    if kind == "residual":
        o.flags |= networks.CONV_NORM_ADD
        o.aux, o.ld_aux = r.data_ptr(), 512
    o.in_, o.w, o.bias, o.out, o.scale = x.data_ptr(), packed[cin].data_ptr(), bias.data_ptr(), out.data_ptr(), scale.data_ptr()
    o.stats, o.groups, o.nchunks = stats.data_ptr(), G, nchunks
    return (networks.XlOp * 1)(o)


st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
forms = [("NORM", 512), ("residual", 512), ("plain", 256), ("plain", 512)]
if os.environ.get("XL_PAIR_CLK"):               # (the phase clocks synchronise after every launch: their own run)
    for kind, cin in forms:
        for _ in range(3):
            networks._check(L.xl_cnn_run(op(kind, cin), 1, st))
    torch.cuda.synchronize()
    sys.exit(0)
for kind, cin in forms:
    arr = op(kind, cin)
    for _ in range(5):
        networks._check(L.xl_cnn_run(arr, 1, st))
    times = []
    for _ in range(5):                           # five groups of ten launches: the spread beside the mean
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            networks._check(L.xl_cnn_run(arr, 1, st))
        e1.record(); torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 10)
    times.sort()
    fl = 3 * 2.0 * M * N * cin
    print("%-8s %d -> %d  %.4f ms (min %.4f, max %.4f)  %.0f TFLOP/s on the pipe" % (kind, cin, N, times[2], times[0], times[-1], fl / times[2] / 1e9))
