"""GPU parity of the CNN kernels (through the C ABI op list) against plain PyTorch fp32 on the CPU and
against the golden outputs of the imported reference network.  Tolerances are fp32 summation-order level:
|err| <= 2e-4 * max|ref| per op, 1e-3 end to end (29 convs + 28 GroupNorms)."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import guarded                             # noqa: E402
torch = guarded.torch_proxy()              # empty / zeros / full (_like) on the device: between guard bands
import torch.nn as nn                      # noqa: E402
import torch.nn.functional as F            # noqa: E402

from crossloc_amd import networks          # noqa: E402
from crossloc_amd.weights import seeded_state_dict   # noqa: E402
from oracle import cnn_oracle              # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "net_forward.npz"))
MEAN = torch.tensor([-455.934, 417.50, 520.31])


@pytest.fixture(autouse=True)
def _guard_bands(monkeypatch):
    """Every device tensor this module allocates (and every packed operand) sits between guard bands: checked after each test."""
    yield from guarded.op_module_check(monkeypatch, networks, __name__)


def _run(ops):
    L = networks._bind()
    arr = (networks.XlOp * len(ops))(*ops)
    networks._check(L.xl_cnn_run(arr, len(ops), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _close(got, ref, tol=2e-4):
    err = (got - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1e-6)
    assert err <= tol * scale, "max err %g vs scale %g" % (err, scale)


@pytest.mark.parametrize("cin,cout,k,s,B,H,W", [
    (32, 64, 3, 2, 2, 20, 28), (64, 128, 3, 2, 2, 18, 22), (128, 256, 3, 2, 1, 16, 24),
    (256, 256, 3, 1, 2, 9, 13), (256, 512, 3, 1, 1, 8, 12), (512, 512, 3, 1, 3, 9, 13),
    (256, 256, 1, 1, 2, 9, 13), (256, 512, 1, 1, 1, 8, 12), (512, 512, 1, 1, 2, 15, 9),
    (1536, 512, 3, 1, 1, 8, 12), (1536, 512, 1, 1, 1, 8, 12), (512, 512, 3, 1, 1, 60, 90)])
def test_igemm_conv_vs_torch(cin, cout, k, s, B, H, W):
    g = torch.Generator().manual_seed(cin * 7 + cout + k + s)
    x = torch.randn(B, cin, H, W, generator=g)
    conv = nn.Conv2d(cin, cout, k, s, k // 2)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (cin * k * k)) ** 0.5)
        conv.bias.copy_(torch.randn(cout, generator=g))
        ref = conv(x)
    L = networks._bind()
    xd = _nhwc(x).cuda()
    wsrc = conv.weight.detach().cuda().contiguous()
    wd = torch.empty_like(wsrc)
    networks._check(L.xl_cnn_pack_conv_weight(wsrc.data_ptr(), wd.data_ptr(), cout, cin, k, None))
    bd = conv.bias.detach().cuda()
    Ho, Wo = ref.shape[2], ref.shape[3]
    out = torch.full((B, Ho, Wo, cout), float("nan"), device="cuda")
    op = networks.XlOp()
    op.type = networks.XL_OP_CONV
    op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout = B, H, W, cin, Ho, Wo, cout
    op.ksize, op.stride, op.ld_in, op.ld_out = k, s, cin, cout
    op.in_, op.w, op.bias, op.out = xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr()
    _run([op])
    _close(out.cpu().permute(0, 3, 1, 2), ref)


@pytest.mark.parametrize("cin,cout,B,H,W,relu", [(512, 512, 3, 12, 16, True), (256, 256, 2, 13, 17, True), (512, 512, 2, 60, 90, True),
                                                   (1536, 512, 2, 12, 16, False), (512, 512, 1, 16, 8, True)])
def test_conv1x1_normalise_on_load_with_statistics(cin, cout, B, H, W, relu):
    """XL_CONV_NORM_IN: the conv consumes the RAW output of its producer and applies the producer's GroupNorm (+ReLU) to
    the A operand on its way into LDS (per-(image, channel) {scale, shift} pairs).  Tiles straddle image boundaries
    (H*W is not a multiple of 128), and the launch also emits the GroupNorm statistics of its own output."""
    g = torch.Generator().manual_seed(cin + cout + B + H)
    x = torch.randn(B, cin, H, W, generator=g) * 3.0 + 1.0
    coef = torch.stack([torch.rand(B, cin, generator=g) + 0.5, torch.randn(B, cin, generator=g)], 2)     # [B][C][{scale, shift}]
    conv = nn.Conv2d(cin, cout, 1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / cin) ** 0.5)
        conv.bias.copy_(torch.randn(cout, generator=g))
        xn = x.double() * coef[:, :, 0, None, None].double() + coef[:, :, 1, None, None].double()
        if relu:
            xn = xn.clamp(min=0)
        ref = F.conv2d(xn, conv.weight.double(), conv.bias.double())
    L = networks._bind()
    xd = _nhwc(x).cuda()
    wsrc = conv.weight.detach().cuda().contiguous()
    wd = torch.empty_like(wsrc)
    networks._check(L.xl_cnn_pack_conv_weight(wsrc.data_ptr(), wd.data_ptr(), cout, cin, 1, None))
    bd, cd = conv.bias.detach().cuda(), coef.contiguous().cuda()
    out = torch.full((B, H, W, cout), float("nan"), device="cuda")
    G, tile = 32, 128
    nchunks = (H * W + tile - 1) // tile + 1
    stats = torch.zeros(B * nchunks * G * 2, dtype=torch.float64, device="cuda")
    op = networks.XlOp()
    op.type = networks.XL_OP_CONV
    op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout = B, H, W, cin, H, W, cout
    op.ksize, op.stride, op.ld_in, op.ld_out = 1, 1, cin, cout
    op.flags = networks.CONV_NORM_IN | (networks.CONV_NORM_RELU if relu else 0)
    op.in_, op.w, op.bias, op.out, op.aux2 = xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), cd.data_ptr()
    op.stats, op.groups, op.nchunks = stats.data_ptr(), G, nchunks
    _run([op])
    got = out.cpu().permute(0, 3, 1, 2).double()
    _close(got, ref)
    # statistics of the output: per (image, group) sum and sum of squares over all tiles
    st = stats.cpu().view(B, nchunks, G, 2).sum(1)
    grp = got.reshape(B, G, -1)
    assert torch.allclose(st[:, :, 0], grp.sum(2), rtol=1e-5, atol=1e-3)
    assert torch.allclose(st[:, :, 1], (grp * grp).sum(2), rtol=1e-5)


@pytest.mark.parametrize("cin,cout,B,H,W,norm,relu,stats,pad,per_image", [
    (512, 512, 3, 24, 37, True, True, True, 0, False),     # 888 pixels per image: tiles straddle images, last tile ragged
    (512, 512, 3, 24, 37, True, True, True, 0, True),      # ... tiles that start at image boundaries (batch-invariant plans)
    (512, 512, 2, 60, 90, True, False, True, 0, False),
    (512, 512, 2, 60, 90, False, False, True, 0, True),
    (256, 512, 3, 20, 31, False, False, True, 0, False),   # the res2 skip layer's shape
    (512, 512, 5, 16, 16, False, False, False, 32, False), # exactly one tile per image; operands inside wider tensors
    (512, 256, 2, 33, 20, True, True, False, 64, True),
    (64, 1024, 1, 40, 52, False, False, False, 0, False),
    (512, 512, 8, 60, 90, True, True, True, 0, False),     # 338 tiles on 256 workgroups: second tiles (stores in flight)
    (32, 512, 7, 64, 80, True, True, True, 0, False),      # two K-steps per tile: the operand stream is a tile ahead
    (96, 256, 9, 48, 70, False, False, True, 0, True)])    # six K-steps; per-image tiles of a 3360-pixel map
def test_conv1x1_on_the_split_bf16_pipe(cin, cout, B, H, W, norm, relu, stats, pad, per_image):
    """XL_CONV_SPLIT_BF16 | XL_CONV_SPLIT_IL without batching: a 1x1 convolution whose weights were split into three bf16
    planes on the host and whose fp32 activations are normalised (optionally) and split by the kernel - same tolerance as
    the fp32-MFMA kernel, plus the GroupNorm statistics of the output from 256-row tiles."""
    g = torch.Generator().manual_seed(cin + cout + B + H)
    x = torch.randn(B, cin, H, W, generator=g) * 3.0 + 1.0
    coef = torch.stack([torch.rand(B, cin, generator=g) + 0.5, torch.randn(B, cin, generator=g)], 2)
    conv = nn.Conv2d(cin, cout, 1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / cin) ** 0.5)
        conv.bias.copy_(torch.randn(cout, generator=g))
        xn = x.double()
        if norm:
            xn = xn * coef[:, :, 0, None, None].double() + coef[:, :, 1, None, None].double()
            if relu:
                xn = xn.clamp(min=0)
        ref = F.conv2d(xn, conv.weight.double(), conv.bias.double())
    wide_in = torch.full((B, H, W, cin + pad), float("nan"))
    wide_in[..., pad:] = _nhwc(x)
    xd = wide_in.cuda()
    wd = networks._Plan.split_bf16_interleaved(conv.weight.detach().reshape(cout, cin).cuda(), cin)
    bd, cd = conv.bias.detach().cuda(), coef.contiguous().cuda()
    out = torch.full((B, H, W, cout + pad), float("nan"), device="cuda")
    G, tile = cout // 16, 256
    nchunks = (H * W + tile - 1) // tile + 1
    st = torch.zeros(B * nchunks * G * 2, dtype=torch.float64, device="cuda")
    op = networks.XlOp()
    op.type = networks.XL_OP_CONV
    op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout = B, H, W, cin, H, W, cout
    op.ksize, op.stride, op.ld_in, op.ld_out = 1, 1, cin + pad, cout + pad
    op.flags = networks.CONV_SPLIT_BF16 | networks.CONV_SPLIT_IL
    if norm:
        op.flags |= networks.CONV_NORM_IN | (networks.CONV_NORM_RELU if relu else 0)
        op.aux2 = cd.data_ptr()
    op.in_, op.w, op.bias, op.out = xd.data_ptr() + 4 * pad, wd.data_ptr(), bd.data_ptr(), out.data_ptr()
    if stats:
        op.stats, op.groups, op.nchunks = st.data_ptr(), G, nchunks
    if per_image:
        op.reserved_i = -256
    _run([op, op])                                        # twice: the second launch must overwrite, not accumulate
    got = out.cpu()
    if pad:
        assert torch.isnan(got[..., cout:]).all()
    got = got[..., :cout].permute(0, 3, 1, 2).double()
    _close(got, ref)
    # fp32-class: the same layer through the fp32-MFMA kernel (operand normalised on the host, no statistics), both against
    # the float64 result - the split path must be within a small factor of the fp32 kernel's own rounding error
    with torch.no_grad():
        xin = xn.float() if norm else x
    xf = torch.zeros((B, H, W, cin + pad))
    xf[..., pad:] = _nhwc(xin)
    xfd = xf.cuda()
    wsrc = conv.weight.detach().cuda().contiguous()
    wpk = torch.empty_like(wsrc)
    networks._check(networks._bind().xl_cnn_pack_conv_weight(wsrc.data_ptr(), wpk.data_ptr(), cout, cin, 1, None))
    out32 = torch.full((B, H, W, cout), float("nan"), device="cuda")
    o32 = networks.XlOp()
    o32.type = networks.XL_OP_CONV
    o32.B, o32.Hi, o32.Wi, o32.Cin, o32.Ho, o32.Wo, o32.Cout = B, H, W, cin, H, W, cout
    o32.ksize, o32.stride, o32.ld_in, o32.ld_out = 1, 1, cin + pad, cout
    o32.in_, o32.w, o32.bias, o32.out = xfd.data_ptr() + 4 * pad, wpk.data_ptr(), bd.data_ptr(), out32.data_ptr()
    _run([o32])
    scale = ref.abs().max().item()
    e32 = (out32.cpu().permute(0, 3, 1, 2).double() - ref).abs().max().item() / scale
    esp = (got - ref).abs().max().item() / scale
    assert esp < 2e-6 and esp < 4 * e32 + 2e-7, (esp, e32)
    if stats:
        sums = st.cpu().view(B, nchunks, G, 2)
        if per_image:                                     # one entry per tile of the image's own grid, nothing beyond
            assert (sums[:, (H * W + 255) // 256:] == 0).all()
        sums = sums.sum(1)
        grp = got.reshape(B, G, -1)
        assert torch.allclose(sums[:, :, 0], grp.sum(2), rtol=1e-5, atol=1e-3)
        assert torch.allclose(sums[:, :, 1], (grp * grp).sum(2), rtol=1e-5)


@pytest.mark.parametrize("cin,cout,B,H,W,pad,stats,form", [
    (512, 512, 2, 60, 90, 0, True, 0),        # fc1 behind the decoder's res3 block: the shape the plans use
    (512, 512, 3, 24, 37, 32, True, 0),       # tiles straddle images, ragged last tile, operands inside wider tensors
    (256, 512, 9, 60, 90, 0, False, 0),       # 190 tiles on 256 workgroups... several K-step counts
    (512, 256, 1, 60, 90, 0, True, 128),      # single-frame forms: 128 x 128 tiles
    (512, 512, 1, 60, 90, 0, True, 192)])     # ... 256 x 128
def test_conv1x1_residual_epilogue_on_load_vs_float64(cin, cout, B, H, W, pad, stats, form):
    """XL_CONV_NORM_ADD (round 4, split_conv1x1_res_kernel): the 1x1 layer consumes the RAW output x of a convolution and the
    residual r of its block and applies the block's whole epilogue while loading its operand -
    v = max(max(fmaf(x, scale, shift), 0) + r, 0) - so that GroupNorm + ReLU + residual + ReLU has no pass of its own.  Against a
    float64 convolution of the float64 epilogue, and EQUAL TO THE BIT to the plain NORM-less kernel fed with the epilogue computed
    in fp32 on the host in the same order (fmaf, max, add, max)."""
    g = torch.Generator().manual_seed(cin + cout + B + H)
    x = torch.randn(B, cin, H, W, generator=g) * 2.0 + 0.5
    r = torch.randn(B, cin, H, W, generator=g).clamp(min=0) * 1.5             # (a residual is itself behind a ReLU)
    coef = torch.stack([torch.rand(B, cin, generator=g) + 0.5, torch.randn(B, cin, generator=g)], 2)
    conv = nn.Conv2d(cin, cout, 1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / cin) ** 0.5)
        conv.bias.copy_(torch.randn(cout, generator=g))
        sc, sh = coef[:, :, 0, None, None], coef[:, :, 1, None, None]
        v64 = ((x.double() * sc.double() + sh.double()).clamp(min=0) + r.double()).clamp(min=0)
        ref = F.conv2d(v64, conv.weight.double(), conv.bias.double())
        # the kernel's arithmetic in fp32: one fused multiply-add (float64 product and sum rounded once = fmaf for these magnitudes)
        v32 = ((x.double() * sc.double() + sh.double()).float().clamp(min=0) + r).clamp(min=0)

    def wide(t):
        w = torch.full((B, H, W, cin + pad), float("nan"))
        w[..., pad:] = _nhwc(t)
        return w.cuda()
    xd, rd, vd = wide(x), wide(r), wide(v32)
    wd = networks._Plan.split_bf16_interleaved(conv.weight.detach().reshape(cout, cin).cuda(), cin)
    bd, cd = conv.bias.detach().cuda(), coef.contiguous().cuda()
    G, tile = cout // 16, 128 if form == 128 else 256
    nchunks = (H * W + tile - 1) // tile + 1

    def run(res_form):
        out = torch.full((B, H, W, cout), float("nan"), device="cuda")
        st = torch.zeros(B * nchunks * G * 2, dtype=torch.float64, device="cuda")
        op = networks.XlOp()
        op.type = networks.XL_OP_CONV
        op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout = B, H, W, cin, H, W, cout
        op.ksize, op.stride, op.ld_in, op.ld_out, op.reserved_i = 1, 1, cin + pad, cout, form
        op.flags = networks.CONV_SPLIT_BF16 | networks.CONV_SPLIT_IL
        op.w, op.bias, op.out = wd.data_ptr(), bd.data_ptr(), out.data_ptr()
        if res_form:
            op.flags |= networks.CONV_NORM_IN | networks.CONV_NORM_RELU | networks.CONV_NORM_ADD
            op.in_, op.aux, op.ld_aux, op.aux2 = xd.data_ptr() + 4 * pad, rd.data_ptr() + 4 * pad, cin + pad, cd.data_ptr()
        else:
            op.in_ = vd.data_ptr() + 4 * pad
        if stats:
            op.stats, op.groups, op.nchunks = st.data_ptr(), G, nchunks
        _run([op, op])
        return out.cpu(), st.cpu()
    got, st_res = run(True)
    plain, st_plain = run(False)
    assert torch.equal(got, plain), (got - plain).abs().max()
    assert torch.equal(st_res, st_plain)
    _close(got.permute(0, 3, 1, 2).double(), ref)
    esp = (got.permute(0, 3, 1, 2).double() - ref).abs().max().item() / ref.abs().max().item()
    assert esp < 2e-6, esp


@pytest.mark.parametrize("cin,cout,B,H,W,norm", [(512, 512, 8, 60, 90, True), (96, 256, 1, 60, 90, False), (64, 1024, 3, 17, 23, True)])
def test_conv1x1_split_tile_forms_give_the_same_bits(cin, cout, B, H, W, norm):
    """reserved_i = 256 / 192 / 128: 256 x 256, 256 x 128 and 128 x 128 tiles of the same kernel.  Every output element
    accumulates its K-steps in the same order in all three, so the convolution output is BITWISE the same; the GroupNorm
    partial sums are one entry per row tile (256 rows for the first two forms, 128 for the third) of the same elements."""
    g = torch.Generator().manual_seed(cin + cout + B)
    xd = (torch.randn(B, H, W, cin, generator=g) * 2.0 + 0.5).cuda()
    cd = torch.stack([torch.rand(B, cin, generator=g) + 0.5, torch.randn(B, cin, generator=g)], 2).contiguous().cuda()
    wd = networks._Plan.split_bf16_interleaved((torch.randn(cout, cin, generator=g) * (2.0 / cin) ** 0.5).cuda(), cin)
    bd = torch.randn(cout, generator=g).cuda()
    G = cout // 16
    outs, sums = [], []
    for form in (256, 192, 384, 128):
        rows = 128 if form == 128 else 256
        nchunks = (H * W + rows - 1) // rows + 1
        st = torch.zeros(B * nchunks * G * 2, dtype=torch.float64, device="cuda")
        out = torch.full((B, H, W, cout), float("nan"), device="cuda")
        op = networks.XlOp()
        op.type = networks.XL_OP_CONV
        op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout = B, H, W, cin, H, W, cout
        op.ksize, op.stride, op.ld_in, op.ld_out, op.reserved_i = 1, 1, cin, cout, form
        op.flags = networks.CONV_SPLIT_BF16 | networks.CONV_SPLIT_IL | ((networks.CONV_NORM_IN | networks.CONV_NORM_RELU) if norm else 0)
        op.aux2 = cd.data_ptr() if norm else None
        op.in_, op.w, op.bias, op.out = xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr()
        op.stats, op.groups, op.nchunks = st.data_ptr(), G, nchunks
        _run([op, op])
        outs.append(out.cpu())
        sums.append(st.cpu().view(B, nchunks, G, 2).sum(1))
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    grp = outs[0].double().reshape(B, H * W, G, 16).permute(0, 2, 1, 3).reshape(B, G, -1)
    for s in sums:
        assert torch.allclose(s[:, :, 0], grp.sum(2), rtol=1e-6, atol=1e-3)      # (lane partials are fp32, then fp64)
        assert torch.allclose(s[:, :, 1], (grp * grp).sum(2), rtol=1e-6)


def test_conv_reads_and_writes_channel_slices():
    """ld/offset addressing used by the concat-free MLR fusion."""
    g = torch.Generator().manual_seed(3)
    B, H, W = 1, 6, 10
    wide = torch.randn(B, H, W, 96, generator=g)
    x = wide[..., 32:64].permute(0, 3, 1, 2).contiguous()
    conv = nn.Conv2d(32, 64, 3, 1, 1)
    with torch.no_grad():
        ref = conv(x)
    L = networks._bind()
    wd = torch.empty(conv.weight.shape, device="cuda")
    ws = conv.weight.detach().cuda().contiguous()
    networks._check(L.xl_cnn_pack_conv_weight(ws.data_ptr(), wd.data_ptr(), 64, 32, 3, None))
    xin = wide.cuda()
    outw = torch.zeros(B, H, W, 192, device="cuda")
    op = networks.XlOp()
    op.type = networks.XL_OP_CONV
    op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout = B, H, W, 32, H, W, 64
    op.ksize, op.stride, op.ld_in, op.ld_out = 3, 1, 96, 192
    bd = conv.bias.detach().cuda()
    op.in_, op.w, op.bias, op.out = xin.data_ptr() + 4 * 32, wd.data_ptr(), bd.data_ptr(), outw.data_ptr() + 4 * 64
    _run([op])
    got = outw.cpu()
    _close(got[..., 64:128].permute(0, 3, 1, 2), ref)
    assert got[..., :64].abs().max() == 0 and got[..., 128:].abs().max() == 0


@pytest.mark.parametrize("cin", [3, 1])
def test_conv1_vs_torch(cin):
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 24, 40
    x = torch.rand(B, cin, H, W, generator=g)
    conv = nn.Conv2d(cin, 32, 3, 1, 1)
    with torch.no_grad():
        ref = conv(x)
    wd = conv.weight.detach().permute(2, 3, 1, 0).contiguous().cuda()
    bd = conv.bias.detach().cuda()
    xd = x.cuda()
    out = torch.empty(B, H, W, 32, device="cuda")
    op = networks.XlOp()
    op.type = networks.XL_OP_CONV1
    op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout, op.ld_out = B, H, W, cin, H, W, 32, 32
    op.in_, op.w, op.bias, op.out = xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr()
    _run([op])
    _close(out.cpu().permute(0, 3, 1, 2), ref, 1e-5)


@pytest.mark.parametrize("B,H,W,ppt", [(2, 24, 40, 5), (3, 37, 53, 2), (1, 64, 96, 1),
                                       (2, 24, 40, 0), (3, 37, 53, 0), (1, 64, 96, 0), (2, 100, 203, 0), (1, 480, 720, 0),
                                       (2, 17, 65, 0), (2, 31, 127, 0), (1, 33, 129, 0)])   # one row / column into, one short of, a 16 x 64 tile
def test_conv1_inference_form_vs_torch(B, H, W, ppt):
    """XL_OP_CONV1 with `stats` (statistics-only evaluation), GN_FINAL, XL_OP_CONV1 with aux2 (second evaluation that
    writes relu(groupnorm(conv))) against torch conv2d -> group_norm(32 groups) -> relu; 37x53 leaves a ragged last
    workgroup.  ppt = 0: the matrix-pipe form (conv1_mfma_kernel, exact three-term bf16 splits of image and weights), one
    workgroup per 16 x 64 output tile; ppt > 0: the packed-VALU form."""
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.rand(B, 3, H, W, generator=g)
    conv = nn.Conv2d(3, 32, 3, 1, 1)
    gamma = 1.0 + 0.2 * torch.randn(32, generator=g)
    beta = 0.3 * torch.randn(32, generator=g)
    with torch.no_grad():
        raw = conv(x.double().float()).double()
        ref = torch.relu(F.group_norm(raw, 32, gamma.double(), beta.double(), 1e-5))
    wd = conv.weight.detach().permute(2, 3, 1, 0).contiguous().cuda()
    bd, xd, gd, btd = conv.bias.detach().cuda(), x.cuda(), gamma.cuda(), beta.cuda()
    nch = -(-(H * W) // (256 * ppt)) if ppt else -(-H // 16) * -(-W // 64)
    stats = torch.full((B, nch, 32, 2), float("nan"), dtype=torch.float64, device="cuda")
    coeff = torch.full((B, 32, 2), float("nan"), device="cuda")
    out = torch.full((B, H, W, 32), float("nan"), device="cuda")

    def conv1():
        op = networks.XlOp()
        op.type = networks.XL_OP_CONV1
        op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout, op.ld_out = B, H, W, 3, H, W, 32, 32
        op.groups, op.nchunks, op.reserved_i = 32, nch, ppt
        op.in_, op.w, op.bias = xd.data_ptr(), (wd if ppt else wfr).data_ptr(), bd.data_ptr()
        return op
    wfr = networks._Plan.conv1_fragments(conv.weight.detach().cuda())
    a = conv1()
    a.stats = stats.data_ptr()
    f = networks.XlOp()
    f.type = networks.XL_OP_GN_FINAL
    f.B, f.Hi, f.Wi, f.Cin, f.groups, f.nchunks, f.eps = B, H, W, 32, 32, nch, 1e-5
    f.stats, f.w, f.bias, f.out = stats.data_ptr(), gd.data_ptr(), btd.data_ptr(), coeff.data_ptr()
    b = conv1()
    b.aux2, b.out, b.flags = coeff.data_ptr(), out.data_ptr(), networks.GN_RELU_IN
    _run([a, f, b])
    st = stats.sum(1).cpu()                                              # [B, 32, 2]: per-channel sums
    # (against a float64 convolution: the fp32 CPU convolution above carries its own rounding, whose sum over 345600 pixels
    #  depends on the host's blocking - one box in twenty missed 1e-4 on a channel whose sum is near zero)
    with torch.no_grad():
        raw64 = F.conv2d(x.double(), conv.weight.double(), conv.bias.double(), padding=1)
    assert torch.allclose(st[..., 0], raw64.sum((2, 3)), rtol=1e-6, atol=2e-4)
    assert torch.allclose(st[..., 1], (raw64 * raw64).sum((2, 3)), rtol=1e-6, atol=2e-4)
    got = out.cpu().permute(0, 3, 1, 2).double()
    assert torch.isfinite(got).all()
    print("conv1 inference form %dx%dx%d ppt %d: %.2e of max (bound 2e-5)" % (B, H, W, ppt, (got - ref).abs().max().item() / ref.abs().max().item()))
    _close(got, ref, 2e-5)
    bad = conv1()                                                        # too few workgroups for the image
    bad.stats, bad.nchunks = stats.data_ptr(), max(nch - 1, 0)
    with pytest.raises(RuntimeError):
        _run([bad])


@pytest.mark.parametrize("C,H,W,flags", [(32, 24, 40, 1), (64, 12, 20, 1), (128, 6, 10, 1), (256, 9, 13, 7),
                                          (512, 9, 13, 6), (512, 60, 90, 7), (1536, 8, 12, 0), (32, 480, 720, 1)] +
                         # 255, 256 and 257 pixels: one short of, exactly and one past a 256-pixel chunk of the statistics
                         [(C, H, W, 7) for C in (64, 512) for H, W in ((15, 17), (16, 16), (1, 257))])
def test_groupnorm_vs_torch(C, H, W, flags):
    g = torch.Generator().manual_seed(C + H)
    B = 2
    x = torch.randn(B, C, H, W, generator=g) * 3.0 + 1.5
    aux = torch.randn(B, C, H, W, generator=g)
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    ref = F.group_norm(x, 32, gamma, beta, eps=1e-5)
    if flags & 1:
        ref = F.relu(ref)
    if flags & 2:
        ref = ref + aux
    if flags & 4:
        ref = F.relu(ref)
    xd, ad = _nhwc(x).cuda(), _nhwc(aux).cuda()
    gd, bd = gamma.cuda(), beta.cuda()
    nch = max(1, min(128, (H * W + 255) // 256))
    stats = torch.zeros(B * nch * 32 * 2, dtype=torch.float64, device="cuda")
    out = torch.empty_like(xd)
    st = networks.XlOp()
    st.type = networks.XL_OP_GN_STATS
    st.B, st.Hi, st.Wi, st.Cin, st.groups, st.nchunks, st.ld_in = B, H, W, C, 32, nch, C
    st.in_, st.stats = xd.data_ptr(), stats.data_ptr()
    ap = networks.XlOp()
    ap.type = networks.XL_OP_GN_APPLY
    ap.B, ap.Hi, ap.Wi, ap.Cin, ap.groups, ap.nchunks, ap.ld_in, ap.ld_out, ap.ld_aux = B, H, W, C, 32, nch, C, C, C
    ap.flags, ap.eps = flags, 1e-5
    ap.in_, ap.w, ap.bias, ap.aux, ap.stats, ap.out = (xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), ad.data_ptr(),
                                                       stats.data_ptr(), out.data_ptr())
    _run([st, ap])
    got = out.cpu().permute(0, 3, 1, 2)
    print("groupnorm C %d %dx%d flags %d: %.2e of max (bound 2e-5)" % (C, H, W, flags, (got - ref).abs().max().item() / ref.abs().max().item()))
    _close(got, ref, 2e-5)


def test_head_vs_torch():
    g = torch.Generator().manual_seed(9)
    B, H, W, C = 2, 9, 13, 512
    x = torch.randn(B, C, H, W, generator=g)
    fc3 = nn.Conv2d(C, 4, 1)
    with torch.no_grad():
        fc3.weight.mul_(20.0)                                     # reach both hardtanh bounds
        sc = fc3(x)
        ref = torch.cat([sc[:, :3] + MEAN[None, :, None, None], torch.exp(F.hardtanh(sc[:, 3:], -16.10, 13.82))], 1)
    xd = _nhwc(x).cuda()
    wd = fc3.weight.detach().reshape(4, C).contiguous().cuda()
    bd, md = fc3.bias.detach().cuda(), MEAN.cuda()
    out = torch.empty(B, 4, H, W, device="cuda")
    op = networks.XlOp()
    op.type = networks.XL_OP_HEAD
    op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout, op.n_task, op.n_pos, op.ld_in = B, H, W, C, H, W, 4, 3, 1, C
    op.clamp_lo, op.clamp_hi = -16.10, 13.82
    op.in_, op.w, op.bias, op.aux, op.out = xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), md.data_ptr(), out.data_ptr()
    _run([op])
    got = out.cpu()
    _close(got[:, :3] - MEAN[None, :, None, None], ref[:, :3] - MEAN[None, :, None, None], 1e-4)
    assert torch.allclose(got[:, 3], ref[:, 3], rtol=2e-4)
    assert (got[:, 3] >= np.exp(-16.10) * 0.999).all() and (got[:, 3] <= np.exp(13.82) * 1.001).all()


def test_a_refused_op_is_named_in_the_error():
    """Round 6: a launcher that refuses an op returns a bare status; xl_cnn_run says WHICH op of the list it was (index, type,
    shapes, flags) - the tiny network's head (128 channels) was found that way - and keeps a launcher's own text in front."""
    from crossloc_amd import _lib
    x = torch.zeros(1, 8, 12, 6, device="cuda")
    op = networks.XlOp()
    op.type = networks.XL_OP_HEAD
    op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout, op.n_task, op.n_pos, op.ld_in = 1, 8, 12, 6, 8, 12, 4, 3, 1, 6    # Cin % 4 != 0
    op.in_ = op.w = op.bias = op.aux = op.out = x.data_ptr()
    good = networks.XlOp()
    good.type = networks.XL_OP_HEAD
    good.B, good.Hi, good.Wi, good.Cin, good.Ho, good.Wo, good.Cout, good.n_task, good.n_pos, good.ld_in = 1, 2, 3, 8, 2, 3, 4, 3, 1, 8
    buf = torch.zeros(256, device="cuda")
    good.in_ = good.w = good.bias = good.aux = buf.data_ptr()
    good.out = torch.zeros(64, device="cuda").data_ptr()
    with pytest.raises(_lib.XlError) as e:
        _run([good, op])
    msg = str(e.value)
    assert "op 1 refused" in msg and "type %d" % networks.XL_OP_HEAD in msg and "6 -> 4 channels" in msg, msg
    _run([good])                                                          # (and the library is usable afterwards)


@pytest.mark.parametrize("tag,num_mlr", [("single", 0), ("mlr3", 3)])
def test_network_matches_reference_golden(tag, num_mlr):
    net = networks.TransPoseNet(MEAN, False, False, 2, 2, 3, 1, 32, num_mlr, 0, False)
    net.load_state_dict(seeded_state_dict(net, seed=2021), strict=True)
    net = net.cuda().eval()
    with torch.no_grad():
        y = net(torch.from_numpy(GOLD[tag + "_x"]).cuda()).cpu()
    ref = torch.from_numpy(GOLD[tag + "_y"])
    assert y.shape == ref.shape
    _close(y[:, :3] - MEAN[None, :, None, None], ref[:, :3] - MEAN[None, :, None, None], 1e-3)
    assert torch.allclose(y[:, 3], ref[:, 3], rtol=2e-3)


def test_four_encoder_network_matches_reference_golden():
    """The 4-encoder "CrossLoc-SE" fusion: four encoders write channel slices of one 2048-channel tensor,
    GroupNorm(32, 2048), 1x1 2048->512 skip + 3 fusion layers; fixture generated from the reference network."""
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "net_forward_mlr4.npz"))
    net = networks.TransPoseNet(MEAN, False, False, 1, 1, 3, 1, 32, 4, 0, False)
    net.load_state_dict(seeded_state_dict(net, seed=44), strict=True)
    net = net.cuda().eval()
    with torch.no_grad():
        y = net(torch.from_numpy(gold["mlr4_x"]).cuda()).cpu()
    ref = torch.from_numpy(gold["mlr4_y"])
    assert y.shape == ref.shape == (2, 4, 9, 13)
    _close(y[:, :3] - MEAN[None, :, None, None], ref[:, :3] - MEAN[None, :, None, None], 1e-3)
    assert torch.allclose(y[:, 3], ref[:, 3], rtol=2e-3)


def test_network_full_size_vs_oracle_and_determinism():
    """480x720 (the BASELINE frame size), batch 2: fp32 restatement on the CPU as the checker."""
    net = networks.TransPoseNet(MEAN, False, False, 2, 2, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=3))
    x = torch.rand(2, 3, 480, 720, generator=torch.Generator().manual_seed(1))
    ref = cnn_oracle.transposenet_forward(net.state_dict(), x, 0, 2, 2)
    net = net.cuda()
    y = net(x.cuda())
    y2 = net(x.cuda())
    assert y.shape == (2, 4, 60, 90)
    assert torch.equal(y, y2)                                       # fixed-order reductions: bitwise repeatable
    y = y.cpu()
    _close(y[:, :3] - MEAN[None, :, None, None], ref[:, :3] - MEAN[None, :, None, None], 1e-3)
    assert torch.allclose(y[:, 3], ref[:, 3], rtol=2e-3)
    # per-image results do not depend on the batch they are in (GroupNorm is per image).  The fp64 partial sums of the
    # statistics are grouped by conv tile, and tiles straddle image boundaries differently for other batch sizes, so
    # the match is to the last fp32 bit or two rather than bitwise
    y1 = net(x[1:].cuda()).cpu()
    assert torch.allclose(y1[0, :3], y[1, :3], rtol=0, atol=2e-4)        # |X| ~ 500 m: 2e-4 = 3 ulp
    assert torch.allclose(y1[0, 3], y[1, 3], rtol=1e-4)                  # sigma = exp(s) amplifies the last bits of s


def test_fused_forms_match_the_plain_form_at_full_size(monkeypatch):
    """BASELINE frame size, batch 3: the default inference plan (Winograd F(4x4,3x3), conv-epilogue statistics, GroupNorm
    folded into the Winograd input transform, first layer evaluated twice) against the plainest lowering of the same
    network (direct convolutions, separate statistics and apply passes, first layer materialised) - two independent HIP
    paths, no CPU oracle in the loop, so the check runs at the full size."""
    x = torch.rand(3, 3, 480, 720, generator=torch.Generator().manual_seed(8)).cuda()

    def run():
        net = networks.TransPoseNet(MEAN, False, False, 2, 2, 3, 1)
        net.load_state_dict(seeded_state_dict(net, seed=12))
        net = net.cuda().eval()
        with torch.no_grad():
            return net(x).cpu()
    fused = run()
    for k in ("XL_NO_WINOGRAD", "XL_NO_FUSED_STATS", "XL_NO_DEFERRED_GN", "XL_NO_CONV1_FUSED"):
        monkeypatch.setenv(k, "1")
    plain = run()
    assert torch.isfinite(fused).all() and fused.shape == (3, 4, 60, 90)
    assert (fused[:, :3] - plain[:, :3]).abs().max().item() < 5e-4      # metres at |X| ~ 500 m (1 ulp = 6e-5)
    assert torch.allclose(fused[:, 3], plain[:, 3], rtol=1e-3)


def test_batch_invariant_mode_is_bitwise_batch_independent():
    """net.batch_invariant = True (what the test harness sets: results must not depend on the rank count): the GroupNorm
    sums are chunked per image, and a frame's result is bitwise the same in any batch (the default groups them by conv
    tile: equal to the last bit or two, see the test above)."""
    net = networks.TransPoseNet(MEAN, False, False, 1, 1, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=5))
    net.batch_invariant = True
    net = net.cuda().eval()
    x = torch.rand(3, 3, 128, 192, generator=torch.Generator().manual_seed(2)).cuda()
    with torch.no_grad():
        y = net(x)
        assert torch.equal(net(x[2:])[0], y[2]) and torch.equal(net(x[:2])[1], y[1])


def test_weight_update_invalidates_packed_weights():
    net = networks.TransPoseNet(MEAN, False, False, 0, 0).cuda()
    x = torch.rand(1, 3, 64, 96, device="cuda")
    y0 = net(x)
    with torch.no_grad():
        net.decoder.fc2.weight.mul_(1.5)
        net.encoder.conv3.weight.mul_(0.5)
    y1 = net(x)
    ref = cnn_oracle.transposenet_forward(net.state_dict(), x, 0, 0, 0)
    assert not torch.equal(y0, y1)
    _close(y1.cpu()[:, :3] - MEAN[None, :, None, None], ref[:, :3] - MEAN[None, :, None, None], 1e-3)


@pytest.mark.parametrize("n_task,n_pos,mean", [(1, 1, [241.47]), (2, 1, [0.0, 0.0]), (3, 0, [-455.934, 417.50, 520.31])])
def test_depth_normal_and_plain_heads(n_task, n_pos, mean):
    """The depth (1+1 channels, label mean utils/learning.py:116) and normal (2+1) encoders of CrossLoc and the
    uncertainty-free coord net share the graph; only the head width changes."""
    m = torch.tensor(mean)
    net = networks.TransPoseNet(m, False, False, 1, 1, n_task, n_pos)
    net.load_state_dict(seeded_state_dict(net, seed=17))
    x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(4))
    ref = cnn_oracle.transposenet_forward(net.state_dict(), x, 0, 1, 1, n_task, n_pos)
    y = net.cuda()(x.cuda()).cpu()
    assert y.shape == (2, n_task + n_pos, 8, 12)
    _close(y[:, :n_task] - m[None, :, None, None], ref[:, :n_task] - m[None, :, None, None], 1e-3)
    if n_pos:
        assert torch.allclose(y[:, n_task:], ref[:, n_task:], rtol=2e-3)


def test_batches_past_the_32bit_tensor_boundary():
    """50 frames of 480x720: the 32-channel full-resolution activation (44 MB per frame) passes 2 GiB at 48 frames, so
    the stride-2 stem conv is issued per image range inside the library (launch_igemm); no Python-side split.  Frames on
    both sides of the range boundary must equal what a small batch gives for them (to the last fp32 bits: conv tiles
    straddle image boundaries differently, see test_network_full_size_vs_oracle_and_determinism)."""
    net = networks.TransPoseNet(MEAN, False, False, 0, 0, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=14))
    net = net.cuda().eval()
    x = torch.rand(50, 3, 480, 720, generator=torch.Generator().manual_seed(2)).cuda()
    pick = [0, 1, 46, 47, 48, 49]
    with torch.no_grad():
        full = net(x)
        small = net(x[pick].contiguous())
    assert full.shape == (50, 4, 60, 90) and torch.isfinite(full).all()
    assert len([k for k in net._plans if k[0] == 50]) == 1
    assert torch.allclose(full[pick][:, :3], small[:, :3], rtol=0, atol=3e-4)
    assert torch.allclose(full[pick][:, 3], small[:, 3], rtol=2e-4)
    # the batch-invariant lowering must be bitwise independent of the batch, across the range boundary too
    net.batch_invariant = True
    with torch.no_grad():
        assert torch.equal(net(x)[pick], net(x[pick].contiguous()))


@pytest.mark.parametrize("H,W,gray", [(100, 140, False), (72, 88, True), (57, 91, False)])
def test_odd_image_sizes_and_grayscale(H, W, gray):
    """Sizes that are not multiples of 8 (three stride-2 convs: ceil division each time) and 1-channel input."""
    net = networks.TransPoseNet(MEAN, False, gray, 1, 0, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=29))
    x = torch.rand(2, 1 if gray else 3, H, W, generator=torch.Generator().manual_seed(H))
    ref = cnn_oracle.transposenet_forward(net.state_dict(), x, 0, 1, 0)
    with torch.no_grad():
        y = net.cuda()(x.cuda()).cpu()
    assert y.shape == ref.shape
    _close(y[:, :3] - MEAN[None, :, None, None], ref[:, :3] - MEAN[None, :, None, None], 1e-3)
    assert torch.allclose(y[:, 3], ref[:, 3], rtol=2e-3)


# ------------------------------------------------------------------------------------------ Winograd op sequence

def _wino_weights(w, m, dgrad=False):
    """[(m+2)^2][Cout][Cin] operands exactly as the plan packs them (crossloc_amd.networks._Plan._pack)."""
    plan = networks._Plan.__new__(networks._Plan)
    plan.device = torch.device("cuda")
    src = w.detach().cuda().float().contiguous()
    dst = torch.empty((m + 2) ** 2 * src.shape[0] * src.shape[1], dtype=torch.float32, device="cuda")
    plan._pack(dst, src, "wino%d%s" % (m, "d" if dgrad else ""))
    return dst


def _wino_conv(x_nhwc, U, bias, m, B, H, W, cin, cout, out, ld_out, stats=None, groups=1, accumulate=False):
    Th, Tw = -(-H // m), -(-W // m)
    T, nf = B * Th * Tw, (m + 2) ** 2
    V = torch.empty(nf * T * cin, device="cuda")
    Mb = torch.empty(nf * T * cout, device="cuda")
    a = networks.XlOp()
    a.type, a.ksize = networks.XL_OP_WINO_IN, m
    a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.ld_in = B, H, W, cin, Th, Tw, cin
    a.in_, a.out = x_nhwc.data_ptr(), V.data_ptr()
    g = networks.XlOp()
    g.type = networks.XL_OP_CONV
    g.B, g.Hi, g.Wi, g.Cin, g.Ho, g.Wo, g.Cout = B, Th, Tw, cin, Th, Tw, cout
    g.ksize, g.stride, g.ld_in, g.ld_out, g.nchunks2 = 1, 1, cin, cout, nf
    g.in_, g.w, g.out = V.data_ptr(), U.data_ptr(), Mb.data_ptr()
    tpb = 32 if m == 2 else 16
    o = networks.XlOp()
    o.type, o.ksize = networks.XL_OP_WINO_OUT, m
    o.B, o.Hi, o.Wi, o.Cin, o.ld_out, o.groups = B, H, W, cout, ld_out, groups
    o.nchunks, o.reserved_i = -(-(Th * Tw) // tpb), tpb
    o.flags = networks.CONV_ACCUMULATE if accumulate else 0
    o.in_, o.out = Mb.data_ptr(), out.data_ptr()
    if bias is not None:
        o.bias = bias.data_ptr()
    if stats is not None:
        o.stats = stats.data_ptr()
    _run([a, g, o])
    return o.nchunks


@pytest.mark.parametrize("m,cin,cout,B,H,W", [(4, 256, 256, 2, 8, 12), (4, 512, 512, 1, 10, 14), (4, 256, 512, 2, 9, 13),
                                              (4, 1536, 512, 1, 8, 12), (2, 256, 256, 2, 8, 12), (2, 512, 128, 1, 10, 14),
                                              (6, 256, 256, 2, 12, 18), (6, 512, 512, 1, 10, 14), (6, 256, 512, 2, 9, 13),
                                              (6, 1536, 512, 1, 8, 12), (6, 512, 512, 2, 60, 90),
                                              (6, 128, 128, 3, 13, 20), (6, 256, 1024, 1, 12, 12), (6, 512, 512, 5, 25, 31)])
def test_winograd_conv_with_statistics_vs_float64(m, cin, cout, B, H, W):
    """Input transform + batched GEMMs + output transform (bias, GroupNorm partial sums) against a float64 convolution;
    9x13 and 10x14 exercise the partial tiles of F(4x4,3x3) and F(6x6,3x3); 60x90 is the BASELINE feature map."""
    g = torch.Generator().manual_seed(m * 1000 + cin + cout + H)
    x = torch.relu(torch.randn(B, cin, H, W, generator=g))
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    out = torch.full((B, H, W, cout), float("nan"), device="cuda")
    G = 32
    tpb = 32 if m == 2 else 16
    nch = -(-(-(-H // m) * -(-W // m)) // tpb)
    stats = torch.full((B, nch, G, 2), float("nan"), dtype=torch.float64, device="cuda")
    _wino_conv(_nhwc(x).cuda(), _wino_weights(w, m), b.cuda(), m, B, H, W, cin, cout, out, cout, stats, G)
    got = out.permute(0, 3, 1, 2).cpu().double()
    assert torch.isfinite(got).all()
    _close(got, ref, {2: 5e-6, 4: 3e-5, 6: 6e-5}[m])
    st = stats.sum(1).cpu()                                    # [B, G, 2]
    y = got.reshape(B, G, cout // G, H * W)
    # (fp32 partial sums per thread, fp64 across threads and workgroups)
    assert torch.allclose(st[..., 0], y.sum((2, 3)), rtol=1e-5, atol=2e-3)
    assert torch.allclose(st[..., 1], (y * y).sum((2, 3)), rtol=1e-5, atol=2e-3)


@pytest.mark.parametrize("cin,cout,B,H,W", [(512, 512, 2, 12, 18), (256, 512, 1, 10, 14), (512, 512, 2, 60, 90), (1536, 512, 1, 8, 12)])
@pytest.mark.parametrize("interleaved", [False, True])
def test_winograd_split_bf16_gemm_matches_float64_like_fp32(cin, cout, B, H, W, interleaved):
    """Opt-in GEMM path (csrc/xl_gemm_split.hip): V and U as three bf16 planes each (exact 24-bit splits), six bf16 MFMA
    passes with fp32 accumulation.  Same tolerance as the fp32-MFMA F(6x6,3x3) path, and the two paths agree with each
    other far below it: the error is Winograd's, not the GEMM's."""
    m = 6
    g = torch.Generator().manual_seed(cin + cout + H)
    x = torch.relu(torch.randn(B, cin, H, W, generator=g))
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    Th, Tw = -(-H // m), -(-W // m)
    T, nf = B * Th * Tw, 64
    xd = _nhwc(x).cuda()
    U = _wino_weights(w, m)
    planes = networks._Plan.split_bf16(U)
    assert torch.equal(planes.view(torch.bfloat16).float().sum(0), U)          # the split is exact
    if interleaved:                               # [64][Cout][Cin/16][3][16]: the operand form of the 256 x 256 kernel
        planes = networks._Plan.split_bf16_interleaved(U.view(64, cout, cin), cin)
        assert torch.equal(planes.view(torch.bfloat16).float().sum(-2).reshape(U.shape), U)
    sflags = networks.CONV_SPLIT_BF16 | (networks.CONV_SPLIT_IL if interleaved else 0)
    outs, Ms, V32 = [], [], None
    for split in (False, True):
        V = torch.zeros(nf * T * cin * (3 if split else 2) // 2, device="cuda")
        Mb = torch.full((nf * T * cout,), float("nan"), device="cuda")
        out = torch.full((B, H, W, cout), float("nan"), device="cuda")
        a = networks.XlOp()
        a.type, a.ksize = networks.XL_OP_WINO_IN, m
        a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.ld_in = B, H, W, cin, Th, Tw, cin
        a.in_, a.out = xd.data_ptr(), V.data_ptr()
        gm = networks.XlOp()
        gm.type = networks.XL_OP_CONV
        gm.B, gm.Hi, gm.Wi, gm.Cin, gm.Ho, gm.Wo, gm.Cout = B, Th, Tw, cin, Th, Tw, cout
        gm.ksize, gm.stride, gm.ld_in, gm.ld_out, gm.nchunks2 = 1, 1, cin, cout, nf
        gm.in_, gm.w, gm.out = V.data_ptr(), (planes if split else U).data_ptr(), Mb.data_ptr()
        if split:
            a.flags = gm.flags = sflags
        o = networks.XlOp()
        o.type, o.ksize = networks.XL_OP_WINO_OUT, m
        o.B, o.Hi, o.Wi, o.Cin, o.ld_out, o.groups = B, H, W, cout, cout, 1
        o.nchunks, o.reserved_i = -(-(Th * Tw) // 16), 16
        o.in_, o.out, o.bias = Mb.data_ptr(), out.data_ptr(), b.cuda().data_ptr()
        bias_keep = b.cuda()
        o.bias = bias_keep.data_ptr()
        _run([a, gm, o])
        outs.append(out.permute(0, 3, 1, 2).cpu().double())
        Ms.append(Mb.view(nf, T, cout).double())
        if not split:
            V32 = V.view(nf, T, cin).double()
    assert torch.isfinite(outs[1]).all()
    _close(outs[1], ref, 6e-5)
    _close(outs[1], outs[0], 6e-5)            # two roundings of the same ill-conditioned transform chain
    # the GEMM itself: both paths against a float64 product of the same fp32 operands - the split path is fp32-class
    Mref = torch.matmul(V32, U.view(nf, cout, cin).double().transpose(1, 2))
    scale = Mref.abs().max().item()
    e32 = (Ms[0] - Mref).abs().max().item() / scale
    esp = (Ms[1] - Mref).abs().max().item() / scale
    assert esp < 2e-6 and esp < 4 * e32 + 2e-7, (esp, e32)


@pytest.mark.parametrize("m", [4, 6])
@pytest.mark.parametrize("relu", [True, False])
def test_winograd_input_transform_applies_deferred_groupnorm(relu, m):
    """XL_OP_WINO_IN with aux2 = per-(image, channel) {scale, shift}: the transform of relu(x*scale+shift) without the
    separate GN_APPLY pass; zero padding stays zero (the affine map is applied to in-image pixels only)."""
    B, C, H, W = 2, 64, 9, 13
    g = torch.Generator().manual_seed(5 + relu)
    x = torch.randn(B, H, W, C, generator=g)
    co = torch.randn(B, C, 2, generator=g)
    co[..., 1] += 0.5                                                    # non-zero shift: padding must not pick it up
    Th, Tw = -(-H // m), -(-W // m)
    T = B * Th * Tw

    def transform(inp, coeff):
        V = torch.full(((m + 2) ** 2, T, C), float("nan"), device="cuda")
        a = networks.XlOp()
        a.type, a.ksize = networks.XL_OP_WINO_IN, m
        a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.ld_in = B, H, W, C, Th, Tw, C
        a.in_, a.out = inp.data_ptr(), V.data_ptr()
        if coeff is not None:
            a.aux2 = coeff.data_ptr()
            a.flags = networks.GN_RELU_IN if relu else 0
        _run([a])
        return V.cpu()

    # the apply is one fused multiply-add (every apply site, fused or not, rounds once): the product of two floats is exact
    # in float64 and the sum rounds to float like fmaf does
    y = (x.double() * co[:, None, None, :, 0].double() + co[:, None, None, :, 1].double()).float()
    if relu:
        y = torch.relu(y)
    ref = transform(y.cuda().contiguous(), None)
    got = transform(x.cuda().contiguous(), co.cuda().contiguous())
    assert torch.isfinite(got).all()
    assert torch.allclose(got, ref, rtol=1e-6, atol=1e-5 if m == 4 else 1e-4)      # B^T entries reach 5.25^2 for m = 6
    bad = networks.XlOp()                                                # the F(2x2,3x3) transform has no deferred form
    bad.type, bad.ksize = networks.XL_OP_WINO_IN, 2
    bad.B, bad.Hi, bad.Wi, bad.Cin, bad.Ho, bad.Wo, bad.ld_in = B, 8, 12, C, 4, 6, C
    xs = torch.zeros(B, 8, 12, C, device="cuda")
    Vs = torch.zeros(16 * B * 24 * C, device="cuda")
    bad.in_, bad.out, bad.aux2 = xs.data_ptr(), Vs.data_ptr(), co.cuda().data_ptr()
    with pytest.raises(RuntimeError):
        _run([bad])


# every (H mod m, W mod m) class of the partial tiles: two rows of tiles by three columns, the last of each from 1 to m pixels
WINO_SWEEP = [(4, H, W) for H in range(5, 9) for W in range(9, 13)] + [(6, H, W) for H in range(7, 13) for W in range(13, 19)]


@pytest.mark.parametrize("cin,cout,B,H,W,m", [(ci, co, B, H, W, m) for m in (4, 6)
                                              for ci, co, B, H, W in ((256, 256, 2, 8, 12), (512, 256, 1, 9, 13), (128, 64, 2, 12, 16))] +
                         [(128, 64, 2, H, W, m) for m, H, W in WINO_SWEEP if (m, H, W) != (6, 12, 16)])        # (12 x 16 is in the list above)
def test_winograd_data_gradient_vs_autograd_and_accumulate(cin, cout, B, H, W, m):
    """dX of a stride-1 3x3 convolution as F(m x m,3x3) with the flipped, channel-swapped kernel; written into a channel
    slice of a wider gradient tensor, then accumulated a second time."""
    g = torch.Generator().manual_seed(cin + cout + W)
    x = torch.randn(B, cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    dy = torch.randn(B, cout, H, W, generator=g)
    F.conv2d(x, w.double(), padding=1).backward(dy.double())
    ref = x.grad
    wide = torch.zeros((B, H, W, cin + 64), device="cuda")
    sl = wide[..., 32:32 + cin]
    U = _wino_weights(w, m, dgrad=True)
    _wino_conv(_nhwc(dy).cuda(), U, None, m, B, H, W, cout, cin, sl, cin + 64)
    got = sl.permute(0, 3, 1, 2).cpu().double()
    print("winograd dgrad m %d %dx%d: %.2e of max (bound %g)" % (m, H, W, (got - ref).abs().max().item() / ref.abs().max().item(),
                                                                 3e-5 if m == 4 else 6e-5))
    _close(got, ref, 3e-5 if m == 4 else 6e-5)
    assert float(wide[..., :32].abs().max()) == 0.0 and float(wide[..., 32 + cin:].abs().max()) == 0.0
    _wino_conv(_nhwc(dy).cuda(), U, None, m, B, H, W, cout, cin, sl, cin + 64, accumulate=True)
    _close(sl.permute(0, 3, 1, 2).cpu().double(), 2 * ref, 3e-5 if m == 4 else 6e-5)


@pytest.mark.parametrize("m,cin,cout,B,H,W", [(4, 256, 256, 2, 16, 24), (4, 128, 256, 4, 9, 13), (4, 512, 512, 2, 16, 20),
                                              (4, 64, 128, 4, 12, 12), (6, 256, 256, 3, 18, 24), (6, 128, 256, 6, 9, 13),
                                              (6, 512, 512, 2, 24, 30), (6, 64, 128, 4, 18, 18)])
def test_winograd_weight_gradient_vs_autograd(m, cin, cout, B, H, W):
    """dW of a stride-1 3x3 layer through F(m x m,3x3): V = B^T x B, dM = A dY A^T, (m+2)^2 batched tile-GEMMs, G^T dU G;
    9x13 has partial tiles on both edges."""
    _winograd_weight_gradient(m, cin, cout, B, H, W)


@pytest.mark.parametrize("m,H,W", WINO_SWEEP)
def test_winograd_weight_gradient_over_every_partial_tile_class(m, H, W):
    """64 -> 128 channels over every (H mod m, W mod m) class.  Two frames of these maps are 12 tiles, and the tile-GEMM (the tiles are
    its K dimension, 32 per step) refuses fewer than 32 by name - plans take the direct weight gradient below 64 tiles
    (forms.wino_wgrad_ok).  So: the refusal at two frames, then six frames (36 tiles: one full K-step and a ragged one of 4) against
    float64 at the bound above."""
    from crossloc_amd import _lib
    with pytest.raises(_lib.XlError) as e:
        _winograd_weight_gradient(m, 64, 128, 2, H, W)
    msg = str(e.value)
    assert "op 2 refused" in msg and "type %d" % networks.XL_OP_WGRAD in msg and "64 -> 128 channels" in msg, msg
    _winograd_weight_gradient(m, 64, 128, 6, H, W)


def _winograd_weight_gradient(m, cin, cout, B, H, W):
    g = torch.Generator().manual_seed(cin * 3 + cout + H)
    x = torch.relu(torch.randn(B, cin, H, W, generator=g))
    dy = torch.randn(B, cout, H, W, generator=g)
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, padding=1).backward(dy.double())
    ref = w.grad
    Th, Tw = -(-H // m), -(-W // m)
    nf = (m + 2) ** 2
    T = B * Th * Tw
    xd, dyd = _nhwc(x).cuda(), _nhwc(dy).cuda()
    V = torch.empty(nf * T * cin, device="cuda")
    dM = torch.empty(nf * T * cout, device="cuda")
    dU = torch.empty(nf * cout * cin, device="cuda")
    splits = 2
    part = torch.empty(nf * splits * cout * cin, device="cuda")
    dw = torch.full((cout, cin, 3, 3), float("nan"), device="cuda")
    a = networks.XlOp()
    a.type, a.ksize = networks.XL_OP_WINO_IN, m
    a.B, a.Hi, a.Wi, a.Cin, a.Ho, a.Wo, a.ld_in = B, H, W, cin, Th, Tw, cin
    a.in_, a.out = xd.data_ptr(), V.data_ptr()
    d = networks.XlOp()
    d.type, d.ksize = networks.XL_OP_WINO_DY, m
    d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.ld_in = B, H, W, cout, Th, Tw, cout
    d.in_, d.out = dyd.data_ptr(), dM.data_ptr()
    wg = networks.XlOp()
    wg.type = networks.XL_OP_WGRAD
    wg.B, wg.Hi, wg.Wi, wg.Cin, wg.Ho, wg.Wo, wg.Cout = 1, T, 1, cin, T, 1, cout
    wg.ksize, wg.stride, wg.ld_in, wg.ld_aux, wg.groups, wg.nchunks2 = 1, 1, cin, cout, nf, splits
    wg.in_, wg.aux, wg.out, wg.stats2 = V.data_ptr(), dM.data_ptr(), dU.data_ptr(), part.data_ptr()
    f = networks.XlOp()
    f.type, f.ksize = networks.XL_OP_WINO_WFINAL, m
    f.Cin, f.Cout = cin, cout
    f.in_, f.out = dU.data_ptr(), dw.data_ptr()
    _run([a, d, wg, f])
    got = dw.cpu().double()
    print("winograd wgrad m %d %dx%dx%d: %.2e of max (bound 1e-4)" % (m, B, H, W, (got - ref).abs().max().item() / ref.abs().max().item()))
    _close(got, ref, 1e-4)


@pytest.mark.skipif(bool(os.environ.get("XL_NO_WINOGRAD")), reason="asserts the Winograd forms of the default plans (measurement switch set)")
@pytest.mark.skipif(any(os.environ.get(k) for k in ("XL_NO_FOLD_GN", "XL_NO_DEFERRED_GN", "XL_WINO_V_SPLIT", "XL_NO_AUX_FOLD"))
                    or os.environ.get("XL_GEMM_SPLIT_BF16") in ("0", "1"), reason="a switch that disables the fold form is set")
def test_folded_groupnorm_apply_is_bitwise_the_separate_pass(monkeypatch):
    """Inference plans leave the GroupNorm(+ReLU, +residual, +ReLU) apply of a block's last layer to the F(6x6,3x3) input
    transform of the next block, which also writes the activation for the residual branch (XL_OP_WINO_IN with out2).  Same
    arithmetic in the same order as gn_apply_kernel: the network output must not change by a bit."""
    net = networks.TransPoseNet(MEAN, False, False, 2, 2, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=9))
    net = net.cuda().eval()
    x = torch.rand(3, 3, 192, 288, generator=torch.Generator().manual_seed(8)).cuda()    # 24 x 36 grid: 6 divides both
    with torch.no_grad():
        y = net(x)
    plan = list(net._plans.values())[0]
    folds = [op for op in plan.ops if op.type == networks.XL_OP_WINO_IN and op.out2]
    assert len(folds) >= 5, len(folds)                 # conv4, res1, res2 skip, and the blocks that feed another block
    assert any(op.flags & networks.GN_ADD for op in folds) and any(not (op.flags & networks.GN_ADD) for op in folds)
    n_apply = sum(op.type == networks.XL_OP_GN_APPLY for op in plan.ops)
    # one of the folds also normalises its residual while reading it (res2_conv3's GroupNorm + ReLU, whose only consumer is the
    # addition to the skip branch): `w` = the residual's own coefficient table
    n_aux = sum(1 for op in plan.op_array if op.type == networks.XL_OP_WINO_IN and op.out2 and op.w)
    assert n_aux == 1
    monkeypatch.setenv("XL_NO_AUX_FOLD", "1")
    net.invalidate()
    with torch.no_grad():
        y1 = net(x)
    plan1 = list(net._plans.values())[0]
    assert sum(op.type == networks.XL_OP_GN_APPLY for op in plan1.ops) == n_apply + 1
    assert not any(op.type == networks.XL_OP_WINO_IN and op.out2 and op.w for op in plan1.op_array)
    assert torch.equal(y, y1)
    monkeypatch.delenv("XL_NO_AUX_FOLD")
    monkeypatch.setenv("XL_NO_FOLD_GN", "1")
    net.invalidate()
    with torch.no_grad():
        y0 = net(x)
    plan0 = list(net._plans.values())[0]
    assert not any(op.type == networks.XL_OP_WINO_IN and op.out2 for op in plan0.ops)
    assert sum(op.type == networks.XL_OP_GN_APPLY for op in plan0.ops) == n_apply + len(folds) + n_aux
    assert torch.equal(y, y0)
    # ragged 6x6 tiles (a 16 x 24 grid): the owner of a pixel is the tile whose footprint holds it, also at the edges
    monkeypatch.delenv("XL_NO_FOLD_GN")
    net.invalidate()
    x2 = torch.rand(2, 3, 128, 192, generator=torch.Generator().manual_seed(9)).cuda()
    with torch.no_grad():
        ya = net(x2)
    monkeypatch.setenv("XL_NO_FOLD_GN", "1")
    net.invalidate()
    with torch.no_grad():
        yb = net(x2)
    assert torch.equal(ya, yb)


@pytest.mark.parametrize("cin,cout,B,H,W,norm,relu,pad", [
    (32, 64, 2, 40, 56, False, False, 0),       # conv2's shape class: plain input (conv1 writes it normalised)
    (32, 64, 3, 37, 61, True, True, 0),         # odd sizes: the far-edge taps fall on the padding; tiles straddle images
    (64, 128, 3, 33, 47, True, True, 0),        # conv3
    (128, 256, 2, 35, 49, True, True, 32),      # conv4, operands inside wider tensors
    (128, 256, 5, 120, 180, True, False, 0),    # conv4 at its real size: 106 tiles per... 27000 rows, several tiles per CU later
    (64, 128, 9, 96, 120, True, True, 0),       # 102 tiles on <= 256 workgroups with second tiles (stores in flight)
    (32, 64, 40, 80, 96, True, True, 0)] +      # 300 tiles: every workgroup past its first tile
    # all four parity classes of every stem layer (even sizes: the far-edge taps are inside the image; odd: on the padding)
    [(ci, co, 2, H, W, True, True, 0) for ci, co in ((32, 64), (64, 128), (128, 256)) for H in (33, 34) for W in (41, 42)])
def test_stride2_stem_conv_on_the_split_bf16_pipe(cin, cout, B, H, W, norm, relu, pad):
    """XL_OP_CONV 3x3 stride 2 with XL_CONV_SPLIT_BF16 | XL_CONV_SPLIT_IL (csrc/xl_stem_split.hip): weights split on the host
    (K tap-major), fp32 activations gathered per tap, optionally normalised (the producer's GroupNorm + ReLU applied to
    in-image pixels only: the zero padding stays zero - the shift is non-zero here) and split by the kernel.  Against a
    float64 convolution, and within a small factor of the fp32-MFMA kernel's own rounding error."""
    g = torch.Generator().manual_seed(cin + cout + B + H)
    x = torch.randn(B, cin, H, W, generator=g) * 3.0 + 1.0
    coef = torch.stack([torch.rand(B, cin, generator=g) + 0.5, torch.randn(B, cin, generator=g) + 0.7], 2)
    conv = nn.Conv2d(cin, cout, 3, 2, 1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (9 * cin)) ** 0.5)
        conv.bias.copy_(torch.randn(cout, generator=g))
        xn = x.double()
        if norm:
            xn = xn * coef[:, :, 0, None, None].double() + coef[:, :, 1, None, None].double()
            if relu:
                xn = xn.clamp(min=0)
        ref = F.conv2d(xn, conv.weight.double(), conv.bias.double(), stride=2, padding=1)
    Ho, Wo = ref.shape[2], ref.shape[3]
    wide_in = torch.full((B, H, W, cin + pad), float("nan"))
    wide_in[..., pad:] = _nhwc(x)
    xd = wide_in.cuda()
    wd = networks._Plan.split_bf16_interleaved(networks._Plan._stem_rows(conv.weight.detach().cuda()), 9 * cin)
    bd, cd = conv.bias.detach().cuda(), coef.contiguous().cuda()
    out = torch.full((B, Ho, Wo, cout + pad), float("nan"), device="cuda")
    op = networks.XlOp()
    op.type = networks.XL_OP_CONV
    op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout = B, H, W, cin, Ho, Wo, cout
    op.ksize, op.stride, op.ld_in, op.ld_out = 3, 2, cin + pad, cout + pad
    op.flags = networks.CONV_SPLIT_BF16 | networks.CONV_SPLIT_IL
    if norm:
        op.flags |= networks.CONV_NORM_IN | (networks.CONV_NORM_RELU if relu else 0)
        op.aux2 = cd.data_ptr()
    op.in_, op.w, op.bias, op.out = xd.data_ptr() + 4 * pad, wd.data_ptr(), bd.data_ptr(), out.data_ptr()
    # round 4: the GroupNorm statistics of the output (32 groups) from the epilogue - one fp64 {sum, sum of squares} entry per
    # (image, tile overlapping it, row block of waves, group)
    bm, wm = {64: (128, 4), 128: (128, 2), 256: (256, 2)}[cout]
    HWo = Ho * Wo
    nchunks = (-(-HWo // bm) + 1) * wm
    stats = torch.full((B, nchunks, 32, 2), float("nan"), dtype=torch.float64, device="cuda")
    op.stats, op.groups, op.nchunks = stats.data_ptr(), 32, nchunks
    _run([op, op])                                        # twice: the second launch must overwrite, not accumulate
    got = out.cpu()
    if pad:
        assert torch.isnan(got[..., cout:]).all()
    got = got[..., :cout].permute(0, 3, 1, 2).double()
    _close(got, ref)
    st = stats.cpu()
    grouped = got.reshape(B, 32, cout // 32, HWo)
    for n in range(B):
        valid = (((n + 1) * HWo - 1) // bm - (n * HWo) // bm + 1) * wm
        assert torch.isfinite(st[n, :valid]).all() and torch.isnan(st[n, valid:]).all(), (n, valid)
        s1, s2 = st[n, :valid, :, 0].sum(0), st[n, :valid, :, 1].sum(0)
        r1, r2 = grouped[n].sum((1, 2)), (grouped[n] ** 2).sum((1, 2))
        # fp32 partial sums (<= 8 channels x 4 rows per lane, a 32- or 64-lane tree), fp64 across entries
        assert ((s1 - r1).abs() <= 2e-6 * grouped[n].abs().sum((1, 2))).all(), (n, (s1 - r1).abs().max())
        assert torch.allclose(s2, r2, rtol=2e-6, atol=0), (n, ((s2 - r2) / r2).abs().max())
    # the same layer through the fp32-MFMA kernel (operand normalised on the host)
    xfd = _nhwc(xn.float()).cuda()
    wsrc = conv.weight.detach().cuda().contiguous()
    wpk = torch.empty_like(wsrc)
    networks._check(networks._bind().xl_cnn_pack_conv_weight(wsrc.data_ptr(), wpk.data_ptr(), cout, cin, 3, None))
    out32 = torch.full((B, Ho, Wo, cout), float("nan"), device="cuda")
    o32 = networks.XlOp()
    o32.type = networks.XL_OP_CONV
    o32.B, o32.Hi, o32.Wi, o32.Cin, o32.Ho, o32.Wo, o32.Cout = B, H, W, cin, Ho, Wo, cout
    o32.ksize, o32.stride, o32.ld_in, o32.ld_out = 3, 2, cin, cout
    o32.in_, o32.w, o32.bias, o32.out = xfd.data_ptr(), wpk.data_ptr(), bd.data_ptr(), out32.data_ptr()
    _run([o32])
    scale = ref.abs().max().item()
    e32 = (out32.cpu().permute(0, 3, 1, 2).double() - ref).abs().max().item() / scale
    esp = (got - ref).abs().max().item() / scale
    print("six-pass stem %d -> %d %dx%dx%d: %.2e of max, fp32 MFMA %.2e (bound 2e-6 and 4 x + 2e-7)" % (cin, cout, B, H, W, esp, e32))
    assert esp < 2e-6 and esp < 4 * e32 + 2e-7, (esp, e32)


@pytest.mark.parametrize("m", [2, 4, 6])
@pytest.mark.parametrize("dgrad", [0, 1])
def test_winograd_weight_transform_kernel_vs_float64_einsum(m, dgrad):
    """xl_cnn_pack_wino_weight (csrc/xl_pack.hip): U = G g G^T per channel pair in float64, rounded once - against torch's
    float64 einsum (what the plans ran before round 3), in the fp32 form and in both split forms (whose three planes must
    add up to the fp32 value exactly)."""
    import ctypes
    L = networks._bind()
    cout, cin = 96, 64
    w = torch.randn(cout, cin, 3, 3, generator=torch.Generator().manual_seed(m + dgrad)).cuda()
    G = torch.tensor(networks._Plan._WINO_G[m], dtype=torch.float64, device="cuda")
    g = w.double()
    if dgrad:
        g = g.flip(2, 3).permute(1, 0, 2, 3)
    ref = torch.einsum("ia,ocab,jb->ijoc", G, g, G)                              # [m+2][m+2][rows][K]
    rows, K, nf = g.shape[0], g.shape[1], (m + 2) ** 2
    u32 = torch.full((nf, rows, K), float("nan"), device="cuda")
    networks._check(L.xl_cnn_pack_wino_weight(w.data_ptr(), u32.data_ptr(), cout, cin, m, dgrad, 0, None))
    torch.cuda.synchronize()
    want = ref.reshape(nf, rows, K)
    # rounded once: every element within half an fp32 ulp of the float64 value (plus float64 noise).  Not "== want.float()":
    # exact ties are common (the sum of three fp32 weights divisible by 3, times 1/24, is a 25-bit number) and an ulp of
    # float64 decides them
    half_ulp = 2.0 ** -24 * want.abs().clamp(min=2.0 ** -126)                # half an ulp is at most 2^-24 |x|
    assert ((u32.double() - want).abs() <= half_ulp * (1 + 1e-6)).all()
    assert (u32 == want.float()).float().mean().item() > 0.98
    p1 = torch.zeros(3, nf, rows, K, dtype=torch.int16, device="cuda")
    networks._check(L.xl_cnn_pack_wino_weight(w.data_ptr(), p1.data_ptr(), cout, cin, m, dgrad, 1, None))
    assert torch.equal(p1, networks._Plan.split_bf16(u32))
    p2 = torch.zeros(nf, rows, K // 16, 3, 16, dtype=torch.int16, device="cuda")
    networks._check(L.xl_cnn_pack_wino_weight(w.data_ptr(), p2.data_ptr(), cout, cin, m, dgrad, 2, None))
    assert torch.equal(p2.reshape(-1), networks._Plan.split_bf16_interleaved(u32, K).reshape(-1))
    back = p2.view(torch.bfloat16).float().sum(3).reshape(nf, rows, K)     # the three planes add up exactly
    assert torch.equal(back, u32)


def test_split_weight_kernel_is_the_exact_three_term_split():
    L = networks._bind()
    w1 = torch.randn(256, 96, generator=torch.Generator().manual_seed(1)).cuda()
    p = torch.zeros(3 * w1.numel(), dtype=torch.int16, device="cuda")
    networks._check(L.xl_cnn_split_weight(w1.data_ptr(), p.data_ptr(), 256, 96, 1, None))
    assert torch.equal(p, networks._Plan.split_bf16_interleaved(w1, 96).reshape(-1))
    w3 = torch.randn(64, 32, 3, 3, generator=torch.Generator().manual_seed(2)).cuda()
    p = torch.zeros(3 * w3.numel(), dtype=torch.int16, device="cuda")
    networks._check(L.xl_cnn_split_weight(w3.data_ptr(), p.data_ptr(), 64, 288, 9, None))
    assert torch.equal(p, networks._Plan.split_bf16_interleaved(networks._Plan._stem_rows(w3), 288).reshape(-1))
    assert L.xl_cnn_split_weight(w3.data_ptr(), p.data_ptr(), 64, 280, 9, None) != 0      # K % 16


@pytest.mark.skipif(os.environ.get("XL_GEMM_SPLIT_BF16") in ("0", "1"), reason="the tile forms belong to the split-pipe kernels")
def test_small_batch_forward_as_a_hip_graph_and_small_tile_form(monkeypatch):
    """Latency path: on a created stream a plan of <= 8 frames replays its op list as ONE HIP graph (first call eager, second
    captures, later ones replay) - bitwise the eager result; new images and new weights are picked up.  1x1 layers whose
    256 x 256 tiles would leave the chip idle run on 128 x 128 tiles: every convolution output is bitwise the same (same
    K order per element), but the GroupNorm partial sums are grouped per tile, so the network output agrees with the
    throughput tiles to the last fp32 bit or two at |X| ~ 500 m, like a frame inside another batch."""
    net = networks.TransPoseNet(MEAN, False, False, 1, 1, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=19))
    net = net.cuda().eval()
    xs = [torch.rand(1, 3, 480, 720, generator=torch.Generator().manual_seed(s)).cuda() for s in (1, 2, 3)]
    monkeypatch.setenv("XL_CNN_GRAPH", "0")
    with torch.no_grad():
        want = [net(x).clone() for x in xs]                          # eager, latency tiles
    plan = list(net._plans.values())[0]
    assert any(op.type == networks.XL_OP_CONV and (op.flags & networks.CONV_SPLIT_IL) and op.reserved_i == 128 for op in plan.ops)
    monkeypatch.setenv("XL_NO_SMALL_TILES", "1")
    net.invalidate()
    with torch.no_grad():
        big = net(xs[0]).clone()                                      # eager, throughput tiles
    assert torch.allclose(big[:, :3], want[0][:, :3], rtol=0, atol=3e-4) and torch.allclose(big[:, 3], want[0][:, 3], rtol=2e-4)
    monkeypatch.delenv("XL_NO_SMALL_TILES")
    monkeypatch.delenv("XL_CNN_GRAPH")
    net.invalidate()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st), torch.no_grad():
        got = [net(x) for x in xs] + [net(xs[0])]
    st.synchronize()
    plan = list(net._plans.values())[0]
    assert plan.graph is not None and plan.graph_runs == 4
    for g, w in zip(got, want + [want[0]]):
        assert torch.equal(g, w)
    with torch.no_grad():                                   # an in-place weight update reaches the replayed graph
        net.decoder.fc2.weight.mul_(1.25)
    with torch.cuda.stream(st), torch.no_grad():
        y2 = net(xs[1])
    st.synchronize()
    monkeypatch.setenv("XL_CNN_GRAPH", "0")
    net.invalidate()
    with torch.no_grad():
        assert torch.equal(net(xs[1]), y2) and not torch.equal(y2, want[1])


@pytest.mark.skipif(os.environ.get("XL_GEMM_SPLIT_BF16") in ("0", "1") or os.environ.get("XL_CNN_GRAPH") == "0", reason="graph path switched off")
def test_default_stream_calls_replay_the_graph_on_a_private_stream(monkeypatch):
    """Round 5 (the reference's unchanged loop, test_single_task.py:347: `network(image.cuda())` on the DEFAULT stream): HIP
    cannot capture on the default stream, so the plan captures its graph on a private stream - and (round 6) LAUNCHES it on the
    default stream itself: copy-in, graph and result copy in stream order, no event brackets (the bracketed replay on the private
    stream stays as the fallback for a runtime that refuses, and is exercised here by switching the plan to it).
    Bitwise the eager op list, new images picked up, the result usable at once by default-stream work and by `.cpu()`; a call
    from a created stream afterwards falls back to the eager list (one stream per plan)."""
    net = networks.TransPoseNet(MEAN, False, False, 1, 1, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=23))
    net = net.cuda().eval()
    xs = [torch.rand(1, 3, 480, 720, generator=torch.Generator().manual_seed(s)).cuda() for s in (4, 5, 6)]
    monkeypatch.setenv("XL_CNN_GRAPH", "0")
    with torch.no_grad():
        want = [net(x).clone() for x in xs]
    monkeypatch.delenv("XL_CNN_GRAPH")
    net.invalidate()
    torch.cuda.synchronize()
    assert torch.cuda.current_stream().cuda_stream == 0
    with torch.no_grad():
        got = []
        for x in xs + [xs[0]]:
            y = net(x)
            got.append((y * 2.0).cpu())                      # consumed on the default stream straight away, then on the host
    plan = list(net._plans.values())[0]
    assert plan.graph is not None and plan.graph_runs == 4 and plan.graph_stream == 0 and hasattr(plan, "graph_private")
    for g, w in zip(got, want + [want[0]]):
        assert torch.equal(g, (w * 2.0).cpu())
    st = torch.cuda.Stream()
    with torch.cuda.stream(st), torch.no_grad():
        y = net(xs[1])
    st.synchronize()
    assert torch.equal(y, want[1]) and plan.graph_runs == 5
    assert getattr(plan, "graph_on_null_stream", True)                  # the direct launch was accepted
    plan.graph_on_null_stream = False                                   # the round-5 form: replay on the private stream between events
    with torch.no_grad():
        y = net(xs[2])
    assert torch.equal((y * 2.0).cpu(), (want[2] * 2.0).cpu()) and plan.graph_runs == 6


@pytest.mark.skipif(bool(os.environ.get("XL_NO_WINOGRAD")), reason="asserts the Winograd forms of the default plans (measurement switch set)")
@pytest.mark.skipif(bool(os.environ.get("XL_WINO_V_SPLIT")) or os.environ.get("XL_GEMM_SPLIT_BF16") in ("0", "1"),
                    reason="the tile-major product belongs to the GEMM form that reads an fp32 V")
def test_tile_major_winograd_product_is_bitwise_the_plane_major_form(monkeypatch):
    """XL_WINO_M_TILE_MAJOR=1 (XL_CONV_M_TILE_MAJOR on the batched GEMM and on the output transform): M as [tiles][64][C]
    instead of [64][tiles][C] - a layout choice only."""
    net = networks.TransPoseNet(MEAN, False, False, 1, 1, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=23))
    net = net.cuda().eval()
    x = torch.rand(3, 3, 192, 288, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        y0 = net(x).clone()
    monkeypatch.setenv("XL_WINO_M_TILE_MAJOR", "1")
    net.invalidate()
    with torch.no_grad():
        y1 = net(x)
    plan = list(net._plans.values())[0]
    assert any(op.flags & networks.CONV_M_TILE_MAJOR for op in plan.ops if op.type == networks.XL_OP_WINO_OUT)
    assert torch.equal(y0, y1)


@pytest.mark.skipif(os.environ.get("XL_GEMM_SPLIT_BF16") in ("0", "1"), reason="these forms belong to the split-pipe plans (measurement switch set)")
@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (1, 70, 100), (3, 41, 57), (2, 480, 720),
                                   (2, 42, 57), (2, 41, 58), (2, 42, 58)])                 # H and W of opposite parity; both even off the tile
def test_fused_stem_is_bitwise_the_two_kernel_path(B, H, W, monkeypatch):
    """Round 4: conv1 + GroupNorm + ReLU evaluated inside conv2's operand stage (XL_OP_STEM12, csrc/xl_stem_fused.hip) against the
    two-kernel path (conv1 writes its raw output, conv2 normalises and splits it on load; XL_NO_STEM12=1).  Same term pairs, same
    K order, same conversion instructions: the network outputs are equal to the bit.  70 x 100 / 41 x 57: ragged tiles of 8 x 16
    conv2 outputs, odd image sizes (the last conv1 row / column is conv2's zero padding, not a convolution over padding)."""
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(H + W)).cuda()
    monkeypatch.setenv("XL_NO_STEM_STATS", "1")    # (conv2's statistics by the same pass on both sides: the kernels are what is compared)

    def run():
        net = networks.TransPoseNet(MEAN, False, False, 1, 1, 3, 1)
        net.load_state_dict(seeded_state_dict(net, seed=5))
        net = net.cuda().eval()
        with torch.no_grad():
            y = net(x)
        plan = list(net._plans.values())[0]
        return y.cpu(), [op.type for op in plan.ops]
    y_new, ops_new = run()
    monkeypatch.setenv("XL_NO_STEM12", "1")
    y_old, ops_old = run()
    assert networks.XL_OP_STEM12 in ops_new and networks.XL_OP_STEM12 not in ops_old
    assert torch.isfinite(y_new).all()
    assert torch.equal(y_new, y_old), (y_new - y_old).abs().max()


@pytest.mark.skipif(os.environ.get("XL_GEMM_SPLIT_BF16") in ("0", "1"), reason="these forms belong to the split-pipe plans (measurement switch set)")
def test_residual_epilogue_applied_by_the_consuming_1x1_layer_is_bitwise_the_apply_pass(monkeypatch):
    """Round 4: the GroupNorm + ReLU + residual + ReLU of the decoder's res3 block has ONE consumer, the 1x1 layer fc1, which applies
    it while loading its operand (XL_CONV_NORM_ADD) instead of a pass of its own (XL_NO_ADD_ON_LOAD=1).  Same arithmetic in the same
    order (fmaf, max, add, max): the network output is equal to the bit, at 480 x 720 and on a ragged small map."""
    for B, H, W in ((2, 480, 720), (3, 136, 200)):
        x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(H)).cuda()

        def run():
            net = networks.TransPoseNet(MEAN, False, False, 1, 1, 3, 1)
            net.load_state_dict(seeded_state_dict(net, seed=9))
            net = net.cuda().eval()
            with torch.no_grad():
                y = net(x)
            plan = list(net._plans.values())[0]
            return y.cpu(), sum(1 for op in plan.ops if op.type == networks.XL_OP_CONV and op.flags & networks.CONV_NORM_ADD), \
                sum(1 for op in plan.ops if op.type == networks.XL_OP_GN_APPLY)
        y_new, n_add, n_apply = run()
        monkeypatch.setenv("XL_NO_ADD_ON_LOAD", "1")
        y_old, n_add_old, n_apply_old = run()
        monkeypatch.delenv("XL_NO_ADD_ON_LOAD")
        assert n_add == 1 and n_add_old == 0 and n_apply == n_apply_old - 1
        assert torch.equal(y_new, y_old), (y_new - y_old).abs().max()


@pytest.mark.skipif(os.environ.get("XL_GEMM_SPLIT_BF16") in ("0", "1"), reason="these forms belong to the split-pipe plans (measurement switch set)")
@pytest.mark.parametrize("B,H,W", [(2, 480, 720), (3, 136, 200), (5, 130, 260)])
def test_stem_statistics_from_the_conv_epilogues_vs_the_statistics_pass(B, H, W, monkeypatch):
    """Round 4: conv2 (inside the fused stem kernel), conv3 and conv4 sum the GroupNorm statistics of their outputs in their
    epilogues - per lane fp32 over 8 channels x its rows, fp64 over the wave, one fp64 entry per tile and row block of waves -
    instead of XL_OP_GN_STATS passes over the tensors (XL_NO_STEM_STATS=1).  Only the summation order differs: the network output
    agrees to a few fp32 steps, the three statistics passes are gone, and repeated runs are equal to the bit (fixed order, one
    writer per entry although the fused stem hands its tiles out dynamically).  136 x 200 / 130 x 260: tiles that straddle two
    frames, ragged last tiles, a batch whose tile boundaries fall differently in every frame."""
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(B + H)).cuda()

    def run():
        net = networks.TransPoseNet(MEAN, False, False, 1, 1, 3, 1)
        net.load_state_dict(seeded_state_dict(net, seed=21))
        net = net.cuda().eval()
        with torch.no_grad():
            y = net(x).clone()
            y2 = net(x)
        assert torch.equal(y, y2)
        plan = list(net._plans.values())[0]
        return y.cpu(), sum(1 for op in plan.ops if op.type == networks.XL_OP_GN_STATS)
    y_new, n_new = run()
    monkeypatch.setenv("XL_NO_STEM_STATS", "1")
    y_old, n_old = run()
    assert n_new == n_old - 3, (n_new, n_old)
    # the coordinates are stored around the scene mean (|y| ~ 500: one fp32 step is 3e-5): 4 steps; the uncertainty channel 2e-4 (30 layers
    # of an untrained net amplify the 1e-7 of the statistics; tests/...stride2_stem_conv... pins the sums themselves to 2e-6)
    assert (y_new[:, :3] - y_old[:, :3]).abs().max() <= 4 * 3.06e-5
    assert torch.allclose(y_new[:, 3], y_old[:, 3], rtol=2e-4, atol=1e-9)
