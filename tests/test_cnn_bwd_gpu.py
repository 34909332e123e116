"""GPU parity of the CNN backward pass (loss.backward() through crossloc_amd.TransPoseNet) against PyTorch
autograd in float64 on the CPU restatement of the reference graph (oracle/cnn_oracle.py, itself pinned to
reference goldens).  Every parameter gradient (116 tensors single-task, the trainable subset for the 3-encoder
net) is compared.

Two levels, because ReLU'(0) makes whole-network gradients discontinuous: a pre-activation within fp32 rounding
of zero gets a different ReLU mask under a different summation order.  One such element changes one channel of one
d beta by O(1 %) and everything upstream by O(0.1 %); it happens on the GPU *and* in PyTorch's own fp32 CPU run
relative to float64 (observed: one flipped element, 1 of 512 channels of one layer, everything else 1e-6).
  * per-op tests (data gradient, weight gradient, GroupNorm/ReLU/residual backward) on random data pin the
    arithmetic of every kernel at <= 2e-5 / 5e-6 — flips are measure-zero there and masks are compared exactly;
  * network tests pin the wiring (tape, accumulation order, slices of the MLR concat, frozen encoders): every
    tensor within 5e-2 of its max (a wiring error — a missing accumulation, a wrong slice — is O(1); a single
    flipped element on a 12x16 map was measured at 5e-2 on one d beta), typically 3e-6.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import guarded                             # noqa: E402
torch = guarded.torch_proxy()              # empty / zeros / full (_like) on the device: between guard bands

from crossloc_amd import networks                      # noqa: E402
from crossloc_amd.weights import seeded_state_dict     # noqa: E402
from oracle import cnn_oracle                          # noqa: E402
from size_classes import MIXED_PARITY, ids             # noqa: E402

pytestmark = pytest.mark.gpu
MEAN = torch.tensor([-455.934, 417.50, 520.31])


@pytest.fixture(autouse=True)
def _guard_bands(monkeypatch):
    """Every device tensor this module allocates (and every packed operand) sits between guard bands: checked after each test."""
    yield from guarded.op_module_check(monkeypatch, networks, __name__)


def _reference_grads(sd, x, wgt, enc_add, dec_add, n_task=3, n_pos=1, in_ch=3):
    """Autograd in float64 on the CPU: the reference must not have ReLU-mask flips of its own (an fp32 CPU run
    does, now and then, relative to fp64 — see the module docstring).  n_task / n_pos: the head's channels (coord 3 + 1, depth
    1 + 1, normal 2 + 1, no uncertainty 3 + 0); in_ch: 3 (RGB) or 1 (grayscale)."""
    assert x.shape[1] == in_ch == sd["encoder.conv1.weight"].shape[1] and wgt.shape[1] == n_task + n_pos
    assert sd["decoder.fc3.weight"].shape[0] == n_task + n_pos
    sd = {k: (v.double().clone().requires_grad_(True) if v.dtype.is_floating_point and not k.endswith("mean")
              else (v.double() if v.dtype.is_floating_point else v)) for k, v in sd.items()}
    x, wgt = x.double(), wgt.double()
    leaves = {k: v for k, v in sd.items() if v.requires_grad}
    # cnn_oracle.transposenet_forward detaches its inputs; call its two halves with live tensors
    res = cnn_oracle.encoder_forward(sd, x, "encoder", enc_add, 32)
    y = cnn_oracle.decoder_forward(sd, res, dec_add, n_task, n_pos, 32)
    (y * wgt).sum().backward()
    return y.detach().float(), {k: v.grad.float() for k, v in leaves.items()}


def _check_direct_form(worst, worst2):
    """Criterion of the direct-convolution training plans against float64 autograd (lists of (error, name), any order).
    Without ReLU-mask flips every tensor is within 5e-2 of its max (3e-6 typical).  A pre-activation that float64 puts
    within an fp32 ulp of zero may land on the other side in the fp32 forward pass; that flip moves single elements of
    the parameter gradients of ONE layer (conv weight / bias, norm weight / bias) by one pixel's contribution - visible in
    the max norm at 8 x 12 pixels and, through the data gradient of that one pixel, a percent or two in the L2 norm of the
    layers before it.  So: relative L2 <= 5e-2 for every tensor (a wiring error moves a whole tensor: O(1)), max norm <= 5e-2 for all but at most four tensors, which stay below 0.5."""
    over = sorted((a, b) for a, b in worst if a > 5e-2)
    assert max(a for a, _ in worst2) <= 5e-2, sorted(worst2, reverse=True)[:5]
    assert len(over) <= 4 and all(a <= 0.5 for a, _ in over), over


@pytest.mark.parametrize("form", ["direct", "winograd"])
@pytest.mark.parametrize("B,H,W,enc_add,dec_add,tiny", [(2, 64, 96, 1, 1, False), (1, 128, 192, 2, 2, False), (3, 40, 56, 0, 0, False),
                                                        (2, 64, 96, 1, 1, True), (1, 128, 192, 0, 2, True)])
def test_parameter_gradients_vs_autograd(B, H, W, enc_add, dec_add, tiny, form, monkeypatch):
    """form: training plans run the stride-1 3x3 layers (forward and data gradient) as Winograd F(4x4,3x3) by default;
    "direct" pins the direct implicit-GEMM kernels (XL_NO_WINOGRAD_TRAIN=1, read when the plan is built).  Winograd's
    forward rounding noise is ~10x the direct form's, so more pre-activations land on the other side of ReLU'(0) than
    in the float64 reference: the max-norm criterion stays on the direct form, the Winograd form is held to a relative
    L2 error per tensor (a flipped mask moves a few elements; a wiring error moves the whole tensor).
    tiny (round 6): the 128-channel network of `--tiny` (networks.py:133-135, 194-198, 245-247)."""
    _check_parameter_gradients(form, monkeypatch, B, H, W, enc_add, dec_add, tiny)


def _out_size(n):
    """Three stride-2 3x3 pad-1 convolutions: ceil division each time."""
    for _ in range(3):
        n = (n + 1) // 2
    return n


_LAST_REFERENCE = [None, None]


def _check_parameter_gradients(form, monkeypatch, B, H, W, enc_add, dec_add, tiny, n_task=3, n_pos=1, gray=False, mean=MEAN):
    if form == "direct":
        monkeypatch.setenv("XL_NO_WINOGRAD_TRAIN", "1")
    in_ch = 1 if gray else 3
    net = networks.TransPoseNet(mean, tiny, gray, enc_add, dec_add, n_task, n_pos)
    net.load_state_dict(seeded_state_dict(net, seed=11))
    g = torch.Generator().manual_seed(B * 100 + H)
    x = torch.rand(B, in_ch, H, W, generator=g)
    Ho, Wo = _out_size(H), _out_size(W)
    wgt = torch.randn(B, n_task + n_pos, Ho, Wo, generator=g)
    wgt[:, n_task:] *= 0.1
    # (the float64 reference of a configuration is computed once for both forms: seeded weights, seeded inputs; never written to)
    key = (B, H, W, enc_add, dec_add, tiny, n_task, n_pos, gray, tuple(mean.tolist()))
    if _LAST_REFERENCE[0] != key:
        _LAST_REFERENCE[:] = [key, _reference_grads(net.state_dict(), x, wgt, enc_add, dec_add, n_task, n_pos, in_ch)]
    yref, gref = _LAST_REFERENCE[1]

    net = net.cuda().train()
    y = net(x.cuda())
    assert y.requires_grad and tuple(y.shape) == (B, n_task + n_pos, Ho, Wo)
    (y * wgt.cuda()).sum().backward()
    torch.cuda.synchronize()
    scale = max(1.0, (yref[:, :n_task] - mean[None, :, None, None]).abs().max().item())
    assert (y.detach().cpu()[:, :n_task] - yref[:, :n_task]).abs().max().item() <= 1e-3 * scale
    worst, worst2 = [], []
    gmax = max(v.abs().max().item() for v in gref.values())
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        ref = gref[name]
        d = (p.grad.cpu() - ref).double()
        err = d.abs().max().item()
        # per-tensor scale, floored at 1e-4 of the largest gradient in the network: conv1.bias is exactly 0 in
        # exact arithmetic (GroupNorm(32,32) is an instance norm), so both sides hold rounding noise only
        sc = max(ref.abs().max().item(), 1e-4 * gmax)
        worst.append((err / sc, name))
        worst2.append((d.norm().item() / max(ref.double().norm().item(), 1e-4 * gmax * ref.numel() ** 0.5), name))
    worst.sort(reverse=True)
    worst2.sort(reverse=True)
    worst = [w for w in worst if w[1] != "encoder.conv1.bias"]   # exactly 0 here; the reference holds noise
    worst2 = [w for w in worst2 if w[1] != "encoder.conv1.bias"]
    print("%s: worst max-norm error %.2e (%s), worst L2 error %.2e (%s), median %.2e" % (
        form, worst[0][0], worst[0][1], worst2[0][0], worst2[0][1], worst[len(worst) // 2][0]))
    if form == "direct":
        _check_direct_form(worst, worst2)
    else:
        assert worst2[0][0] <= 1e-1 and worst[0][0] <= 0.5, (worst2[:5], worst[:5])
    assert net.encoder.conv1.bias.grad.abs().max().item() == 0.0


@pytest.mark.parametrize("form", ["direct", "winograd"])
@pytest.mark.parametrize("B,H,W,gray,n_task,n_pos,mean", [
    (2, 57, 91, False, 3, 1, MEAN), (1, 75, 109, False, 3, 1, MEAN),            # odd sizes (the augmentation's frames)
    (2, 57, 91, True, 3, 1, MEAN),                                              # --grayscale
    (2, 64, 96, False, 1, 1, torch.tensor([241.47])), (2, 64, 96, False, 2, 1, torch.tensor([0.0, 0.0])),   # depth, normal
    (2, 64, 96, False, 3, 0, MEAN)])                                            # --uncertainty None
def test_parameter_gradients_in_the_training_driver_configurations(B, H, W, gray, n_task, n_pos, mean, form, monkeypatch):
    """What train_single_task offers beyond the RGB coordinate network at multiples of 8: frames of int(480 s) x int(720 s)
    (every stride-2 layer rounds up, the single-row tail of conv1's weight gradient, ragged Winograd tiles), one input
    channel, the depth (1 + 1) and normal (2 + 1) heads and the head without a positive channel.  Criteria per form as in
    test_parameter_gradients_vs_autograd, unchanged."""
    _check_parameter_gradients(form, monkeypatch, B, H, W, 1, 1, False, n_task, n_pos, gray, mean)


@pytest.mark.parametrize("form", ["direct", "winograd"])
@pytest.mark.parametrize("H,W", MIXED_PARITY, ids=ids(MIXED_PARITY))
def test_parameter_gradients_at_mixed_parity(H, W, form, monkeypatch):
    """The eight frames of tests/size_classes.py whose H and W have opposite parity (every value of H mod 8 and of W mod 8 once):
    the wiring - chunk counts, slices, tape - at the size classes the per-op sweeps pin arithmetically.  One frame, no additional
    blocks; criteria per form as in test_parameter_gradients_vs_autograd, unchanged."""
    _check_parameter_gradients(form, monkeypatch, 1, H, W, 0, 0, False)


def test_gradients_accumulate_and_second_step_matches():
    net = networks.TransPoseNet(MEAN, False, False, 0, 0, 3, 1)
    net.load_state_dict(seeded_state_dict(net, seed=3))
    net = net.cuda().train()
    x = torch.rand(1, 3, 64, 96, device="cuda")
    net(x).sum().backward()
    g1 = {n: p.grad.clone() for n, p in net.named_parameters()}
    net(x).sum().backward()                              # accumulates
    for n, p in net.named_parameters():
        assert torch.allclose(p.grad, 2 * g1[n], rtol=1e-5, atol=1e-6 * g1[n].abs().max().item() + 1e-12), n
    # an SGD step changes the weights -> the plan repacks and the next forward differs
    with torch.no_grad():
        for p in net.parameters():
            p -= 1e-3 * p.grad
    net.zero_grad()
    y2 = net(x)
    y2.sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in net.parameters())


def test_training_forms_agree_at_full_size(monkeypatch):
    """BASELINE configs[1] frame size (480x720, batch 2 here): the default training plan (Winograd forward / data /
    weight gradients, conv-epilogue statistics, coefficient tables) against the direct-convolution plan with separate
    statistics passes - two HIP lowerings, no CPU oracle in the loop.  Relative L2 per tensor: ReLU-mask flips between
    the two forward roundings move single elements (module docstring), not norms."""
    _training_forms_agree(monkeypatch, 480, 720)


def test_training_forms_agree_at_an_augmented_size(monkeypatch):
    """The same at 323 x 485 = int(480 s) x int(720 s) for s = 0.674, a frame of the training augmentation: odd in both
    directions, 41 x 61 cells (ragged Winograd tiles, ragged 128- and 256-row GEMM tiles, conv-epilogue statistics whose last
    tile straddles the image boundary).  Criteria of test_training_forms_agree_at_full_size."""
    _training_forms_agree(monkeypatch, 323, 485)


def _training_forms_agree(monkeypatch, H, W):
    x = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(6)).cuda()
    wgt = torch.randn(2, 4, _out_size(H), _out_size(W), generator=torch.Generator().manual_seed(7)).cuda()

    def run():
        net = networks.TransPoseNet(MEAN, False, False, 2, 2, 3, 1)
        net.load_state_dict(seeded_state_dict(net, seed=21))
        net = net.cuda().train()
        y = net(x)
        (y * wgt).sum().backward()
        return y.detach().cpu(), {n: p.grad.detach().cpu() for n, p in net.named_parameters()}
    y_w, g_w = run()
    for k in ("XL_NO_WINOGRAD_TRAIN", "XL_NO_FUSED_STATS"):
        monkeypatch.setenv(k, "1")
    y_d, g_d = run()
    assert (y_w[:, :3] - y_d[:, :3]).abs().max().item() < 5e-4
    assert len(g_w) == len(g_d) == 114                                  # 116 state_dict entries minus the two `mean` buffers
    worst = 0.0
    for n in g_d:
        assert torch.isfinite(g_w[n]).all(), n
        den = g_d[n].double().norm().item()
        if den > 0:
            worst = max(worst, (g_w[n].double() - g_d[n].double()).norm().item() / den)
    assert worst < 5e-2, worst


def test_frozen_parameters_and_no_grad_inference():
    net = networks.TransPoseNet(MEAN, False, False, 0, 0, 3, 1).cuda()
    for p in net.encoder.parameters():
        p.requires_grad = False
    x = torch.rand(1, 3, 64, 96, device="cuda")
    net(x).sum().backward()
    assert all(p.grad is None for p in net.encoder.parameters())
    assert all(p.grad is not None for p in net.decoder.parameters())
    with torch.no_grad():
        y = net(x)
    assert not y.requires_grad


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _run(ops):
    import ctypes
    L = networks._bind()
    arr = (networks.XlOp * len(ops))(*ops)
    networks._check(L.xl_cnn_run(arr, len(ops), None))
    torch.cuda.synchronize()


@pytest.mark.parametrize("cin,cout,k,s,B,H,W", [(512, 512, 1, 1, 1, 12, 16), (512, 512, 3, 1, 2, 9, 13), (256, 512, 3, 1, 1, 8, 12),
                                                (128, 256, 3, 2, 2, 17, 23), (64, 128, 3, 2, 1, 32, 48), (32, 64, 3, 2, 2, 40, 56)])
def test_conv_dgrad_and_wgrad_vs_autograd(cin, cout, k, s, B, H, W):
    import torch.nn as nn
    L = networks._bind()
    g = torch.Generator().manual_seed(cin + cout + k + s)
    x = torch.randn(B, cin, H, W, generator=g, requires_grad=True)
    conv = nn.Conv2d(cin, cout, k, s, k // 2)
    y = conv(x)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    Ho, Wo = y.shape[2], y.shape[3]
    ws = conv.weight.detach().cuda().contiguous()
    wd = torch.empty_like(ws)
    networks._check(L.xl_cnn_pack_conv_weight_dgrad(ws.data_ptr(), wd.data_ptr(), cout, cin, k, None))
    dyd = _nhwc(dy).cuda()
    gx = torch.full((B, H, W, cin), float("nan"), device="cuda")
    op = networks.XlOp()
    op.type, op.flags = networks.XL_OP_CONV, networks.CONV_DGRAD
    op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout = B, Ho, Wo, cout, H, W, cin
    op.ksize, op.stride, op.ld_in, op.ld_out = k, s, cout, cin
    op.in_, op.w, op.out = dyd.data_ptr(), wd.data_ptr(), gx.data_ptr()
    _run([op])
    ref = x.grad
    assert ((gx.cpu().permute(0, 3, 1, 2) - ref).abs().max() / ref.abs().max()).item() < 2e-5
    # accumulate epilogue: a second launch doubles the result
    op.flags |= networks.CONV_ACCUMULATE
    _run([op])
    assert ((gx.cpu().permute(0, 3, 1, 2) - 2 * ref).abs().max() / ref.abs().max()).item() < 4e-5
    xd = _nhwc(x.detach()).cuda()
    for splits in (1, 3):
        dw = torch.full(conv.weight.shape, float("nan"), device="cuda")
        scratch = torch.empty(splits * k * k * cout * cin, device="cuda")
        op = networks.XlOp()
        op.type = networks.XL_OP_WGRAD
        op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout = B, H, W, cin, Ho, Wo, cout
        op.ksize, op.stride, op.ld_in, op.ld_aux, op.nchunks2 = k, s, cin, cout, splits
        op.in_, op.aux, op.out, op.stats2 = xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), scratch.data_ptr()
        _run([op])
        ref = conv.weight.grad
        assert ((dw.cpu() - ref).abs().max() / ref.abs().max()).item() < 2e-5


@pytest.mark.parametrize("B,H,W,C", [(1, 12, 16, 512), (2, 8, 12, 256), (2, 24, 32, 64), (1, 48, 64, 32), (1, 8, 12, 1536)] +
                         # 255, 256 and 257 pixels: on both sides of a 256-pixel chunk of the forward sums and of a 64-pixel one of the backward's
                         [(2, H, W, C) for C in (64, 512) for H, W in ((15, 17), (16, 16), (1, 257))])
@pytest.mark.parametrize("flags", [1, 7, 6, 0])
def test_groupnorm_backward_vs_autograd(B, H, W, C, flags):
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(C + flags)
    x = (torch.randn(B, C, H, W, generator=g) * 2 + 0.5).requires_grad_(True)
    aux = torch.randn(B, C, H, W, generator=g).requires_grad_(True)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).requires_grad_(True)
    beta = (0.3 * torch.randn(C, generator=g)).requires_grad_(True)
    o = F.group_norm(x, 32, gamma, beta, 1e-5)
    if flags & 1:
        o = F.relu(o)
    if flags & 2:
        o = o + aux
    if flags & 4:
        o = F.relu(o)
    dout = torch.randn(o.shape, generator=g)
    o.backward(dout)
    HW = H * W
    nch = max(1, min(128, (HW + 255) // 256))
    xd, ad, dd = _nhwc(x.detach()).cuda(), _nhwc(aux.detach()).cuda(), _nhwc(dout).cuda()
    gd, bd = gamma.detach().cuda(), beta.detach().cuda()
    stats = torch.zeros(B * nch * 32 * 2, dtype=torch.float64, device="cuda")
    outf = torch.empty_like(xd)
    st = networks.XlOp()
    st.type = networks.XL_OP_GN_STATS
    st.B, st.Hi, st.Wi, st.Cin, st.groups, st.nchunks, st.ld_in = B, H, W, C, 32, nch, C
    st.in_, st.stats = xd.data_ptr(), stats.data_ptr()
    ap = networks.XlOp()
    ap.type = networks.XL_OP_GN_APPLY
    ap.B, ap.Hi, ap.Wi, ap.Cin, ap.groups, ap.nchunks, ap.ld_in, ap.ld_out, ap.ld_aux = B, H, W, C, 32, nch, C, C, C
    ap.flags, ap.eps = flags, 1e-5
    ap.in_, ap.w, ap.bias, ap.aux, ap.stats, ap.out = (xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), ad.data_ptr(),
                                                       stats.data_ptr(), outf.data_ptr())
    table = torch.full((B * C * 4,), float("nan"), device="cuda")       # {scale, shift} pairs, then {mean, rstd} pairs
    fin = networks.XlOp()
    fin.type = networks.XL_OP_GN_FINAL
    fin.B, fin.Hi, fin.Wi, fin.Cin, fin.groups, fin.nchunks, fin.eps = B, H, W, C, 32, nch, 1e-5
    fin.stats, fin.w, fin.bias = stats.data_ptr(), gd.data_ptr(), bd.data_ptr()
    fin.out, fin.out2 = table.data_ptr(), table.data_ptr() + 4 * B * C * 2
    ap.aux2 = table.data_ptr()
    nch2 = max(1, min(128, (HW + 63) // 64))
    scratch = torch.zeros(B * nch2 * C * 3 + B * C * 6 + (B * C * 3 + 1) // 2, dtype=torch.float64, device="cuda")
    dx = torch.full_like(xd, float("nan"))
    daux = torch.full_like(xd, float("nan"))
    dg, db, dbias = (torch.empty(C, device="cuda") for _ in range(3))
    ops = [st, fin, ap]
    for typ in (networks.XL_OP_GNB_STATS, networks.XL_OP_GNB_FINAL, networks.XL_OP_GNB_APPLY, networks.XL_OP_GNB_PARAMS):
        op = networks.XlOp()
        op.type = typ
        op.B, op.Hi, op.Wi, op.Cin, op.groups = B, H, W, C, 32
        op.nchunks2, op.flags, op.eps = nch2, flags, 1e-5
        op.ld_in, op.ld_aux, op.ld_out = C, C, C
        op.in_, op.w, op.bias, op.stats, op.aux, op.aux2 = (xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), table.data_ptr(),
                                                            dd.data_ptr(), outf.data_ptr())
        op.stats2 = scratch.data_ptr()
        if typ == networks.XL_OP_GNB_APPLY:
            op.out, op.out2 = dx.data_ptr(), daux.data_ptr()
        if typ == networks.XL_OP_GNB_PARAMS:
            op.out, op.out2, op.aux2 = dg.data_ptr(), db.data_ptr(), dbias.data_ptr()
        ops.append(op)
    _run(ops)

    def rel(a, b):
        return ((a - b).abs().max() / b.abs().max()).item()
    print("groupnorm backward C %d %dx%dx%d flags %d: dx %.2e, dgamma %.2e, dbeta %.2e of max (bound 5e-6)"
          % (C, B, H, W, flags, rel(dx.cpu().permute(0, 3, 1, 2), x.grad), rel(dg.cpu(), gamma.grad), rel(db.cpu(), beta.grad)))
    assert rel(dx.cpu().permute(0, 3, 1, 2), x.grad) < 5e-6
    assert rel(dg.cpu(), gamma.grad) < 5e-6 and rel(db.cpu(), beta.grad) < 5e-6
    if flags & 2:
        assert torch.equal(daux.cpu().permute(0, 3, 1, 2), aux.grad)
    if C > 32:
        assert rel(dbias.cpu(), x.grad.sum((0, 2, 3))) < 2e-5        # closed-form conv-bias gradient
    else:
        assert dbias.abs().max().item() == 0.0                        # instance norm: exactly zero


@pytest.mark.parametrize("form", ["direct", "winograd"])
def test_mlr_network_backward_with_frozen_encoders(form, monkeypatch):
    """finetune_decoder_single_task.py configuration: TransPoseNet(num_mlr=3, num_unfrozen_encoder=1)
    (utils/learning.py:294-305) — gradients flow through the fusion block into encoder 1 only.  Criteria per form as
    in test_parameter_gradients_vs_autograd."""
    if form == "direct":
        monkeypatch.setenv("XL_NO_WINOGRAD_TRAIN", "1")
    B, H, W = 1, 64, 96
    net = networks.TransPoseNet(MEAN, False, False, 1, 1, 3, 1, 32, 3, 1, False)
    net.load_state_dict(seeded_state_dict(net, seed=23))
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, 3, H, W, generator=g)
    wgt = torch.randn(B, 4, H // 8, W // 8, generator=g)
    wgt[:, 3] *= 0.1
    trainable = {n for n, p in net.named_parameters() if p.requires_grad}
    assert not any(n.startswith("mlr_encoder_2") or n.startswith("mlr_encoder_3") for n in trainable)
    sd = {k: (v.double().clone().requires_grad_(True) if k in trainable else (v.double() if v.dtype.is_floating_point else v.clone()))
          for k, v in net.state_dict().items()}
    import torch.nn.functional as F
    xd = x.double()
    mlr = torch.cat([cnn_oracle.encoder_forward(sd, xd, "mlr_encoder_%d" % (i + 1), 1, 32) for i in range(3)], dim=1)
    res = cnn_oracle._cgr(sd, mlr, "mlr_skip.0", "mlr_skip.1", groups=32, relu=False)
    m2 = F.group_norm(mlr, 32, sd["mlr_norm.weight"], sd["mlr_norm.bias"], eps=1e-5)
    res = F.relu(res + cnn_oracle._res_block(sd, "mlr_forward", m2, 32))
    yref = cnn_oracle.decoder_forward(sd, res, 1, 3, 1, 32)
    (yref * wgt.double()).sum().backward()
    yref = yref.detach().float()

    net = net.cuda().train()
    y = net(x.cuda())
    (y * wgt.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert (y.detach().cpu()[:, :3] - yref[:, :3]).abs().max().item() < 1e-3 * max(1.0, (yref[:, :3] - MEAN[None, :, None, None]).abs().max().item())
    gmax = max(sd[n].grad.abs().max().item() for n in trainable)
    worst, worst2 = [], []
    for name, p in net.named_parameters():
        if name not in trainable:
            assert p.grad is None, name
            continue
        ref = sd[name].grad.float()
        sc = max(ref.abs().max().item(), 1e-4 * gmax)
        d = (p.grad.cpu() - ref).double()
        worst.append((d.abs().max().item() / sc, name))
        worst2.append((d.norm().item() / max(ref.double().norm().item(), 1e-4 * gmax * ref.numel() ** 0.5), name))
    worst = sorted(w for w in worst if w[1] != "mlr_encoder_1.conv1.bias")
    worst2 = sorted(w for w in worst2 if w[1] != "mlr_encoder_1.conv1.bias")
    if form == "direct":
        _check_direct_form(worst, worst2)
    else:
        assert worst2[-1][0] <= 1e-1 and worst[-1][0] <= 0.5, (worst2[-3:], worst[-3:])


@pytest.mark.parametrize("cin,cout,B,H,W", [(512, 512, 2, 20, 31), (256, 512, 3, 16, 16), (512, 1024, 1, 24, 37)])
def test_conv1x1_data_gradient_on_the_split_pipe_with_accumulate(cin, cout, B, H, W):
    """Training plans (round 3): dX = dY W of a 1x1 layer as a plain 1x1 convolution of dY with the TRANSPOSED weight matrix
    on the split-bf16 pipe (weights split by xl_cnn_split_weight with taps = 0), the second producer of a gradient
    accumulating in the epilogue (XL_CONV_ACCUMULATE) - against autograd, at the fp32 kernels' tolerance."""
    import torch.nn as nn
    L = networks._bind()
    g = torch.Generator().manual_seed(cin + cout + H)
    x = torch.randn(B, cin, H, W, generator=g, requires_grad=True)
    conv = nn.Conv2d(cin, cout, 1)
    y = conv(x)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    ws = conv.weight.detach().cuda().contiguous()
    planes = torch.zeros(3 * ws.numel(), dtype=torch.int16, device="cuda")
    networks._check(L.xl_cnn_split_weight(ws.data_ptr(), planes.data_ptr(), cin, cout, 0, None))
    assert torch.equal(planes, networks._Plan.split_bf16_interleaved(ws.reshape(cout, cin).t().contiguous(), cout).reshape(-1))
    dyd = _nhwc(dy).cuda()
    gx = torch.full((B, H, W, cin), float("nan"), device="cuda")
    op = networks.XlOp()
    op.type, op.flags = networks.XL_OP_CONV, networks.CONV_SPLIT_BF16 | networks.CONV_SPLIT_IL
    op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout = B, H, W, cout, H, W, cin
    op.ksize, op.stride, op.ld_in, op.ld_out, op.reserved_i = 1, 1, cout, cin, 256
    op.in_, op.w, op.out = dyd.data_ptr(), planes.data_ptr(), gx.data_ptr()
    _run([op])
    ref = x.grad
    assert ((gx.cpu().permute(0, 3, 1, 2) - ref).abs().max() / ref.abs().max()).item() < 2e-5
    op.flags |= networks.CONV_ACCUMULATE
    _run([op, op])
    assert ((gx.cpu().permute(0, 3, 1, 2) - 3 * ref).abs().max() / ref.abs().max()).item() < 6e-5


@pytest.mark.parametrize("cin,cout,M,Z,splits", [(512, 512, 2 * 20 * 31, 1, 3), (256, 512, 1500, 1, 1), (512, 256, 777, 4, 2),
                                                 (512, 512, 2400, 36, 1), (256, 256, 300, 2, 5)])
def test_weight_gradient_products_on_the_split_pipe(cin, cout, M, Z, splits):
    """XL_OP_WGRAD with XL_CONV_SPLIT_BF16 (csrc/xl_wgrad_split.hip): P_z = dY_z^T X_z with the pixels / Winograd tiles as the
    K dimension, both operands fp32 and split inside the kernel, split-K partials reduced in fixed order - against float64,
    and within a small factor of the fp32-MFMA kernel's own rounding error.  Ragged K (not a multiple of 16) included."""
    g = torch.Generator().manual_seed(cin + cout + M + Z)
    x = torch.randn(Z, M, cin, generator=g)
    dy = torch.randn(Z, M, cout, generator=g)
    ref = torch.einsum("zto,ztc->zoc", dy.double(), x.double())
    xd, dyd = x.cuda(), dy.cuda()

    def run(flags, sp):
        out = torch.full((Z, cout, cin), float("nan"), device="cuda")
        scratch = torch.full((Z * sp * cout * cin,), float("nan"), device="cuda")
        op = networks.XlOp()
        op.type, op.flags = networks.XL_OP_WGRAD, flags
        op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout = 1, M, 1, cin, M, 1, cout
        op.ksize, op.stride, op.ld_in, op.ld_aux, op.groups, op.nchunks2 = 1, 1, cin, cout, Z, sp
        op.in_, op.aux, op.out, op.stats2 = xd.data_ptr(), dyd.data_ptr(), out.data_ptr(), scratch.data_ptr()
        _run([op])
        return out.cpu().double()
    got = run(networks.CONV_SPLIT_BF16, splits)
    scale = ref.abs().max().item()
    esp = (got - ref).abs().max().item() / scale
    e32 = (run(0, splits) - ref).abs().max().item() / scale
    assert esp < 2e-6 and esp < 4 * e32 + 2e-7, (esp, e32)


@pytest.mark.parametrize("CO,CI,B,H,W", [(64, 32, 2, 64, 96), (64, 32, 1, 41, 57), (128, 64, 2, 32, 48), (128, 64, 1, 35, 50)] +
                         [(CO, CI, 2, H, W) for CO, CI in ((64, 32), (128, 64)) for H in (33, 34) for W in (49, 50)])      # all four parity classes
def test_stride2_data_gradient_on_the_split_pipe_vs_float64(CO, CI, B, H, W):
    """XL_OP_S2_DGRAD (csrc/xl_stem_dgrad.hip, round 4): dX of a 3x3 stride-2 pad-1 convolution from dY, one launch over 16 x 32
    tiles of the result, against torch.nn.grad.conv2d_input in float64.  41 x 57 / 35 x 50: odd sizes and ragged tiles (the last
    input row / column is reached by fewer taps).  fp32-class: three-term bf16 splits, six MFMA passes, fp32 accumulation."""
    import ctypes
    g = torch.Generator().manual_seed(CO + H)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w = torch.randn(CO, CI, 3, 3, generator=g) * (2.0 / (9 * CI)) ** 0.5
    dy = torch.randn(B, CO, Ho, Wo, generator=g)
    ref = torch.nn.grad.conv2d_input((B, CI, H, W), w.double(), dy.double(), stride=2, padding=1)
    frag = networks._Plan.s2_dgrad_fragments(w.cuda())
    dy_d = dy.permute(0, 2, 3, 1).contiguous().cuda()
    dx = torch.full((B, H, W, CI), float("nan"), device="cuda")
    queue = torch.zeros(4, dtype=torch.int32, device="cuda")
    op = networks.XlOp()
    op.type = networks.XL_OP_S2_DGRAD
    op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout = B, Ho, Wo, CO, H, W, CI
    op.ksize, op.stride, op.ld_in, op.ld_out = 3, 2, CO, CI
    op.in_, op.w, op.out, op.stats = dy_d.data_ptr(), frag.data_ptr(), dx.data_ptr(), queue.data_ptr()
    arr = (networks.XlOp * 1)(op)
    for _ in range(2):                                   # twice: the tile queue must be left as it was found
        networks._check(networks._bind().xl_cnn_run(arr, 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert int(queue.abs().sum()) == 0
    got = dx.permute(0, 3, 1, 2).cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    print("stride-2 dgrad %d -> %d %dx%dx%d: %.2e of max (bound 2e-6)" % (CO, CI, B, H, W, err))
    assert err <= 2e-6, err


def test_fill0_zeroes_exactly_the_bytes_it_is_given():
    """XL_OP_FILL0 (the head of a backward op list zeroes the gradient-maximum slots with it): `Cin` bytes at `out`."""
    buf = torch.full((64,), float("nan"), device="cuda")
    op = networks.XlOp()
    op.type, op.Cin, op.out = networks.XL_OP_FILL0, 4 * 24, buf.data_ptr() + 4 * 8
    _run([op])
    got = buf.cpu()
    assert torch.isnan(got[:8]).all() and torch.isnan(got[32:]).all() and (got[8:32] == 0).all()


def test_groupnorm_parameter_gradients_of_a_layer_list_in_one_launch():
    """XL_OP_GNB_PARAMS_LIST: d gamma / d beta / d conv-bias of several layers in one launch from the sums their
    XL_OP_GNB_FINAL ops wrote to buffers of their own (op.scale) - against autograd (5e-6 / 2e-5, as
    test_groupnorm_backward_vs_autograd) and bitwise against XL_OP_GNB_PARAMS per layer.  Three layers of different widths,
    sizes and batch counts, one of them without a convolution in front (dbias NULL)."""
    import torch.nn.functional as F
    layers = [(2, 9, 13, 64, 1), (1, 12, 16, 512, 7), (3, 5, 7, 256, 0)]
    keep, items, results = [], [], []
    for li, (B, H, W, C, flags) in enumerate(layers):
        g = torch.Generator().manual_seed(C + flags)
        x = (torch.randn(B, C, H, W, generator=g) * 2 + 0.5).requires_grad_(True)
        aux = torch.randn(B, C, H, W, generator=g)
        gamma = (1 + 0.2 * torch.randn(C, generator=g)).requires_grad_(True)
        beta = (0.3 * torch.randn(C, generator=g)).requires_grad_(True)
        o = F.group_norm(x, 32, gamma, beta, 1e-5)
        if flags & 1:
            o = F.relu(o)
        if flags & 2:
            o = o + aux
        if flags & 4:
            o = F.relu(o)
        dout = torch.randn(o.shape, generator=g)
        o.backward(dout)
        HW = H * W
        nch, nch2 = max(1, min(128, (HW + 255) // 256)), max(1, min(128, (HW + 63) // 64))
        xd, ad, dd = _nhwc(x.detach()).cuda(), _nhwc(aux).cuda(), _nhwc(dout).cuda()
        gd, bd = gamma.detach().cuda(), beta.detach().cuda()
        stats = torch.zeros(B * nch * 32 * 2, dtype=torch.float64, device="cuda")
        outf = torch.empty_like(xd)
        table = torch.full((B * C * 4,), float("nan"), device="cuda")
        scratch = torch.zeros(B * nch2 * C * 3 + B * C * 6 + (B * C * 3 + 1) // 2, dtype=torch.float64, device="cuda")
        sums = torch.full((B * C * 6,), float("nan"), dtype=torch.float64, device="cuda")
        per_layer = [torch.full((C,), float("nan"), device="cuda") for _ in range(3)]
        listed = [torch.full((C,), float("nan"), device="cuda") for _ in range(3)]
        no_bias = li == 2

        def gn_op(typ):
            op = networks.XlOp()
            op.type = typ
            op.B, op.Hi, op.Wi, op.Cin, op.groups, op.nchunks, op.nchunks2 = B, H, W, C, 32, nch, nch2
            op.flags, op.eps = flags, 1e-5
            op.ld_in, op.ld_aux, op.ld_out = C, C, C
            op.in_, op.w, op.bias = xd.data_ptr(), gd.data_ptr(), bd.data_ptr()
            return op
        st, fin, ap = gn_op(networks.XL_OP_GN_STATS), gn_op(networks.XL_OP_GN_FINAL), gn_op(networks.XL_OP_GN_APPLY)
        st.stats = fin.stats = ap.stats = stats.data_ptr()
        fin.out, fin.out2 = table.data_ptr(), table.data_ptr() + 4 * B * C * 2
        ap.aux, ap.aux2, ap.out = ad.data_ptr(), table.data_ptr(), outf.data_ptr()
        ops = [st, fin, ap]
        for typ, own in ((networks.XL_OP_GNB_STATS, False), (networks.XL_OP_GNB_FINAL, False), (networks.XL_OP_GNB_PARAMS, False),
                         (networks.XL_OP_GNB_FINAL, True)):
            op = gn_op(typ)
            op.stats, op.aux, op.aux2, op.stats2 = table.data_ptr(), dd.data_ptr(), outf.data_ptr(), scratch.data_ptr()
            if typ == networks.XL_OP_GNB_PARAMS:
                op.out, op.out2, op.aux2 = per_layer[0].data_ptr(), per_layer[1].data_ptr(), per_layer[2].data_ptr()
                if no_bias:
                    op.flags = flags | networks.GN_NO_CONV_BIAS
            if own:
                op.scale = sums.data_ptr()
            ops.append(op)
        _run(ops)
        items.append((sums.data_ptr(), gd.data_ptr(), listed[0].data_ptr(), listed[1].data_ptr(),
                      0 if no_bias else listed[2].data_ptr(), B, C, 32, HW))
        keep.append((xd, ad, dd, gd, bd, stats, outf, table, scratch, sums))
        results.append((per_layer, listed, gamma.grad, beta.grad, x.grad.sum((0, 2, 3)), no_bias))
    tab = torch.from_numpy(np.array(items, dtype=networks.GNB_PARAMS_ITEM_DTYPE).view(np.uint8).copy()).cuda()
    op = networks.XlOp()
    op.type, op.Cin, op.Cout, op.in_ = networks.XL_OP_GNB_PARAMS_LIST, len(items), max(i[6] for i in items), tab.data_ptr()
    _run([op])

    def rel(a, b):
        return ((a - b).abs().max() / b.abs().max()).item()
    for per_layer, listed, dg, db, dbias, no_bias in results:
        assert rel(listed[0].cpu(), dg) < 5e-6 and rel(listed[1].cpu(), db) < 5e-6
        assert torch.equal(listed[0], per_layer[0]) and torch.equal(listed[1], per_layer[1])
        if no_bias:
            assert torch.isnan(listed[2]).all() and torch.isnan(per_layer[2]).all()       # neither form writes it
        else:
            assert rel(listed[2].cpu(), dbias) < 2e-5 and torch.equal(listed[2], per_layer[2])
