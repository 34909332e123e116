"""GPU, per op: XL_OP_HEAD / XL_OP_HEAD_BWD and XL_OP_DUC_HEAD / XL_OP_DUC_HEAD_BWD (with duc_trim_bwd_kernel and
partial_sum_kernel behind them) driven through xl_cnn_run on inputs built here, against float64 references on the CPU
(tests/head_refs.py, pinned to oracle/cnn_oracle.py by tests/test_head_refs.py) with autograd for the gradients.

The whole-network gradient tests reach these ops too, but their criterion has to absorb ReLU-mask flips (5e-2); a wrong
interpolation weight, a window one row short or a mis-gated clamp stays below it.  Here there is no ReLU, so the project's
per-op criteria apply: outputs within 1e-4 of the largest task-channel value (mean removed) and rtol 2e-4 on the positive
channel (test_head_vs_torch), gradients within 2e-5 of max |reference| (test_conv_dgrad_and_wgrad_vs_autograd).

Every output buffer is NaN before the launch; dx is written with a pixel stride wider than its channels into a NaN buffer,
the gaps (and the floats behind every dense result) must still be NaN afterwards.

The clamp: fc3's positive row is mapped affinely so that a fixed share of the cells lies beyond each hardtanh bound
(asserted on the float64 reference BEFORE anything runs: >= 5 % at each bound, >= 50 % strictly inside; cells within fp32 rounding of a
bound get no upstream gradient, see _mask_ambiguous).  A second
backward launch with a zero gradient on the task channels must return exactly 0 for the saturated cells.  One pixel cannot
hold three states: the single-pixel case is launched four times (below, above, twice inside) and the census is taken over
the four launches."""
import math

import pytest

torch = pytest.importorskip("torch")
import guarded                             # noqa: E402
torch = guarded.torch_proxy()              # empty / zeros / full (_like) on the device: between guard bands

import head_refs                                        # noqa: E402
from crossloc_amd import networks                      # noqa: E402

pytestmark = pytest.mark.gpu
LO, HI = head_refs.CLAMP_LO, head_refs.CLAMP_HI
MEAN = [-455.934, 417.50, 520.31, 241.47, 0.0, 12.5]
NAN = float("nan")
BOUNDS = {"task": 1e-4, "pos": 2e-4, "dx": 2e-5, "dW": 2e-5, "db": 2e-5}      # the per-op criteria (module docstring)


@pytest.fixture(autouse=True)
def _guard_bands(monkeypatch):
    """Every device tensor this module allocates (and every packed operand) sits between guard bands: checked after each test."""
    yield from guarded.op_module_check(monkeypatch, networks, __name__)


def _run(ops):
    arr = (networks.XlOp * len(ops))(*ops)
    networks._check(networks._bind().xl_cnn_run(arr, len(ops), None))
    torch.cuda.synchronize()


def _nan(n):
    return torch.full((n,), NAN, dtype=torch.float32, device="cuda")


def _strided(x_nhwc, ld, off):
    """[..., C] -> NaN buffer [pixels, ld] on the GPU holding x at channel offset off."""
    C = x_nhwc.shape[-1]
    buf = torch.full((x_nhwc.numel() // C, ld), NAN, dtype=torch.float32)
    buf[:, off:off + C] = x_nhwc.reshape(-1, C)
    return buf.cuda()


def _rel(got, ref):
    return (got.double() - ref.double()).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _census_ok(sc_pos):
    lo, hi, inside = head_refs.clamp_census(sc_pos)
    assert lo >= 0.05 and hi >= 0.05 and inside >= 0.5, (lo, hi, inside)


def _mask_ambiguous(dout, sc, sc32, n_task):
    """Zero the upstream gradient of positive-channel cells whose float64 raw value sc is close to a hardtanh bound: the
    derivative jumps there (by exp(HI) = 1e6 at the upper bound) and an fp32 forward pass may land on either side.  Close =
    within 4 x the largest error of the raw value in plain fp32 on the CPU (sc32), at least 1e-4: about 1e-4 for the 1x1 head,
    up to 1e-2 at the augmentation-sized DUC case, where the fp32 source coordinates of the bilinear resize cost 2.6e-3.
    The forward comparison keeps those cells: the output is continuous."""
    margin = max(1e-4, 4.0 * (sc32[:, n_task:].double() - sc[:, n_task:]).abs().max().item())
    amb = ((sc[:, n_task:] - LO).abs() < margin) | ((sc[:, n_task:] - HI).abs() < margin)
    dout[:, n_task:][amb] = 0.0
    return amb[:, 0]


def _check_forward(got, ref, n_task, mean, tag, bounds=None):
    bounds = bounds or BOUNDS
    m = mean[None, :, None, None]
    et = (got[:, :n_task] - m - (ref[:, :n_task] - m)).abs().max().item() / max((ref[:, :n_task] - m).abs().max().item(), 1e-6)
    print("%s: task channels %.2e of max" % (tag, et))
    assert et <= bounds["task"], ("task", et)
    if got.shape[1] > n_task:
        ep = ((got[:, n_task:] - ref[:, n_task:]).abs() / ref[:, n_task:].abs()).max().item()
        print("%s: positive channel rel %.2e" % (tag, ep))
        assert ep <= bounds["pos"], ("pos", ep)


HEAD_CHANNELS = [(512, 4, 3, 1), (512, 3, 2, 1), (512, 2, 1, 1), (512, 3, 3, 0), (512, 1, 1, 0), (128, 4, 3, 1), (128, 2, 1, 1)]
HEAD_PIXELS = [(1, 1, 1), (1, 7, 9), (2, 9, 13), (3, 61, 91)]        # 1, 63, 234 and 16653 pixels (> the 1024 waves of HEAD_BWD)


def _head_once(x, w, b, mean, n_task, n_pos, ld_in, off_in, seed, tag):
    """One forward + two backward launches on given fp32 tensors; returns the float64 raw output of fc3."""
    B, Cin, H, W = x.shape
    Cout, HW = n_task + n_pos, H * W
    g = torch.Generator().manual_seed(seed)
    dout = torch.randn(B, Cout, H, W, generator=g)
    xr = x.double().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref, sc = head_refs.head_reference(xr, wr, br, mean.double(), n_task, n_pos)
    sat = amb = None
    if n_pos:
        sat = ((sc[:, n_task:] <= LO) | (sc[:, n_task:] >= HI)).detach()[:, 0]            # [B,H,W]
        with torch.no_grad():
            sc32 = head_refs.head_reference(x, w, b, mean, n_task, n_pos)[1]
        amb = _mask_ambiguous(dout, sc.detach(), sc32, n_task)
    (ref * dout.double()).sum().backward()
    # plain fp32 on the CPU, for the record: the figure the issue's fall-back bound would be derived from
    x32, w32, b32 = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    r32, _ = head_refs.head_reference(x32, w32, b32, mean, n_task, n_pos)
    (r32 * dout).sum().backward()

    xd = _strided(x.permute(0, 2, 3, 1), ld_in, off_in)
    wd, bd, md, dd = w.contiguous().cuda(), b.cuda(), mean.cuda(), dout.cuda()
    out = _nan(B * Cout * HW + 16)
    op = networks.XlOp()
    op.type = networks.XL_OP_HEAD
    op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout, op.n_task, op.n_pos, op.ld_in = B, H, W, Cin, H, W, Cout, n_task, n_pos, ld_in
    op.clamp_lo, op.clamp_hi = LO, HI
    op.in_, op.w, op.bias, op.aux, op.out = xd.data_ptr() + 4 * off_in, wd.data_ptr(), bd.data_ptr(), md.data_ptr(), out.data_ptr()
    _run([op])
    assert torch.isnan(out[B * Cout * HW:]).all()
    got = out[:B * Cout * HW].reshape(B, Cout, H, W).cpu()
    assert torch.isfinite(got).all()
    _check_forward(got, ref.detach(), n_task, mean, tag)

    ld_dx, off_dx = Cin + 8, 4
    waves = 4 * max(1, min(256, (B * HW + 63) // 64))
    for task_grad in (True, False):
        dd2 = dd.clone()
        if not task_grad:
            if not n_pos:
                break
            dd2[:, :n_task] = 0.0
        dx = torch.full((B * HW, ld_dx), NAN, device="cuda")
        dw, db, scratch = _nan(Cout * Cin + 4), _nan(Cout + 4), _nan(waves * Cout * (Cin + 1))
        bw = networks.XlOp()
        bw.type = networks.XL_OP_HEAD_BWD
        bw.B, bw.Hi, bw.Wi, bw.Cin, bw.Cout, bw.n_task, bw.n_pos = B, H, W, Cin, Cout, n_task, n_pos
        bw.ld_in, bw.ld_out = ld_in, ld_dx
        bw.clamp_lo, bw.clamp_hi = LO, HI
        bw.in_, bw.w, bw.aux, bw.aux2 = xd.data_ptr() + 4 * off_in, wd.data_ptr(), dd2.data_ptr(), out.data_ptr()
        bw.out, bw.out2, bw.stats, bw.stats2 = dx.data_ptr() + 4 * off_dx, dw.data_ptr(), db.data_ptr(), scratch.data_ptr()
        _run([bw])
        dxh = dx.cpu()
        assert torch.isnan(dxh[:, :off_dx]).all() and torch.isnan(dxh[:, off_dx + Cin:]).all()
        assert torch.isnan(dw[Cout * Cin:]).all() and torch.isnan(db[Cout:]).all()
        gx = dxh[:, off_dx:off_dx + Cin].reshape(B, H, W, Cin).permute(0, 3, 1, 2)
        gw, gb = dw[:Cout * Cin].reshape(Cout, Cin).cpu(), db[:Cout].cpu()
        assert torch.isfinite(gx).all() and torch.isfinite(gw).all() and torch.isfinite(gb).all()
        if task_grad:
            for name, a, r, r32_ in (("dx", gx, xr.grad, x32.grad), ("dW", gw, wr.grad, w32.grad), ("db", gb, br.grad, b32.grad)):
                e = _rel(a, r)
                print("%s: %s %.2e of max (fp32 on the CPU: %.2e)" % (tag, name, e, _rel(r32_, r)))
                assert e <= 2e-5, (name, e)
        else:
            # only the positive channel carries a gradient: saturated cells get exactly nothing
            assert (gx.permute(0, 2, 3, 1)[sat] == 0).all()
            inside = ~sat & ~amb
            want = (dout[:, n_task].double() * ref[:, n_task].detach())[~sat].sum().item()
            assert gb[:n_task].abs().max().item() == 0.0
            assert abs(gb[n_task].item() - want) <= 2e-5 * max(abs(want), br.grad.abs().max().item())
            if inside.any():
                assert (gx.permute(0, 2, 3, 1)[inside].abs().amax(1) > 0).all()
    return sc.detach()


def _head_case(Cin, Cout, n_task, n_pos, B, H, W, ld_in=None, off_in=0):
    import torch.nn as nn
    assert Cout == n_task + n_pos
    ld_in = ld_in or Cin
    seed = Cin + 10 * Cout + 100 * n_pos + B * H * W
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    bound = 20.0 / math.sqrt(Cin)                                    # nn.Conv2d's default initialisation, times 20 (test_head_vs_torch)
    w = (torch.rand(Cout, Cin, generator=g) * 2 - 1) * bound
    b = (torch.rand(Cout, generator=g) * 2 - 1) * bound
    mean = torch.tensor(MEAN[:n_task])
    tag = "head %d->%d+%d, %dx%dx%d" % (Cin, n_task, n_pos, B, H, W)
    if not n_pos:
        _head_once(x, w, b, mean, n_task, n_pos, ld_in, off_in, seed, tag)
        return
    z = torch.nn.functional.conv2d(x.double(), w.double()[:, :, None, None], b.double())[:, n_task]
    if B * H * W >= 9:
        head_refs.map_positive_row(w, b, z, n_task)
        _, sc = head_refs.head_reference(x.double(), w.double(), b.double(), mean.double(), n_task, n_pos)
        _census_ok(sc[:, n_task:])                                   # before anything runs on the GPU
        _head_once(x, w, b, mean, n_task, n_pos, ld_in, off_in, seed, tag)
        return
    # a single pixel: four launches, the bias puts the cell below LO, above HI and twice inside
    raws = []
    targets = (LO - 3.0, HI + 3.0, -5.0, 9.0)
    plans = []
    for t in targets:
        b2 = b.clone()
        b2[n_task] = float(b[n_task].double().item() + t - z.flatten()[0].item())
        _, sc = head_refs.head_reference(x.double(), w.double(), b2.double(), mean.double(), n_task, n_pos)
        raws.append(sc[:, n_task:].flatten())
        plans.append(b2)
    _census_ok(torch.cat(raws))
    for t, b2 in zip(targets, plans):
        _head_once(x, w, b2, mean, n_task, n_pos, ld_in, off_in, seed, tag + " raw %.1f" % t)


@pytest.mark.parametrize("B,H,W", HEAD_PIXELS)
@pytest.mark.parametrize("Cin,Cout,n_task,n_pos", HEAD_CHANNELS)
def test_head_and_head_backward_vs_float64(Cin, Cout, n_task, n_pos, B, H, W):
    _head_case(Cin, Cout, n_task, n_pos, B, H, W)


@pytest.mark.parametrize("Cin,Cout,n_task,n_pos", [(512, 4, 3, 1), (128, 2, 1, 1)])
def test_head_reads_a_channel_slice(Cin, Cout, n_task, n_pos):
    """x is channels [32, 32 + Cin) of a buffer Cin + 64 wide (ld_in > Cin); everything around the slice is NaN."""
    _head_case(Cin, Cout, n_task, n_pos, 2, 9, 13, ld_in=Cin + 64, off_in=32)


# (B, Hs, Ws, H, W): pure shuffle, bilinear trim in both / one direction, a one-row strip, one augmentation-sized frame
# (2 x 323 x 485 = 313310 pixels: 1224 blocks of 256, past the backward's cap of 1024 - its grid-stride loop runs)
DUC_SHAPES = [(2, 8, 12, 64, 96), (3, 1, 1, 8, 8),
              (2, 8, 12, 60, 92), (2, 8, 12, 57, 91), (2, 8, 12, 64, 91), (2, 8, 12, 57, 96), (3, 1, 2, 1, 9),
              (2, 41, 61, 323, 485)]


def _duc_inputs(C, n_task, n_pos, B, Hs, Ws, H, W):
    """Inputs of one DUC case, the float64 reference with its gradients and the same in plain fp32 on the CPU."""
    seed = C * 1000 + Hs * Ws + H + W
    g = torch.Generator().manual_seed(seed)
    Cin = C * 64
    x = torch.randn(B, Cin, Hs, Ws, generator=g)
    bound = 20.0 / math.sqrt(C)
    w = (torch.rand(C, C, generator=g) * 2 - 1) * bound
    b = (torch.rand(C, generator=g) * 2 - 1) * bound
    mean = torch.tensor(MEAN[:n_task])
    dout = torch.randn(B, C, H, W, generator=g)
    if n_pos:
        _, sc = head_refs.duc_head_reference(x.double(), w.double(), b.double(), mean.double(), n_task, n_pos, (H, W))
        head_refs.map_positive_row(w, b, sc[:, n_task], n_task)
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref, sc = head_refs.duc_head_reference(xr, wr, br, mean.double(), n_task, n_pos, (H, W))
    if n_pos:
        _census_ok(sc[:, n_task:].detach())                          # before anything runs on the GPU
        with torch.no_grad():
            sc32 = head_refs.duc_head_reference(x, w, b, mean, n_task, n_pos, (H, W))[1]
        _mask_ambiguous(dout, sc.detach(), sc32, n_task)
    (ref * dout.double()).sum().backward()
    x32, w32, b32 = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    r32, _ = head_refs.duc_head_reference(x32, w32, b32, mean, n_task, n_pos, (H, W))
    (r32 * dout).sum().backward()

    return x, w, b, mean, dout, (xr, wr, br, ref, sc), (x32, w32, b32, r32)


# Cases of the bilinear trim that miss a per-op criterion, and why it is no error of the kernels: the source coordinate
# sy * (y + 0.5) - 0.5 is an fp32 expression (in the reference's F.interpolate as in duc_head_kernel), so an interpolation
# weight carries an absolute error that grows with the coordinate, and fc3's positive row - about 10 per unit of activation,
# so that the raw value spans both clamp bounds - turns it into a RELATIVE error of exp().  PyTorch's own fp32 kernels on the
# CPU show the same figures against float64 (the GPU's agree with them to three digits).  For these entries the bound is
# 4 x the error of plain fp32 PyTorch on the CPU against the float64 reference, which is the number recorded here
# ((C, H, W) -> quantity -> fp32-CPU error; every quantity not listed keeps its per-op criterion):
DUC_FP32_CPU_ERROR = {
    (6, 323, 485): {"dx": 4.89e-05, "dW": 3.32e-05},
    (4, 60, 92): {"pos": 3.19e-04, "dx": 7.73e-05, "dW": 3.77e-05},
    (4, 57, 91): {"pos": 5.46e-04, "dx": 1.90e-04, "dW": 2.22e-04, "db": 5.66e-04},
    (4, 64, 91): {"pos": 5.09e-04, "dx": 6.48e-05, "dW": 6.64e-05},
    (4, 57, 96): {"dx": 4.02e-05, "dW": 2.16e-05},
    (4, 323, 485): {"pos": 2.61e-03, "dx": 8.20e-04, "dW": 1.75e-04, "db": 3.96e-04},
}


@pytest.mark.parametrize("B,Hs,Ws,H,W", DUC_SHAPES)
@pytest.mark.parametrize("C,n_task,n_pos", [(6, 6, 0), (4, 3, 1)])
def test_duc_head_and_backward_vs_float64(C, n_task, n_pos, B, Hs, Ws, H, W):
    """C = 6: the semantics head.  C = 4 (3 + 1): accepted by the op, and the only way the clamp gate of the DUC kernels runs.
    Bounds: the per-op criteria (BOUNDS), except for the entries of DUC_FP32_CPU_ERROR: 4 x the recorded fp32-CPU error, e.g.
    2 x 323 x 485 with C = 4: positive channel 1.04e-2 (from 2.61e-3), dx 3.28e-3 (8.20e-4), dW 7.0e-4 (1.75e-4), db 1.58e-3
    (3.96e-4); 57 x 91 with C = 4: 2.18e-3 (5.46e-4), 7.6e-4 (1.90e-4), 8.9e-4 (2.22e-4), 2.26e-3 (5.66e-4); the rest as
    the table above reads."""
    tag = "duc C=%d %dx%dx%d -> %dx%d" % (C, B, Hs, Ws, H, W)
    bounds = dict(BOUNDS)
    bounds.update({k: 4.0 * v for k, v in DUC_FP32_CPU_ERROR.get((C, H, W), {}).items()})
    Cin = C * 64
    x, w, b, mean, dout, (xr, wr, br, ref, sc), (x32, w32, b32, r32) = _duc_inputs(C, n_task, n_pos, B, Hs, Ws, H, W)
    ld_in, off_in, ld_dx, off_dx = Cin + 8, 4, Cin + 16, 8
    xd = _strided(x.permute(0, 2, 3, 1), ld_in, off_in)
    wd, bd, md, dd = w.contiguous().cuda(), b.cuda(), mean.cuda(), dout.cuda()
    n_out = B * C * H * W
    out = _nan(n_out + 16)
    op = networks.XlOp()
    op.type = networks.XL_OP_DUC_HEAD
    op.B, op.Hi, op.Wi, op.Cin, op.Ho, op.Wo, op.Cout, op.n_task, op.n_pos, op.ld_in = B, Hs, Ws, Cin, H, W, C, n_task, n_pos, ld_in
    op.clamp_lo, op.clamp_hi = LO, HI
    op.in_, op.w, op.bias, op.aux, op.out = xd.data_ptr() + 4 * off_in, wd.data_ptr(), bd.data_ptr(), md.data_ptr(), out.data_ptr()
    _run([op])
    assert torch.isnan(out[n_out:]).all()
    got = out[:n_out].reshape(B, C, H, W).cpu()
    assert torch.isfinite(got).all()
    _check_forward(got, ref.detach(), n_task, mean, tag, bounds)

    blocks = max(1, min(1024, (B * H * W + 255) // 256))
    n_scratch = (blocks + 1) * (C * C + C) + n_out
    for task_grad in (True, False):
        dd2 = dd.clone()
        if not task_grad:
            if not n_pos:
                break
            dd2[:, :n_task] = 0.0
        dx = torch.full((B * Hs * Ws, ld_dx), NAN, device="cuda")
        dw, db, scratch = _nan(C * C + 4), _nan(C + 4), _nan(n_scratch + 16)
        bw = networks.XlOp()
        bw.type = networks.XL_OP_DUC_HEAD_BWD
        bw.B, bw.Hi, bw.Wi, bw.Cin, bw.Ho, bw.Wo, bw.Cout, bw.n_task, bw.n_pos = B, Hs, Ws, Cin, H, W, C, n_task, n_pos
        bw.ld_in, bw.ld_out = ld_in, ld_dx
        bw.clamp_lo, bw.clamp_hi = LO, HI
        bw.in_, bw.w, bw.aux, bw.aux2 = xd.data_ptr() + 4 * off_in, wd.data_ptr(), dd2.data_ptr(), out.data_ptr()
        bw.out, bw.out2, bw.stats, bw.stats2 = dx.data_ptr() + 4 * off_dx, dw.data_ptr(), db.data_ptr(), scratch.data_ptr()
        _run([bw])
        dxh = dx.cpu()
        assert torch.isnan(dxh[:, :off_dx]).all() and torch.isnan(dxh[:, off_dx + Cin:]).all()
        assert torch.isnan(dw[C * C:]).all() and torch.isnan(db[C:]).all() and torch.isnan(scratch[n_scratch:]).all()
        gx = dxh[:, off_dx:off_dx + Cin].reshape(B, Hs, Ws, Cin).permute(0, 3, 1, 2)
        gw, gb = dw[:C * C].reshape(C, C).cpu(), db[:C].cpu()
        assert torch.isfinite(gx).all() and torch.isfinite(gw).all() and torch.isfinite(gb).all()
        if task_grad:
            errs = []
            for name, a, r, r32_ in (("dx", gx, xr.grad, x32.grad), ("dW", gw, wr.grad, w32.grad), ("db", gb, br.grad, b32.grad)):
                e = _rel(a, r)
                print("%s: %s %.2e of max (fp32 on the CPU: %.2e)" % (tag, name, e, _rel(r32_, r)))
                errs.append((name, e))
            for name, e in errs:
                assert e <= bounds[name], (name, e, bounds[name])
        else:
            # only the positive channel carries a gradient: where every output cell is saturated, nothing comes back
            sat = ((sc[:, n_task] <= LO) | (sc[:, n_task] >= HI)).detach()
            want = (dout[:, n_task].double() * ref[:, n_task].detach())[~sat].sum().item()
            assert gb[:n_task].abs().max().item() == 0.0
            assert abs(gb[n_task].item() - want) <= bounds["db"] * max(abs(want), br.grad.abs().max().item())
            xz = x.double().requires_grad_(True)
            rz, _ = head_refs.duc_head_reference(xz, w.double(), b.double(), mean.double(), n_task, n_pos, (H, W))
            (rz[:, n_task:] * dout[:, n_task:].double()).sum().backward()
            dead = xz.grad == 0                                     # elements that only saturated cells read
            assert (gx[dead] == 0).all()
            assert _rel(gx, xz.grad) <= bounds["dx"]
