"""GPU, per op: XL_OP_CONV1_WGRAD (conv1_wgrad_kernel in both instantiations + conv1_wgrad_reduce_kernel) through
xl_cnn_run on inputs built here, against float64 on the CPU (tests/head_refs.py).  Training plans reach the op at one
setting (three input channels, 8 rows per workgroup, even heights) and throw its bias sum away (the plan takes conv1's
bias gradient from the GroupNorm sums), so until now nothing read slot 27 of the kernel, and the single-channel staging,
the single-row tail of an odd height and the > 64 KiB dynamic-LDS configuration never ran in a gradient test.

Criterion: 2e-5 of max |reference| for dW and db (test_conv_dgrad_and_wgrad_vs_autograd).  Results and scratch are NaN
before the launch; the floats behind dW / db must still be NaN afterwards."""
import pytest

torch = pytest.importorskip("torch")
import guarded                             # noqa: E402
torch = guarded.torch_proxy()              # empty / zeros / full (_like) on the device: between guard bands

import head_refs                                        # noqa: E402
from crossloc_amd import networks                      # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(autouse=True)
def _guard_bands(monkeypatch):
    """Every device tensor this module allocates (and every packed operand) sits between guard bands: checked after each test."""
    yield from guarded.op_module_check(monkeypatch, networks, __name__)


def _run(ops):
    arr = (networks.XlOp * len(ops))(*ops)
    networks._check(networks._bind().xl_cnn_run(arr, len(ops), None))
    torch.cuda.synchronize()


def _nan(n, dtype=torch.float32):
    return torch.full((n,), NAN, dtype=dtype, device="cuda")


def _strided(x_nchw, ld):
    """NCHW -> NHWC rows of `ld` floats on the GPU, NaN behind the channels."""
    B, C, H, W = x_nchw.shape
    buf = torch.full((B * H * W, ld), NAN, dtype=torch.float32)
    buf[:, :C] = x_nchw.permute(0, 2, 3, 1).reshape(-1, C)
    return buf.cuda()


def _rel(got, ref):
    return (got.double() - ref.double()).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _wgrad_op(img_d, dy_d, ld_aux, B, Cin, H, W, rows):
    """The plain op with fresh NaN results; returns (op, dW buffer, db buffer, keep-alive)."""
    rpb = rows if rows > 0 else 16
    dw, db = _nan(32 * Cin * 9 + 4), _nan(32 + 4)
    scratch = _nan(B * ((H + rpb - 1) // rpb) * 28 * 32)
    op = networks.XlOp()
    op.type = networks.XL_OP_CONV1_WGRAD
    op.B, op.Hi, op.Wi, op.Cin, op.Cout, op.ld_aux, op.reserved_i = B, H, W, Cin, 32, ld_aux, rows
    op.in_, op.aux, op.out, op.out2, op.stats2 = img_d.data_ptr(), dy_d.data_ptr(), dw.data_ptr(), db.data_ptr(), scratch.data_ptr()
    return op, dw, db, scratch


def _results(dw, db, Cin):
    assert torch.isnan(dw[32 * Cin * 9:]).all() and torch.isnan(db[32:]).all()
    gw, gb = dw[:32 * Cin * 9].reshape(32, Cin, 3, 3).cpu(), db[:32].cpu()
    assert torch.isfinite(gw).all() and torch.isfinite(gb).all()
    return gw, gb


# (1, 41, 57): odd height - the last step of a workgroup is a single row; (3, 7, 5) / (1, 1, 1): frames smaller than a step
# of 32 pixels; (1, 9, 1100): 4 staged rows of 1102 float4 = 70528 bytes of LDS, past the 64 KiB a kernel gets unasked
# (2, 42, 57) / (2, 41, 58): height and width of opposite parity
SHAPES = [(2, 40, 56), (1, 41, 57), (3, 7, 5), (1, 1, 1), (1, 9, 1100), (2, 42, 57), (2, 41, 58)]


@pytest.mark.parametrize("rows", [0, 8, 3, "H"])
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("Cin", [1, 3])
def test_conv1_weight_and_bias_gradient_vs_float64(Cin, B, H, W, rows):
    """rows = image rows per workgroup (reserved_i): 0 = the default 16, 8 = the plans' value, 3 = every workgroup ends on a
    single-row step, H = one workgroup per image."""
    _plain_case(Cin, B, H, W, H if rows == "H" else rows, 32)


def _plain_case(Cin, B, H, W, rows, ld_aux):
    g = torch.Generator().manual_seed(Cin * 1000 + H * W + rows)
    img = torch.rand(B, Cin, H, W, generator=g)
    dy = torch.randn(B, 32, H, W, generator=g)
    rw, rb = head_refs.conv1_wgrad_reference(img.double(), dy.double())
    w32, b32 = head_refs.conv1_wgrad_reference(img, dy)
    op, dw, db, keep = _wgrad_op(img.cuda(), _strided(dy, ld_aux), ld_aux, B, Cin, H, W, rows)
    _run([op])
    gw, gb = _results(dw, db, Cin)
    ew, eb = _rel(gw, rw), _rel(gb, rb)
    print("conv1 wgrad Cin %d %dx%dx%d rows %d: dW %.2e, db %.2e of max (fp32 on the CPU: %.2e, %.2e)"
          % (Cin, B, H, W, rows, ew, eb, _rel(w32, rw), _rel(b32, rb)))
    assert ew <= 2e-5 and eb <= 2e-5, (ew, eb)


@pytest.mark.parametrize("Cin", [1, 3])
def test_conv1_weight_gradient_reads_a_strided_gradient(Cin):
    """dY as 32 channels of rows 48 floats wide (ld_aux > 32), NaN behind them."""
    _plain_case(Cin, 2, 41, 57, 8, 48)


@pytest.mark.parametrize("Cin,B,H,W,rows,relu,ld", [(3, 2, 40, 56, 8, True, 32), (3, 1, 41, 57, 0, True, 32), (1, 2, 41, 57, 3, True, 32),
                                                    (1, 1, 7, 5, 7, True, 32), (3, 2, 41, 57, 8, False, 40), (3, 1, 9, 1100, 8, True, 32)])
def test_folded_conv1_weight_gradient_vs_autograd_and_the_separate_apply_pass(Cin, B, H, W, rows, relu, ld):
    """aux2 set: the op takes the gradient w.r.t. the OUTPUT of conv1's GroupNorm(32, 32) + ReLU and applies the GroupNorm
    backward while it loads.  The chain is built like test_groupnorm_backward_vs_autograd's (GN_STATS, GN_FINAL, GN_APPLY for
    the activation, GNB_STATS, GNB_FINAL), `w` = the forward table, `bias` = the coefficient block inside the scratch buffer.
      * against float64 autograd of conv1 -> GroupNorm -> ReLU w.r.t. conv1.weight, 2e-5 of max;
      * bitwise against XL_OP_GNB_APPLY followed by the plain form at the same rows per workgroup (the kernel comment promises
        the same operations in the same order), weight gradient and bias sum.
    Cells whose normalised value is within 1e-4 of zero get no upstream gradient: ReLU' jumps there and fp32 may land on the
    other side (the conv1 output the kernels read is the float64 one rounded to fp32)."""
    C, flags = 32, (networks.GN_RELU_IN if relu else 0)
    g = torch.Generator().manual_seed(Cin + H * W + rows)
    img = torch.rand(B, Cin, H, W, generator=g)
    w = (torch.randn(32, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5)
    b = torch.randn(32, generator=g) * 0.1
    gamma, beta = 1 + 0.2 * torch.randn(32, generator=g), 0.3 * torch.randn(32, generator=g)
    dout = torch.randn(B, 32, H, W, generator=g)
    wr = w.double().requires_grad_(True)
    o, raw = head_refs.conv1_gn_relu(img.double(), wr, b.double(), gamma.double(), beta.double(), relu)
    if relu:
        pre = torch.nn.functional.group_norm(raw.detach(), 32, gamma.double(), beta.double(), 1e-5)
        dout[pre.abs() < 1e-4] = 0.0
    (o * dout.double()).sum().backward()

    HW = H * W
    nch, nch2 = max(1, min(128, (HW + 255) // 256)), max(1, min(128, (HW + 63) // 64))
    xd, dd = _strided(raw.detach().float(), ld), _strided(dout, ld)
    img_d, gd, bd = img.cuda(), gamma.cuda(), beta.cuda()
    stats = torch.zeros(B * nch * 32 * 2, dtype=torch.float64, device="cuda")
    table = _nan(B * C * 4)
    outf = torch.full((B * HW, ld), NAN, device="cuda")
    n_sd = B * nch2 * C * 3 + B * C * 6
    scratch = torch.zeros(n_sd + (B * C * 3 + 1) // 2, dtype=torch.float64, device="cuda")
    dx = torch.full((B * HW, ld), NAN, device="cuda")

    def gn_op(typ):
        op = networks.XlOp()
        op.type = typ
        op.B, op.Hi, op.Wi, op.Cin, op.groups, op.nchunks, op.nchunks2 = B, H, W, C, 32, nch, nch2
        op.flags, op.eps = flags, 1e-5
        op.ld_in, op.ld_aux, op.ld_out = ld, ld, ld
        op.in_, op.w, op.bias = xd.data_ptr(), gd.data_ptr(), bd.data_ptr()
        return op
    st = gn_op(networks.XL_OP_GN_STATS)
    st.stats = stats.data_ptr()
    fin = gn_op(networks.XL_OP_GN_FINAL)
    fin.stats, fin.out, fin.out2 = stats.data_ptr(), table.data_ptr(), table.data_ptr() + 4 * B * C * 2
    ap = gn_op(networks.XL_OP_GN_APPLY)
    ap.stats, ap.aux2, ap.out = stats.data_ptr(), table.data_ptr(), outf.data_ptr()
    chain = [st, fin, ap]
    for typ in (networks.XL_OP_GNB_STATS, networks.XL_OP_GNB_FINAL, networks.XL_OP_GNB_APPLY):
        op = gn_op(typ)
        op.stats, op.aux, op.aux2, op.stats2 = table.data_ptr(), dd.data_ptr(), outf.data_ptr(), scratch.data_ptr()
        if typ == networks.XL_OP_GNB_APPLY:
            op.out = dx.data_ptr()
        chain.append(op)
    plain, dw_p, db_p, keep_p = _wgrad_op(img_d, dx, ld, B, Cin, H, W, rows)
    fold, dw_f, db_f, keep_f = _wgrad_op(img_d, dd, ld, B, Cin, H, W, rows)
    fold.aux2, fold.ld_in, fold.flags = xd.data_ptr(), ld, flags
    fold.w, fold.bias = table.data_ptr(), scratch.data_ptr() + 8 * n_sd
    _run(chain + [plain, fold])
    gw_p, gb_p = _results(dw_p, db_p, Cin)
    gw_f, gb_f = _results(dw_f, db_f, Cin)
    e = _rel(gw_f, wr.grad)
    print("folded conv1 wgrad Cin %d %dx%dx%d rows %d: dW %.2e of max" % (Cin, B, H, W, rows, e))
    assert e <= 2e-5, e
    assert torch.equal(gw_f, gw_p) and torch.equal(gb_f, gb_p)
    if ld > C:
        assert torch.isnan(dx[:, C:]).all() and torch.isnan(outf[:, C:]).all()
