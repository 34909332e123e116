"""GPU: the op lists that ship, run with every buffer the plan owns between guard bands (tests/guarded.py).

Every case builds a network and runs it as always, then builds the same network again (same seeded weights) while the name
`torch` is proxied in networks, lower_forward, lower_backward and packing - workspace, statistics, coefficient tables, pair
scales, packed operands, graph input and output, backward scratch, the flat gradient buffer and the kept V then all come from
the registry - and runs it on the same input.  Required:

  * outputs (and the flat gradient buffer of a training plan) BITWISE equal to the unguarded run: where a buffer lies must not
    change a bit, and since `empty` interiors are NaN-filled, a kernel that reads workspace nobody wrote in this pass differs;
  * every guard band intact: no kernel stored before or behind a tensor it was given.

Sizes: frames (128 + a, 136 + (3a + 1) mod 8), a = 0..7 - H and W of opposite parity, every residue mod 8 once on each side,
cell grids of 16-17 x 17-18 (>= 272 cells): the smallest grids at which the 1x1 layers and the stride-2 stem layers are eligible
for the matrix pipe (forms.py: H*W >= 256, Ho*Wo >= 256), ragged against the 6x6 and the 4x4 Winograd tiles.  Batch 3: the
256-row tiles straddle both image boundaries and the last one is partial (816 - 870 rows).  `_check_forms` asserts from
plan.ops that these sizes select those forms (no size had to be raised for it).

A guarded training plan hands out a fresh gradient result buffer on every backward pass (guarded.py, `_sole_owner`); the
comparison reads the plan's own flat buffer."""
import os

import pytest

torch = pytest.importorskip("torch")

import guarded                                                                  # noqa: E402
from crossloc_amd import lower_backward, lower_forward, networks, packing     # noqa: E402
from crossloc_amd.weights import seeded_state_dict                             # noqa: E402

pytestmark = pytest.mark.gpu
MEAN = torch.tensor([-455.934, 417.50, 520.31])
B = 3
SIZES = [(128 + a, 136 + (3 * a + 1) % 8) for a in range(8)]
IDS = ["%dx%d" % s for s in SIZES]
PLAN_MODULES = (networks, lower_forward, lower_backward, packing)
SINGLE = (MEAN, False, False, 1, 1, 3, 1)


def _net(args, batch_invariant=False):
    net = networks.TransPoseNet(*args)
    net.load_state_dict(seeded_state_dict(net, seed=31))
    net.batch_invariant = batch_invariant
    return net.cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(net, x, train, dout):
    """Inference: the eager call, the call that captures the HIP graph, a replay.  Training: forward and run_backward on `dout`
    (None: a seeded random one of the output's shape).  Returns (tensors to compare, plan, dout)."""
    if not train:
        net.eval()
        with torch.no_grad():
            ys = [net(x).clone() for _ in range(3)]
        torch.cuda.synchronize()
        plan = [p for p in net._plans.values() if not p.train][0]
        if os.environ.get("XL_CNN_GRAPH") != "0" and os.environ.get("XL_GEMM_SPLIT_BF16") not in ("0", "1"):
            assert plan.graph is not None and plan.graph_runs == 3
        return ys, plan, None
    net.train()
    y = net(x)
    plan = [p for p in net._plans.values() if p.train][0]
    if dout is None:
        dout = torch.randn(y.shape, generator=torch.Generator().manual_seed(y.shape[-1])).cuda()
    grads = plan.run_backward(dout)
    torch.cuda.synchronize()
    assert len(grads) > 0 and plan.grad_flat.numel() >= sum(g.numel() for _, g in grads)
    return [y.detach().clone(), plan.grad_flat.clone()], plan, dout


def _case(monkeypatch, args, H, W, train=False, in_ch=3, batch_invariant=False, forms=None):
    x = torch.rand(B, in_ch, H, W, generator=torch.Generator().manual_seed(1000 * H + W)).cuda()
    want, plan, dout = _run(_net(args, batch_invariant), x, train, None)
    for t in want:
        assert torch.isfinite(t).all()
    if forms is not None:
        forms(plan)
    plan = None
    guarded.guard_modules(monkeypatch, *PLAN_MODULES)
    try:
        got, plan, _ = _run(_net(args, batch_invariant), x, train, dout)
        n = guarded.handed_out()
        print("plan guards %s %dx%d: %d buffers between guard bands" % ("train" if train else "eval", H, W, n))
        assert n > 10
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape
            differ = int((_bits(a) != _bits(b)).sum())
            assert differ == 0, ("tensor %d of the guarded run differs from the unguarded one in %d of %d elements (NaN: %d)"
                                 % (i, differ, a.numel(), int(torch.isnan(a).sum())))
        guarded.assert_intact()
    finally:
        plan = None
        guarded.stop()


# ---- which forms the sizes are meant to select (the switches test_bench_plan_gpu.py honours are honoured here)

def _env(name, default=None):
    return os.environ.get(name, default)


def _switches():
    wino = not any(_env(k) for k in ("XL_NO_WINOGRAD", "XL_WINOGRAD"))
    split = _env("XL_GEMM_SPLIT_BF16", "il") not in ("", "0", "1")
    pairs = split and _env("XL_GEMM_PAIR", "1") not in ("", "0")
    return wino, split, pairs


def _sorted_ops(plan):
    conv = [op for op in plan.ops if op.type == networks.XL_OP_CONV]
    wino = [op for op in conv if op.nchunks2 in (36, 64)]
    s2 = [op for op in conv if op.ksize == 3 and op.stride == 2]
    one = [op for op in conv if op.ksize == 1 and op.stride == 1 and op.nchunks2 <= 1]
    return wino, s2, one


def _describe(ops):
    return [(op.Cin, op.Cout, op.Hi, op.Wi, op.nchunks2, hex(op.flags)) for op in ops]


def _check_forms(plan, stem12=True):
    """Default lowering at these sizes: the fused stem op (RGB inference), every stride-2 layer and every 1x1 layer of 16-channel
    groups as fp16 pairs (training plans keep res1_conv2, 8 channels per group, off the matrix pipe), the stride-1 3x3 layers as
    batched Winograd products of 64 or 36 frequencies with WINO_IN / WINO_OUT around them, the F(6x6) products as pairs."""
    wino_on, split, pairs = _switches()
    wino, s2, one = _sorted_ops(plan)
    types = {op.type for op in plan.ops}
    assert all(op.B == B for op in wino + s2 + one)
    assert all(op.Ho * op.Wo >= 256 for op in one + s2), "the maps are too small for the matrix-pipe forms"
    if split and stem12 and not plan.train:
        assert networks.XL_OP_STEM12 in types
    if not stem12 and not plan.train:
        # (a grayscale inference plan materialises conv1's GroupNorm output: conv2 reads it through the six-pass kernel, the
        #  pair form of a stem layer is the one that normalises on load - lower_forward.conv)
        assert any(op.Cin == 32 and op.flags & networks.CONV_SPLIT_BF16 for op in s2) or not split
        s2 = [op for op in s2 if op.Cin > 32]
    if pairs:
        assert len(s2) >= 2 and all(op.flags & networks.CONV_PAIR_F16 for op in s2), _describe(s2)
        wide = [op for op in one if not plan.train or op.Cout // 32 == 16]
        assert len(wide) >= 6 and all(op.flags & networks.CONV_PAIR_F16 for op in wide), _describe(one)
    if wino_on:
        assert len(wino) >= 6 and networks.XL_OP_WINO_IN in types and networks.XL_OP_WINO_OUT in types
        if pairs:
            assert all(op.flags & networks.CONV_PAIR_F16 for op in wino if op.nchunks2 == 64), _describe(wino)


# ---- the cases

@pytest.mark.parametrize("H,W", SIZES, ids=IDS)
def test_inference_plan_between_guard_bands(monkeypatch, H, W):
    _case(monkeypatch, SINGLE, H, W, forms=_check_forms)


@pytest.mark.parametrize("H,W", SIZES[::2], ids=IDS[::2])
def test_training_plan_between_guard_bands(monkeypatch, H, W):
    """Forward and backward of the default training plan: output and flat gradient buffer."""
    _case(monkeypatch, SINGLE, H, W, train=True, forms=_check_forms)


def test_batch_invariant_plan_between_guard_bands(monkeypatch):
    """batch_invariant = True: row tiles start at image boundaries, statistics in passes of their own."""
    H, W = SIZES[3]
    _case(monkeypatch, SINGLE, H, W, batch_invariant=True, forms=_check_forms)


def test_three_encoder_plan_between_guard_bands(monkeypatch):
    """The MLR network: every encoder writes its 512 channels into a slice of the 1536-wide concatenation."""
    H, W = SIZES[5]

    def forms(plan):
        _check_forms(plan)
        assert any(op.ld_out == 1536 for op in plan.ops), "no op writes a slice of the concatenation"
    _case(monkeypatch, (MEAN, False, False, 1, 1, 3, 1, 32, 3, 0, False), H, W, forms=forms)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_four_encoder_semantics_plan_between_guard_bands(monkeypatch, train):
    """Four encoders (2048-wide concatenation, the first one trainable) and the full-size DUC head with its bilinear trim."""
    H, W = SIZES[6]

    def forms(plan):
        _check_forms(plan)
        assert any(op.ld_out == 2048 for op in plan.ops), "no op writes a slice of the concatenation"
        assert any(op.type == networks.XL_OP_DUC_HEAD for op in plan.ops)
    _case(monkeypatch, (torch.zeros(6), False, False, 1, 1, 6, 0, 32, 4, 1, True), H, W, train=train, forms=forms)


def test_grayscale_plan_between_guard_bands(monkeypatch):
    H, W = SIZES[1]
    _case(monkeypatch, (MEAN, False, True, 1, 1, 3, 1), H, W, in_ch=1, forms=lambda plan: _check_forms(plan, stem12=False))


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_direct_kernels_between_guard_bands(monkeypatch, train):
    """XL_NO_WINOGRAD=1: every 3x3 layer through the direct implicit-GEMM kernel."""
    monkeypatch.setenv("XL_NO_WINOGRAD", "1")
    H, W = SIZES[7]

    def forms(plan):
        _check_forms(plan)
        assert not _sorted_ops(plan)[0] and not any(op.type == networks.XL_OP_WINO_IN for op in plan.ops)
    _case(monkeypatch, SINGLE, H, W, train=train, forms=forms)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_six_pass_kernels_between_guard_bands(monkeypatch, train):
    """XL_GEMM_PAIR=0: the six-pass bf16 kernels, which share the 1x1 launcher with the pair kernels."""
    monkeypatch.setenv("XL_GEMM_PAIR", "0")
    H, W = SIZES[2]

    def forms(plan):
        _check_forms(plan)
        wino, s2, one = _sorted_ops(plan)
        assert not any(op.flags & networks.CONV_PAIR_F16 for op in plan.ops)
        if _switches()[1]:
            assert all(op.flags & networks.CONV_SPLIT_BF16 for op in s2) and sum(1 for op in one if op.flags & networks.CONV_SPLIT_BF16) >= 6
    _case(monkeypatch, SINGLE, H, W, train=train, forms=forms)
