"""GPU: the whole network over every frame-size class of the training augmentation (tests/size_classes.py: all 64
(H mod 8, W mod 8) classes - every combination of round-ups through the three stride-2 layers, all four parity classes at every
level - and every (mod 6, mod 6) / (mod 4, mod 4) class of the cell grid), batch 2 so that row tiles straddle images.

Reference: oracle/cnn_oracle.py evaluated in float64 on the CPU, once per size, shared by the inference and the training sweep.
Bound: that of test_odd_image_sizes_and_grayscale (tests/test_cnn_gpu.py), unchanged - 1e-3 of the largest |coordinate - mean|,
rtol 2e-3 on the uncertainty channel.  Each case also pins the output shape, finiteness and bitwise repeatability (inference: the
eager call, the call that captures the HIP graph and a replay of it).

One network per module: a plan per size and mode, built once; the plans of the size before are dropped (they hold the packed
weights of every layer)."""
import os

import pytest

torch = pytest.importorskip("torch")

from size_classes import MIXED_PARITY, SIZES, ids, o       # noqa: E402
from crossloc_amd import networks                          # noqa: E402
from crossloc_amd.weights import seeded_state_dict         # noqa: E402
from oracle import cnn_oracle                              # noqa: E402

pytestmark = pytest.mark.gpu
MEAN = torch.tensor([-455.934, 417.50, 520.31])
B = 2
_NETS, _REFS = {}, {}


def _net(gray):
    if gray not in _NETS:
        net = networks.TransPoseNet(MEAN, False, gray, 1, 1, 3, 1)
        net.load_state_dict(seeded_state_dict(net, seed=29))
        sd = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in net.state_dict().items()}
        _NETS[gray] = (net.cuda(), sd)
    return _NETS[gray]


def _case(H, W, gray):
    """(image, float64 reference) of a size: computed once, never written to."""
    key = (H, W, gray)
    if key not in _REFS:
        _, sd = _net(gray)
        x = torch.rand(B, 1 if gray else 3, H, W, generator=torch.Generator().manual_seed(1000 * H + W))
        with torch.no_grad():
            ref = cnn_oracle.decoder_forward(sd, cnn_oracle.encoder_forward(sd, x.double(), "encoder", 1, 32), 1, 3, 1, 32)
        _REFS[key] = (x, ref)
    return _REFS[key]


def _sweep_case(H, W, gray, train):
    net, _ = _net(gray)
    x, ref = _case(H, W, gray)
    net.drop_plans_except(B, H, W)
    xd = x.cuda()
    if train:
        net.train()
        ys = [net(xd).detach().clone() for _ in range(2)]
        assert [p.train for p in net._plans.values()].count(True) == 1          # both calls on the one training plan
    else:
        net.eval()
        with torch.no_grad():
            ys = [net(xd).clone() for _ in range(3)]            # eager, graph capture, graph replay
        plan = [p for p in net._plans.values() if not p.train][0]
        if os.environ.get("XL_CNN_GRAPH") != "0" and os.environ.get("XL_GEMM_SPLIT_BF16") not in ("0", "1"):
            assert plan.graph is not None and plan.graph_runs == 3
    torch.cuda.synchronize()
    y = ys[0].cpu()
    assert tuple(y.shape) == (B, 4, o(H), o(W)) == tuple(ref.shape)
    assert torch.isfinite(y).all()
    for other in ys[1:]:
        assert torch.equal(ys[0], other), (ys[0] - other).abs().max()
    m = MEAN.double()[None, :, None, None]
    got, want = y.double()[:, :3] - m, ref[:, :3] - m
    err, scale = (got - want).abs().max().item(), max(want.abs().max().item(), 1e-6)
    rel = ((y.double()[:, 3] - ref[:, 3]).abs() / ref[:, 3].abs()).max().item()
    print("size sweep %s%s %dx%d: coordinates %.2e of max (bound 1e-3), uncertainty %.2e relative (bound 2e-3)"
          % ("train" if train else "eval", " gray" if gray else "", H, W, err / scale, rel))
    assert err <= 1e-3 * scale, "max err %g vs scale %g" % (err, scale)
    assert torch.allclose(y.double()[:, 3], ref[:, 3], rtol=2e-3)


@pytest.mark.parametrize("H,W", SIZES, ids=ids(SIZES))
def test_inference_plan_over_every_size_class(H, W):
    """eval(), no_grad: the default inference plan (Winograd by multiply count, fused stem, conv-epilogue statistics, HIP-graph
    replay from the second call on)."""
    _sweep_case(H, W, False, False)


@pytest.mark.parametrize("H,W", SIZES, ids=ids(SIZES))
def test_training_plan_forward_over_every_size_class(H, W):
    """train(): the forward pass of the default training plan (F(4x4,3x3) / F(6x6,3x3) with an fp32 V, stem layers as separate
    kernels, the activations the backward pass reads kept)."""
    _sweep_case(H, W, False, True)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("H,W", MIXED_PARITY, ids=ids(MIXED_PARITY))
def test_grayscale_over_the_mixed_parity_sizes(H, W, train):
    """One input channel (--grayscale): conv1's single-channel forms at H, W of opposite parity, every H mod 8 and W mod 8."""
    _sweep_case(H, W, True, train)
