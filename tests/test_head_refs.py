"""CPU: the float64 reference helpers of the per-op head / conv1 weight-gradient GPU tests (tests/head_refs.py) against
the restatement of the reference graph that the golden outputs pin (oracle/cnn_oracle.py): the helpers must reproduce the
tail of cnn_oracle.decoder_forward on the same tensors, so the references of the GPU tests are themselves checked on a
machine without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import head_refs
from crossloc_amd import networks
from crossloc_amd.weights import seeded_state_dict
from oracle import cnn_oracle


def _sd64(net, seed):
    return {k: (v.double() if v.dtype.is_floating_point else v) for k, v in seeded_state_dict(net, seed=seed).items()}


def _decoder_trunk(sd, res):
    """cnn_oracle.decoder_forward up to the input of the head (dec_add = 0)."""
    p = "decoder."
    x = cnn_oracle._cgr(sd, res, p + "res3_conv1", p + "res3_norm1")
    x = cnn_oracle._cgr(sd, x, p + "res3_conv2", p + "res3_norm2")
    x = cnn_oracle._cgr(sd, x, p + "res3_conv3", p + "res3_norm3")
    res = F.relu(res + x)
    sc = cnn_oracle._cgr(sd, res, p + "fc1", p + "fc1_norm")
    return cnn_oracle._cgr(sd, sc, p + "fc2", p + "fc2_norm")


@pytest.mark.parametrize("n_task,n_pos,mean", [(3, 1, [-455.934, 417.50, 520.31]), (1, 1, [241.47]), (2, 1, [0.0, 0.0]),
                                               (3, 0, [-455.934, 417.50, 520.31])])
def test_head_reference_is_the_tail_of_the_decoder_oracle(n_task, n_pos, mean):
    net = networks.TransPoseNet(torch.tensor(mean), False, False, 0, 0, n_task, n_pos)
    sd = _sd64(net, 5)
    res = torch.randn(2, 512, 5, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(n_task + n_pos))
    if n_pos:                                                              # the positive channel reaches both clamp bounds
        w, b = sd["decoder.fc3.weight"].float(), sd["decoder.fc3.bias"].float()
        z = F.conv2d(_decoder_trunk(sd, res), w.double(), b.double())[:, n_task]
        head_refs.map_positive_row(w, b, z, n_task)
        sd["decoder.fc3.weight"], sd["decoder.fc3.bias"] = w.double(), b.double()
    want = cnn_oracle.decoder_forward(sd, res, 0, n_task, n_pos)
    got, sc = head_refs.head_reference(_decoder_trunk(sd, res), sd["decoder.fc3.weight"], sd["decoder.fc3.bias"],
                                       sd["decoder.mean"], n_task, n_pos)
    assert got.dtype == torch.float64 and torch.equal(got, want)
    if n_pos:
        lo, hi, inside = head_refs.clamp_census(sc[:, n_task:])
        assert lo >= 0.05 and hi >= 0.05 and inside >= 0.5 and lo + hi + inside == pytest.approx(1.0)


@pytest.mark.parametrize("hw", [(64, 96), (57, 91), (64, 91)])
def test_duc_head_reference_is_the_tail_of_the_decoder_oracle(hw):
    net = networks.TransPoseNet(torch.zeros(6), False, False, 0, 0, 6, 0, 32, 0, 0, True)
    sd = _sd64(net, 6)
    res = torch.randn(1, 512, 8, 12, dtype=torch.float64, generator=torch.Generator().manual_seed(hw[0]))
    want = cnn_oracle.decoder_forward(sd, res, 0, 6, 0, up_hw=hw)
    duc = cnn_oracle._cgr(sd, _decoder_trunk(sd, res), "decoder.duc_upsample.conv", "decoder.duc_upsample.norm")
    got, _ = head_refs.duc_head_reference(duc, sd["decoder.fc3.weight"], sd["decoder.fc3.bias"], sd["decoder.mean"], 6, 0, hw)
    assert tuple(got.shape) == (1, 6) + hw and torch.equal(got, want)


@pytest.mark.parametrize("cin", [1, 3])
def test_conv1_references_are_autograd_of_the_oracle_layer(cin):
    g = torch.Generator().manual_seed(cin)
    img = torch.rand(2, cin, 9, 11, dtype=torch.float64, generator=g)
    sd = {"c.weight": torch.randn(32, cin, 3, 3, dtype=torch.float64, generator=g).requires_grad_(True),
          "c.bias": torch.randn(32, dtype=torch.float64, generator=g).requires_grad_(True),
          "n.weight": torch.randn(32, dtype=torch.float64, generator=g), "n.bias": torch.randn(32, dtype=torch.float64, generator=g)}
    want = cnn_oracle._cgr(sd, img, "c", "n")
    got, raw = head_refs.conv1_gn_relu(img, sd["c.weight"], sd["c.bias"], sd["n.weight"], sd["n.bias"])
    assert torch.equal(got, want)
    dy = torch.randn(raw.shape, dtype=torch.float64, generator=g)
    gw, gb = torch.autograd.grad(raw, [sd["c.weight"], sd["c.bias"]], dy)
    dw, db = head_refs.conv1_wgrad_reference(img, dy)
    assert torch.allclose(dw, gw, rtol=1e-12, atol=1e-12) and torch.allclose(db, gb, rtol=1e-12, atol=1e-12)
