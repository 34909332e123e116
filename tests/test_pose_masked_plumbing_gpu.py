"""The masked quality / refinement passes through evaluation.localize_batch, PipelinedLocalizer.submit and
crossloc_amd.mask_single_task: the new modes equal the direct calls chained by hand, the tuples have the documented order, the
modes refuse what they must, and mask_max_sigma hands the passes the mask cell_mask would build."""
import sys

import numpy as np
import pytest
import torch

import pose_masked_cases as mc
from crossloc_amd import synth

pytestmark = pytest.mark.gpu

SUB = mc.SUB


class _PlantNet(torch.nn.Module):
    """A network whose output is zeros with `sigma` in the uncertainty channel; the solver reads scene_coords"""
    num_task_channel = 3
    OUTPUT_SUBSAMPLE = SUB

    def __init__(self, sigma=None):
        super().__init__()
        self.sigma = sigma

    def forward(self, images, plan_slot=0):
        B, _, H, W = images.shape
        out = torch.zeros((B, 3 if self.sigma is None else 4, H // SUB, W // SUB), device=images.device)
        if self.sigma is not None:
            out[:, 3] = self.sigma
        return out


def _by_hand(co, m, sg, n_hyp, Ho, Wo, refine, quality, image0=3):
    """forward_rgb_masked_batch, refine_pose_masked_batch, pose_quality_masked_batch chained by hand"""
    import dsacstar
    intr = (mc.THR, synth.FOCAL, Wo * SUB / 2.0, Ho * SUB / 2.0)
    poses = torch.zeros((co.shape[0], 4, 4), device="cuda")
    status = dsacstar.forward_rgb_masked_batch(co, m, poses, n_hyp, *intr, mc.ALPHA, mc.MAX_REPROJ, SUB, image0=image0)
    out = dict(status=status)
    if refine:
        poses, out["refine"] = dsacstar.refine_pose_masked_batch(co, m, sg, poses, *intr, mc.MAX_REPROJ, SUB)
    if quality:
        out["quality"] = dsacstar.pose_quality_masked_batch(co, m, poses, *intr, mc.ALPHA, mc.MAX_REPROJ, SUB)
    out["poses"] = poses
    return out


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) \
        and torch.equal(torch.isnan(a), torch.isnan(b))


def test_localize_batch_and_pipelined_localizer():
    from crossloc_amd import evaluation
    Ho, Wo, n_hyp = 24, 36, 16
    H, W = Ho * SUB, Wo * SUB
    bt = mc.batch(40, Ho, Wo)
    co, m, sigma = torch.from_numpy(bt["coords"]).cuda(), torch.from_numpy(bt["mask"]).cuda(), torch.from_numpy(bt["sigma"]).cuda()
    images = torch.zeros((3, 3, H, W), device="cuda")
    net, net_sigma = _PlantNet(), _PlantNet(sigma)
    loc, loc_sigma = evaluation.PipelinedLocalizer(net, n_hyp, synth.FOCAL, H, W), evaluation.PipelinedLocalizer(net_sigma, n_hyp, synth.FOCAL, H, W)
    common = dict(image0=3, scene_coords=co)

    cases = [(dict(quality="masked"), False, True, None, ("quality",)),
             (dict(refine="masked_sigma"), True, False, sigma, ("refine",)),
             (dict(refine="masked_sigma", quality="masked"), True, True, sigma, ("quality", "refine")),
             (dict(refine="masked_inliers", quality="masked"), True, True, None, ("quality", "refine"))]
    for kw, refine, quality, sg, names in cases:
        want = _by_hand(co, m, sg, n_hyp, Ho, Wo, refine, quality)
        outs = [evaluation.localize_batch(net_sigma, images, n_hyp, synth.FOCAL, H, W, mask=m, **common, **kw),
                loc_sigma.submit(images, mask=m, **common, **kw)]
        if sg is not None:                                  # sigma as a side input to a network without the channel
            outs.append(evaluation.localize_batch(net, images, n_hyp, synth.FOCAL, H, W, mask=m, sigma=sigma, **common, **kw))
            outs.append(loc.submit(images, mask=m, sigma=sigma, **common, **kw))
        loc.finish()
        loc_sigma.finish()
        torch.cuda.synchronize()
        for got in outs:
            assert len(got) == 3 + len(names), kw                                           # (poses, pred, [rows..], status)
            assert _eq(got[0], want["poses"]) and _eq(got[-1], want["status"]), kw
            for i, name in enumerate(names):
                assert tuple(got[2 + i].shape) == (3, 64) and _eq(got[2 + i], want[name]), (kw, name)
        if refine:
            assert not torch.equal(want["poses"], _by_hand(co, m, None, n_hyp, Ho, Wo, False, False)["poses"])   # refined poses first

    # mask_max_sigma: the solver and both passes read the mask cell_mask(sigma=..., max_sigma=...) gives
    built = evaluation.cell_mask(sigma=sigma, max_sigma=1.0)
    assert 0 < int(built.sum()) < built.numel()
    want = _by_hand(co, built, sigma, n_hyp, Ho, Wo, True, True)
    outs = [evaluation.localize_batch(net_sigma, images, n_hyp, synth.FOCAL, H, W, mask_max_sigma=1.0, refine="masked_sigma",
                                      quality="masked", **common),
            loc_sigma.submit(images, mask_max_sigma=1.0, refine="masked_sigma", quality="masked", **common)]
    loc_sigma.finish()
    torch.cuda.synchronize()
    for got in outs:
        assert len(got) == 5 and _eq(got[0], want["poses"]) and _eq(got[2], want["quality"]) and _eq(got[3], want["refine"])
        assert got[2][:, 58].tolist() == (built == 0).sum((1, 2)).tolist() and _eq(got[4], want["status"])

    # refusals: the new modes without a mask, with depth / cam_coords; a mask with the modes that read every cell
    depth = torch.ones((3, Ho, Wo), device="cuda")
    refused = [dict(quality="masked"), dict(refine="masked_sigma"), dict(refine="masked_inliers"),
               dict(quality="masked", depth=depth), dict(refine="masked_inliers", depth=depth),
               dict(mask=m, quality="masked", depth=depth), dict(mask=m, refine="masked_sigma", depth=depth),
               dict(mask=m, quality="masked", cam_coords=torch.ones((3, 3, Ho, Wo), device="cuda")),
               dict(mask=m, quality=True), dict(mask=m, quality="rgbd"), dict(mask=m, refine="sigma"),
               dict(mask=m, refine="masked_sigma", quality=True), dict(mask=m, quality="masked", refine="inliers")]
    for kw in refused:
        with pytest.raises(RuntimeError):
            evaluation.localize_batch(net_sigma, images, n_hyp, synth.FOCAL, H, W, scene_coords=co, **kw)
        with pytest.raises(RuntimeError):
            loc_sigma.submit(images, scene_coords=co, **kw)
    with pytest.raises(RuntimeError, match="masked"):                  # the old refusal now names the masked modes
        evaluation.localize_batch(net_sigma, images, n_hyp, synth.FOCAL, H, W, scene_coords=co, mask=m, quality=True)
    with pytest.raises(RuntimeError, match="masked_sigma"):
        evaluation.localize_batch(net_sigma, images, n_hyp, synth.FOCAL, H, W, scene_coords=co, mask=m, refine="sigma")
    with pytest.raises(RuntimeError, match="uncertainty channel"):
        evaluation.localize_batch(net, images, n_hyp, synth.FOCAL, H, W, scene_coords=co, mask=m, refine="masked_sigma")
    loc_sigma.finish()
    torch.cuda.synchronize()


def _report(main, extra, monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["driver", "--synthetic", "8", "--batch", "8"] + extra)
    main()
    out = capsys.readouterr().out
    return out[out.index("Accuracy:"):].strip()


def test_mask_single_task_refine(monkeypatch, capsys):
    """`--refine none` prints the report `--mask truth` printed before the option existed (the call it makes is the same);
    `--refine sigma` runs the masked refinement to its report, and with `--mask none` the unmasked one."""
    import dsacstar
    from crossloc_amd import mask_single_task
    decoy = ["--decoy", "0.6", "--mask", "truth"]
    calls = []
    real = dsacstar.refine_pose_masked_batch
    monkeypatch.setattr(dsacstar, "refine_pose_masked_batch", lambda *a, **k: calls.append(1) or real(*a, **k))
    parent = _report(mask_single_task.main, decoy, monkeypatch, capsys)
    assert _report(mask_single_task.main, decoy + ["--refine", "none"], monkeypatch, capsys) == parent and not calls
    refined = _report(mask_single_task.main, decoy + ["--refine", "sigma"], monkeypatch, capsys)
    assert "Median Error" in refined and len(calls) == 1
    unmasked = _report(mask_single_task.main, ["--decoy", "0.6", "--mask", "none", "--refine", "inliers"], monkeypatch, capsys)
    assert "Median Error" in unmasked and len(calls) == 1
    from crossloc_amd import test_single_task
    assert test_single_task.evaluation.__name__ == "crossloc_amd.evaluation"
