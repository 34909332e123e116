"""crossloc_amd.mask_single_task on the GPU: test_single_task.main() run unchanged behind views of `evaluation` and `synth`.
The drivers run in this process (their main() with the command line patched), eight frames each."""
import sys

import pytest

pytestmark = pytest.mark.gpu

COMMON = ["--synthetic", "8", "--batch", "8"]


def _report(main, extra, monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["driver"] + COMMON + extra)
    main()
    out = capsys.readouterr().out
    return out[out.index("Accuracy:"):].strip()


def _median_t(report):
    line = [ln for ln in report.splitlines() if ln.startswith("Median Error")][0]
    return float(line.split(",")[1].strip().split()[0])


def test_report_is_unchanged_without_a_mask(monkeypatch, capsys):
    """with `--mask none` the report is test_single_task's own, character for character"""
    from crossloc_amd import mask_single_task, test_single_task
    plain = _report(test_single_task.main, [], monkeypatch, capsys)
    assert "Median Error" in plain
    assert _report(mask_single_task.main, ["--mask", "none"], monkeypatch, capsys) == plain
    assert test_single_task.evaluation.__name__ == "crossloc_amd.evaluation"          # the views are gone after the call
    # a sigma mask that admits every cell goes through the masked solver and, by identity A, prints the same report
    assert _report(mask_single_task.main, ["--mask", "sigma", "--mask_max_sigma", "1e30"], monkeypatch, capsys) == plain


def test_decoy_frames_are_localised_with_their_mask(monkeypatch, capsys):
    """Without the mask the solver returns the second camera, whose centre is drawn uniformly within +-300 m of the scene mean on
    two axes, like the true one: the distance between the two has a median of some 300 m, and 50 m is far below what a median
    over eight frames can reach.  With the mask the frame is an ordinary one with 0.5 m noise on 40 % of its cells; 5 m is the
    report's own `5m5deg` bucket."""
    from crossloc_amd import mask_single_task
    without = _report(mask_single_task.main, ["--decoy", "0.6"], monkeypatch, capsys)
    masked = _report(mask_single_task.main, ["--decoy", "0.6", "--mask", "truth"], monkeypatch, capsys)
    print("median translation error on decoy frames: unmasked %.2f m, masked %.2f m" % (_median_t(without), _median_t(masked)))
    assert _median_t(without) > 50.0 and _median_t(masked) < 5.0
    with pytest.raises(RuntimeError, match="--decoy"):
        _report(mask_single_task.main, ["--mask", "truth"], monkeypatch, capsys)
