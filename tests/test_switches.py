"""crossloc_amd/switches.py keeps the three truth conventions the scattered `os.environ` reads had."""
import pytest

from crossloc_amd import switches

VALUES = (None, "", "0", "1", "il")          # None: unset


def _env(name, value):
    return {} if value is None else {name: value}


@pytest.mark.parametrize("value", VALUES)
def test_flag_kind(value):
    # the old reads: `os.environ.get("XL_NO_WINOGRAD")` used as a truth value - ANY non-empty string, "0" included, is ON
    env = _env("XL_NO_WINOGRAD", value)
    old = bool(env.get("XL_NO_WINOGRAD"))
    assert switches.read("XL_NO_WINOGRAD", env) is old
    assert switches.Snapshot(env).NO_WINOGRAD is old
    assert old == {None: False, "": False, "0": True, "1": True, "il": True}[value]


@pytest.mark.parametrize("value", VALUES)
def test_default_on_kind(value):
    # the old reads: `os.environ.get("XL_GEMM_PAIR", "1") not in ("", "0")`
    env = _env("XL_GEMM_PAIR", value)
    old = env.get("XL_GEMM_PAIR", "1") not in ("", "0")
    assert switches.read("XL_GEMM_PAIR", env) is old
    assert switches.Snapshot(env).GEMM_PAIR is old
    assert old == {None: True, "": False, "0": False, "1": True, "il": True}[value]
    # ... and `os.environ.get("XL_TRAIN_PAIR", "1") in ("", "0")` for "off"
    env = _env("XL_TRAIN_PAIR", value)
    assert (not switches.Snapshot(env).TRAIN_PAIR) is (env.get("XL_TRAIN_PAIR", "1") in ("", "0"))


@pytest.mark.parametrize("value", VALUES)
def test_value_kind(value):
    # the old reads: `os.environ.get("XL_GEMM_SPLIT_BF16", "il")` as a string, and `... not in ("", "0", "1")` for split_on
    env = _env("XL_GEMM_SPLIT_BF16", value)
    assert switches.Snapshot(env).GEMM_SPLIT_BF16 == env.get("XL_GEMM_SPLIT_BF16", "il")
    old = env.get("XL_GEMM_SPLIT_BF16", "il") not in ("", "0", "1")
    assert switches.Snapshot(env).split_on is old
    assert old == {None: True, "": False, "0": False, "1": False, "il": True}[value]
    # a value switch without a default: `os.environ.get("XL_WINO_OUT_TPB")`, `os.environ.get("XL_WINOGRAD", "6")`
    env = _env("XL_WINO_OUT_TPB", value)
    assert switches.Snapshot(env).WINO_OUT_TPB == env.get("XL_WINO_OUT_TPB")
    assert switches.Snapshot({}).WINOGRAD == "6"


@pytest.mark.parametrize("a", VALUES)
@pytest.mark.parametrize("b", VALUES)
@pytest.mark.parametrize("c", VALUES)
def test_wino_train_on(a, b, c):
    env = {}
    for name, v in (("XL_NO_WINOGRAD", a), ("XL_NO_WINOGRAD_TRAIN", b), ("XL_NO_WINOGRAD_WGRAD", c)):
        env.update(_env(name, v))
    old = (not env.get("XL_NO_WINOGRAD") and not env.get("XL_NO_WINOGRAD_TRAIN") and not env.get("XL_NO_WINOGRAD_WGRAD"))
    assert switches.Snapshot(env).wino_train_on is old


def test_table_is_consistent(monkeypatch):
    names = [row[0] for row in switches.LOWERING + switches.LIVE]
    assert len(names) == len(set(names))
    assert all(kind in (switches.FLAG, switches.DEFAULT_ON, switches.VALUE) and meaning for _, kind, _, meaning in
               switches.LOWERING + switches.LIVE)
    assert not {"XL_CNN_GRAPH", "XL_NO_BATCHED_REPACK"} & {row[0] for row in switches.LOWERING}      # tests flip these on a live plan
    monkeypatch.setenv("XL_NO_BATCHED_REPACK", "0")
    assert switches.live("XL_NO_BATCHED_REPACK") is True
    monkeypatch.setenv("XL_NO_WINOGRAD", "1")
    sw = switches.Snapshot()
    monkeypatch.delenv("XL_NO_WINOGRAD")
    assert sw.NO_WINOGRAD and not switches.Snapshot().NO_WINOGRAD       # a snapshot does not follow the environment
