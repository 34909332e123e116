"""GPU: the 1x1 pair GEMMs (csrc/xl_gemm_pair.hip) give the BITS they gave before their epilogue was made scratch-free.

tests/golden/pair1x1_bitwise.npz was recorded by tools/pair1x1_golden.py from the commit before that change: per case the sha256 of
the output tensor, the fp64 GroupNorm partial sums in full and a 64-bit sum of the output's bit patterns per 32 rows.  The cases are
the NORM, plain, residual and accumulate forms at 512 -> 512 and 256 -> 512 on the smallest shapes at which the epilogue can go
wrong: a tile that ends inside an image's last rows (5400 pixels, M no multiple of 256), a tile that straddles two images (both
statistics slots live), tiles per image, a second tile per workgroup (338 tiles: the stores of one tile in flight under the next
K-loop), and the Z-batched instantiations.  Recording and test run the same seeded inputs (the tool's run_case)."""
import importlib.util
import os

import pytest

torch = pytest.importorskip("torch")
np = pytest.importorskip("numpy")

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PAIRS_OFF = os.environ.get("XL_GEMM_PAIR") in ("", "0") or os.environ.get("XL_GEMM_SPLIT_BF16") in ("0", "1")


def _tool():
    spec = importlib.util.spec_from_file_location("pair1x1_golden", os.path.join(ROOT, "tools", "pair1x1_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()


@pytest.fixture(scope="module")
def golden():
    return np.load(TOOL.GOLDEN)


def test_the_record_holds_every_case(golden):
    want = {"%s/%s" % (c[0], k) for c in TOOL.CASES for k in (("sha256", "blocks") if c[1] in ("acc", "z") else ("sha256", "blocks", "stats"))}
    assert set(golden.files) == want


@pytest.mark.skipif(_PAIRS_OFF, reason="the fp16-pair forms are switched off (measurement switch set)")
@pytest.mark.parametrize("case", TOOL.CASES, ids=[c[0] for c in TOOL.CASES])
def test_pair_conv1x1_bits_are_those_of_the_record(case, golden):
    out, st = TOOL.run_case(case)
    got = TOOL.digest(out, st)
    name = case[0]
    if st is not None:
        want = golden[name + "/stats"]
        diff = np.nonzero(want != got["stats"])[0]
        assert diff.size == 0, "%s: %d of %d statistics entries differ, first at %d (%r, recorded %r)" % (
            name, diff.size, want.size, diff[0], got["stats"][diff[0]:diff[0] + 1].view(np.float64)[0], want[diff[0]:diff[0] + 1].view(np.float64)[0])
        assert np.count_nonzero(want) > 0, "the recorded statistics are all zero"
    blocks = np.nonzero(golden[name + "/blocks"] != got["blocks"])[0]
    assert blocks.size == 0, "%s: the output differs in %d blocks of 32 rows, first rows %d..%d" % (name, blocks.size, 32 * blocks[0], 32 * blocks[0] + 31)
    assert bytes(got["sha256"]) == bytes(golden[name + "/sha256"]), "%s: the output's bytes differ from the record" % name
