"""GPU: the guard-band check of tests/guarded.py sees a real op of the library.  XL_OP_FILL0 is given a guarded buffer of n floats
and a byte count of 4 * (n + 1): the extra float lies in the back band of the SAME allocation (nothing is written outside an
allocation), and the check must name it."""
import ctypes

import pytest

torch = pytest.importorskip("torch")

import guarded                                          # noqa: E402
from crossloc_amd import networks                       # noqa: E402

pytestmark = pytest.mark.gpu


def _fill0(ptr, nbytes):
    op = networks.XlOp()
    op.type, op.Cin, op.out = networks.XL_OP_FILL0, nbytes, ptr
    arr = (networks.XlOp * 1)(op)
    networks._check(networks._bind().xl_cnn_run(arr, 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


@pytest.mark.parametrize("n", [24, 1000])
def test_an_overrun_of_one_float_is_caught_and_located(n):
    reg = guarded.Registry()
    reg.reset()
    try:
        other = reg.zeros(64, device="cuda")
        buf = reg.empty(n, device="cuda")               # <- named by the report
        assert torch.isnan(buf).all() and (other == 0).all() and buf.data_ptr() % 512 == 0      # (the allocator's own granule)
        _fill0(buf.data_ptr(), 4 * n)                   # exactly the tensor: intact
        reg.assert_intact()
        assert (buf == 0).all()
        _fill0(buf.data_ptr(), 4 * (n + 1))             # one float more, into the tensor's own back band
        with pytest.raises(AssertionError) as e:
            reg.assert_intact()
        msg = str(e.value)
        assert "1 guard band(s)" in msg and "back band" in msg and "offset %d " % (4 * n) in msg and "4 bytes damaged" in msg
        assert "float32 [%d]" % n in msg and "test_guarded_gpu.py" in msg and "in test_an_overrun" in msg
    finally:
        reg.stop()
