"""CPU: the guard-band allocator of tests/guarded.py on host tensors - what it hands out, what it reports, what it lets through."""
import pytest

torch = pytest.importorskip("torch")

import guarded                                          # noqa: E402


@pytest.fixture
def reg():
    r = guarded.Registry(device_types=("cpu",))
    r.reset()
    yield r
    r.stop()


def _before(t, n=1):
    """The `n` elements in front of a guarded tensor's interior (inside its own allocation: the front band)."""
    return torch.empty(0, dtype=t.dtype).set_(t.untyped_storage(), t.storage_offset() - n, (n,))


def _after(t, n=1):
    return torch.empty(0, dtype=t.dtype).set_(t.untyped_storage(), t.storage_offset() + t.numel(), (n,))


def test_an_untouched_registry_passes_and_fills_are_what_was_asked_for(reg):
    e = reg.empty(3, 5)
    z = reg.zeros((7,), dtype=torch.float64)
    f = reg.full((2, 3), 1.5)
    i = reg.empty(4, dtype=torch.int16)
    zi = reg.zeros(4, dtype=torch.int32)
    el, zl, fl = reg.empty_like(f), reg.zeros_like(f), reg.full_like(f, 2.0, dtype=torch.float64)
    assert e.shape == (3, 5) and e.dtype == torch.float32 and torch.isnan(e).all()
    assert z.dtype == torch.float64 and (z == 0).all()
    assert f.dtype == torch.float32 and (f == 1.5).all()
    assert (i.view(torch.uint8) == guarded.PATTERN).all() and (zi == 0).all()
    assert torch.isnan(el).all() and el.shape == f.shape and (zl == 0).all()
    assert fl.dtype == torch.float64 and (fl == 2.0).all()
    assert all(t.is_contiguous() and t.data_ptr() % 64 == 0 for t in (e, z, f, i, zi, el, zl, fl))
    assert reg.handed_out == 8
    e.fill_(1.0); z.fill_(2.0); i.fill_(3)              # every interior element may be written
    reg.assert_intact()


def test_like_keeps_the_strides_torch_would_give(reg):
    src = torch.zeros(2, 3, 4, 5).permute(0, 2, 3, 1)
    got, want = reg.empty_like(src), torch.empty_like(src)
    assert got.shape == want.shape and got.stride() == want.stride()
    got.fill_(0.0)
    reg.assert_intact()


def test_a_write_one_element_before_the_interior_is_named(reg):
    reg.zeros(16)
    t = reg.empty(10, 3)                                # <- the site the report must name
    line = _line_of("t = reg.empty(10, 3)")
    _before(t).fill_(0.0)
    with pytest.raises(AssertionError) as e:
        reg.assert_intact()
    msg = str(e.value)
    assert "1 guard band(s)" in msg and "front band" in msg and "offset -4 " in msg and "4 bytes damaged" in msg
    assert "float32 [10, 3]" in msg and "test_guarded_cpu.py:%d" % line in msg


def test_a_write_one_element_after_the_interior_is_named_and_every_damaged_buffer_is_listed(reg):
    a = reg.empty(10, 3, dtype=torch.float64)
    b = reg.zeros(5, dtype=torch.int16)
    reg.full((4,), 7.0)
    _after(a).fill_(1.0)
    _after(b, 3)[2] = 1
    with pytest.raises(AssertionError) as e:
        reg.assert_intact()
    msg = str(e.value)
    assert "2 guard band(s)" in msg
    assert "float64 [10, 3]" in msg and "back band damaged, first byte at offset 240 " in msg and "8 bytes damaged" in msg
    # int16 value 1 = bytes 01 00: both differ from the pattern; the third element after 5 int16 starts at byte 14
    assert "int16 [5]" in msg and "offset 14 " in msg and "2 bytes damaged" in msg


def test_host_tensors_pass_through_a_device_registry_and_an_inactive_one_guards_nothing():
    r = guarded.Registry()                              # guards "cuda" only
    r.reset()
    t = r.zeros(8)
    assert r.handed_out == 0 and t.untyped_storage().nbytes() == 32
    r.stop()
    c = guarded.Registry(device_types=("cpu",))         # never started
    assert c.empty(8).untyped_storage().nbytes() == 32 and c.handed_out == 0


def test_the_proxy_forwards_everything_but_the_allocation_functions(reg):
    p = guarded.torch_proxy(reg)
    assert p.float32 is torch.float32 and p.Tensor is torch.Tensor and p.nn is torch.nn and p.cuda is torch.cuda
    assert p.arange(3).tolist() == [0, 1, 2] and isinstance(p.ones(2), p.Tensor)
    t = p.zeros(6, dtype=p.float32, device="cpu")
    u = p.full_like(t, float("nan"))
    assert reg.handed_out == 2 and t.untyped_storage().nbytes() == 2 * guarded.BAND + 24 and torch.isnan(u).all()
    assert p.empty(3, pin_memory=False).shape == (3,) and reg.handed_out == 3
    reg.assert_intact()


def _line_of(text):
    with open(__file__) as f:
        return [n for n, l in enumerate(f, 1) if l.strip().startswith(text)][0]
