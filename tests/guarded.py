"""Guard bands around the tensors that kernels write: an overrun lands in a band of known bytes instead of in whatever the
caching allocator happened to put next to the tensor, and a read of workspace that nobody wrote in this pass reads NaN.

A `Registry` hands out tensors that are interior views of a larger allocation,

    [ front band, 2 MiB | interior, exactly the bytes asked for | back band, 2 MiB ]

Both bands are filled with one byte pattern (0xA5).  2 MiB is one 256-row tile of the widest tensor any plan holds (256 rows
x 2048 channels x 4 B), and a multiple of 4 KiB, so the interior keeps the alignment torch gives an allocation of its own
(the device allocator's 512-byte granule).
`empty` interiors are pre-filled with NaN (floating types) or the band pattern (integer types); `zeros` and `full` keep the
fill they were asked for - plans rely on zeroed statistics and scale slots.  Only tensors on the registry's device types
(default: "cuda") are guarded; host and pinned allocations pass through to torch unchanged.

`assert_intact()` synchronises, compares every band with the pattern on the device and raises one AssertionError that lists
EVERY damaged buffer: creation site, shape, dtype, which band, the first damaged byte as an offset relative to the interior's
first byte (negative in the front band, >= the interior's byte count in the back band) and the number of damaged bytes.

`torch_proxy()` stands in for the name `torch` inside a module (`monkeypatch.setattr(module, "torch", proxy)`, or
`torch = guarded.torch_proxy()` at the top of a test module): `empty`, `zeros`, `full` and their `_like` forms go through the
registry WHILE IT IS ACTIVE (between `reset()` and `stop()`), every other attribute is the real torch's.

Limits.  A guard detects a write that lands inside the guarded allocation: up to 2 MiB before or after the tensor.  A wilder
write is as invisible as before, and out-of-bounds READS are out of scope altogether (a read of a band returns the pattern,
a tiny negative float (-2.9e-16) or an ordinary integer: nothing flags it).  No test writes or reads outside an allocation on
purpose: the self-test of the check (tests/test_guarded_gpu.py) overruns a tensor by one float INTO ITS OWN back band.

`networks._sole_owner`.  The registry keeps the parent allocation of every tensor it hands out, so the storage of a guarded
tensor always has one owner more than the tensor itself: a guarded training plan finds its gradient result buffers "shared"
and hands out a fresh result buffer on every backward pass - the path networks.run_backward documents as correct (the fused
optimizer then rebuilds its pointer tables each step).  Values do not depend on it.
"""
import os
import sys

import torch as _torch

BAND = 2 << 20
PATTERN = 0xA5
_ALLOC = ("empty", "zeros", "full", "empty_like", "zeros_like", "full_like")
_HERE = os.path.abspath(__file__)
TESTS_DIR = os.path.dirname(_HERE)


class _Record:
    __slots__ = ("parent", "nbytes", "site", "shape", "dtype")

    def __init__(self, parent, nbytes, site, shape, dtype):
        self.parent, self.nbytes, self.site, self.shape, self.dtype = parent, nbytes, site, tuple(shape), dtype

    def describe(self):
        return "%s %s allocated at %s" % (str(self.dtype).replace("torch.", ""), list(self.shape), self.site)


def _site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:
        return "?"
    return "%s:%d in %s" % (os.path.relpath(f.f_code.co_filename, os.path.dirname(TESTS_DIR)), f.f_lineno, f.f_code.co_name)


def _size_of(args, kwargs):
    """The shape of torch.empty / zeros (varargs or one sequence, or size=...) and what is left of the positional arguments."""
    if "size" in kwargs:
        return tuple(kwargs.pop("size")), args
    if args and isinstance(args[0], (tuple, list, _torch.Size)):
        return tuple(args[0]), args[1:]
    n = 0
    while n < len(args) and isinstance(args[n], int) and not isinstance(args[n], bool):
        n += 1
    return tuple(args[:n]), args[n:]


class Registry:
    def __init__(self, device_types=("cuda",)):
        self.device_types = tuple(device_types)
        self.records = []
        self.active = False
        self.handed_out = 0                  # since the last reset()

    # ---- life cycle
    def reset(self):
        """Forget every buffer (their memory goes back to torch once the tensors handed out die) and start guarding."""
        self.records = []
        self.handed_out = 0
        self.active = True

    def stop(self):
        """Stop guarding (allocation functions pass through to torch again) and forget every buffer."""
        self.records = []
        self.active = False

    # ---- allocation
    def _guards(self, device):
        return self.active and _torch.device(device if device is not None else "cpu").type in self.device_types

    def _interior(self, shape, dtype, device, strides=None):
        """An uninitialised interior of `shape` between two pattern-filled bands; contiguous unless dense `strides` are given."""
        numel = 1
        for s in shape:
            numel *= int(s)
        nbytes = numel * dtype.itemsize
        parent = _torch.empty(2 * BAND + nbytes, dtype=_torch.uint8, device=device)
        parent[:BAND].fill_(PATTERN)
        parent[BAND + nbytes:].fill_(PATTERN)
        flat = parent[BAND:BAND + nbytes].view(dtype)
        t = flat.view(tuple(shape)) if strides is None else flat.as_strided(tuple(shape), tuple(strides))
        self.records.append(_Record(parent, nbytes, _site(), shape, dtype))
        self.handed_out += 1
        return t

    def _prefill(self, t):
        if t.dtype.is_floating_point or t.dtype.is_complex:
            t.fill_(float("nan"))
        elif t.dtype == _torch.bool:
            t.fill_(True)
        else:                                # the integer whose bytes are the band pattern
            t.fill_(_torch.full((t.element_size(),), PATTERN, dtype=_torch.uint8).view(t.dtype)[0].item())
        return t

    def _finish(self, t, requires_grad):
        return t.requires_grad_(True) if requires_grad else t

    def _plain(self, kwargs):
        """True when the remaining keyword arguments ask for nothing a guarded view cannot give (pinned memory, out=, ...)."""
        return all(v is None or v is False or (k == "layout" and v == _torch.strided) or
                   (k == "memory_format" and v in (_torch.contiguous_format, _torch.preserve_format))
                   for k, v in kwargs.items())

    def _new(self, name, args, kwargs):
        kw = dict(kwargs)
        device, dtype, rg = kw.pop("device", None), kw.pop("dtype", None), kw.pop("requires_grad", False)
        if not self._guards(device):
            return getattr(_torch, name)(*args, **kwargs)
        shape, rest = _size_of(args, kw)
        fill = None
        if name == "full":
            fill = kw.pop("fill_value") if "fill_value" in kw else rest[0]
            rest = rest[1:] if "fill_value" not in kwargs else rest
            if dtype is None:
                dtype = (_torch.bool if isinstance(fill, bool) else _torch.int64 if isinstance(fill, int)
                         else _torch.get_default_dtype())
        if rest or not self._plain(kw):
            return getattr(_torch, name)(*args, **kwargs)
        if dtype is None:
            dtype = _torch.get_default_dtype()
        t = self._interior(shape, dtype, device)
        if name == "empty":
            self._prefill(t)
        elif name == "zeros":
            t.zero_()
        else:
            t.fill_(fill)
        return self._finish(t, rg)

    def _like(self, name, args, kwargs):
        kw = dict(kwargs)
        src = kw.pop("input") if "input" in kw else args[0]
        rest = args[1:] if "input" not in kwargs else args
        device, dtype, rg = kw.pop("device", None), kw.pop("dtype", None), kw.pop("requires_grad", False)
        device = src.device if device is None else device
        if not self._guards(device) or src.layout != _torch.strided:
            return getattr(_torch, name)(*args, **kwargs)
        fill = None
        if name == "full_like":
            fill = kw.pop("fill_value") if "fill_value" in kw else rest[0]
            rest = rest[1:] if "fill_value" not in kwargs else rest
        if rest or not self._plain(kw):
            return getattr(_torch, name)(*args, **kwargs)
        dtype = src.dtype if dtype is None else dtype
        # the strides torch itself would give (a dense permutation of the source keeps its order): asked of a meta tensor
        fmt = {"memory_format": kw["memory_format"]} if kw.get("memory_format") is not None else {}
        strides = _torch.empty_like(src, dtype=dtype, device="meta", **fmt).stride()
        t = self._interior(tuple(src.shape), dtype, device, strides)
        if name == "empty_like":
            self._prefill(t)
        elif name == "zeros_like":
            t.zero_()
        else:
            t.fill_(fill)
        return self._finish(t, rg)

    def empty(self, *a, **k):
        return self._new("empty", a, k)

    def zeros(self, *a, **k):
        return self._new("zeros", a, k)

    def full(self, *a, **k):
        return self._new("full", a, k)

    def empty_like(self, *a, **k):
        return self._like("empty_like", a, k)

    def zeros_like(self, *a, **k):
        return self._like("zeros_like", a, k)

    def full_like(self, *a, **k):
        return self._like("full_like", a, k)

    # ---- the check
    def damage(self):
        """[(record, "front" | "back", first damaged byte offset relative to the interior, damaged byte count)], all buffers."""
        if any(r.parent.is_cuda for r in self.records):
            _torch.cuda.synchronize()
        counts = []
        for r in self.records:
            p = r.parent
            counts.append((p[:BAND] != PATTERN).sum())
            counts.append((p[BAND + r.nbytes:] != PATTERN).sum())
        if not counts:
            return []
        by_device = {}
        for i, c in enumerate(counts):
            by_device.setdefault(c.device, []).append((i, c))
        host = [0] * len(counts)
        for lst in by_device.values():                      # one transfer per device, not one per band
            vals = _torch.stack([c for _, c in lst]).cpu().tolist()
            for (i, _), v in zip(lst, vals):
                host[i] = v
        found = []
        for n, r in enumerate(self.records):
            for side, cnt in (("front", host[2 * n]), ("back", host[2 * n + 1])):
                if cnt:
                    band = r.parent[:BAND] if side == "front" else r.parent[BAND + r.nbytes:]
                    first = int((band != PATTERN).nonzero()[0, 0])
                    found.append((r, side, first - BAND if side == "front" else r.nbytes + first, int(cnt)))
        return found

    def assert_intact(self):
        found = self.damage()
        if found:
            lines = ["%s: %s band damaged, first byte at offset %d relative to the interior (%d bytes long), %d bytes damaged"
                     % (r.describe(), side, off, r.nbytes, cnt) for r, side, off, cnt in found]
            raise AssertionError("%d guard band(s) written to:\n  " % len(found) + "\n  ".join(lines))


class _TorchProxy:
    """Stands in for the module `torch`: the six allocation functions go through `registry`, the rest is torch's own."""

    def __init__(self, registry):
        self.__dict__["_registry"] = registry
        for name in _ALLOC:
            self.__dict__[name] = getattr(registry, name)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        setattr(_torch, name, value)

    def __repr__(self):
        return "<guarded proxy of %r>" % (_torch,)


REGISTRY = Registry()                        # the one the GPU tests share


def torch_proxy(registry=None):
    return _TorchProxy(REGISTRY if registry is None else registry)


def reset():
    REGISTRY.reset()


def stop():
    REGISTRY.stop()


def assert_intact():
    REGISTRY.assert_intact()


def handed_out():
    return REGISTRY.handed_out


COUNTS = {}                                  # test module -> buffers handed out to its tests so far (op_module_check)


def op_module_check(monkeypatch, bind_owner, name):
    """Body of the autouse fixture of an op-level test module `name`
    (`yield from guarded.op_module_check(monkeypatch, networks, __name__)`): start guarding - the module's own `torch` is a
    proxy, packing.py's becomes one for the test - run the test, require every band intact and, in a test whose own code (a
    file of tests/) launched an op list through `bind_owner._bind()`, that the registry handed out at least one buffer, so that
    adoption cannot lapse."""
    real_bind = bind_owner._bind
    launches = [0]

    def counting_bind():
        if os.path.dirname(os.path.abspath(sys._getframe(1).f_code.co_filename)) == TESTS_DIR:
            launches[0] += 1
        return real_bind()
    monkeypatch.setattr(bind_owner, "_bind", counting_bind)
    # the destinations of the weight packs that tests reach through _Plan's static methods are allocated in packing.py
    monkeypatch.setattr(sys.modules[bind_owner.__package__ + ".packing"], "torch", torch_proxy())
    reset()
    try:
        yield REGISTRY
        n = handed_out()
        COUNTS[name] = COUNTS.get(name, 0) + n
        assert_intact()
        assert not launches[0] or n > 0, "this test launched ops from its own code but allocated nothing through tests/guarded.py"
    finally:
        stop()


def guard_modules(monkeypatch, *modules):
    """Proxy the name `torch` in the given modules (until monkeypatch undoes it) and start guarding."""
    proxy = torch_proxy()
    for m in modules:
        monkeypatch.setattr(m, "torch", proxy)
    reset()
    return proxy
