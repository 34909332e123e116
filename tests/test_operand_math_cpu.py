"""CPU pin of crossloc_amd/csrc/xl_operand_math.h, the operand arithmetic of the split (bf16) and pair (fp16) GEMM pipes.

tests/operand_math_ref.cpp applies the header's functions to arrays; it is built here for the CPU with ROCm's clang++ (nothing
from HIP) into a temporary directory and loaded with ctypes.  Every assertion is bitwise, against restatements written here:
bf16 rounding as integer operations on the float's bits (another expression than the header's), fp16 through np.float16.
NaN and infinity are outside the header's contract.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from crossloc_amd.packing import _Packing

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "crossloc_amd", "csrc")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    hipcc = shutil.which("hipcc")
    cands = ["/opt/rocm/llvm/bin/clang++"] + ([os.path.join(os.path.dirname(hipcc), "clang++")] if hipcc else [])
    cxx = next((c for c in cands if os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no clang++ of a ROCm installation (the header needs ext_vector_type, __bf16 and _Float16)")
    out = os.path.join(str(tmp_path_factory.mktemp("operand_math_ref")), "liboperand_math_ref.so")
    subprocess.check_call([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-function",
                           "-I" + CSRC, "-shared", "-o", out, os.path.join(HERE, "operand_math_ref.cpp")])
    return ctypes.CDLL(out)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def values():
    """A few thousand finite floats: normals at every magnitude the plan allows (its activation bound is 2^14), exact ties
    of both roundings and their neighbours, values whose fp16 residual is subnormal, +-0.  |x| < 65504: hi is finite in fp16."""
    rng = np.random.default_rng(20240611)
    parts = [(rng.standard_normal(96) * 2.0 ** e).astype(np.float32) for e in range(-20, 15)]
    sign = rng.integers(0, 2, 256).astype(np.uint32) << 31
    # bf16 ties: dropped 16 bits exactly 0x8000 behind an even or odd kept part; fp16 ties: a normal fp16 value plus half of its
    # last place (dropped 13 bits 0x1000)
    for lo_expo, keep, drop in ((127 - 20, 7, 16), (127 - 14, 10, 13)):
        top = sign | (rng.integers(lo_expo, 127 + 15, 256).astype(np.uint32) << 23) | (rng.integers(0, 1 << keep, 256).astype(np.uint32) << drop)
        tie = 1 << (drop - 1)
        parts += [_f32(top | tie), _f32(top[:64] | (tie - 1)), _f32(top[:64] | (tie + 1))]
    # residuals x - hi below 2^-14 (fp16 subnormals); around 2^-17 they stay there after the 2^11 of the scaled form
    parts += [(rng.standard_normal(256) * 2.0 ** e).astype(np.float32) for e in (-8, -17)]
    parts.append(np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 65503.0], np.float32))
    x = np.concatenate(parts)
    assert x.size % 8 == 0 and 3000 < x.size < 8000 and np.all(np.isfinite(x)) and np.abs(x).max() < 65504.0
    return x


def np_bf16_rn(x):
    """bf16 bits, round to nearest even: truncate; up when the dropped half is above the tie, or on it behind an odd kept part"""
    u = x.view(np.uint32).astype(np.uint64)
    kept, dropped = u >> 16, u & 0xffff
    return (kept + ((dropped > 0x8000) | ((dropped == 0x8000) & ((kept & 1) == 1)))).astype(np.uint16)


def np_bf16_f(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def np_split3(x):
    p0 = np_bf16_rn(x)
    r1 = x - np_bf16_f(p0)
    p1 = np_bf16_rn(r1)
    return np.stack([p0, p1, np_bf16_rn(r1 - np_bf16_f(p1))])


def test_three_bf16_planes(ref, values):
    """the integer form, the packed form and its scalar-argument overload: the same planes, which sum back to the input"""
    want = np_split3(values)
    for form in (0, 1, 2):
        planes = np.zeros((3, values.size), np.uint16)
        ref.xo_bf16_split3(_ptr(values), values.size, form, _ptr(planes))
        assert np.array_equal(planes, want), form
    total = np_bf16_f(want).astype(np.float64).sum(0)               # three terms of at most 8 bits each: exact in float64
    assert np.array_equal(total, values.astype(np.float64))
    assert np.array_equal(np.signbit(np_bf16_f(want[0])), np.signbit(values))


def test_packing_split_bf16_gives_the_same_planes(values):
    """the host-side split of the plans (pure torch, runs without the library) states the same arithmetic"""
    planes = _Packing.split_bf16(torch.from_numpy(values.copy())).numpy().view(np.uint16)
    assert np.array_equal(planes, np_split3(values))


@pytest.mark.parametrize("scaled", [0, 1])
def test_f16_pair_forms(ref, values, scaled):
    want_hi = values.astype(np.float16)
    r = values - want_hi.astype(np.float32)
    want_lo = (r * np.float32(2048.0) if scaled else r).astype(np.float16).view(np.uint16)
    assert np.all(np.isfinite(want_hi))
    assert np.count_nonzero(((want_lo >> 10) & 0x1f == 0) & (want_lo & 0x3ff != 0)) > 100     # subnormal residuals are reached
    for form in (scaled, 2 + scaled):                               # one value at a time, and the f32x2 variant
        hi, lo = np.zeros(values.size, np.uint16), np.zeros(values.size, np.uint16)
        ref.xo_f16_pair(_ptr(values), values.size, form, _ptr(hi), _ptr(lo))
        assert np.array_equal(hi, want_hi.view(np.uint16)) and np.array_equal(lo, want_lo), form


def test_f16_hs(ref, values):
    hi = np.ascontiguousarray(values.astype(np.float16))
    hs = np.zeros(hi.size, np.uint16)
    ref.xo_f16_hs(_ptr(hi), hi.size, _ptr(hs))
    # the product of two fp16 values is exact in float32: one rounding, to fp16 (subnormal below 2^-14)
    assert np.array_equal(hs, (hi.astype(np.float32) * np.float32(2.0 ** -11)).astype(np.float16).view(np.uint16))


def test_pair_scale_of_max(ref):
    rng = np.random.default_rng(7)
    mags = np.concatenate([np.array([0.0, 2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 2.0 ** -120, 2.0 ** 120, 3.0e38], np.float32),
                           np.array([1.0, 1.5, 2.0 ** 14, 2.0 ** 15 - 1, 2.0 ** 15], np.float32),
                           np.abs(rng.standard_normal(256)).astype(np.float32) * (2.0 ** rng.integers(-60, 60, 256)).astype(np.float32)])
    got = np.zeros(mags.size, np.float32)
    ref.xo_pair_scale_of_max(_ptr(mags.view(np.uint32)), mags.size, _ptr(got))
    assert np.all(got[:3] == 1.0)                                   # zero and subnormal maxima: no scaling
    e = np.clip(14 - np.floor(np.log2(mags[3:].astype(np.float64))), -100, 100)
    assert np.array_equal(got[3:], (2.0 ** e).astype(np.float32))
    assert np.all((mags[7:] * got[7:] >= 2.0 ** 14) & (mags[7:] * got[7:] < 2.0 ** 15))
