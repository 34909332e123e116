"""What the ctypes loaders of the three RGB-D restatements share — TEST INFRASTRUCTURE ONLY: compiler flags, pointer and stride
helpers, the marshalling of one image's input (tests/rgbd_ref_common.h: RgbdSrc) and the two ways a restatement is built."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "crossloc_amd", "csrc")
CFLAGS = ["-std=c99", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Wno-unused-function", "-I" + CSRC, "-I" + HERE]
i64, ci, cf, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
SRC_ARGTYPES = [vp, i64, i64, i64, vp, i64, i64, i64, vp, i64, i64, ci, ci]         # coords, cam, depth with strides; Ho, Wo
INTR_ARGTYPES = [cf, cf, cf, ci]                                                    # focal, ppx, ppy, sub


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _el_strides(a):
    return [s // a.itemsize for s in a.strides]


def source_args(coords, cam, depth, focal, ppx, ppy, sub):
    """One image: coords float32 [3,Ho,Wo], and cam float32 [3,Ho,Wo] or depth float32 [Ho,Wo] (any strides).  Returns the argument
    prefix (pointers, element strides, Ho, Wo), the intrinsics (focal, ppx, ppy, sub; the principal point defaults to the image
    centre) and the arrays themselves, which must outlive the call."""
    coords = np.asarray(coords)
    assert coords.dtype == np.float32 and coords.ndim == 3 and coords.shape[0] == 3
    _, Ho, Wo = coords.shape
    cs, ds = [0, 0, 0], [0, 0]
    if cam is not None:
        cam = np.asarray(cam)
        assert cam.dtype == np.float32 and cam.shape == coords.shape
        cs = _el_strides(cam)
    if depth is not None:
        depth = np.asarray(depth)
        assert depth.dtype == np.float32 and depth.shape == (Ho, Wo)
        ds = _el_strides(depth)
    ppx = Wo * sub / 2.0 if ppx is None else ppx
    ppy = Ho * sub / 2.0 if ppy is None else ppy
    prefix = [_ptr(coords), *_el_strides(coords), _ptr(cam), *cs, _ptr(depth), *ds, Ho, Wo]
    return prefix, [float(focal), float(ppx), float(ppy), int(sub)], (coords, cam, depth)


def compile_lib(tmpdir, src, name):
    """`src` as a shared library in `tmpdir` (gcc -O2 -ffp-contract=off, a second): nothing is written into the repository tree"""
    out = os.path.join(str(tmpdir), "lib%s.so" % name)
    subprocess.check_call(["gcc", "-O2", "-fPIC"] + CFLAGS + ["-shared", "-o", out, src, "-lm"])
    return out


def compile_program(tmpdir, src, name, main_macro, sanitize=True):
    """`src` with its own main() (-D`main_macro`) as an executable; with `sanitize` under AddressSanitizer and UBSan."""
    out = os.path.join(str(tmpdir), name + ("_san" if sanitize else "_prog"))
    # the sanitizer runtimes are linked statically: the program then runs in whatever environment it inherits
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
           "-static-libasan", "-static-libubsan"] if sanitize else []
    subprocess.check_call(["gcc", "-O1", "-D" + main_macro] + san + CFLAGS + ["-o", out, src, "-lm"])
    return out
