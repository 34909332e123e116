"""CPU: register and scratch budget of the 256 x 256 pair GEMMs (csrc/xl_gemm_pair.hip), read from the compiler's own remarks.

The 8-wave workgroups run two waves per SIMD, i.e. 256 registers per lane, and their K-loops use most of them.  What the epilogue
derives from the thread index was once hoisted in front of the tile loop and spilled: 14 to 32 registers per lane went to scratch
and came back between the output stores.  This test compiles the file for gfx950 (device code only, the flags of the build plus
-Rpass-analysis=kernel-resource-usage) and holds every 256-column instantiation to no spilled register and no scratch."""
import os
import re
import shutil
import subprocess

import pytest

from crossloc_amd import build

SRC = os.path.join(build.CSRC, "xl_gemm_pair.hip")
FIELDS = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{demangled kernel name without spaces: {field: value}} from the remark lines"""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc is not installed: the resource remarks cannot be produced")
    obj = str(tmp_path_factory.mktemp("res") / "xl_gemm_pair.o")
    p = subprocess.run([hipcc] + build.FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", SRC, "-o", obj],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            name = subprocess.run([filt, m.group(1)], capture_output=True, text=True, check=True).stdout.strip()
            name = re.sub(r"\(anonymous namespace\)::|^void |\(.*\)$| ", "", name)
            cur = out.setdefault(name, {})
            continue
        m = re.search(r"remark: +([A-Za-z]+(?: [A-Za-z]+)?(?: \[[^\]]+\])?): (\d+)", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = int(m.group(2))
    assert out, "no kernel-resource-usage remark in the compiler's output:\n" + p.stderr[-2000:]
    return out


def _tile256(name):
    """pair_conv1x1_kernel<NORM,ACC,8,ZB,256> and pair_conv1x1_res_kernel<8,256>"""
    return re.fullmatch(r"pair_conv1x1_kernel<(true|false),(true|false),8,\d,256>|pair_conv1x1_res_kernel<8,256>", name) is not None


def test_the_256_column_1x1_forms_neither_spill_nor_use_scratch(usage):
    names = sorted(n for n in usage if _tile256(n))
    # plain, NORM, accumulate, the two Z-batched forms and the residual form: what the launcher can select
    assert len(names) == 6 and "pair_conv1x1_res_kernel<8,256>" in names, names
    for n in names:
        u = usage[n]
        print("%-48s %s" % (n, u))
        assert u["VGPRs Spill"] == 0, (n, u)
        assert u["ScratchSize [bytes/lane]"] == 0, (n, u)
        assert u["VGPRs"] + u["AGPRs"] <= 256 and u["Occupancy [waves/SIMD]"] >= 2, (n, u)


def test_the_residual_form_on_128_columns_does_not_spill_either(usage):
    u = usage["pair_conv1x1_res_kernel<8,128>"]
    assert u["VGPRs Spill"] == 0 and u["ScratchSize [bytes/lane]"] == 0, u


def test_the_winograd_pair_gemm_keeps_its_budget(usage):
    u = usage["pair_gemm_kernel<512,0,2>"]
    assert u["VGPRs Spill"] == 0 and u["ScratchSize [bytes/lane]"] == 0, u
    assert u["Occupancy [waves/SIMD]"] == 2, u
