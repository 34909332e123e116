#!/usr/bin/env python
"""Per-kernel diff of the gfx950 assembly of two source trees: what a refactor that claims "no kernel changed" is held to.

    python tools/kernel_asm_diff.py OLD_TREE NEW_TREE [--jobs N] [--asm-dir DIR]

Every crossloc_amd/csrc/*.hip of both trees is compiled with the flags of crossloc_amd/build.py plus --cuda-device-only -S.
Functions are matched by mangled name over the WHOLE tree (hipcc mangles anonymous-namespace kernels without a per-file
suffix, so a kernel that moved to another file keeps its name) and compared as text: the instructions and, for kernels, the
.amdhsa_kernel descriptor block, after dropping comments and renumbering the function-local labels.  One line per function
of the old tree - SAME, DIFF or MISSING - then NEW for functions only the new tree has, then a summary line.  Exit status 1
unless everything is SAME.  With --asm-dir the .s files are kept there (old/, new/) and reused while they are newer than the
source and every header beside it."""
import argparse
import ast
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile


def flags(tree):
    with open(os.path.join(tree, "crossloc_amd", "build.py")) as f:
        return next(ast.literal_eval(line.split("=", 1)[1].strip()) for line in f if line.startswith("FLAGS ="))


def compile_tree(tree, out, jobs):
    csrc = os.path.join(tree, "crossloc_amd", "csrc")
    os.makedirs(out, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    headers = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    headers += [os.path.join(tree, "include", f) for f in os.listdir(os.path.join(tree, "include"))]
    newest_header = max(os.path.getmtime(h) for h in headers)
    todo, asm = [], []
    for name in sorted(os.listdir(csrc)):
        if not name.endswith(".hip"):
            continue
        src, dst = os.path.join(csrc, name), os.path.join(out, name[:-4] + ".s")
        asm.append(dst)
        if not os.path.exists(dst) or os.path.getmtime(dst) < max(os.path.getmtime(src), newest_header):
            todo.append([hipcc] + flags(tree) + ["--cuda-device-only", "-S", src, "-o", dst])
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        for cmd, p in zip(todo, pool.map(lambda c: subprocess.run(c, capture_output=True, text=True), todo)):
            if p.returncode != 0:
                sys.exit("hipcc failed: %s\n%s" % (" ".join(cmd), p.stderr[-3000:]))
    return asm


def normalise(lines):
    out = []
    for line in lines:
        line = line.split(";")[0].rstrip()
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
        if line.strip():
            out.append(line)
    return out


def functions(asm_files):
    """mangled name -> normalised text (body, then the kernel descriptor if it is a kernel)"""
    found = {}
    for path in asm_files:
        with open(path) as f:
            lines = f.read().splitlines()
        names = {m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", l) for l in lines) if m}
        i = 0
        while i < len(lines):
            m = re.match(r"(\S+):", lines[i])
            if m and m.group(1) in names:
                j = i
                while not re.match(r"\.Lfunc_end\d+:", lines[j]):
                    j += 1
                found[m.group(1)] = normalise(lines[i:j + 1])
                i = j
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
            if m:
                j = i
                while ".end_amdhsa_kernel" not in lines[j]:
                    j += 1
                found[m.group(1)] += normalise(lines[i:j + 1])
                i = j
            i += 1
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--asm-dir")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        base = a.asm_dir or tmp
        old = functions(compile_tree(a.old, os.path.join(base, "old"), a.jobs))
        new = functions(compile_tree(a.new, os.path.join(base, "new"), a.jobs))
    count = {"SAME": 0, "DIFF": 0, "MISSING": 0, "NEW": 0}
    for name in sorted(old):
        verdict = "MISSING" if name not in new else "SAME" if old[name] == new[name] else "DIFF"
        count[verdict] += 1
        print("%-7s %s" % (verdict, name))
    for name in sorted(set(new) - set(old)):
        count["NEW"] += 1
        print("%-7s %s" % ("NEW", name))
    print("%d functions of the old tree: %d SAME, %d DIFF, %d MISSING; %d only in the new tree" % (
        len(old), count["SAME"], count["DIFF"], count["MISSING"], count["NEW"]))
    return 0 if count["SAME"] == len(old) and not count["NEW"] else 1


if __name__ == "__main__":
    sys.exit(main())
