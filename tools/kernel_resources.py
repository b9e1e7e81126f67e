#!/usr/bin/env python3
"""Per-kernel registers, LDS and scratch of csrc translation units, from the .amdhsa metadata of a device-only -S compile.

    python tools/kernel_resources.py loss.hip criteria.hip                    # this tree
    python tools/kernel_resources.py --against <other checkout> loss.hip ...  # both trees side by side, differences marked

Needs hipcc only (no GPU).  Flags: those of pointcloudpdf_amd/build.py for the file.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pointcloudpdf_amd import build  # noqa: E402

FIELDS = [("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"), ("scratch", ".private_segment_fixed_size")]


def demangle(names):
    r = subprocess.run(["c++filt", "-p"], input="\n".join(names), capture_output=True, text=True)
    return r.stdout.split("\n")[: len(names)] if r.returncode == 0 else names


def resources(root, src):
    """{demangled kernel name: (vgpr, sgpr, lds, scratch)} of root/pointcloudpdf_amd/csrc/src"""
    path = os.path.join(root, "pointcloudpdf_amd", "csrc", src)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        cmd = [build._hipcc()] + build.COMMON + build.EXTRA.get(src, []) + ["--cuda-device-only", "-S", path, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr)
        if r.stderr.strip():
            print(r.stderr, file=sys.stderr)
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):text.index("amdhsa.target:")]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:   # one entry per kernel; its own keys sit at four columns (argument entries deeper)
        block = "    " + block
        name = re.search(r"^    \.name:\s+(\S+)", block, re.M).group(1)
        kernels[name] = tuple(int(re.search(r"^    " + re.escape(key) + r":\s+(\d+)", block, re.M).group(1)) for _, key in FIELDS)
    names = list(kernels)
    return {d: kernels[n] for n, d in zip(names, demangle(names))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", help="root of another checkout: print both and mark the kernels that differ")
    ap.add_argument("files", nargs="+")
    a = ap.parse_args()
    head = " ".join(f"{n:>7}" for n, _ in FIELDS)
    print(f"{'kernel':<72} {head}" + (f" | {head}  (other tree)" if a.against else ""))
    for src in a.files:
        mine = resources(ROOT, src)
        other = resources(a.against, src) if a.against else {}
        print(f"# {src}")
        for name in sorted(set(mine) | set(other)):
            row = lambda v: " ".join(f"{x:>7}" for x in v) if v else " ".join(f"{'-':>7}" for _ in FIELDS)  # noqa: E731
            line = f"{name[:72]:<72} {row(mine.get(name))}"
            if a.against:
                line += f" | {row(other.get(name))}" + ("" if mine.get(name) == other.get(name) else "  <-- differs")
            print(line)


if __name__ == "__main__":
    main()
