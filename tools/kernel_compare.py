#!/usr/bin/env python3
"""Per-kernel comparison of one HIP unit's device code between two source trees (CPU only).

    python tools/kernel_compare.py TREE_A TREE_B UNIT [--must-match REGEX] [--out FILE]

Compiles razor_amd/csrc/rfec_UNIT.hip of each tree to gfx950 assembly with the build's flags
(razor_amd/build.py: -O3 -std=c++17 -fPIC), splits the assembly per kernel, demangles the names and prints, per
kernel and side, instructions, VGPRs, SGPRs, LDS bytes and scratch bytes, and whether the instruction text is the
same line by line (labels renumbered in order of appearance, comments and directives dropped).  Kernels present on
one side only are listed after the table.  Exit status 1 if a kernel whose name matches --must-match differs or
is missing on either side.
"""
from __future__ import annotations

import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROCM = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
ARCH = os.environ.get("RFEC_OFFLOAD_ARCH", "gfx950")
FLAGS = ["-O3", "-std=c++17", "-fPIC"]  # razor_amd/build.py's


def tool(name: str, sub: str = "bin") -> str:
    p = ROCM / sub / name
    return str(p) if p.exists() else name


def assembly(tree: Path, unit: str, tmp: Path, side: str) -> str:
    src = tree / "razor_amd" / "csrc" / f"rfec_{unit}.hip"
    out = tmp / f"{side}.s"
    subprocess.run([tool("hipcc"), f"--offload-arch={ARCH}", *FLAGS, f"-I{tree / 'include'}", f"-I{src.parent}",
                    "--cuda-device-only", "-S", str(src), "-o", str(out)], check=True)
    return out.read_text()


def demangle(names):
    if not names:
        return {}
    filt = shutil.which("c++filt") or tool("llvm-cxxfilt", "lib/llvm/bin")
    r = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
    short = {}
    for n, d in zip(names, r.stdout.splitlines()):
        depth, end = 0, len(d)
        for i, ch in enumerate(d):  # cut the parameter list: the first '(' outside template brackets that is not
            if ch == "<":           # "(anonymous namespace)"
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0 and not d.startswith("(anonymous namespace)", i):
                end = i
                break
        d = d[:end].replace("(anonymous namespace)::", "")
        short[n] = d[5:] if d.startswith("void ") else d
    return short


LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def kernels(asm: str) -> dict:
    """demangled name -> (instruction lines, (vgpr, sgpr, lds, scratch))"""
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", asm.split(".amdgpu_metadata", 1)[1])[1:]:
        f = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)\s*$", blk, re.M))
        meta[f["name"]] = tuple(int(f[k]) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size",
                                                     "private_segment_fixed_size"))
    text = {}
    for name in meta:
        body = re.search(rf"^{re.escape(name)}:.*?\n(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S).group(1)
        lines, labels = [], {}

        def renumber(m):
            return labels.setdefault(m.group(0), f".L{len(labels)}")

        for ln in body.splitlines():
            ln = ln.split(";", 1)[0].strip()
            if not ln or (ln.startswith(".") and not ln.endswith(":")):
                continue  # comments and directives
            lines.append(LABEL.sub(renumber, ln))
        text[name] = lines
    short = demangle(sorted(meta))
    return {short[n]: (text[n], meta[n]) for n in meta}


def natural(name: str):
    return [int(p) if p.isdigit() else p for p in re.split(r"(\d+)", name)]


def figures(k) -> str:
    lines, m = k
    n = sum(1 for ln in lines if not ln.endswith(":"))
    return f"{n:5d} {m[0]:3d} {m[1]:3d} {m[2]:4d} {m[3]:2d}"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("tree_a", type=Path, help="the parent's checkout")
    ap.add_argument("tree_b", type=Path, help="the tree to compare with it")
    ap.add_argument("unit", help="cascade for razor_amd/csrc/rfec_cascade.hip")
    ap.add_argument("--must-match", metavar="REGEX", help="kernels (demangled names) that must not differ")
    ap.add_argument("--out", type=Path, help="also write the table to this file")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        ka = kernels(assembly(a.tree_a.resolve(), a.unit, Path(tmp), "a"))
        kb = kernels(assembly(a.tree_b.resolve(), a.unit, Path(tmp), "b"))
    must = re.compile(a.must_match) if a.must_match else None
    out = [f"rfec_{a.unit}.hip compiled for {ARCH} ({' '.join(FLAGS)}) at the parent commit and on this tree, per "
           "kernel by demangled name:",
           "instructions, VGPRs, SGPRs, LDS bytes, scratch bytes; 'same' = the instruction text is identical line "
           "by line.", "", f"{'kernel':<50} {'parent':>19}          {'tree':>19}"]
    both = sorted(set(ka) & set(kb), key=natural)
    diff = [n for n in both if ka[n][0] != kb[n][0] or ka[n][1] != kb[n][1]]
    for n in both:
        out.append(f"{n:<50} {figures(ka[n])}          {figures(kb[n])}  {'DIFF' if n in diff else 'same'}")
    out += ["", f"{len(both) - len(diff)} of the {len(both)} kernels on both sides: the same"]
    for title, only, k in (("on the parent only:", set(ka) - set(kb), ka), ("new on this tree:", set(kb) - set(ka), kb)):
        if only:
            out += ["", title]
            pad = "" if k is ka else " " * 29
            out += [f"{n:<50} {pad}{figures(k[n])}" for n in sorted(only, key=natural)]
    failed = []
    if must:
        failed = [n for n in diff if must.search(n)] + [n for n in set(ka) ^ set(kb) if must.search(n)]
        out += ["", f"--must-match {a.must_match}: " +
                ("every matching kernel the same" if not failed else "FAILED for " + ", ".join(sorted(failed, key=natural)))]
    print("\n".join(out))
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text("\n".join(out) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
