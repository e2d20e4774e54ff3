#!/usr/bin/env python3
"""Are the kernels of two builds the same device code?  For refactors that move kernels between translation units.

    hipcc <the flags build.py gives the file> --cuda-device-only -S old/qsv_kernels.hip -o old.s      (and so on)
    python tools/device_code_diff.py --old old.s --new gate12.s gatek.s sequence.s pass.s state.s

(the split of the gate-kernel file qsv_kernels.hip into its five families; profiles/r11_gate_split_device_code.txt)

Each side is a list of assembly files whose kernels are pooled.  Per kernel three things are compared as text: the
instructions, the .amdhsa_ descriptor block, and the kernel's entry in the metadata (argument offsets and sizes, register
and LDS use).  Before the comparison
  * symbols are demangled and namespace qualifiers dropped -- "(anonymous namespace)::k(qsv_layout::BigArgs)" and
    "k(BigArgs)" are the same kernel, so a type or a helper may move into a header's namespace;
  * comments go, and the function number inside local labels (.LBB12_3 -> .LBB_3, .Lfunc_end12, .LJTI12_0, .Ltmp7);
  * section switches go (.section, .text): after its descriptor a kernel with external linkage returns to .text, one in an
    anonymous namespace to a section of its own, so a kernel may move into an anonymous namespace.
Static LDS arrays need no rule: the compiler addresses them by number, and their demangled names do not reach the text.
Prints the kernel counts, the kernels that exist on one side only and those that differ; exit status 1 if there are any.
"""
from __future__ import annotations

import argparse
import re
import shutil
import subprocess
import sys
from pathlib import Path

MANGLED = re.compile(r"_Z[A-Za-z0-9_]+")


def demangler() -> str:
    for cand in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt")):
        if cand and Path(cand).exists():
            return cand
    raise SystemExit("no llvm-cxxfilt / c++filt found")


def demangle_all(texts: list[str]) -> dict[str, str]:
    names = sorted({m for t in texts for m in MANGLED.findall(t)})
    out = subprocess.run([demangler()], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: plain(d) for n, d in zip(names, out)}


def plain(demangled: str) -> str:
    prev = None
    while prev != demangled:      # drop qualifiers, innermost first; "f(double&)::sx" keeps its function scope
        prev = demangled
        demangled = re.sub(r"(\(anonymous namespace\)|\b[A-Za-z_]\w*)::(?=[A-Za-z_(])", "", demangled)
    return demangled


def normalise(line: str, names: dict[str, str]) -> str:
    line = line.split(";", 1)[0].rstrip()
    line = MANGLED.sub(lambda m: names.get(m.group(0), m.group(0)), line)
    line = re.sub(r"\.(LBB|LJTI|LCPI)\d+_", r".\1_", line)
    line = re.sub(r"\.(Lfunc_end|Lfunc_begin|Ltmp)\d+", r".\1", line)
    return line


def kernels_of(path: Path, names: dict[str, str], text: str) -> dict[str, dict[str, list[str]]]:
    lines = text.split("\n")
    found: dict[str, dict[str, list[str]]] = {}
    kernel_syms = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    for sym in kernel_syms:
        start = next(i for i, l in enumerate(lines) if l.startswith(f"{sym}:"))
        body, desc, where = [], [], "body"
        for l in lines[start + 1:]:
            s = l.strip()
            if s.startswith(".Lfunc_end"):
                break
            if s.startswith(".amdhsa_kernel "):
                where = "desc"
            elif s == ".end_amdhsa_kernel":
                where = "body"
            elif where == "desc":
                desc.append(normalise(s, names))
            elif s and s != ".text" and not s.startswith((".section", ".p2align")):
                n = normalise(l, names).strip()
                if n:
                    body.append(n)
        found[names.get(sym, sym)] = {"instructions": body, "descriptor": desc}
    # metadata: the entries of amdhsa.kernels, each beginning with "  - "
    begin = lines.index("amdhsa.kernels:")
    entry: list[str] = []
    entries = []
    for l in lines[begin + 1:]:
        if l.startswith("  - ") or not l.startswith("    "):
            if entry:
                entries.append(entry)
            entry = []
            if not l.startswith("  - "):
                break
        entry.append(normalise(l.replace("  - ", "    ", 1) if l.startswith("  - ") else l, names))
    for e in entries:
        name = next(l.split(":", 1)[1].strip() for l in e if l.strip().startswith(".name:"))
        if name not in found:
            raise SystemExit(f"{path}: metadata for {name} without a kernel")
        found[name]["metadata"] = e
    return found


def pool(paths: list[Path]) -> dict[str, dict[str, list[str]]]:
    texts = [p.read_text() for p in paths]
    names = demangle_all(texts)
    all_kernels: dict[str, dict[str, list[str]]] = {}
    for p, t in zip(paths, texts):
        for name, parts in kernels_of(p, names, t).items():
            if name in all_kernels:
                raise SystemExit(f"{p}: kernel {name} appears twice on one side")
            all_kernels[name] = parts
    return all_kernels


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", nargs="+", type=Path, required=True)
    ap.add_argument("--new", nargs="+", type=Path, required=True)
    ap.add_argument("--show", type=int, default=0, metavar="N", help="print the first N differing lines of each differing kernel")
    args = ap.parse_args()
    old, new = pool(args.old), pool(args.new)
    print(f"kernels: {len(old)} old, {len(new)} new")
    bad = 0
    for name in sorted(set(old) - set(new)):
        print(f"only in old: {name}")
        bad += 1
    for name in sorted(set(new) - set(old)):
        print(f"only in new: {name}")
        bad += 1
    for name in sorted(set(old) & set(new)):
        parts = [part for part in ("instructions", "descriptor", "metadata") if old[name].get(part) != new[name].get(part)]
        if parts:
            bad += 1
            print(f"differs ({', '.join(parts)}): {name}")
            for part in parts[:1] if args.show else []:
                a, b = old[name].get(part) or [], new[name].get(part) or []
                shown = 0
                for i in range(max(len(a), len(b))):
                    x, y = (a[i] if i < len(a) else "<end>"), (b[i] if i < len(b) else "<end>")
                    if x != y and shown < args.show:
                        print(f"    {part}[{i}]  old: {x}\n    {' ' * len(part)}     new: {y}")
                        shown += 1
    print("identical" if not bad else f"{bad} kernels differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
