#!/usr/bin/env python3
"""What the compiler made of k_pass_tile: registers, and the instruction mix of every basic block that does gate arithmetic.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Iquantum_computations_amd/csrc --cuda-device-only -S \
          -mllvm -structurizecfg-skip-uniform-regions quantum_computations_amd/csrc/qsv_pass.hip -o pass.s
    python tools/pass_kernel_isa.py pass.s [--kernel k_pass_tileILb1E]

A gate body is one basic block (no control on register bits) or one block per register index (with such controls), so the
blocks are listed by their instruction mix: how many blocks have it, FMAs, v_cndmask (selects), vector moves (copies of
amplitudes), scalar loads and s_waitcnt per block.  Compile-time facts only; no timing."""
from __future__ import annotations

import argparse
import collections
import re
import sys


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="k_pass_tileILb1E", help="substring of the mangled kernel name")
    ap.add_argument("--min-fma", type=int, default=8, help="list blocks with at least this many FMAs / multiplies")
    args = ap.parse_args()
    lines = open(args.asm).read().split("\n")
    start = next((i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % re.escape(args.kernel), l)), None)
    if start is None:
        print(f"no kernel matching {args.kernel} in {args.asm}")
        return 1
    name = lines[start].split(":")[0]
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    kinds = [("fma", r"v_fma_f64|v_fmac_f64"), ("mul", r"v_mul_f64"), ("cndmask", r"v_cndmask"),
             ("vmov", r"v_mov_b64|v_mov_b32|v_accvgpr"), ("s_load", r"s_load_|s_buffer_load"), ("waitcnt", r"s_waitcnt"),
             ("ds", r"ds_read|ds_write|ds_load"), ("branch", r"s_cbranch|s_branch")]
    blocks, label, total = [], "entry", collections.Counter()
    cur = collections.Counter()
    for l in lines[start + 1:end]:
        t = l.strip()
        if re.match(r"^\.LBB\d+_\d+:", t):
            blocks.append((label, cur))
            label, cur = t.split(":")[0], collections.Counter()
            continue
        if not t or t.startswith((";", ".")):
            continue
        cur["insts"] += 1
        for k, pat in kinds:
            if re.match(pat, t):
                cur[k] += 1
    blocks.append((label, cur))
    for _, c in blocks:
        total.update(c)
    mine, entry = {}, {}
    for l in lines[end:]:                      # the amdhsa.kernels metadata: one list item per kernel
        if l.startswith("  - "):
            entry = {}
            l = "    " + l[4:]
        m = re.match(r"\s+\.(name|vgpr_count|sgpr_count|agpr_count|private_segment_fixed_size|group_segment_fixed_size|"
                     r"vgpr_spill_count|sgpr_spill_count):\s+(\S+)", l)
        if m:
            entry[m.group(1)] = m.group(2)
            if entry.get("name") == name:
                mine = entry
    name = name.split(":")[0]
    print(f"{name}")
    print("  " + ", ".join(f"{k} {v}" for k, v in sorted(mine.items()) if k != "name"))
    print(f"  {len(blocks)} basic blocks, {total['insts']} instructions (about {8 * total['insts'] // 1024} KiB)")
    print("  whole kernel: " + ", ".join(f"{k} {total[k]}" for k, _ in kinds))
    mixes = collections.Counter()
    for _, c in blocks:
        if c["fma"] + c["mul"] >= args.min_fma:
            mixes[tuple(c[k] for k, _ in kinds)] += 1
    print(f"  blocks with at least {args.min_fma} FMAs + multiplies, by instruction mix:")
    print("    blocks " + " ".join(f"{k:>8s}" for k, _ in kinds))
    for mix, n in sorted(mixes.items(), key=lambda kv: (-kv[0][0], kv[0])):
        print(f"    {n:6d} " + " ".join(f"{v:8d}" for v in mix))
    big = [(lab, c) for lab, c in blocks if c["vmov"] >= 16 and c["fma"] == 0]
    print(f"  blocks that only copy registers (16 or more vector moves, no FMA): {len(big)}"
          + "".join(f"\n    {lab}: {c['vmov']} moves" for lab, c in big[:12]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
