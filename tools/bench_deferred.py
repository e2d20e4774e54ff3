#!/usr/bin/env python3
"""Plan of the deferred gate queue for the benchmark circuit, and what each pass cost on the GPU.

    python tools/bench_deferred.py [--steps S] [--trace kernel_trace.csv]

Prints, for S back-to-back passes of the cfg2 circuit (n = 28, 100 gates, seed 100) queued one by one as bench.py
queues them, the launches the library makes (quantum_computations_amd/csrc/qsv_plan.h through
tests/defer_plan/plan_driver.cpp, compiled here): per launch the kind (pass or single gate), the gates it applies, the
tile bits, the fraction of tiles it loads and the groups the kernel applies the gates in (qsv_plan::cut_groups through
tests/defer_plan/groups_driver.cpp: gates per group and each group's register bits as tile indices).  With ``--trace``
(rocprofv3 --kernel-trace of ``bench.py --steps S-1 --warmup 1``) the k_pass_tile durations are matched to the planned
passes in launch order and a least-squares plane ms = a + b * groups + c * gates is fitted (the cost model's PASS_BASE /
PASS_PER_GROUP / PASS_PER_GATE, in units of the 1.31 ms per-gate pass)."""
from __future__ import annotations

import argparse
import csv
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

from quantum_computations_amd import workloads as W  # noqa: E402
from test_defer_plan_host import WINDOW, classify, compiler, tile_index  # noqa: E402


def plan(n, recs):
    with tempfile.TemporaryDirectory() as tmp:
        exe = Path(tmp) / "plan_driver"
        subprocess.run([compiler(), "-std=c++17", "-O2", f"-I{REPO / 'quantum_computations_amd' / 'csrc'}",
                        str(REPO / "tests" / "defer_plan" / "plan_driver.cpp"), "-o", str(exe)], check=True)
        text = f"{n} {WINDOW} {len(recs)}\n" + "\n".join(f"{r.need} {r.ctrl_mask} {int(r.exact)} {r.cost:.6f}" for r in recs)
        out = subprocess.run([str(exe)], input=text + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    passes, i = [], 1
    while i < len(out) and out[i].startswith("pass"):
        _, fused, tile, count = out[i].split()
        gates = [tuple(int(v) for v in out[i + 1 + j].split()[1:]) for j in range(int(count))]
        passes.append((fused == "1", int(tile), gates))
        i += 1 + int(count)
    return passes


def groups_of(recs, passes):
    """Per fused pass, [(first, count, (reg0..reg3))] as the library cuts it (diagonal gates and phases have no targets)."""
    need = [[0 if recs[g].kind in ("diag", "phase") else sum(1 << tile_index(b, tile) for b in recs[g].targets)
             for g, _, _ in gates] for f, tile, gates in passes if f]
    with tempfile.TemporaryDirectory() as tmp:
        exe = Path(tmp) / "groups_driver"
        subprocess.run([compiler(), "-std=c++17", "-O2", f"-I{REPO / 'quantum_computations_amd' / 'csrc'}",
                        str(REPO / "tests" / "defer_plan" / "groups_driver.cpp"), "-o", str(exe)], check=True)
        text = "".join(f"{len(p)} " + " ".join(map(str, p)) + "\n" for p in need)
        out = iter(subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n"))
    cuts = []
    for line in out:
        if line.startswith("groups "):
            rows = [[int(v) for v in next(out).split()[1:]] for _ in range(int(line.split()[1]))]
            cuts.append([(r[0], r[1], tuple(r[2:])) for r in rows])
    return cuts


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--trace", type=Path)
    args = ap.parse_args()
    n = 28
    ops = W.random_circuit(n, 100, 100) * args.steps
    recs = [classify(o, n) for o in ops]
    passes = plan(n, recs)
    fused = [p for p in passes if p[0]]
    cuts = groups_of(recs, passes)
    by_pass = iter(cuts)
    print(f"{len(ops)} gates -> {len(passes)} launches ({len(fused)} passes, {len(passes) - len(fused)} single gates): "
          f"{100 * len(passes) / len(ops):.1f} launches per 100 gates")
    for k, (f, tile, gates) in enumerate(passes):
        bits = [b for b in range(n) if (tile >> b) & 1]
        names = [ops[g]["name"] for g, _, _ in gates]
        frac = min(1.0, sum(2.0 ** -bin(out).count("1") for _, _, out in gates))
        grp = next(by_pass) if f else []
        print(f"  {k:3d} {'pass ' if f else 'alone'} gates={len(gates):2d} groups={len(grp):2d} tile={bits} "
              f"loads {100 * frac:5.1f}% " + " ".join(names)
              + "".join(f" | {count}@{','.join(map(str, reg))}" for _, count, reg in grp))
    print(f"{sum(len(g) for _, _, g in fused)} gates in {len(fused)} passes are cut into {sum(len(c) for c in cuts)} groups")
    if args.trace:
        rows = [r for r in csv.DictReader(open(args.trace)) if "k_pass_tile" in r["Kernel_Name"]]
        ms = np.array([(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows])
        sizes = np.array([len(g) for f, _, g in passes if f], dtype=float)
        if len(ms) != len(sizes):
            print(f"trace holds {len(ms)} passes, plan {len(sizes)}: run bench.py with --steps {args.steps - 1} --warmup 1")
            return 1
        ngroups = np.array([len(c) for c in cuts], dtype=float)
        A = np.vstack([np.ones_like(sizes), ngroups, sizes]).T
        (a, b, c), *_ = np.linalg.lstsq(A, ms, rcond=None)
        resid = ms - A @ np.array([a, b, c])
        print(f"k_pass_tile: {len(ms)} passes, {ms.mean():.3f} ms average ({ms.min():.3f} .. {ms.max():.3f}), "
              f"{sizes.mean():.1f} gates in {ngroups.mean():.1f} groups per pass; fit ms = {a:.3f} + {b:.4f} * groups + "
              f"{c:.4f} * gates (= {a / 1.31:.2f} + {b / 1.31:.3f} * groups + {c / 1.31:.3f} * gates in 1.31 ms passes), "
              f"rms residual {np.sqrt(np.mean(resid ** 2)):.3f} ms")
        for k, (t, gr, g) in enumerate(zip(ms, ngroups, sizes)):
            print(f"  pass {k:3d}: {int(g):2d} gates in {int(gr):2d} groups, {t:.3f} ms")
    return 0


if __name__ == "__main__":
    sys.exit(main())
