#!/usr/bin/env python3
"""TEST INFRASTRUCTURE: the AddressSanitizer + UBSan host binary of qsv_expect_pauli_sum's driver.

    python tests/sanitize/build_pauli_sum.py      # -> tests/sanitize/_build/qsv_pauli_sum_san

``build.py`` compiles the library's HIP sources host-only with the sanitizers and ``hip_stub.cpp``; this links the same
objects with ``pauli_sum_driver.cpp`` in place of ``driver.cpp``.  Stand-alone program with its own ``main``: nothing
here is loaded into Python.
"""
from __future__ import annotations

import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import build as base  # noqa: E402

PLAN_HEADER = base.CSRC / "qsv_pauli_plan.h"


def build(verbose: bool = False) -> Path:
    import subprocess

    def run(cmd):
        if verbose:
            print(" ".join(map(str, cmd)), flush=True)
        subprocess.run(cmd, check=True)

    # build.py does not know the planner's header: objects older than it are compiled again
    for name in base.SOURCES:
        obj = base.OUT / (name + ".o")
        if obj.exists() and obj.stat().st_mtime < PLAN_HEADER.stat().st_mtime:
            obj.unlink()
    base.build(verbose)
    objs = [base.OUT / (name + ".o") for name in base.SOURCES] + [base.OUT / "hip_stub.cpp.o"]
    driver = base.OUT / "pauli_sum_driver.cpp.o"
    if base.stale(driver, [HERE / "pauli_sum_driver.cpp", base.REPO / "include" / "qsv.h"]):
        run([base.CLANG, "-std=c++17", *base.SAN, *base.INC, "-c", HERE / "pauli_sum_driver.cpp", "-o", driver])
    exe = base.OUT / "qsv_pauli_sum_san"
    if base.stale(exe, objs + [driver, base.OUT / "fatbins.c"]):
        run([base.CLANG, *base.SAN, "-x", "c", base.OUT / "fatbins.c", "-x", "none", *objs, driver, "-ldl", "-lpthread", "-o", exe])
    return exe


if __name__ == "__main__":
    print(build(verbose=True))
