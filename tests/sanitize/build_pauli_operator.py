#!/usr/bin/env python3
"""TEST INFRASTRUCTURE: the AddressSanitizer + UBSan host binary of the driver of qsv_apply_pauli_sum,
qsv_pauli_transition_sum and qsv_pauli_rotations_adjoint.

    python tests/sanitize/build_pauli_operator.py      # -> tests/sanitize/_build/qsv_pauli_operator_san

``build.py`` compiles the library's HIP sources host-only with the sanitizers and ``hip_stub.cpp``; this links the same
objects with ``pauli_operator_driver.cpp`` in place of ``driver.cpp``.  Stand-alone program with its own ``main``:
nothing here is loaded into Python.
"""
from __future__ import annotations

import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import build as base  # noqa: E402

PLAN_HEADERS = [base.CSRC / "qsv_pauli_plan.h", base.CSRC / "qsv_pauli_rotation_plan.h"]


def build(verbose: bool = False) -> Path:
    import subprocess

    def run(cmd):
        if verbose:
            print(" ".join(map(str, cmd)), flush=True)
        subprocess.run(cmd, check=True)

    # build.py does not know the planners' headers: objects older than either are compiled again
    newest = max(header.stat().st_mtime for header in PLAN_HEADERS)
    for name in base.SOURCES:
        obj = base.OUT / (name + ".o")
        if obj.exists() and obj.stat().st_mtime < newest:
            obj.unlink()
    base.build(verbose)
    objs = [base.OUT / (name + ".o") for name in base.SOURCES] + [base.OUT / "hip_stub.cpp.o"]
    driver = base.OUT / "pauli_operator_driver.cpp.o"
    if base.stale(driver, [HERE / "pauli_operator_driver.cpp", base.REPO / "include" / "qsv.h", *PLAN_HEADERS]):
        run([base.CLANG, "-std=c++17", *base.SAN, *base.INC, "-c", HERE / "pauli_operator_driver.cpp", "-o", driver])
    exe = base.OUT / "qsv_pauli_operator_san"
    if base.stale(exe, objs + [driver, base.OUT / "fatbins.c"]):
        run([base.CLANG, *base.SAN, "-x", "c", base.OUT / "fatbins.c", "-x", "none", *objs, driver, "-ldl", "-lpthread", "-o", exe])
    return exe


if __name__ == "__main__":
    print(build(verbose=True))
