"""AddressSanitizer + UBSan pass over the HOST side of qsv_expect_pauli_sum (CPU only).

``tests/sanitize/build_pauli_sum.py`` links the host-only, sanitized objects of the library and the host-memory stand-in
for the HIP runtime (``tests/sanitize/hip_stub.cpp``) with ``tests/sanitize/pauli_sum_driver.cpp``, a stand-alone program
that walks the entry point: null pointers, a negative count, decreasing offsets, a term of 65 letters, repeated and
out-of-range qubits, a bad letter -- each refused before any launch -- and then valid lists on registers of 1 to 18
qubits, on a view and on a mode register: parsing, planning, one launch per planned pass, the copy of the partials and
their sums.  Kernels do not execute (there is no device code in this build).
"""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "sanitize"))


def test_pauli_sum_host_side_is_clean_under_asan_and_ubsan():
    import build_pauli_sum as san_build

    if not san_build.base.CLANG.exists():
        pytest.skip("ROCm clang not installed")
    exe = san_build.build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    report = proc.stdout[-2000:] + proc.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in report and "runtime error:" not in report and "LeakSanitizer" not in report, report
    assert proc.returncode == 0, report
    assert "0 failed expectations" in proc.stdout
    launches = int(proc.stdout.split("sanitized Pauli-sum driver: ")[1].split()[0])
    assert launches > 100          # the driver really went through the launch path
