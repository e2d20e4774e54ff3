"""AddressSanitizer + UBSan pass over the HOST side of the diagonal-operator entry points (CPU only).

``tests/sanitize/build_diagonal.py`` links the host-only, sanitized objects of the library and the host-memory stand-in
for the HIP runtime (``tests/sanitize/hip_stub.cpp``) with ``tests/sanitize/diagonal_driver.cpp``, a stand-alone program
with its own ``main`` that walks every new entry point: null handles, bad sizes and devices, options other than the grid
cap, windows of upload and download out of bounds, X / Y letters, qubits out of range or repeated, 65 letters, registers
and diagonals of different sizes, a destination that is too small or meets its source, mode registers -- each refused
before any launch and with every deferred queue left alone -- and then valid calls for 0 to 18 qubits with 0, 1, 2, 63,
64, 65 and 200 terms, windows at both ends and ``accumulate``.  Launches are counted: one per build whatever the number
of terms, one per pass.  Kernels do not execute (there is no device code in this build).
"""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "sanitize"))


def test_diagonal_host_side_is_clean_under_asan_and_ubsan():
    import build_diagonal as san_build

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
    launches = int(proc.stdout.split("sanitized diagonal driver: ")[1].split()[0])
    assert launches > 1000          # the driver really went through the launch paths
