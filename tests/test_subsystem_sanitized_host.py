"""AddressSanitizer + UBSan pass over the HOST side of the subsystem read-out (CPU only).

``tests/sanitize/build_subsystem.py`` links the host-only, sanitized objects of the library and the host-memory stand-in
for the HIP runtime (``tests/sanitize/hip_stub.cpp``) with ``tests/sanitize/subsystem_driver.cpp``, a stand-alone program
with its own ``main`` that walks ``qsv_reduced_density_state`` and ``qsv_marginal_probabilities``: null pointers, k = 0,
k = 13, k > n, a marginal of 27 qubits, qubits repeated or out of range, a density register of the wrong size, on another
device (the driver answers the library's device queries itself, so that a second device exists), equal to the ket or a
view, mode registers -- each refused before any launch and with the deferred queue left as it was -- and then valid calls
for 1 to 18 qubits on three placements, with and without a grid cap, with launch counts and kernel names per form, and a
call that finds gates queued on both registers.  Kernels do not execute (there is no device code in this build), and
nothing is loaded into Python under a sanitizer.
"""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "sanitize"))


def test_subsystem_host_side_is_clean_under_asan_and_ubsan():
    import build_subsystem as san_build

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
    launches = int(proc.stdout.split("sanitized subsystem driver: ")[1].split()[0])
    assert launches > 500          # the driver really went through the launch paths
