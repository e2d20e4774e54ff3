"""AddressSanitizer + UBSan pass over the HOST side of the trajectory-ensemble entry points (CPU only).

``tests/sanitize/build_ensemble.py`` links the host-only, sanitized objects of the library and the host-memory stand-in for
the HIP runtime (``tests/sanitize/hip_stub.cpp``) with ``tests/sanitize/ensemble_driver.cpp``, a stand-alone program with
its own ``main`` that walks ``qsv_ensemble_broadcast``, ``qsv_ensemble_apply_channel``, ``qsv_ensemble_log_read``,
``qsv_ensemble_norm2`` and ``qsv_ensemble_expect_pauli_sum``: null pointers, a member size outside ``k .. n_total``, target
and term qubits outside a member or repeated, a draw outside [0, 1) or a forced branch out of range in any member, mode
registers, views, a channel on another device -- each refused before any launch and with the deferred queue left as it was
-- and then valid calls for members of 1 to 16 qubits, 1 to 64 of them, on every target bit.  Launches are counted: a general
call adds the same three whatever the number of Kraus operators and members, a mixed-unitary call has no read pass.  A log of
300 steps, more than its device slots, is read back complete.  Kernels do not execute (there is no device code in this
build), so what the log holds is the stand-in's zeroed memory; its order is checked on the device (test_gpu_ensemble.py).
"""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "sanitize"))


def test_ensemble_host_side_is_clean_under_asan_and_ubsan():
    import build_ensemble as san_build

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
    launches = int(proc.stdout.split("sanitized ensemble driver: ")[1].split()[0])
    assert launches > 1000          # the driver really went through the launch paths
