"""AddressSanitizer + UBSan pass over the HOST side of the noise entry points (CPU only).

``tests/sanitize/build_channel.py`` links the host-only, sanitized objects of the library and the host-memory stand-in for
the HIP runtime (``tests/sanitize/hip_stub.cpp``) with ``tests/sanitize/channel_driver.cpp``, a stand-alone program with its
own ``main`` that walks ``qsv_channel_*``, ``qsv_apply_channel``, ``qsv_channel_log_read`` and ``qsv_density_expect_paulis``:
null pointers, bad sizes and devices, draws outside [0, 1), forced branches out of range, qubits repeated or out of range,
mode registers, a channel on another device (the driver answers the library's device queries itself, so that a second
device exists), density registers with an odd number of qubits, bad term lists -- each refused before any launch and with
the deferred queue left as it was -- and then valid calls for 1 to 18 qubits on every target bit, with and without the
streaming forms and the grid cap.  Launches are counted: a mixed-unitary call on a deferring register adds none at call
time, a general call adds the same four whatever the number of Kraus operators.  A log of 900 entries, 600 of them in
device slots, is read back complete and in call order.  Kernels do not execute (there is no device code in this build).
"""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "sanitize"))


def test_channel_host_side_is_clean_under_asan_and_ubsan():
    import build_channel as san_build

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
    launches = int(proc.stdout.split("sanitized channel driver: ")[1].split()[0])
    assert launches > 1000          # the driver really went through the launch paths
