"""AddressSanitizer + UBSan pass over the HOST side of ``qsv_layer_adjoint`` and ``qsv_layer_transition`` (CPU only).

``tests/sanitize/layer_adjoint_driver.cpp`` is linked with the sanitized host objects of the library and the host-memory
stand-in for the HIP runtime, exactly as ``layer_driver.cpp`` is: a stand-alone program with its own ``main``.  It walks every
refusal of both calls (null handles and arrays, ``k`` out of range, repeated and out-of-range qubits, entries that are not
finite, registers of different sizes and devices, overlapping registers for the adjoint call, a mode register) on plain and
deferring registers with ``qsv_defer_stats`` unchanged, ``k = 0``, ``bra == ket`` accepted, and valid calls for ``n = 1 .. 30``
on all bits, bits 0..5, the top bit and random subsets, whose launches must equal the plan's passes: the sums add no launch.
Kernels do not execute, and nothing is loaded into Python under a sanitizer.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "sanitize"))

DRIVER, MIN_LAUNCHES, TIMEOUT = "layer_adjoint_driver", 500, 600


def test_layer_adjoint_host_side_is_clean_under_asan_and_ubsan():
    import build as san_build

    if not san_build.CLANG.exists():
        pytest.skip("ROCm clang not installed")
    assert DRIVER in san_build.DRIVERS          # picked up by its name pattern
    exe = san_build.build(DRIVER)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=TIMEOUT, env=env)
    report = proc.stdout[-2000:] + proc.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in report and "runtime error:" not in report and "LeakSanitizer" not in report, report
    assert proc.returncode == 0, report
    assert "0 failed expectations" in proc.stdout
    launches = int(re.search(r"sanitized \S+ driver: (\d+) kernel launches prepared", proc.stdout).group(1))
    assert launches > MIN_LAUNCHES
