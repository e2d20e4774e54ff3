"""AddressSanitizer + UBSan pass over the HOST side of qsv_lincomb and qsv_inner_many (CPU only).

``tests/sanitize/build_krylov.py`` links the host-only, sanitized objects of the library and the host-memory stand-in for
the HIP runtime (``tests/sanitize/hip_stub.cpp``) with ``tests/sanitize/krylov_driver.cpp``, a stand-alone program that
walks both entry points: null handles and arrays, a null entry inside an array, negative counts, the destination among
the sources, views whose windows meet the destination's, registers of different sizes, a destination that is too small,
mode registers -- each refused before any launch and with every deferred queue left alone -- and then valid calls with
0 to 40 operands on registers of 1 to 18 qubits and on views (repeated and overlapping sources, x_k = y), with and without
beta and the norm: the split into passes, the argument builders, the slices of the scratch buffer and one launch per
pass, counted against ceil(operands / 8).  Kernels do not execute (there is no device code in this build).
"""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "sanitize"))


def test_krylov_host_side_is_clean_under_asan_and_ubsan():
    import build_krylov as san_build

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
    launches = int(proc.stdout.split("sanitized Krylov driver: ")[1].split()[0])
    assert launches > 1000          # the driver really went through the launch paths
