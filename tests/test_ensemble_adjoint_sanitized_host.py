"""AddressSanitizer + UBSan pass over the HOST side of the per-member adjoint calls -- ``qsv_ensemble_inner``,
``qsv_ensemble_apply_diag_mul``, ``qsv_ensemble_pauli_rotations_adjoint`` and ``qsv_ensemble_diag_phase_adjoint`` (CPU only).

``tests/sanitize/ensemble_adjoint_driver.cpp`` is linked with the sanitized host objects of the library and the host-memory
stand-in for the HIP runtime, exactly as ``layer_adjoint_driver.cpp`` is: a stand-alone program with its own ``main``.  It walks
every refusal of the four calls (null pointers, a view, ``member_qubits`` out of range, qubits out of range or repeated, bad
letters, offsets and lengths, angles and gammas that are not finite, registers of different sizes and devices, the same
register twice, a diagonal of another size or device, a mode register, a change of the member size while the ensemble log holds
steps) on plain and deferring registers with ``qsv_defer_stats`` of both unchanged, ``n_terms = 0``, ``a == b`` for the inner
product, and valid calls for members of 1 .. 20 qubits as 1 .. 4096 members, whose launches must equal the plan's passes plus
one per-member sum per pass.  Kernels do not execute, and nothing is loaded into Python under a sanitizer.
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

DRIVER, MIN_LAUNCHES, TIMEOUT = "ensemble_adjoint_driver", 500, 600


def test_ensemble_adjoint_host_side_is_clean_under_asan_and_ubsan():
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
