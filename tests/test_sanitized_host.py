"""AddressSanitizer + UBSan pass over the HOST side of libqsv (CPU only).

``tests/sanitize/build.py`` compiles every HIP source of the library host-only with ``-fsanitize=address,undefined`` and
links that one set of objects, with a host-memory stand-in for the HIP runtime (``tests/sanitize/hip_stub.cpp``), with each
driver of ``tests/sanitize``: a stand-alone program with its own ``main`` that walks the validation branches and the launch
preparation of one group of C-ABI entry points (the head comment of each ``.cpp`` says which).  Kernels do not execute
(there is no device code in this build), and nothing is loaded into Python under a sanitizer.
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

# driver, launches it must exceed (it really went through the launch paths), seconds
DRIVERS = [
    ("driver", 5000, 900),
    ("pauli_sum_driver", 100, 600),
    ("pauli_rotation_driver", 1000, 600),
    ("pauli_operator_driver", 1000, 600),
    ("krylov_driver", 1000, 600),
    ("diagonal_driver", 1000, 600),
    ("channel_driver", 1000, 600),
    ("ensemble_driver", 1000, 600),
    ("subsystem_driver", 500, 600),
]


@pytest.mark.parametrize("driver,min_launches,timeout", DRIVERS, ids=["host" if d == "driver" else d.replace("_driver", "") for d, _, _ in DRIVERS])
def test_host_side_is_clean_under_asan_and_ubsan(driver, min_launches, timeout):
    import build as san_build

    if not san_build.CLANG.exists():
        pytest.skip("ROCm clang not installed")
    exe = san_build.build(driver)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout, env=env)
    report = proc.stdout[-2000:] + proc.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in report and "runtime error:" not in report and "LeakSanitizer" not in report, report
    assert proc.returncode == 0, report
    assert "0 failed expectations" in proc.stdout
    launches = int(re.search(r"sanitized \S+ driver: (\d+) kernel launches prepared", proc.stdout).group(1))
    assert launches > min_launches
