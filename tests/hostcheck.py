"""TEST HELPER: how a stand-alone, sanitized host program of the header-only drivers is compiled, run and judged.

The drivers under tests/layout, tests/defer_plan and tests/pauli_plan include one header of quantum_computations_amd/csrc
each, are compiled with AddressSanitizer + UBSan into a program with its own main, take requests as text on stdin and
answer one line per request.  Nothing here is loaded into Python.  What the answer lines mean is each test's business.
"""
from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
CSRC = REPO / "quantum_computations_amd" / "csrc"
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", f"-I{CSRC}"]
SANITIZER_ENV = {"ASAN_OPTIONS": "detect_leaks=1:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


def compiler() -> str:
    for cand in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("no C++ compiler found for the host drivers")


def compile_driver(source: Path, out_dir: Path) -> Path:
    exe = out_dir / source.stem
    subprocess.run([compiler(), *FLAGS, str(source), "-o", str(exe)], check=True)
    return exe


def run_clean(exe: Path, stdin_text: str | None = None, timeout: float = 600) -> subprocess.CompletedProcess:
    proc = subprocess.run([str(exe)], input=stdin_text, capture_output=True, text=True, env=dict(os.environ, **SANITIZER_ENV), timeout=timeout)
    assert proc.returncode == 0 and "runtime error" not in proc.stderr and "Sanitizer" not in proc.stderr, proc.stderr[-4000:]
    return proc


def ask(exe: Path, requests: list[str], timeout: float = 600) -> list[str]:
    """One answer line per request."""
    lines = run_clean(exe, "\n".join(requests) + "\n", timeout).stdout.split("\n")[:-1]
    assert len(lines) == len(requests)
    return lines


# ---- tokens of tests/layout/layout_driver.cpp: doubles go in as round-trip decimals and come back as hexadecimal floats ------
def nums(tokens):
    return [int(t) for t in tokens]


def floats(tokens):
    return np.array([float.fromhex(t) for t in tokens])


def text(values):
    return " ".join(repr(float(v)) for v in values)
