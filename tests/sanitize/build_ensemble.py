#!/usr/bin/env python3
"""TEST INFRASTRUCTURE: the AddressSanitizer + UBSan host binary of the driver of the trajectory-ensemble entry points.

    python tests/sanitize/build_ensemble.py      # -> tests/sanitize/_build/qsv_ensemble_san

``build.py`` compiles the library's HIP sources host-only with the sanitizers and ``hip_stub.cpp``; this compiles
``qsv_channel.hip`` and ``qsv_ensemble.hip`` the same way and links all of them with ``ensemble_driver.cpp`` in place of
``driver.cpp``.  Stand-alone program with its own ``main``: nothing here is loaded into Python.
"""
from __future__ import annotations

import re
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import build as base  # noqa: E402

EXTRA_SOURCES = ["qsv_channel.hip", "qsv_ensemble.hip"]
EXTRA_HEADERS = [base.CSRC / "qsv_channel_layout.h", base.CSRC / "qsv_ensemble_layout.h", base.CSRC / "qsv_pauli_plan.h",
                 base.CSRC / "qsv_pauli_rotation_plan.h", base.CSRC / "qsv_internal.h", base.CSRC / "qsv_device.h",
                 base.CSRC / "qsv_readout_layout.h", base.CSRC / "qsv_layout.h", base.REPO / "include" / "qsv.h"]


def build(verbose: bool = False) -> Path:
    def run(cmd):
        if verbose:
            print(" ".join(map(str, cmd)), flush=True)
        subprocess.run(cmd, check=True)

    base.build(verbose)
    objs = [base.OUT / (name + ".o") for name in base.SOURCES] + [base.OUT / "hip_stub.cpp.o"]
    for name in EXTRA_SOURCES:
        extra = base.OUT / (name + ".o")
        if base.stale(extra, [base.CSRC / name] + EXTRA_HEADERS):
            run([base.CLANG, "-x", "hip", "--offload-host-only", "--rocm-path=/opt/rocm", "-nogpulib", "-std=c++17", *base.SAN, *base.INC,
                 "-c", base.CSRC / name, "-o", extra])
        objs.append(extra)
    driver = base.OUT / "ensemble_driver.cpp.o"
    if base.stale(driver, [HERE / "ensemble_driver.cpp", base.REPO / "include" / "qsv.h"]):
        run([base.CLANG, "-std=c++17", *base.SAN, *base.INC, "-c", HERE / "ensemble_driver.cpp", "-o", driver])
    # the host stubs reference the embedded device image of each translation unit; there is none in a host-only build
    fat = base.OUT / "ensemble_fatbins.c"
    names = set()
    for obj in objs:
        names |= set(re.findall(r"U (__hip_fatbin_\w+)", subprocess.run(["nm", str(obj)], capture_output=True, text=True).stdout))
    text = "".join(f"const char {n}[8] = {{0}};\n" for n in sorted(names))
    if not fat.exists() or fat.read_text() != text:
        fat.write_text(text)
    exe = base.OUT / "qsv_ensemble_san"
    if base.stale(exe, objs + [driver, fat]):
        # the stand-in runtime has one device; the driver answers the library's two device queries itself (--wrap) so that it
        # can put a register on a second one and walk the "channel on another device" refusal
        run([base.CLANG, *base.SAN, "-Wl,--wrap=hipGetDeviceCount", "-Wl,--wrap=hipSetDevice", "-x", "c", fat, "-x", "none", *objs, driver,
             "-ldl", "-lpthread", "-o", exe])
    return exe


if __name__ == "__main__":
    print(build(verbose=True))
