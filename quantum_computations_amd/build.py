"""Build libqsv.so (HIP, gfx950 only) in-tree with hipcc.  ``python -m quantum_computations_amd.build``."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
REPO_ROOT = PKG_DIR.parent
CSRC = PKG_DIR / "csrc"
LIB_PATH = PKG_DIR / "libqsv.so"
SOURCES = ["qsv_api.hip", "qsv_gate12.hip", "qsv_gatek.hip", "qsv_sequence.hip", "qsv_pass.hip", "qsv_state.hip", "qsv_readout.hip", "qsv_pauli.hip", "qsv_qft.hip", "qsv_layer.hip", "qsv_layer_adjoint.hip", "qsv_arith.hip", "qsv_krylov.hip", "qsv_diagonal.hip", "qsv_channel.hip", "qsv_ensemble.hip", "qsv_sweep.hip", "qsv_ensemble_adjoint.hip", "qsv_subsystem.hip", "qsv_qudit.hip", "qsv_gemm.hip", "qsv_decomp.hip", "qsv_rsvd.hip", "qsv_panel.hip", "qsv_skinny.hip",
           "qsv_circuit.hip", "qsv_phase_space.hip", "qsv_sampling.hip", "qsv_canonical.hip"]
HEADERS = [CSRC / "qsv_internal.h", CSRC / "qsv_device.h", CSRC / "qsv_linalg.h", CSRC / "qsv_jacobi.h", CSRC / "qsv_split_rules.h", CSRC / "qsv_plan.h", CSRC / "qsv_layout.h",
           CSRC / "qsv_readout_layout.h", CSRC / "qsv_pauli_plan.h", CSRC / "qsv_pauli_rotation_plan.h", CSRC / "qsv_qft_plan.h", CSRC / "qsv_layer_plan.h", CSRC / "qsv_layer_item.h", CSRC / "qsv_arith_layout.h", CSRC / "qsv_krylov_layout.h", CSRC / "qsv_diagonal_layout.h", CSRC / "qsv_channel_layout.h", CSRC / "qsv_ensemble_layout.h", CSRC / "qsv_ensemble_control_layout.h", CSRC / "qsv_sweep_layout.h", CSRC / "qsv_pauli_rotate_item.h",
           CSRC / "qsv_diagonal_device.h", CSRC / "qsv_ensemble_device.h", CSRC / "qsv_subsystem_layout.h", REPO_ROOT / "include" / "qsv.h"]
ARCH = "gfx950"
# Leave regions whose branches are all wave-uniform as they are.  The structurizer otherwise rewrites k_pass_tile's gate
# switch (qsv_pass.hip) into a chain of guarded blocks that keeps a second copy of the 16 amplitudes of a thread (64
# more VGPRs, 32 v_mov_b64 per gate).  The option changes control flow only, never arithmetic.
# The other gate files (qsv_gate12, qsv_gatek, qsv_sequence, qsv_state) take it because the one file they were split from
# did: their kernels stay the device code that was measured.  qsv_readout.hip and qsv_pauli.hip take the option too.  Compiled with and without it (tools/device_code_diff.py), these
# of their kernels come out differently --
#   qsv_readout.hip: k_chunk_sums, k_sample_in_chunk, k_permute_s<1 / 2 / 4>, k_rdm<1 / 2 / 4>, k_rdm_tile<1 / 2 / 4>,
#                    k_rdm_small (12 of 38);
#   qsv_pauli.hip:   k_pauli_rotate_group<1 / 2 / 4 / 8, false, *> (8 of 25) --
# every measurement on record of them was taken with it, and none without.  qsv_sweep.hip takes it because its rotation kernel
# is k_pauli_rotate_group's item body on member-local items.  qsv_layer.hip takes it for k_pass_tile's own reason:
# k_layer_tile's stage switch holds 16 amplitudes per thread, and without the option the compiler's remarks show 155 / 170
# VGPRs (shared / per-member matrices) against 104 / 116 with it -- the second copy of the amplitudes.
# qsv_layer_adjoint.hip takes it for the same reason: k_layer_adjoint_tile's stage switch holds 16 amplitudes of each of two
# registers per thread.  qsv_ensemble_adjoint.hip takes it because its walk kernel is
# k_pauli_adjoint_group's item body (qsv_pauli.hip) on member-local items.
_SKIP_UNIFORM = ["-mllvm", "-structurizecfg-skip-uniform-regions"]
EXTRA_FLAGS = {name: _SKIP_UNIFORM for name in ("qsv_gate12.hip", "qsv_gatek.hip", "qsv_sequence.hip", "qsv_pass.hip", "qsv_state.hip",
                                                "qsv_readout.hip", "qsv_pauli.hip", "qsv_sweep.hip", "qsv_layer.hip", "qsv_layer_adjoint.hip", "qsv_ensemble_adjoint.hip")}


def check_extra_flags() -> None:
    """The options above are LLVM developer options: fail with a plain message where the compiler does not know one,
    instead of in the middle of a long compile (or, worse, building the slower kernel by leaving it out)."""
    probe = subprocess.run([hipcc(), f"--offload-arch={ARCH}", *_SKIP_UNIFORM, "--cuda-device-only", "-x", "hip", "-c", "-",
                            "-o", os.devnull], input="__global__ void k() {}\n", capture_output=True, text=True)
    if probe.returncode != 0:
        raise RuntimeError(f"{hipcc()} does not accept {' '.join(_SKIP_UNIFORM)} (needed for {', '.join(EXTRA_FLAGS)}, see "
                           "DESIGN.md section 10):\n" + probe.stderr[-2000:])


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found: libqsv.so needs the ROCm toolchain (there is no CPU fallback)")


def _stale(target: Path, deps: list[Path]) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(d.stat().st_mtime > t for d in deps)


def build_lib(force: bool = False, verbose: bool = False) -> Path:
    """Compile every HIP source for gfx950 and link libqsv.so next to the package."""
    check_extra_flags()
    objs = []
    build_dir = PKG_DIR / "build"
    build_dir.mkdir(exist_ok=True)
    flags = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
             f"-I{REPO_ROOT / 'include'}", f"-I{CSRC}"]
    for name in SOURCES:
        src = CSRC / name
        obj = build_dir / (name + ".o")
        if force or _stale(obj, [src] + HEADERS):
            cmd = [hipcc(), *flags, *EXTRA_FLAGS.get(name, []), "-c", str(src), "-o", str(obj)]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
        objs.append(obj)
    if force or _stale(LIB_PATH, objs):
        cmd = [hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(LIB_PATH), *map(str, objs), "-ldl"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return LIB_PATH


if __name__ == "__main__":
    path = build_lib(force="--force" in sys.argv, verbose=True)
    print(path)
