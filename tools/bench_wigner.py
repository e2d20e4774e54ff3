#!/usr/bin/env python3
"""Time Wigner functions at the reference's grid (d = 1000 on [-20, 20]) on the notebook's 500 x 500 window of +-3 sqrt(pi):
one mode, and three modes of an MPS in one batched launch.  Prints one JSON line:

  device_ms       qsv_tensor_wigner between HIP events on the stream (upload of q / p, tables, products, epilogue)
  end_to_end_ms   the Python call, density matrices on the device included, W downloaded
  numpy_ms        the NumPy restatement (tests/wigner_reference.py) on the host, timed on a slice of the q window and
                  scaled to the whole window (numpy_columns_timed says how many columns were timed)
  library_gemm_ms the two products of the factorisation as library GEMMs on the same shapes (torch.matmul: rocBLAS /
                  hipBLASLt), R stored explicitly -- the route the fused kernels were measured against
"""
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import torch

from quantum_computations_amd import _lib
from quantum_computations_amd.cv_simulator import utils as U
from quantum_computations_amd.cv_simulator.mps import MPS
from quantum_computations_amd.cv_simulator.states import State
from wigner_reference import wigner_ket

D, WIN, REPS = 1000, 500, 10
X = np.linspace(-20, 20, D)
DX = X[1] - X[0]
Q = np.linspace(-3 * np.sqrt(np.pi), 3 * np.sqrt(np.pi), WIN)
P = Q.copy()


def device_ms(rho, q, p) -> float:
    batch = int(rho.shape[0])
    out = torch.empty((batch, len(p), len(q)), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream()
    dbl = C.POINTER(C.c_double)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run():
        _lib.call("qsv_tensor_wigner", 0, C.c_void_p(stream.cuda_stream), C.c_void_p(rho.data_ptr()), batch, D,
                  float(X[0]), float(DX), q.ctypes.data_as(dbl), len(q), p.ctypes.data_as(dbl), len(p), 0,
                  C.c_void_p(out.data_ptr()))

    run()
    times = []
    for _ in range(REPS):
        start.record(stream)
        run()
        stop.record(stream)
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return float(np.median(times))


def wall_ms(fn) -> float:
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def library_gemm_ms(batch: int) -> float:
    g = torch.randn(WIN, 2 * D - 1, dtype=torch.float64, device="cuda")
    r = torch.randn(2 * D - 1, 2 * D * batch, dtype=torch.float64, device="cuda")
    e = torch.randn(D, WIN, dtype=torch.complex128, device="cuda")

    def run():
        a = torch.view_as_complex((g @ r).view(WIN * batch, D, 2))
        return a @ e

    return wall_ms(run)


def main() -> None:
    torch.cuda.init()
    psi = State.GKP_ZERO.eval(X, 0.3)
    rho1 = torch.from_numpy(np.outer(psi, psi.conj())[None].copy()).cuda()
    mps = MPS(X, [State.GKP_ZERO.eval(X, 0.3), State.GKP_PLUS.eval(X, 0.3), State.VACUUM.eval(X)], layout="sites")
    rho3 = mps.reg.reduced_density_device([0, 1, 2])
    grid_q = X[250:750]                                       # q on the grid: the gather-only path

    flops_1 = 4.0 * WIN * D * D + 8.0 * WIN * D * WIN       # banded first product (d + 31 of 2d - 1 rows) + second
    cols = 10
    t0 = time.perf_counter()
    wigner_ket(X, psi, Q[::WIN // cols][:cols], P)
    numpy_ms = (time.perf_counter() - t0) * 1e3 * WIN / cols

    result = {
        "tool": "bench_wigner", "d": D, "window": [WIN, WIN],
        "single": {"device_ms": device_ms(rho1, Q, P), "end_to_end_ms": wall_ms(lambda: U.wigner(psi, Q, P, domain=X)),
                   "numpy_ms": numpy_ms, "numpy_columns_timed": cols, "library_gemm_ms": library_gemm_ms(1),
                   "gflop": flops_1 / 1e9},
        "single_half_grid": {"device_ms": device_ms(rho1, grid_q, P),
                             "end_to_end_ms": wall_ms(lambda: U.wigner(psi, grid_q, P, domain=X))},
        "three_modes": {"device_ms": device_ms(rho3, Q, P),
                        "end_to_end_ms": wall_ms(lambda: mps.wigner([0, 1, 2], Q, P)),
                        "library_gemm_ms": library_gemm_ms(3), "gflop": 3 * flops_1 / 1e9},
    }
    for key in ("single", "three_modes"):
        result[key]["device_tflops"] = result[key]["gflop"] / result[key]["device_ms"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
