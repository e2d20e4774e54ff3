#!/usr/bin/env python3
"""The quantum Fourier transform on one MI355X: ``DeviceState.apply_qft`` (tile passes of ``k_qft_tile`` plus the qubit
permutation) against what the library offered before, all in one process:

* the gate-by-gate spelling ``workloads.qft_ops`` (H, controlled phases, SWAPs) through the deferred queue -- the phases as
  two-qubit diagonals, which the queue takes (``apply_mcphase`` is never queued);
* the same spelling with the queue off, the phases as ``apply_mcphase`` (a quarter of the register each);
* per pass: a dense 1-qubit gate on the top qubit with the queue off, and the plain copy of the register.

Shapes: the full register with and without swaps, forward and inverse; 8 and 16 qubits on top, at the bottom and scattered.
Timing: HIP events on the register's stream around whole calls (``timer_start`` / ``timer_stop``, which also flush the
deferred queue), every shape warmed first, the contenders alternated inside one repetition loop; min / median / max over
``--reps`` repetitions.  Before anything is timed the transform is checked against its spelling at 13 qubits.

    python tools/bench_qft.py [--n 24 28] [--reps 5] [--out profiles/r19_qft.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from quantum_computations_amd import _lib  # noqa: E402
from quantum_computations_amd import workloads as W  # noqa: E402
from quantum_computations_amd.device import DeviceState  # noqa: E402
from quantum_computations_amd.dv_simulator import numpy_quantum as npq  # noqa: E402


def spelled(dev: DeviceState, ops: list[dict], queued: bool) -> None:
    for o in ops:
        if o["name"] == "H":
            dev.apply_matrix(npq.H, o["indices"])
        elif o["name"] == "SWAP":
            dev.apply_swap(*o["indices"])
        elif queued:
            dev.apply_diagonal([1.0, 1.0, 1.0, o["phase"]], o["indices"])
        else:
            dev.apply_mcphase(o["indices"], o["phase"])


def self_check() -> None:
    n = 13
    rng = np.random.default_rng(2)
    ket = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    ket /= np.linalg.norm(ket)
    for qubits in (list(range(n)), [12, 0, 7, 3, 9]):
        for inverse, swaps in ((False, True), (True, False)):
            a = DeviceState.from_numpy(ket).apply_qft(qubits, inverse=inverse, swaps=swaps)
            for queued in (True, False):
                b = DeviceState.from_numpy(ket)
                b.set_option(_lib.OPT_DEFER, 2 if queued else 0)
                spelled(b, W.qft_ops(qubits, inverse=inverse, swaps=swaps), queued)
                diff = float(np.linalg.norm(a.to_numpy() - b.to_numpy()))
                assert diff < 1e-13, (qubits, inverse, swaps, queued, diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[24, 28])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/r19_qft.json")
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    self_check()
    result = {"tool": "tools/bench_qft.py", "reps": args.reps,
              "timing": "HIP events around whole calls on the register's stream; min / median / max; contenders alternated per repetition",
              "traffic": "not measured: no counter run was made; a pass is one read and one write of the register", "sizes": []}
    for n in args.n:
        dev = DeviceState.random(n, seed=1)
        twin = DeviceState.zeros(n)
        reg_gb = 16 * (1 << n) / 1e9
        u2 = W.haar_unitary(2, np.random.default_rng(7))

        def timed(fn):
            dev.timer_start()
            fn()
            return dev.timer_stop()

        def stats(samples):
            return {"min_ms": round(min(samples), 4), "median_ms": round(statistics.median(samples), 4), "max_ms": round(max(samples), 4)}

        def contest(**contenders):
            for fn in contenders.values():
                fn()
            dev.sync()
            samples = {name: [] for name in contenders}
            for _ in range(args.reps):
                for name, fn in contenders.items():
                    samples[name].append(timed(fn))
            return {name: stats(values) for name, values in samples.items()}

        def defer(mode: int):
            dev.set_option(_lib.OPT_DEFER, mode)

        def dense_1q():
            defer(0)
            dev.apply_matrix(u2, [0])

        base = contest(dense_1q=dense_1q, copy=lambda: dev.copy_into(twin))
        size = {"n_qubits": n, "register_GB": round(reg_gb, 4), "bytes_per_pass": 2 * 16 * (1 << n), "per_pass_baselines": base, "shapes": []}
        print(f"n={n}: dense 1-qubit gate {base['dense_1q']['median_ms']:.3f} ms, copy {base['copy']['median_ms']:.3f} ms", flush=True)
        scattered = [int(q) for q in np.linspace(0, n - 1, 16).round()]
        shapes = [("full", list(range(n)), False, True), ("full, no swaps", list(range(n)), False, False),
                  ("full, inverse", list(range(n)), True, True), ("full, inverse, no swaps", list(range(n)), True, False)]
        for m in (8, 16):
            shapes += [(f"m={m} top", list(range(m)), False, True), (f"m={m} bottom", list(range(n - m, n)), False, True),
                       (f"m={m} scattered", scattered[::16 // m][:m], False, True)]
        for label, qubits, inverse, swaps in shapes:
            ops = W.qft_ops(qubits, inverse=inverse, swaps=swaps)
            passes = dev._apply_qft(qubits, inverse=inverse, swaps=swaps)

            def spelled_with(mode: int):
                defer(mode)
                spelled(dev, ops, queued=mode != 0)

            got = contest(qft=lambda: dev.apply_qft(qubits, inverse=inverse, swaps=swaps), spelled_deferred=lambda: spelled_with(2),
                          spelled_per_gate=lambda: spelled_with(0))
            defer(0)
            t = got["qft"]["median_ms"]
            row = {"shape": label, "qubits": qubits, "inverse": inverse, "swaps": swaps, "launches": passes,
                   "tile_passes": passes - (1 if swaps and len(qubits) >= 2 else 0), "spelling_gates": len(ops), **got,
                   "ms_per_launch": round(t / passes, 4), "launch_over_dense_1q": round(t / passes / base["dense_1q"]["median_ms"], 3),
                   "launch_over_copy": round(t / passes / base["copy"]["median_ms"], 3),
                   "deferred_over_qft": round(got["spelled_deferred"]["median_ms"] / t, 2),
                   "per_gate_over_qft": round(got["spelled_per_gate"]["median_ms"] / t, 2)}
            size["shapes"].append(row)
            print(f"n={n} {label}: qft {t:.3f} ms in {passes} launches, spelled through the queue {got['spelled_deferred']['median_ms']:.2f} ms, "
                  f"gate by gate {got['spelled_per_gate']['median_ms']:.2f} ms ({len(ops)} gates)", flush=True)
        result["sizes"].append(size)
        dev.close()
        twin.close()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
