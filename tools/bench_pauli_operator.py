#!/usr/bin/env python3
"""Pauli sums as operators on one MI355X: ``apply_pauli_sum`` (``k_pauli_sum_apply_group``), ``transition_pauli_sum``
(``k_pauli_transition_group``) and the adjoint gradient ``energy_and_gradient`` (``k_pauli_adjoint_group``), each against
a yardstick from the same process:

(a) ``apply_pauli_sum`` of ``heisenberg_chain_terms(n)`` and ``ising_terms(n, 1.0)``: passes, ms per call and per pass, and
    single passes with and without reading the old destination (the FIRST pass of an overwriting call moves two register
    streams, every other pass three).  Yardstick: ``copy_into`` (two streams); a three-stream pass is compared with 1.5 x
    the copy time.
(b) ``transition_pauli_sum`` of the same lists between two registers.  Yardstick: ``inner`` (two read streams).
(c) ``energy_and_gradient`` for the first-order Trotter list of the Heisenberg chain (3 (n - 1) angles, n - 1 passes) and
    for 16 random weight-8 strings, whole calls and their parts (forward rotations, H psi, <psi|H psi>, the backward
    walk with a destination that already exists).  Contender: the parameter-shift rule through the calls the library had
    before -- per angle and sign: rewind the register by the inverse rotations (no upload), run the shifted list, read
    ``expect_pauli_sum``.  One such evaluation is timed for ``--reps`` different angles and multiplied by 2K (every one
    of the 2K evaluations launches the same passes); the whole loop is also run once where that takes under
    ``--full-loop-seconds``, as a check of the product.

Timing: HIP events on a register's stream around whole calls (``timer_start`` / ``timer_stop``), every shape warmed
first, the contenders alternated inside one repetition loop; medians over ``--reps`` repetitions, minima alongside.
Before anything is timed the gradient is checked against the parameter-shift rule at 10 qubits.

    python tools/bench_pauli_operator.py [--n 28] [--reps 9] [--out profiles/r11_pauli_operator.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from quantum_computations_amd import _lib  # noqa: E402
from quantum_computations_amd import workloads as W  # noqa: E402
from quantum_computations_amd.device import DeviceState, _flat_terms  # noqa: E402
from quantum_computations_amd.dv_simulator import numpy_quantum as npq  # noqa: E402


def apply_passes(dst, src, terms, accumulate=False) -> int:
    count, offsets, qubits, letters, cbuf = _flat_terms(terms)
    passes = C.c_uint64()
    _lib.call("qsv_apply_pauli_sum", dst._h, src._h, count, offsets, qubits, letters, cbuf.ctypes.data_as(C.POINTER(C.c_double)),
              int(accumulate), C.byref(passes))
    return passes.value


def rotation_passes(dev, rotations) -> int:
    count, offsets, qubits, letters, cbuf = _flat_terms(rotations)
    thetas = np.ascontiguousarray(cbuf.view(np.complex128).real)
    passes = C.c_uint64()
    _lib.call("qsv_apply_pauli_rotations", dev._h, count, offsets, qubits, letters, thetas.ctypes.data_as(C.POINTER(C.c_double)),
              C.byref(passes))
    return passes.value


def shifted(rotations, k, sign):
    theta, letters, qubits = rotations[k]
    return rotations[:k] + [(theta + sign * np.pi / 2, letters, qubits)] + rotations[k + 1:]


def inverse(rotations):
    return [(-theta, letters, qubits) for theta, letters, qubits in rotations[::-1]]


def shift_evaluation(dev, rotations, terms, k, sign) -> float:
    """E(theta_k + sign pi/2) from a register that holds psi0, which it holds again afterwards (up to rounding)."""
    moved = shifted(rotations, k, sign)
    dev.apply_pauli_rotations(moved)
    energy = dev.expect_pauli_sum(terms).real
    dev.apply_pauli_rotations(inverse(moved))
    return energy


def parameter_shift(dev, rotations, terms) -> np.ndarray:
    return np.array([0.5 * (shift_evaluation(dev, rotations, terms, k, +1) - shift_evaluation(dev, rotations, terms, k, -1))
                     for k in range(len(rotations))])


def random_weight8(n, count, rng):
    return [(float(rng.uniform(-3, 3)), "".join(rng.choice(list("XYZ"), size=8)), [int(q) for q in rng.permutation(n)[:8]])
            for _ in range(count)]


def self_check():
    n = 10
    rng = np.random.default_rng(3)
    ket = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    ket /= np.linalg.norm(ket)
    terms = W.heisenberg_chain_terms(n)
    for rotations in (npq.trotter_rotations(npq.PauliSum(n, terms), 0.3), random_weight8(n, 16, rng)):
        dev = DeviceState.from_numpy(ket)
        _, grad = dev.energy_and_gradient(rotations, terms)
        diff = float(np.max(np.abs(grad - parameter_shift(DeviceState.from_numpy(ket), rotations, terms))))
        assert diff < 1e-11, diff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--full-loop-seconds", type=float, default=40.0)
    ap.add_argument("--out", default="profiles/r11_pauli_operator.json")
    args = ap.parse_args()
    n, reps = args.n, args.reps
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    self_check()
    psi, other, out = DeviceState.random(n, seed=1), DeviceState.random(n, seed=2), DeviceState.zeros(n)
    reg_gb = 16 * (1 << n) / 1e9
    rng = np.random.default_rng(7)

    def timed(clock, fn):
        clock.timer_start()
        fn()
        return clock.timer_stop()

    def stats(samples):
        return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4)}

    def contest(clock, **contenders):
        """Warm every contender once, then alternate them inside one repetition loop; ``clock``: the register whose
        stream carries the launches (a contender given as ``(register, fn)`` brings its own)."""
        contenders = {name: entry if isinstance(entry, tuple) else (clock, entry) for name, entry in contenders.items()}
        for _, fn in contenders.values():
            fn()
        for dev in (psi, other, out):
            dev.sync()
        samples = {name: [] for name in contenders}
        for _ in range(reps):
            for name, (own_clock, fn) in contenders.items():
                samples[name].append(timed(own_clock, fn))
        return {name: stats(values) for name, values in samples.items()}

    result = {"tool": "tools/bench_pauli_operator.py", "n_qubits": n, "reps": reps, "register_GB": round(reg_gb, 4),
              "timing": "HIP events around whole calls on the stream that carries the launches; medians; contenders alternated per repetition",
              "traffic": "not measured: no counter run was made; stream counts are those of the kernels' loads and stores"}
    lists = {"heisenberg_chain": W.heisenberg_chain_terms(n), "ising_chain": W.ising_terms(n, 1.0)}

    # ---- (a) apply ------------------------------------------------------------------------------------------------------------
    result["apply"] = []
    for name, terms in lists.items():
        passes = apply_passes(out, psi, terms)
        got = contest(out, apply=lambda: psi.apply_pauli_sum(terms, out=out), accumulate=lambda: psi.apply_pauli_sum(terms, out=out, accumulate=True),
                      copy=lambda: psi.copy_into(out))
        copy_ms = got["copy"]["median_ms"]
        row = {"terms_list": name, "terms": len(terms), "passes": passes, **got,
               "ms_per_pass": round(got["apply"]["median_ms"] / passes, 4),
               "accumulate_ms_per_pass": round(got["accumulate"]["median_ms"] / passes, 4),
               "accumulate_pass_over_1p5_copies": round(got["accumulate"]["median_ms"] / passes / (1.5 * copy_ms), 3)}
        result["apply"].append(row)
        print(f"(a) {name}: {len(terms)} terms in {passes} passes: {got['apply']['median_ms']:.2f} ms ({row['ms_per_pass']:.3f} per pass), "
              f"accumulating {got['accumulate']['median_ms']:.2f} ms, copy {copy_ms:.3f} ms", flush=True)
    result["apply_single_pass"] = []
    singles = {"pair pass, 2 terms (XX, YY on a bond)": [(1.0, "XX", [3, 4]), (1.0, "YY", [3, 4])],
               "pair pass, 8 terms": [(1.0 + t, "XY"[t % 2] + "X" + "Z" * (t % 3), [3, 4] + [7 + 2 * j for j in range(t % 3)]) for t in range(8)],
               "diagonal pass, 8 terms": [(1.0 + t, "ZZ", [t, t + 1]) for t in range(8)]}
    for name, terms in singles.items():
        assert apply_passes(out, psi, terms) == 1
        got = contest(out, first=lambda: psi.apply_pauli_sum(terms, out=out), accumulate=lambda: psi.apply_pauli_sum(terms, out=out, accumulate=True),
                      copy=lambda: psi.copy_into(out))
        copy_ms = got["copy"]["median_ms"]
        row = {"pass": name, **got, "first_over_copy": round(got["first"]["median_ms"] / copy_ms, 3),
               "accumulate_over_1p5_copies": round(got["accumulate"]["median_ms"] / (1.5 * copy_ms), 3),
               "first_GB_per_s": round(2 * reg_gb / (got["first"]["median_ms"] * 1e-3), 1),
               "accumulate_GB_per_s": round(3 * reg_gb / (got["accumulate"]["median_ms"] * 1e-3), 1)}
        result["apply_single_pass"].append(row)
        print(f"(a) {name}: FIRST {got['first']['median_ms']:.3f} ms, accumulating {got['accumulate']['median_ms']:.3f} ms, copy {copy_ms:.3f} ms", flush=True)

    # ---- (b) transition ---------------------------------------------------------------------------------------------------------
    result["transition"] = []
    for name, terms in lists.items():
        passes = apply_passes(out, psi, terms)                                  # the same grouping
        got = contest(psi, transition=lambda: psi.transition_pauli_sum(terms, other), expect=lambda: psi.expect_pauli_sum(terms),
                      inner=lambda: psi.inner(other))
        row = {"terms_list": name, "terms": len(terms), "passes": passes, **got, "ms_per_pass": round(got["transition"]["median_ms"] / passes, 4),
               "pass_over_inner": round(got["transition"]["median_ms"] / passes / got["inner"]["median_ms"], 3)}
        result["transition"].append(row)
        print(f"(b) {name}: {passes} passes: transition {got['transition']['median_ms']:.2f} ms ({row['ms_per_pass']:.3f} per pass), "
              f"expect_pauli_sum {got['expect']['median_ms']:.2f} ms, inner {got['inner']['median_ms']:.3f} ms", flush=True)

    # ---- (c) adjoint gradient against parameter shift --------------------------------------------------------------------------------
    result["gradient"] = []
    terms = lists["heisenberg_chain"]
    workloads = {"heisenberg_trotter_step": npq.trotter_rotations(npq.PauliSum(n, terms), 0.05), "random_weight_8_strings": random_weight8(n, 16, rng)}
    for name, rotations in workloads.items():
        K = len(rotations)
        passes = rotation_passes(psi, rotations)
        psi.apply_pauli_rotations(inverse(rotations))
        apply_count = apply_passes(out, psi, terms)
        ks = [int(k) for k in np.linspace(0, K - 1, reps).round()]
        order = iter(ks + ks)                                                  # the warm-up call takes one as well

        def one_shift():
            shift_evaluation(psi, rotations, terms, next(order), +1)

        def walk():
            psi.pauli_rotations_adjoint(rotations, out)

        got = contest(psi, energy_and_gradient=lambda: psi.energy_and_gradient(rotations, terms), shift_evaluation=one_shift,
                      forward=lambda: psi.apply_pauli_rotations(rotations), walk=walk,
                      h_psi=(out, lambda: psi.apply_pauli_sum(terms, out=out)), inner=lambda: psi.inner(out))
        adjoint_ms, shift_ms = got["energy_and_gradient"]["median_ms"], 2 * K * got["shift_evaluation"]["median_ms"]
        row = {"workload": name, "angles": K, "rotation_passes": passes, "hamiltonian_terms": len(terms), "apply_passes": apply_count, **got,
               "parameter_shift_ms": round(shift_ms, 2), "parameter_shift_is": "2 K x the median of one shifted evaluation (rewind, shifted list, expect_pauli_sum)",
               "parameter_shift_over_adjoint": round(shift_ms / adjoint_ms, 2),
               "walk_ms_per_pass": round(got["walk"]["median_ms"] / passes, 4), "forward_ms_per_pass": round(got["forward"]["median_ms"] / passes, 4),
               "walk_pass_over_forward_pass": round(got["walk"]["median_ms"] / got["forward"]["median_ms"], 3),
               "parts_ms": round(sum(got[part]["median_ms"] for part in ("forward", "h_psi", "inner", "walk")), 3)}
        if shift_ms * 1e-3 < args.full_loop_seconds:
            psi.sync()
            start = time.perf_counter()
            parameter_shift(psi, rotations, terms)
            psi.sync()
            row["parameter_shift_full_loop_once_ms"] = round((time.perf_counter() - start) * 1e3, 1)
        result["gradient"].append(row)
        print(f"(c) {name}: {K} angles in {passes} passes: energy_and_gradient {adjoint_ms:.1f} ms, parameter shift {shift_ms:.0f} ms "
              f"({row['parameter_shift_over_adjoint']:.1f} x), walk / forward per pass {row['walk_pass_over_forward_pass']:.2f}"
              + (f", full loop once {row['parameter_shift_full_loop_once_ms']:.0f} ms (host clock)" if "parameter_shift_full_loop_once_ms" in row else ""), flush=True)

    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {path}")


if __name__ == "__main__":
    main()
