#!/usr/bin/env python3
"""Per-member adjoint gradients on one MI355X, everything in one process.

* points per second with ``batch = 256`` at 12, 16 and 20 qubits: ``sweep.energies_and_gradients`` on one Trotter step of the
  open Heisenberg chain (energy of the chain) against the loop of ``DeviceState.energy_and_gradient`` on a fresh register per
  point and against ``sweep.parameter_shift`` per point; ``qaoa.energies_and_gradients`` (3-regular MaxCut, ``p = 4``) against
  the loop of ``qaoa.energy_and_gradient``.  The loops are the baselines and are never the code under test.
* time per pass on two registers of 2^28 amplitudes read as members of 16 and of 20 qubits: one walk pass (pivot on the
  member's top bit, pivot on bit 0, diagonal; one rotation and eight in the pass) against ``k_pauli_adjoint_group`` with the
  same string on the same registers; the cost-phase walk against ``qsv_diag_phase_adjoint`` with a full-size diagonal; ``inner``
  against ``qsv_inner``.  Each row carries the ratio and the run-to-run spread of its yardstick from the same call.

Timing: host clock around whole calls that end in a synchronisation; every contender warmed first, contenders alternated
inside one repetition loop; medians over ``--reps`` repetitions, minima and maxima alongside.  Every section has a time limit
of its own: a case that would start after it is recorded as "not measured", and nothing is ever tried twice.

    python tools/bench_ensemble_adjoint.py [--reps 9] [--out profiles/r24_ensemble_adjoint.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from quantum_computations_amd import DiagonalOperator, _lib, qaoa, sweep  # noqa: E402
from quantum_computations_amd import workloads as W  # noqa: E402
from quantum_computations_amd.device import DeviceState  # noqa: E402
from quantum_computations_amd.ensemble import Ensemble  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--total", type=int, default=28, help="qubits of the registers of the per-pass measurements: n + b")
    ap.add_argument("--sizes", type=int, nargs="*", default=[12, 16, 20])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--serial-points", type=int, default=16)
    ap.add_argument("--shift-points", type=int, default=2)
    ap.add_argument("--member-sizes", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--section-seconds", type=float, default=150.0, help="time limit of each of the three sections")
    ap.add_argument("--out", default="profiles/r24_ensemble_adjoint.json")
    args = ap.parse_args()
    reps = args.reps
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    result = {"tool": "tools/bench_ensemble_adjoint.py", "reps": reps, "batch": args.batch,
              "timing": "host clock around whole calls that end in a synchronisation; medians; contenders alternated per repetition",
              "rotation_points": {}, "qaoa_points": {}, "passes": {}}

    def save():
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1) + "\n")
        print(f"wrote {path}", flush=True)

    def stats(samples):
        return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4)}

    def contest(sync, **contenders):
        for fn in contenders.values():
            fn()
        sync()
        samples = {name: [] for name in contenders}
        for _ in range(reps):
            for name, fn in contenders.items():
                start = time.perf_counter()
                fn()
                sync()
                samples[name].append((time.perf_counter() - start) * 1e3)
        return {name: stats(values) for name, values in samples.items()}

    def rates(got, points):
        serial_rate = points["serial"] / (got["serial"]["median_ms"] * 1e-3)
        row = {}
        for name, s in got.items():
            rate = points[name] / (s["median_ms"] * 1e-3)
            row[name] = {**s, "points": points[name], "points_per_s": round(rate, 1),
                         "points_per_s_range": [round(points[name] / (s["max_ms"] * 1e-3), 1), round(points[name] / (s["min_ms"] * 1e-3), 1)],
                         "over_serial": round(rate / serial_rate, 2)}
        return row

    rng = np.random.default_rng(0)
    batch, serial, shifted = args.batch, args.serial_points, args.shift_points

    # ---- points per second: one Trotter step of the Heisenberg chain, energy and gradient ------------------------------------------
    deadline = time.perf_counter() + args.section_seconds
    for n in args.sizes:
        if time.perf_counter() > deadline:
            result["rotation_points"][f"n{n}"] = "not measured"
            continue
        terms = W.heisenberg_chain_terms(n)
        rotations = [(0.0, letters, qubits) for _, letters, qubits in terms]
        thetas = rng.uniform(-0.3, 0.3, (batch, len(rotations)))

        def serial_loop():
            for row in thetas[:serial]:
                state = DeviceState.zeros(n)
                state.energy_and_gradient([(theta, letters, qubits) for theta, (_, letters, qubits) in zip(row, rotations)], terms)
                state.close()

        def shift_loop():
            for row in thetas[:shifted]:
                sweep.parameter_shift(rotations, row, terms, batch=batch)

        got = contest(lambda: None, serial=serial_loop, parameter_shift=shift_loop,
                      batched=lambda: sweep.energies_and_gradients(rotations, thetas, terms, batch=batch))
        row = rates(got, {"serial": serial, "parameter_shift": shifted, "batched": batch})
        row["rotations"] = len(rotations)
        row["whole_call"] = "register allocation and read-out included on all sides"
        result["rotation_points"][f"n{n}"] = row
        print(f"gradients n={n}: serial {row['serial']['points_per_s']:.1f} points/s, parameter shift {row['parameter_shift']['points_per_s']:.1f}, "
              f"batch {batch}: {row['batched']['points_per_s']:.1f} ({row['batched']['over_serial']:.2f} x serial)", flush=True)
        save()

    # ---- points per second: QAOA, energy and gradient ----------------------------------------------------------------------------
    deadline = time.perf_counter() + args.section_seconds
    for n in args.sizes:
        if time.perf_counter() > deadline:
            result["qaoa_points"][f"n{n}"] = "not measured"
            continue
        op = DiagonalOperator.from_terms(n, W.maxcut_terms(n, W.ring_chord_edges(n)))
        gammas, betas = rng.uniform(-0.6, 0.6, (batch, args.layers)), rng.uniform(-0.6, 0.6, (batch, args.layers))

        def serial_loop():
            for g, b in zip(gammas[:serial], betas[:serial]):
                qaoa.energy_and_gradient(op, g, b)

        got = contest(lambda: None, serial=serial_loop, batched=lambda: qaoa.energies_and_gradients(op, gammas, betas, batch=batch))
        row = rates(got, {"serial": serial, "batched": batch})
        row["layers"] = args.layers
        row["whole_call"] = "register allocation, |+>^n and read-out included on both sides"
        result["qaoa_points"][f"n{n}"] = row
        print(f"qaoa gradients n={n}: serial {row['serial']['points_per_s']:.1f} points/s, batch {batch}: {row['batched']['points_per_s']:.1f} "
              f"({row['batched']['over_serial']:.2f} x)", flush=True)
        op.close()
        save()

    # ---- time per pass on two large registers ----------------------------------------------------------------------------------
    deadline = time.perf_counter() + args.section_seconds
    total = args.total
    reg_gb = 16 * (1 << total) / 1e9
    result["register_qubits"] = total
    result["register_GB"] = round(reg_gb, 4)
    psi, lam = DeviceState.random(total, seed=1), DeviceState.random(total, seed=2)
    full = DiagonalOperator.from_terms(total, [(0.5, "ZZ", [0, total - 1]), (0.25, "Z", [total // 2])])

    def compare(row, name, per_member, yardstick, streams):
        if time.perf_counter() > deadline:
            row[name] = "not measured"
            return
        got = contest(lambda: None, per_member=per_member, yardstick=yardstick)     # every call here ends in its own synchronisation
        mine, ref = got["per_member"], got["yardstick"]
        row[name] = {**got, "ratio": round(mine["median_ms"] / ref["median_ms"], 3),
                     "yardstick_spread": round((ref["max_ms"] - ref["min_ms"]) / ref["median_ms"], 3),
                     "per_member_GB_per_s": round(streams * reg_gb / (mine["median_ms"] * 1e-3), 1)}
        print(f"{name}: per member {mine['median_ms']:.3f} ms, yardstick {ref['median_ms']:.3f} ms, ratio {row[name]['ratio']:.3f} "
              f"(yardstick spread {row[name]['yardstick_spread']:.3f})", flush=True)

    for n in args.member_sizes:
        if n > total:
            continue
        ens, ens_lam = Ensemble(psi, n), Ensemble(lam, n)
        shift = total - n
        row = {}
        for label, letter, qubit in (("pivot_high", "X", 0), ("pivot_bit0", "X", n - 1), ("diagonal", "Z", 0)):
            for count in (1, 8):
                rotations = [(0.1 * (k + 1), letter, [qubit]) for k in range(count)]
                on_register = [(theta, letters, [q + shift for q in qs]) for theta, letters, qs in rotations]
                thetas = rng.uniform(-1.0, 1.0, (ens.members, count))
                name_of = {}

                def yardstick():
                    psi.pauli_rotations_adjoint(on_register, lam)
                    name_of["yardstick"] = psi.last_kernel()

                def per_member():
                    ens.pauli_rotations_adjoint(rotations, ens_lam, thetas)
                    name_of["per_member"] = psi.last_kernel()

                key = f"walk_{label}_T{count}"
                compare(row, key, per_member, yardstick, 4)
                if isinstance(row[key], dict):
                    row[key]["kernel"] = name_of.get("per_member", "")
                    row[key]["yardstick_kernel"] = name_of.get("yardstick", "")
        op = DiagonalOperator.from_terms(n, [(0.5, "ZZ", [0, n - 1]), (0.25, "Z", [n // 2])])
        gammas = rng.uniform(-1.0, 1.0, ens.members)
        compare(row, "cost_phase_walk", lambda: ens.diagonal_phase_adjoint(op, ens_lam, gammas), lambda: psi.diagonal_phase_adjoint(full, lam, 0.3), 4)
        compare(row, "inner", lambda: ens.inner(ens_lam), lambda: psi.inner(lam), 2)
        result["passes"][f"n{n}_members{ens.members}"] = row
        op.close()
        save()
    full.close()
    psi.close()
    lam.close()


if __name__ == "__main__":
    main()
