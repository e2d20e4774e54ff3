#!/usr/bin/env python3
"""Parameter ensembles on one MI355X, everything in one process.

* points per second: ``qaoa.energies`` (3-regular MaxCut, ``p = 4``) and ``sweep.energies`` (one Trotter step of the open
  Heisenberg chain, energy of the chain) with ``batch = 256`` at 12, 16 and 20 qubits, against the serial loop over the same
  kind of points through the existing single-register calls -- ``qaoa.run`` + ``expect_diagonal``, and
  ``apply_pauli_rotations`` + ``expect_pauli_sum`` on a fresh register per point.  The serial loop is the baseline and is
  never the code under test.
* time per pass on a register of 2^28 amplitudes read as members of 16 and of 20 qubits: one per-member rotation pass
  (pivot on the member's top bit, pivot on bit 0, diagonal; one rotation and eight in the pass) against
  ``k_pauli_rotate_group`` on the same register with the same string; the per-member cost phase against
  ``apply_diagonal_phase`` with a full-size diagonal; ``expect_diagonal`` per member against ``norm2`` per member.  Each row
  carries the ratio and the run-to-run spread of its yardstick from the same call.

Timing: host clock around whole calls that end in a synchronisation; every contender warmed first, contenders alternated
inside one repetition loop; medians over ``--reps`` repetitions, minima and maxima alongside.  Every section has a time limit
of its own: a case that would start after it is recorded as "not measured", and nothing is ever tried twice.

    python tools/bench_sweep.py [--reps 9] [--out profiles/r21_sweep.json]
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
    ap.add_argument("--total", type=int, default=28, help="qubits of the register of the per-pass measurements: n + b")
    ap.add_argument("--sizes", type=int, nargs="*", default=[12, 16, 20])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--serial-points", type=int, default=16)
    ap.add_argument("--member-sizes", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--section-seconds", type=float, default=150.0, help="time limit of each of the three sections")
    ap.add_argument("--out", default="profiles/r21_sweep.json")
    args = ap.parse_args()
    reps = args.reps
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    result = {"tool": "tools/bench_sweep.py", "reps": reps, "batch": args.batch,
              "timing": "host clock around whole calls that end in a synchronisation; medians; contenders alternated per repetition",
              "qaoa_points": {}, "rotation_points": {}, "passes": {}}

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
    batch, serial = args.batch, args.serial_points

    # ---- points per second: QAOA -----------------------------------------------------------------------------------------------
    deadline = time.perf_counter() + args.section_seconds
    for n in args.sizes:
        if time.perf_counter() > deadline:
            result["qaoa_points"][f"n{n}"] = "not measured"
            continue
        op = DiagonalOperator.from_terms(n, W.maxcut_terms(n, W.ring_chord_edges(n)))
        gammas, betas = rng.uniform(-0.6, 0.6, (batch, args.layers)), rng.uniform(-0.6, 0.6, (batch, args.layers))

        def serial_loop():
            for g, b in zip(gammas[:serial], betas[:serial]):
                state = qaoa.run(op, g, b)
                state.expect_diagonal(op)
                state.close()

        got = contest(lambda: None, serial=serial_loop, batched=lambda: qaoa.energies(op, gammas, betas, batch=batch))
        row = rates(got, {"serial": serial, "batched": batch})
        row["layers"] = args.layers
        row["whole_call"] = "register allocation, |+>^n and read-out included on both sides"
        result["qaoa_points"][f"n{n}"] = row
        print(f"qaoa n={n}: serial {row['serial']['points_per_s']:.1f} points/s, batch {batch}: {row['batched']['points_per_s']:.1f} "
              f"({row['batched']['over_serial']:.2f} x)", flush=True)
        op.close()
        save()

    # ---- points per second: one Trotter step of the Heisenberg chain ------------------------------------------------------
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
                state.apply_pauli_rotations([(theta, letters, qubits) for theta, (_, letters, qubits) in zip(row, rotations)])
                state.expect_pauli_sum(terms)
                state.close()

        got = contest(lambda: None, serial=serial_loop, batched=lambda: sweep.energies(rotations, thetas, terms, batch=batch))
        row = rates(got, {"serial": serial, "batched": batch})
        row["rotations"] = len(rotations)
        row["whole_call"] = "register allocation and read-out included on both sides"
        result["rotation_points"][f"n{n}"] = row
        print(f"rotations n={n}: serial {row['serial']['points_per_s']:.1f} points/s, batch {batch}: {row['batched']['points_per_s']:.1f} "
              f"({row['batched']['over_serial']:.2f} x)", flush=True)
        save()

    # ---- time per pass on one large register ----------------------------------------------------------------------------------
    deadline = time.perf_counter() + args.section_seconds
    total = args.total
    reg_gb = 16 * (1 << total) / 1e9
    result["register_qubits"] = total
    result["register_GB"] = round(reg_gb, 4)
    state = DeviceState.random(total, seed=1)
    full = DiagonalOperator.from_terms(total, [(0.5, "ZZ", [0, total - 1]), (0.25, "Z", [total // 2])])

    def compare(row, name, per_member, yardstick, sync, streams):
        if time.perf_counter() > deadline:
            row[name] = "not measured"
            return
        got = contest(sync, per_member=per_member, yardstick=yardstick)
        mine, ref = got["per_member"], got["yardstick"]
        row[name] = {**got, "ratio": round(mine["median_ms"] / ref["median_ms"], 3),
                     "yardstick_spread": round((ref["max_ms"] - ref["min_ms"]) / ref["median_ms"], 3),
                     "per_member_GB_per_s": round(streams * reg_gb / (mine["median_ms"] * 1e-3), 1)}
        print(f"{name}: per member {mine['median_ms']:.3f} ms, yardstick {ref['median_ms']:.3f} ms, ratio {row[name]['ratio']:.3f} "
              f"(yardstick spread {row[name]['yardstick_spread']:.3f})", flush=True)

    for n in args.member_sizes:
        if n > total:
            continue
        ens = Ensemble(state, n)
        shift = total - n
        row = {}
        for label, letter, qubit in (("pivot_high", "X", 0), ("pivot_bit0", "X", n - 1), ("diagonal", "Z", 0)):
            for count in (1, 8):
                rotations = [(0.1 * (k + 1), letter, [qubit]) for k in range(count)]
                on_register = [(theta, letters, [q + shift for q in qs]) for theta, letters, qs in rotations]
                thetas = rng.uniform(-1.0, 1.0, (ens.members, count))

                def yardstick():
                    state.apply_pauli_rotations(on_register)
                    name_of["yardstick"] = state.last_kernel()

                name_of = {}
                compare(row, f"rotation_{label}_T{count}", lambda: ens.apply_pauli_rotations(rotations, thetas), yardstick, state.sync, 2)
                if isinstance(row[f"rotation_{label}_T{count}"], dict):
                    ens.apply_pauli_rotations(rotations, thetas)
                    row[f"rotation_{label}_T{count}"]["kernel"] = state.last_kernel()
                    row[f"rotation_{label}_T{count}"]["yardstick_kernel"] = name_of.get("yardstick", "")
                    row[f"rotation_{label}_T{count}"]["table_bytes_per_member"] = 16 * count
        op = DiagonalOperator.from_terms(n, [(0.5, "ZZ", [0, n - 1]), (0.25, "Z", [n // 2])])
        gammas = rng.uniform(-1.0, 1.0, ens.members)
        compare(row, "cost_phase", lambda: ens.apply_diagonal_phase(op, gammas), lambda: state.apply_diagonal_phase(full, 0.3), state.sync, 2)
        compare(row, "expect_diagonal", lambda: ens.expect_diagonal(op), lambda: ens.norm2(), lambda: None, 1)
        result["passes"][f"n{n}_members{ens.members}"] = row
        op.close()
        save()
    full.close()
    state.close()


if __name__ == "__main__":
    main()
