#!/usr/bin/env python3
"""Trajectory ensembles on one MI355X, everything in one process.

* ``run_trajectories`` serial against ``batch = 64 / 256 / 1024`` on the layered noisy circuit of tools/bench_noise.py (a
  dense one-qubit gate and an amplitude damping on every qubit, then CX and a two-qubit channel on neighbouring pairs) at
  12, 16 and 20 qubits, up to ``n + b = 28``: shots per second.  The serial figure is the baseline -- the unchanged serial
  loop, measured here, in the same process.
* one ensemble channel call on a register of 2^28 amplitudes (members of 12, 16, 20 and 24 qubits) against its floor: one
  read pass and one update pass over the same register, ``norm2`` plus a dense gate on the same bits.
* ``expect_pauli_sum`` per member against the single-register call on the same register, per pass.

Timing: host clock around whole calls that end in a synchronisation; every contender warmed first, contenders alternated
inside one repetition loop; medians over ``--reps`` repetitions, minima and maxima alongside.

    python tools/bench_ensemble.py [--reps 9] [--out profiles/r16_ensemble.json]
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

from quantum_computations_amd import _lib, noise  # noqa: E402
from quantum_computations_amd.device import DeviceState  # noqa: E402
from quantum_computations_amd.dv_simulator import gates as G  # noqa: E402
from quantum_computations_amd.ensemble import TrajectoryEnsemble  # noqa: E402
from quantum_computations_amd.noise import Channel, KrausChannel  # noqa: E402


def random_kraus(dim, count, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(dim * count, dim)) + 1j * rng.normal(size=(dim * count, dim))
    q, _ = np.linalg.qr(a)
    return [np.ascontiguousarray(q[j * dim:(j + 1) * dim, :]) for j in range(count)]


def random_unitary(dim, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(dim, dim)) + 1j * rng.normal(size=(dim, dim)))
    return q


def random_ket(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    return v / np.linalg.norm(v)


def layered_circuit(m, layers, ad, two):
    gate1 = [random_unitary(2, 100 + q) for q in range(m)]
    circuit = []
    for layer in range(layers):
        for q in range(m):
            circuit += [G.Gate([q], gate1[q]), Channel(ad, [q])]
        for q in range(layer % 2, m - 1, 2):
            circuit += [G.CX(q, q + 1), Channel(two, [q, q + 1])]
    return circuit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--total", type=int, default=28, help="qubits of the largest register: n + b")
    ap.add_argument("--circuit-sizes", type=int, nargs="*", default=[12, 16, 20])
    ap.add_argument("--batches", type=int, nargs="*", default=[64, 256, 1024])
    ap.add_argument("--serial-shots", type=int, default=16)
    ap.add_argument("--member-sizes", type=int, nargs="*", default=[12, 16, 20, 24])
    ap.add_argument("--out", default="profiles/r16_ensemble.json")
    args = ap.parse_args()
    reps = args.reps
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    result = {"tool": "tools/bench_ensemble.py", "reps": reps,
              "timing": "host clock around whole calls that end in a synchronisation; medians; contenders alternated per repetition",
              "trajectories": {}, "single_calls": {}, "pauli_sums": {}}

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

    ad = KrausChannel.amplitude_damping(0.3)
    two = KrausChannel(random_kraus(4, 3, 42))

    # ---- run_trajectories: serial against batched -------------------------------------------------------------------------------
    for m in args.circuit_sizes:
        circuit = layered_circuit(m, args.layers, ad, two)
        ket = random_ket(m, 3)
        terms = [(1.0, "ZZ", [0, 1]), (0.5, "X", [m // 2]), (-0.75, "ZY", [m - 1, 0])]
        batches = [b for b in args.batches if m + b.bit_length() - 1 <= args.total]
        contenders = {"serial": lambda: noise.run_trajectories(circuit, ket, args.serial_shots, terms=terms, seed=1)}
        for b in batches:
            contenders[f"batch_{b}"] = lambda b=b: noise.run_trajectories(circuit, ket, b, terms=terms, seed=1, batch=b)
        got = contest(lambda: None, **contenders)                       # every run ends in its own download of values and log
        shots = {"serial": args.serial_shots, **{f"batch_{b}": b for b in batches}}
        row = {"noisy_gates": len(circuit) // 2, "layers": args.layers, "whole_call": "upload, register allocation and read-out included"}
        serial_rate = shots["serial"] / (got["serial"]["median_ms"] * 1e-3)
        for name, s in got.items():
            rate = shots[name] / (s["median_ms"] * 1e-3)
            row[name] = {**s, "shots": shots[name], "shots_per_s": round(rate, 1),
                         "shots_per_s_range": [round(shots[name] / (s["max_ms"] * 1e-3), 1), round(shots[name] / (s["min_ms"] * 1e-3), 1)],
                         "over_serial": round(rate / serial_rate, 2)}
            print(f"n={m} {name}: {rate:.1f} shots/s ({rate / serial_rate:.1f} x serial)", flush=True)
        result["trajectories"][f"n{m}"] = row
        save()

    # ---- one ensemble channel call against its floor; Pauli sums per member against the single-register call ----------------------
    total = args.total
    reg_gb = 16 * (1 << total) / 1e9
    result["register_qubits"] = total
    result["register_GB"] = round(reg_gb, 4)
    state = DeviceState.random(total, seed=1)
    rng = np.random.default_rng(0)
    for n in args.member_sizes:
        if n > total:
            continue
        ens = TrajectoryEnsemble(state, n)
        shift = total - n
        cases = [(ad, (b,)) for b in sorted({0, 5, 13, n - 1}) if b < n]
        cases += [(two, bits) for bits in ((0, 1), (5, 13), (n - 2, n - 1)) if max(bits) < n]
        rows = {}
        for channel, bits in cases:
            qubits = [n - 1 - b for b in bits]
            register_qubits = [q + shift for q in qubits]
            dense = random_unitary(1 << len(bits), 7)

            def floor():
                state.norm2()
                state.apply_matrix(dense, register_qubits)

            u = rng.random(ens.members)                                  # drawn outside the clock, as the serial call's scalar is
            got = contest(state.sync,
                          ensemble_channel=lambda: ens.apply_channel(channel, qubits, u=u),
                          floor_norm2_plus_dense_gate=floor)
            ens.channel_log()
            ch_ms, floor_ms = got["ensemble_channel"]["median_ms"], got["floor_norm2_plus_dense_gate"]["median_ms"]
            ens.apply_channel(channel, qubits, u=u)
            kernel = state.last_kernel()
            ens.channel_log()
            name = ("amplitude_damping" if channel is ad else "random3") + "_bits_" + "_".join(map(str, bits))
            rows[name] = {**got, "call_over_floor": round(ch_ms / floor_ms, 3), "GB_per_s": round(3 * reg_gb / (ch_ms * 1e-3), 1), "streams": 3,
                          "kernel": kernel}
            print(f"n={n} x{ens.members} {name}: call {ch_ms:.3f} ms, floor {floor_ms:.3f} ms, ratio {ch_ms / floor_ms:.3f} ({kernel})", flush=True)
        result["single_calls"][f"n{n}_members{ens.members}"] = rows
        # two passes: {ZZ, Z} and {XX}
        terms = [(1.0, "ZZ", [0, 1]), (0.5, "Z", [n - 1]), (0.25, "XX", [0, n - 1])]
        register_terms = [(c, letters, [q + shift for q in qs]) for c, letters, qs in terms]
        got = contest(lambda: None, per_member=lambda: ens.expect_pauli_sum(terms), single_register=lambda: state.expect_pauli_sum(register_terms))
        result["pauli_sums"][f"n{n}_members{ens.members}"] = {
            **got, "passes": 2, "per_member_ms_per_pass": round(got["per_member"]["median_ms"] / 2, 4),
            "single_register_ms_per_pass": round(got["single_register"]["median_ms"] / 2, 4),
            "per_member_over_single": round(got["per_member"]["median_ms"] / got["single_register"]["median_ms"], 3)}
        print(f"n={n} x{ens.members} Pauli sum, 2 passes: per member {got['per_member']['median_ms']:.3f} ms, single register "
              f"{got['single_register']['median_ms']:.3f} ms", flush=True)
        save()
    state.close()


if __name__ == "__main__":
    main()
