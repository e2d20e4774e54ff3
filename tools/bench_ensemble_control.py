#!/usr/bin/env python3
"""Per-member measurement and feed-forward of trajectory ensembles on one MI355X, everything in one process.

* one conditional gate on a register of 2^28 amplitudes (members of 12, 16 and 20 qubits) on bit 0, bit n-1 and the pair
  (n-2, n-1), with none, half (alternating members), half (the first half) and all of the members taking it, against the plain
  dense gate on the same register qubits through the existing kernels: time(f) / time(dense gate).  The claim to record is that
  the time follows the fraction of takers.
* one measurement on the same registers against ``apply_channel`` with the equivalent two-projector ``KrausChannel`` and against
  section 23's floor, ``norm2`` plus a dense gate.
* end to end: one cycle of the distance 3, 5 and 7 bit-flip repetition code (5, 9, 13 qubits: bit-flip channels, syndrome
  extraction, measurement with reset, one correction per data qubit) through ``run_trajectories(batch=256)`` against a loop
  written here from calls that predate the ensemble's measurements: ``measure_probs``, a host pick, the one-qubit gate path and
  host-side control.  Shots per second and the ratio.

Timing: host clock around whole calls that end in a synchronisation; every contender warmed first, contenders alternated
inside one repetition loop; medians over ``--reps`` repetitions, minima and maxima alongside.

    python tools/bench_ensemble_control.py [--reps 9] [--out profiles/r17_ensemble_control.json]
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
from quantum_computations_amd.dv_simulator.simulator import ClassicalControl  # noqa: E402
from quantum_computations_amd.ensemble import TrajectoryEnsemble  # noqa: E402
from quantum_computations_amd.noise import Channel, KrausChannel, Measure, measure_branch  # noqa: E402

THETA, PHI = 1.1, 0.7


def random_unitary(dim, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(dim, dim)) + 1j * rng.normal(size=(dim, dim)))
    return q


def repetition_cycle(d, p):
    """Data qubits 0 .. d-1, syndrome qubits d .. 2d-2.  Correction i reads the syndromes next to data qubit i: a single flip is
    undone, which is all a benchmark asks of the decoder."""
    flip = KrausChannel.bit_flip(p)
    circuit = [Channel(flip, [q]) for q in range(d)]
    for a in range(d - 1):
        circuit += [G.CX(a, d + a), G.CX(a + 1, d + a)]
    circuit += [Measure(d + a, reset=True) for a in range(d - 1)]
    circuit.append(ClassicalControl(G.X(0), [0], [1]))
    circuit += [ClassicalControl(G.X(i), [i - 1, i], []) for i in range(1, d - 1)]
    circuit.append(ClassicalControl(G.X(d - 1), [d - 2], [d - 3]))
    return circuit


def host_loop(circuit, ket, shots, terms, seed):
    """The same shots with what the library had before: the weights come to the host, the host picks, the projector goes back as
    a one-qubit gate, the host decides which corrections to send."""
    rng = np.random.default_rng(seed)
    start = DeviceState.from_numpy(ket)
    work = start.copy()
    values = np.zeros(shots)
    try:
        for s in range(shots):
            start.copy_into(work)
            outcomes = []
            for gate in circuit:
                if isinstance(gate, ClassicalControl):
                    if gate.eval(outcomes):
                        gate.gate.apply(work)
                elif isinstance(gate, Channel):
                    work.apply_channel(gate.channel, gate.indices, rng=rng)
                elif isinstance(gate, Measure):
                    w0, w1 = work.measure_probs(gate.indices[0], *gate.eigenvectors())
                    outcome, _, scale = measure_branch(w0, w1, float(rng.random()))
                    work.apply_matrix(gate.kraus(outcome, scale), gate.indices)
                    outcomes.append(outcome)
                else:
                    gate.apply(work)
            values[s] = float(np.real(work.expect_pauli_sum(terms)))
            work.channel_log()
    finally:
        start.close()
        work.close()
    return values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--total", type=int, default=28, help="qubits of the register: n + b")
    ap.add_argument("--member-sizes", type=int, nargs="*", default=[12, 16, 20])
    ap.add_argument("--distances", type=int, nargs="*", default=[3, 5, 7])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--serial-shots", type=int, default=16)
    ap.add_argument("--out", default="profiles/r17_ensemble_control.json")
    args = ap.parse_args()
    reps = args.reps
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    result = {"tool": "tools/bench_ensemble_control.py", "reps": reps,
              "timing": "host clock around whole calls that end in a synchronisation; medians; contenders alternated per repetition",
              "conditional": {}, "measure": {}, "repetition_code": {}}

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

    total = args.total
    reg_gb = 16 * (1 << total) / 1e9
    result["register_qubits"] = total
    result["register_GB"] = round(reg_gb, 4)
    state = DeviceState.random(total, seed=1)
    rng = np.random.default_rng(0)
    projectors = KrausChannel([Measure(0, THETA, PHI).kraus(0), Measure(0, THETA, PHI).kraus(1)])
    for n in args.member_sizes:
        if n > total:
            continue
        ens = TrajectoryEnsemble(state, n)
        members, shift = ens.members, total - n
        index = np.arange(members, dtype=np.uint64)
        fractions = {"f0": np.zeros(members, dtype=np.uint64), "f_half_alternating": index & np.uint64(1),
                     "f_half_first": (index < members // 2).astype(np.uint64), "f1": np.ones(members, dtype=np.uint64)}
        # ---- a conditional gate against the dense gate ---------------------------------------------------------------------------
        rows = {}
        for bits in ((0,), (n - 1,), (n - 2, n - 1)):
            qubits = [n - 1 - b for b in bits]
            register_qubits = [q + shift for q in qubits]
            dense = random_unitary(1 << len(bits), 7)
            gate = G.Gate(qubits, dense)
            row = {}
            for name, words in fractions.items():
                ens.set_bits(words)
                state.sync()
                got = contest(state.sync, conditional=lambda: ens.apply_conditional(gate, [0]),
                              dense_gate=lambda: state.apply_matrix(dense, register_qubits))
                ratio = got["conditional"]["median_ms"] / got["dense_gate"]["median_ms"]
                row[name] = {**got, "over_dense_gate": round(ratio, 3)}
                ens.apply_conditional(gate, [0])
                row[name]["kernel"] = state.last_kernel()
                print(f"n={n} x{members} bits {bits} {name}: conditional {got['conditional']['median_ms']:.3f} ms, dense gate "
                      f"{got['dense_gate']['median_ms']:.3f} ms, ratio {ratio:.3f}", flush=True)
            rows["bits_" + "_".join(map(str, bits))] = row
        result["conditional"][f"n{n}_members{members}"] = rows
        save()
        # ---- a measurement against the two-projector channel and the floor --------------------------------------------------------------
        rows = {}
        for bit in (0, n - 1):
            q = n - 1 - bit
            dense = random_unitary(2, 8)

            def floor():
                state.norm2()
                state.apply_matrix(dense, [q + shift])

            u = rng.random(members)
            got = contest(state.sync, measure=lambda: ens.measure(q, THETA, PHI, u=u, bit=3),
                          channel_of_two_projectors=lambda: ens.apply_channel(projectors, [q], u=u),
                          floor_norm2_plus_dense_gate=floor)
            ens.channel_log()
            ms = {name: s["median_ms"] for name, s in got.items()}
            ens.measure(q, THETA, PHI, u=u, bit=3)
            kernel = state.last_kernel()
            ens.channel_log()
            rows[f"bit_{bit}"] = {**got, "measure_over_channel": round(ms["measure"] / ms["channel_of_two_projectors"], 3),
                                  "measure_over_floor": round(ms["measure"] / ms["floor_norm2_plus_dense_gate"], 3), "kernel": kernel}
            print(f"n={n} x{members} bit {bit}: measure {ms['measure']:.3f} ms, channel {ms['channel_of_two_projectors']:.3f} ms, floor "
                  f"{ms['floor_norm2_plus_dense_gate']:.3f} ms", flush=True)
        result["measure"][f"n{n}_members{members}"] = rows
        save()
    state.close()

    # ---- end to end: repetition-code cycles ---------------------------------------------------------------------------------------------
    for d in args.distances:
        n = 2 * d - 1
        circuit = repetition_cycle(d, 0.1)
        ket = np.zeros(1 << n, dtype=np.complex128)
        ket[0], ket[((1 << d) - 1) << (d - 1)] = 0.6, 0.8j
        terms = [(1.0, "Z" * d, list(range(d))), (0.5, "X", [d // 2])]
        got = contest(lambda: None,
                      host_loop=lambda: host_loop(circuit, ket, args.serial_shots, terms, 1),
                      serial=lambda: noise.run_trajectories(circuit, ket, args.serial_shots, terms=terms, seed=1),
                      batched=lambda: noise.run_trajectories(circuit, ket, args.batch, terms=terms, seed=1, batch=args.batch))
        shots = {"host_loop": args.serial_shots, "serial": args.serial_shots, "batched": args.batch}
        row = {"qubits": n, "steps": len(circuit), "whole_call": "upload, register allocation and read-out included"}
        base = shots["host_loop"] / (got["host_loop"]["median_ms"] * 1e-3)
        for name, s in got.items():
            rate = shots[name] / (s["median_ms"] * 1e-3)
            row[name] = {**s, "shots": shots[name], "shots_per_s": round(rate, 1), "over_host_loop": round(rate / base, 2)}
            print(f"distance {d} {name}: {rate:.1f} shots/s ({rate / base:.1f} x the host loop)", flush=True)
        result["repetition_code"][f"distance_{d}"] = row
        save()


if __name__ == "__main__":
    main()
