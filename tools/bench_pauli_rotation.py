#!/usr/bin/env python3
"""Pauli-string rotations on one MI355X: ``DeviceState.apply_pauli_rotation(s)`` (one pass per run of rotations that are
diagonal or flip the same qubits, ``k_pauli_rotate_group``) against what the library offered before, all in one process:

(a) one single-term pass with the pivot (highest flipped bit) on bits 0, 2, 3, 6, 14, n - 1 and a diagonal pass, against
    ``apply_matrix`` of a dense 2x2 on the pivot qubit with deferral off (the same bytes moved);
(b) passes of 1, 2, 4 and 8 terms that share an xmask: ms per pass and per term;
(c) weight-k strings, k = 2, 4, 8, 16, n, against the basis change + CX ladder + RZ spelling through the existing gate
    path, with the deferred queue on (the default) and off;
(d) one first-order Trotter step of ``heisenberg_chain_terms(n)`` (3 (n - 1) rotations, n - 1 passes) against the same step
    as n - 1 dense 4x4 bond gates and as 3 (n - 1) dense 4x4 gates, both through the deferred queue.

Timing: HIP events on the register's stream around whole calls (``timer_start`` / ``timer_stop``, which also flush the
deferred queue), every shape warmed first, the contenders alternated inside one repetition loop; medians over ``--reps``
repetitions, minima alongside.  Before anything is timed the spellings are checked against the rotations at 10 qubits.

    python tools/bench_pauli_rotation.py [--n 28] [--reps 9] [--out profiles/r09_pauli_rotation.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from quantum_computations_amd import _lib  # noqa: E402
from quantum_computations_amd import workloads as W  # noqa: E402
from quantum_computations_amd.device import DeviceState  # noqa: E402
from quantum_computations_amd.dv_simulator import gates as G  # noqa: E402
from quantum_computations_amd.dv_simulator import numpy_quantum as npq  # noqa: E402

S_DAGGER_THEN_H = npq.H @ np.diag([1.0, -1.0j])          # maps Y to Z: B Y B^dagger = Z
H_THEN_S = np.diag([1.0, 1.0j]) @ npq.H                  # its inverse


def passes_of(dev, rotations) -> int:
    offsets, qubits, letters = [0], [], ""
    for _, paulis, qs in rotations:
        qubits += list(qs)
        letters += paulis
        offsets.append(len(qubits))
    thetas = (C.c_double * len(rotations))(*[r[0] for r in rotations])
    passes = C.c_uint64()
    _lib.call("qsv_apply_pauli_rotations", dev._h, len(rotations), (C.c_int * len(offsets))(*offsets),
              (C.c_int * max(len(qubits), 1))(*qubits), letters.encode(), thetas, C.byref(passes))
    return passes.value


def spelled(dev, theta, letters, qubits):
    """exp(-i theta/2 P) as the textbook circuit: basis change to Z, CX ladder onto the last qubit, RZ, and back."""
    active = [(letter, q) for letter, q in zip(letters.upper(), qubits) if letter != "I"]
    for letter, q in active:
        if letter == "X":
            dev.apply_matrix(npq.H, [q])
        elif letter == "Y":
            dev.apply_matrix(S_DAGGER_THEN_H, [q])
    chain = [q for _, q in active]
    for a, b in zip(chain, chain[1:]):
        dev.apply_cx(a, b)
    dev.apply_matrix(G.RZ(0, theta).matrix, [chain[-1]])
    for a, b in reversed(list(zip(chain, chain[1:]))):
        dev.apply_cx(a, b)
    for letter, q in active:
        if letter == "X":
            dev.apply_matrix(npq.H, [q])
        elif letter == "Y":
            dev.apply_matrix(H_THEN_S, [q])


def bond_matrix(theta: float) -> np.ndarray:
    """exp(-i theta/2 (XX + YY + ZZ)): the three rotations of one Heisenberg bond commute, so this is their product."""
    out = np.eye(4, dtype=complex)
    for letters in ("XX", "YY", "ZZ"):
        out = G.PauliRotation([0, 1], letters, theta).matrix @ out
    return out


def self_check():
    n = 10
    rng = np.random.default_rng(2)
    ket = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    ket /= np.linalg.norm(ket)
    for letters, qubits in (("XYZ", [0, 4, 9]), ("YY", [9, 3]), ("XZYXZYXZYX", list(range(n)))):
        a, b = DeviceState.from_numpy(ket), DeviceState.from_numpy(ket)
        a.apply_pauli_rotation(0.77, letters, qubits)
        spelled(b, 0.77, letters, qubits)
        diff = float(np.max(np.abs(a.to_numpy() - b.to_numpy())))
        assert diff < 1e-12, (letters, diff)
    terms = W.heisenberg_chain_terms(n)
    a, b, c = (DeviceState.from_numpy(ket) for _ in range(3))
    a.evolve(terms, 0.05)
    for q in range(n - 1):
        b.apply_matrix(bond_matrix(0.1), [q, q + 1])
    for coefficient, letters, qubits in terms:
        c.apply_matrix(G.PauliRotation([0, 1], letters, 0.1 * coefficient).matrix, qubits)
    assert float(np.max(np.abs(a.to_numpy() - b.to_numpy()))) < 1e-12 and float(np.max(np.abs(a.to_numpy() - c.to_numpy()))) < 1e-12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="profiles/r09_pauli_rotation.json")
    args = ap.parse_args()
    n, reps = args.n, args.reps
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    self_check()
    dev = DeviceState.random(n, seed=1)
    reg_gb = 16 * (1 << n) / 1e9
    rng = np.random.default_rng(7)

    def timed(fn):
        dev.timer_start()
        fn()
        return dev.timer_stop()

    def stats(samples):
        return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4)}

    def contest(**contenders):
        """Warm every contender once, then alternate them inside one repetition loop."""
        for fn in contenders.values():
            fn()
        dev.sync()
        samples = {name: [] for name in contenders}
        for _ in range(reps):
            for name, fn in contenders.items():
                samples[name].append(timed(fn))
        return {name: stats(values) for name, values in samples.items()}

    def defer(on: bool):
        dev.set_option(_lib.OPT_DEFER, 1 if on else 0)

    result = {"tool": "tools/bench_pauli_rotation.py", "n_qubits": n, "reps": reps, "register_GB": round(reg_gb, 4),
              "timing": "HIP events around whole calls on the register's stream; medians; contenders alternated per repetition",
              "rotations_per_pass_cap": 8, "bytes_per_pass": 2 * 16 * (1 << n),
              "traffic": "not measured: no counter run was made; bytes_per_pass is one read and one write of the register"}

    # ---- (a) one single-term pass per pivot class, against a dense 2x2 on the pivot qubit with deferral off -------------
    defer(False)
    u2 = W.haar_unitary(2, rng)
    result["single_term_pass"] = []
    for label, bit in [(f"pivot bit {b}", b) for b in sorted({0, 2, 3, 6, 14, n - 1})] + [("diagonal", None)]:
        qubit = n - 1 - (n - 1 if bit is None else bit)
        letter = "Z" if bit is None else "X"
        assert passes_of(dev, [(0.3, letter, [qubit])]) == 1
        got = contest(rotation=lambda: dev.apply_pauli_rotation(0.3, letter, [qubit]), dense_2x2=lambda: dev.apply_matrix(u2, [qubit]))
        ratio = got["rotation"]["median_ms"] / got["dense_2x2"]["median_ms"]
        row = {"pass": label, "qubit": qubit, **got, "rotation_over_dense_2x2": round(ratio, 3),
               "rotation_GB_per_s": round(2 * reg_gb / (got["rotation"]["median_ms"] * 1e-3), 1)}
        if bit is None:
            row["note"] = "the contender is the dense 2x2 on the top bit: the diagonal pass has no pivot"
        result["single_term_pass"].append(row)
        print(f"(a) {label}: rotation {got['rotation']['median_ms']:.3f} ms, dense 2x2 {got['dense_2x2']['median_ms']:.3f} ms, ratio {ratio:.2f}",
              flush=True)

    # ---- (b) passes of 1, 2, 4, 8 terms that share an xmask ---------------------------------------------------------------------
    result["shared_passes"] = []
    rest = list(range(1, n - 4))
    for label, flips in (("diagonal", []), ("flips bits 27 and 3" if n == 28 else f"flips bits {n - 1} and 3", [0, n - 4])):
        for width in (1, 2, 4, 8):
            rotations = []
            for t in range(width):
                zs = sorted({rest[(3 * t + 5 * j) % len(rest)] for j in range(1 + t % 3)})
                head = "".join("XY"[(t + j) % 2] for j in range(len(flips)))
                rotations.append((0.1 + 0.2 * t, head + "Z" * len(zs), flips + zs))
            assert passes_of(dev, rotations) == 1
            got = contest(rotations=lambda: dev.apply_pauli_rotations(rotations))["rotations"]
            result["shared_passes"].append({"pass": label, "terms": width, **got, "ms_per_term": round(got["median_ms"] / width, 4),
                                            "GB_per_s": round(2 * reg_gb / (got["median_ms"] * 1e-3), 1)})
            print(f"(b) {label}, {width} terms: {got['median_ms']:.3f} ms per pass, {got['median_ms'] / width:.3f} ms per term", flush=True)

    # ---- (c) weight-k strings against the basis change + CX ladder + RZ spelling ---------------------------------------------------
    result["weight_k_strings"] = []
    for k in sorted({2, 4, 8, 16, n}):
        qubits = [int(q) for q in np.linspace(0, n - 1, k).round()]
        letters = "".join("XYZ"[j % 3] for j in range(k))
        assert len(set(qubits)) == k

        def spelled_with(on):
            defer(on)
            spelled(dev, 0.3, letters, qubits)

        got = contest(rotation=lambda: dev.apply_pauli_rotation(0.3, letters, qubits),
                      spelled_deferred=lambda: spelled_with(True), spelled_per_gate=lambda: spelled_with(False))
        defer(False)
        one_q = 2 * sum(letter in "XY" for letter in letters) + 1
        row = {"weight": k, "letters": letters, "qubits": qubits, "spelling_gates": {"one_qubit": one_q, "cx": 2 * (k - 1)}, **got,
               "deferred_over_rotation": round(got["spelled_deferred"]["median_ms"] / got["rotation"]["median_ms"], 2),
               "per_gate_over_rotation": round(got["spelled_per_gate"]["median_ms"] / got["rotation"]["median_ms"], 2)}
        result["weight_k_strings"].append(row)
        print(f"(c) weight {k}: rotation {got['rotation']['median_ms']:.3f} ms, spelled with the deferred queue "
              f"{got['spelled_deferred']['median_ms']:.3f} ms, spelled gate by gate {got['spelled_per_gate']['median_ms']:.3f} ms", flush=True)

    # ---- (d) one first-order Trotter step of the Heisenberg chain -------------------------------------------------------------------
    terms = W.heisenberg_chain_terms(n)
    dt = 0.05
    rotations = npq.trotter_rotations(npq.PauliSum(n, terms), dt)
    passes = passes_of(dev, rotations)
    bond = bond_matrix(2 * dt)
    singles = [(G.PauliRotation([0, 1], letters, theta).matrix, qubits) for theta, letters, qubits in rotations]

    def bonds():
        defer(True)
        for q in range(n - 1):
            dev.apply_matrix(bond, [q, q + 1])

    def dense_terms():
        defer(True)
        for matrix, qubits in singles:
            dev.apply_matrix(matrix, qubits)

    got = contest(rotations=lambda: dev.apply_pauli_rotations(rotations), dense_bonds_deferred=bonds, dense_terms_deferred=dense_terms)
    defer(False)
    result["heisenberg_trotter_step"] = {"terms": len(rotations), "passes": passes, **got,
                                         "ms_per_pass": round(got["rotations"]["median_ms"] / passes, 4),
                                         "rotations_over_dense_bonds": round(got["rotations"]["median_ms"] / got["dense_bonds_deferred"]["median_ms"], 2),
                                         "rotations_over_dense_terms": round(got["rotations"]["median_ms"] / got["dense_terms_deferred"]["median_ms"], 2)}
    print(f"(d) Heisenberg step, {len(rotations)} terms in {passes} passes: rotations {got['rotations']['median_ms']:.2f} ms, "
          f"{n - 1} dense bonds through the queue {got['dense_bonds_deferred']['median_ms']:.2f} ms, {len(rotations)} dense 4x4 gates through "
          f"the queue {got['dense_terms_deferred']['median_ms']:.2f} ms", flush=True)

    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
