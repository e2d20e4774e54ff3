#!/usr/bin/env python3
"""The adjoint walk through product layers on one MI355X, everything in one process.

* on 2^28 amplitudes, a full ``RY`` wall: ``layer_adjoint`` against (a) the same wall through ``pauli_rotations_adjoint`` as
  28 ``Y`` rotations -- the route before this call existed --, (b) two ``apply_layer`` calls with the inverse matrices -- the
  un-apply alone, the floor for a four-stream tile pass -- and (c) two plain copies.
* on 28 qubits: ``one_qubit_densities`` against a ``3 n``-term ``expect_pauli_sum`` (X, Y and Z of every qubit).
* ``ansatz.Ansatz.energy_and_gradient`` (4 blocks of ``RY`` wall + ``RZ`` wall + ``cz_line``, Heisenberg-chain terms) against
  ``DeviceState.energy_and_gradient`` on the same circuit spelled as rotations, at 16, 20 and 28 qubits.  The rotation list
  cannot hold CZ: it is spelled as its ``Z``, ``Z`` and ``ZZ`` rotations (``Ansatz.rotations``), three rotations per CZ.
* ``qaoa.energy_and_gradient`` with ``walk="fused"`` against ``walk="calls"`` (``mixer="layer"``, ``p = 4``) at 16, 20 and 24 qubits.
* the observed error of the values against tests/layer_adjoint_reference.py at 12, 13 and 19 qubits, next to its bound.

Timing: host clock around whole calls that end in a synchronisation; every contender warmed first, contenders alternated
inside one repetition loop; medians over ``--reps`` repetitions, minima and maxima alongside; every ratio carries the
(max - min) / median of its yardstick from the same loop and a verdict: ``faster`` / ``slower`` when the ratio leaves
1 -+ that spread, else ``equal within the spread``.  Every section has a time limit of its own: a case that would start after
it is recorded as "not measured", and nothing is ever tried twice.

    python tools/bench_layer_adjoint.py [--reps 7] [--out profiles/r23_layer_adjoint.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))      # the reference statement, for the observed errors

from quantum_computations_amd import DiagonalOperator, _lib, ansatz, layers, qaoa  # noqa: E402
from quantum_computations_amd import workloads as W  # noqa: E402
from quantum_computations_amd.device import DeviceState  # noqa: E402


def heisenberg_chain(n):
    terms = []
    for q in range(n - 1):
        terms += [(1.0, "XX", [q, q + 1]), (0.75, "YY", [q, q + 1]), (-0.5, "ZZ", [q, q + 1])]
    return terms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--total", type=int, default=28, help="qubits of the large register")
    ap.add_argument("--ansatz-sizes", type=int, nargs="*", default=[16, 20, 28])
    ap.add_argument("--qaoa-sizes", type=int, nargs="*", default=[16, 20, 24])
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--section-seconds", type=float, default=150.0, help="time limit of each section")
    ap.add_argument("--out", default="profiles/r23_layer_adjoint.json")
    args = ap.parse_args()
    reps = args.reps
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    result = {"tool": "tools/bench_layer_adjoint.py", "reps": reps,
              "timing": "host clock around whole calls that end in a synchronisation; medians; contenders alternated per repetition; "
                        "spread = (max - min) / median of the yardstick; verdict: faster / slower when the ratio leaves 1 -+ spread",
              "wall": {}, "densities": {}, "ansatz": {}, "qaoa": {}, "observed_value_error": {}}

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

    def spread(s):
        return round((s["max_ms"] - s["min_ms"]) / s["median_ms"], 3)

    def against(got, mine, yardsticks):
        """ratio of `mine` to each yardstick (below 1: `mine` is faster), the yardstick's own spread and the verdict"""
        out = {}
        for y in yardsticks:
            ratio, ys = got[mine]["median_ms"] / got[y]["median_ms"], spread(got[y])
            verdict = "faster" if ratio < 1.0 - ys else "slower" if ratio > 1.0 + ys else "equal within the spread"
            out[f"{mine}_over_{y}"] = {"ratio": round(ratio, 3), "yardstick_spread": ys, "own_spread": spread(got[mine]), "verdict": verdict}
        return out

    def show(section, row, mine, yardsticks):
        print(f"{section}: " + ", ".join(f"{name} {row[name]['median_ms']:.3f} ms" for name in [mine] + yardsticks) + "; " +
              ", ".join(f"/{y} {row[f'{mine}_over_{y}']['ratio']:.3f} ({row[f'{mine}_over_{y}']['verdict']})" for y in yardsticks), flush=True)

    rng = np.random.default_rng(0)

    # ---- a full RY wall on one large register ----------------------------------------------------------------------------------------
    total = args.total
    reg_gb = 16 * (1 << total) / 1e9
    result["register_qubits"] = total
    result["register_GB"] = round(reg_gb, 4)
    psi, lam, other = DeviceState.random(total, seed=1), DeviceState.random(total, seed=2), DeviceState.zeros(total)
    thetas = rng.uniform(-np.pi, np.pi, total)
    forward = layers.ry(thetas)
    inverse = layers.ry(-thetas)
    y_rotations = [(float(t), "Y", [q]) for q, t in enumerate(thetas)]

    def sync_all():
        psi.sync()
        lam.sync()
        other.sync()

    def two_layers():
        psi.apply_layer(inverse)
        lam.apply_layer(inverse)

    def two_copies():
        psi.copy_into(other)
        lam.copy_into(other)

    got = contest(sync_all, layer_adjoint=lambda: psi.layer_adjoint(forward, lam), pauli_rotations_adjoint=lambda: psi.pauli_rotations_adjoint(y_rotations, lam),
                  two_apply_layer=two_layers, two_copies=two_copies)
    yardsticks = ["pauli_rotations_adjoint", "two_apply_layer", "two_copies"]
    passes = psi._layer_adjoint(forward, lam, range(total))[1]
    # a pass reads and writes both registers: four register streams
    row = {**got, **against(got, "layer_adjoint", yardsticks), "passes": passes, "kernel": psi.last_kernel(),
           "GB_per_s": round(4 * reg_gb * passes / (got["layer_adjoint"]["median_ms"] * 1e-3), 1)}
    result["wall"][f"n{total}"] = row
    show(f"RY wall n={total}", row, "layer_adjoint", yardsticks)
    save()

    # ---- one-qubit reduced density matrices ------------------------------------------------------------------------------------------
    xyz = [(1.0, letter, [q]) for q in range(total) for letter in "XYZ"]
    got = contest(psi.sync, one_qubit_densities=lambda: psi.one_qubit_densities(), expect_pauli_sum_3n=lambda: psi.expect_pauli_sum(xyz, return_terms=True))
    row = {**got, **against(got, "one_qubit_densities", ["expect_pauli_sum_3n"]), "passes": psi._layer_transition(psi, range(total))[1], "kernel": psi.last_kernel()}
    result["densities"][f"n{total}"] = row
    show(f"densities n={total}", row, "one_qubit_densities", ["expect_pauli_sum_3n"])
    save()
    for register in (psi, lam, other):
        register.close()

    # ---- ansatz gradients ------------------------------------------------------------------------------------------------------------
    deadline = time.perf_counter() + args.section_seconds
    for n in args.ansatz_sizes:
        if time.perf_counter() > deadline:
            result["ansatz"][f"n{n}"] = "not measured"
            continue
        circuit = ansatz.Ansatz(n)
        for _ in range(args.blocks):
            circuit.rotation_layer("ry").rotation_layer("rz").fixed(ansatz.cz_line(n))
        terms = heisenberg_chain(n)
        params = rng.uniform(-np.pi, np.pi, circuit.num_parameters)
        rotations = circuit.rotations(params)
        a, b = DeviceState.zeros(n), DeviceState.zeros(n)
        got = contest(lambda: None, ansatz_walk=lambda: circuit.energy_and_gradient(params, terms, a), rotation_list=lambda: b.energy_and_gradient(rotations, terms))
        grad = circuit.energy_and_gradient(params, terms, a)[1]
        want = b.energy_and_gradient(rotations, terms)[1][circuit.parameter_positions()]
        row = {**got, **against(got, "ansatz_walk", ["rotation_list"]), "blocks": args.blocks, "parameters": circuit.num_parameters,
               "rotations_in_the_list": len(rotations), "cz": "spelled as Z, Z and ZZ rotations in the list",
               "gradient_difference": float(np.max(np.abs(grad - want)))}
        result["ansatz"][f"n{n}"] = row
        show(f"ansatz n={n}", row, "ansatz_walk", ["rotation_list"])
        a.close()
        b.close()
        save()

    # ---- QAOA gradients --------------------------------------------------------------------------------------------------------------
    deadline = time.perf_counter() + args.section_seconds
    for n in args.qaoa_sizes:
        if time.perf_counter() > deadline:
            result["qaoa"][f"n{n}"] = "not measured"
            continue
        op = DiagonalOperator.from_terms(n, W.maxcut_terms(n, W.ring_chord_edges(n)))
        gammas, betas = rng.uniform(-0.6, 0.6, args.layers), rng.uniform(-0.6, 0.6, args.layers)
        got = contest(lambda: None, fused=lambda: qaoa.energy_and_gradient(op, gammas, betas, mixer="layer", walk="fused"),
                      calls=lambda: qaoa.energy_and_gradient(op, gammas, betas, mixer="layer", walk="calls"))
        fused, calls = qaoa.energy_and_gradient(op, gammas, betas, mixer="layer", walk="fused"), qaoa.energy_and_gradient(op, gammas, betas, mixer="layer")
        row = {**got, **against(got, "fused", ["calls"]), "layers": args.layers, "whole_call": "register allocation and |+>^n included on both sides",
               "d_beta_difference": float(np.max(np.abs(fused[2] - calls[2])))}
        result["qaoa"][f"n{n}"] = row
        show(f"qaoa n={n}", row, "fused", ["calls"])
        op.close()
        save()

    # ---- observed error of the values -------------------------------------------------------------------------------------------------
    import layer_adjoint_reference as A
    import layer_reference as L
    for n in (12, 13, 19):
        ket, bra = L.random_ket(n, 70 + n), 0.9 * L.random_ket(n, 80 + n)
        mats = L.random_unitaries((n,), 10 * n + n)
        a, b = DeviceState.from_numpy(ket), DeviceState.from_numpy(bra)
        T = a.layer_adjoint(np.conjugate(np.swapaxes(mats, 1, 2)), b)
        result["observed_value_error"][f"n{n}"] = {"max_abs_error": float(np.max(np.abs(T - A.layer_adjoint(ket, bra, mats)[0]))),
                                                   "bound": A.value_bound(n, 1.0, 0.9)}
        a.close()
        b.close()
    print("observed value errors:", result["observed_value_error"], flush=True)
    save()


if __name__ == "__main__":
    main()
