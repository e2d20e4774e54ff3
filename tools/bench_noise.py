#!/usr/bin/env python3
"""Kraus channels on one MI355X: the device-decided trajectory step next to its floor and next to
the composition of existing calls it replaces, in the same process.

* n = ``--n`` (28), amplitude damping on bits 0, 5, 13, 27 and a random three-operator channel on bit pairs (0, 1), (5, 13),
  (26, 27): one general ``apply_channel`` call against
  - the floor of one read pass and one update pass: ``norm2`` plus a dense ``apply_matrix`` on the same bits;
  - the composition: ``reduced_density``, a host pick with the same rule, ``apply_matrix`` with the scaled Kraus operator.
* n = 16, 20, 24: a layered noisy circuit (a dense one-qubit gate and an amplitude damping on every qubit, then CX and a
  two-qubit channel on neighbouring pairs), gates per second device-decided against the composition, and the host
  synchronisations each makes: for the composition counted from the calls made here (one per ``reduced_density``); for
  the device-decided run derived from the library's rule (one per drain of the 256 log slots and one per read of the
  log) and marked as derived in the JSON.
* density registers of n = 12 and 13: one channel (its 4 x 4 superoperator on bits q and n + q) against one dense 4 x 4
  gate on the same two bits.

Timing: host clock around whole calls that end in a synchronisation of the register (the composition waits for the host
by construction, so device events alone would flatter it); every contender warmed first, contenders alternated inside one
repetition loop; medians over ``--reps`` repetitions, minima alongside.

    python tools/bench_noise.py [--n 28] [--reps 9] [--out profiles/r14_noise.json]
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

from quantum_computations_amd import _lib  # noqa: E402
from quantum_computations_amd.device import DensityState, DeviceState  # noqa: E402
from quantum_computations_amd.noise import KrausChannel  # noqa: E402

LOG_SLOTS = 256      # CH_LOG_SLOTS of csrc/qsv_channel_layout.h


def random_kraus(dim, count, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(dim * count, dim)) + 1j * rng.normal(size=(dim * count, dim))
    q, _ = np.linalg.qr(a)
    return [np.ascontiguousarray(q[j * dim:(j + 1) * dim, :]) for j in range(count)]


def random_unitary(dim, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(dim, dim)) + 1j * rng.normal(size=(dim, dim)))
    return q


def pick(weights, u):
    """The rule of the select kernel."""
    total = float(sum(weights))
    run, last = 0.0, 0
    for j, w in enumerate(weights):
        run += w
        if w > 0.0:
            last = j
            if run > u * total:
                return j, total
    return last, total


class Composition:
    """The trajectory step from existing calls; counts the host synchronisations it makes."""

    def __init__(self):
        self.syncs = 0

    def step(self, psi, channel, qubits, u):
        rho = psi.reduced_density(qubits)                     # one read pass, a download, a host wait
        self.syncs += 1
        weights = [float(np.real(np.trace(K.conj().T @ K @ rho))) for K in channel.kraus]
        j, total = pick(weights, u)
        scale = np.sqrt(total / weights[j]) if weights[j] > 0.0 else 0.0
        psi.apply_matrix(channel.kraus[j] * scale, qubits)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--circuit-sizes", type=int, nargs="*", default=[16, 20, 24])
    ap.add_argument("--density-sizes", type=int, nargs="*", default=[12, 13])
    ap.add_argument("--out", default="profiles/r14_noise.json")
    args = ap.parse_args()
    n, reps = args.n, args.reps
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    result = {"tool": "tools/bench_noise.py", "reps": reps,
              "timing": "host clock around whole calls, register synchronised at the end; medians; contenders alternated per repetition",
              "single_calls": {}, "circuits": {}, "density": {}}

    def save():
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1) + "\n")
        print(f"wrote {path}", flush=True)

    def stats(samples):
        return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4)}

    def contest(reg, **contenders):
        for fn in contenders.values():
            fn()
        reg.sync()
        samples = {name: [] for name in contenders}
        for _ in range(reps):
            for name, fn in contenders.items():
                start = time.perf_counter()
                fn()
                reg.sync()
                samples[name].append((time.perf_counter() - start) * 1e3)
        return {name: stats(values) for name, values in samples.items()}

    ad = KrausChannel.amplitude_damping(0.3)
    two = KrausChannel(random_kraus(4, 3, 42))
    rng = np.random.default_rng(0)
    comp = Composition()

    # ---- single calls on the large register ----------------------------------------------------------------------------------
    psi = DeviceState.random(n, seed=1)
    reg_gb = 16 * (1 << n) / 1e9
    result["n_qubits"] = n
    result["register_GB"] = round(reg_gb, 4)
    cases = [(ad, (b,)) for b in (0, 5, 13, n - 1)] + [(two, bits) for bits in ((0, 1), (5, 13), (n - 2, n - 1))]
    for channel, bits in cases:
        qubits = [n - 1 - b for b in bits]
        dense = random_unitary(1 << len(bits), 7)

        def floor():
            psi.norm2()
            psi.apply_matrix(dense, qubits)

        got = contest(psi,
                      channel=lambda: psi.apply_channel(channel, qubits, u=float(rng.random())),
                      floor_norm2_plus_dense_gate=floor,
                      composition=lambda: comp.step(psi, channel, qubits, float(rng.random())))
        psi.channel_log()
        ch_ms, floor_ms, comp_ms = (got[k]["median_ms"] for k in ("channel", "floor_norm2_plus_dense_gate", "composition"))
        row = {**got, "channel_over_floor": round(ch_ms / floor_ms, 3),
               "composition_over_channel": round(comp_ms / ch_ms, 3), "channel_GB_per_s": round(3 * reg_gb / (ch_ms * 1e-3), 1),
               "streams": 3, "channel_is_faster_than_composition": bool(ch_ms < comp_ms)}
        psi.apply_channel(channel, qubits, u=0.5)
        row["kernel"] = psi.last_kernel()
        psi.channel_log()
        name = ("amplitude_damping" if channel is ad else "random3") + "_bits_" + "_".join(map(str, bits))
        result["single_calls"][name] = row
        print(f"{name}: channel {ch_ms:.3f} ms, floor {floor_ms:.3f} ms, composition {comp_ms:.3f} ms ({row['kernel']})", flush=True)
        save()
    psi.close()

    # ---- layered noisy circuits ----------------------------------------------------------------------------------------------
    for m in args.circuit_sizes:
        gate1 = [random_unitary(2, 100 + q) for q in range(m)]
        steps = []
        for layer in range(args.layers):
            for q in range(m):
                steps.append((gate1[q], [q], ad))
            for q in range(layer % 2, m - 1, 2):
                steps.append(("cx", [q, q + 1], two))
        reg = DeviceState.random(m, seed=3)
        counts = {"device": 0, "composition": 0}

        def run(device_decided: bool):
            comp.syncs = 0
            for gate, qubits, channel in steps:
                if isinstance(gate, str):
                    reg.apply_cx(*qubits)
                else:
                    reg.apply_matrix(gate, qubits)
                if device_decided:
                    reg.apply_channel(channel, qubits, u=float(rng.random()))
                else:
                    comp.step(reg, channel, qubits, float(rng.random()))
            if device_decided:
                reg.channel_log()
                # DERIVED, not observed: the library has no counter of its waits.  Its rule (csrc/qsv_channel.hip): one wait
                # per drain of the LOG_SLOTS device slots, one for the log read made above
                counts["device"] = (len(steps) - 1) // LOG_SLOTS + 1
            else:
                counts["composition"] = comp.syncs

        got = contest(reg, device_decided=lambda: run(True), composition=lambda: run(False))
        dev_ms, comp_ms = got["device_decided"]["median_ms"], got["composition"]["median_ms"]
        row = {**got, "gates": len(steps), "channels": len(steps), "layers": args.layers,
               "gates_per_s_device_decided": round(len(steps) / (dev_ms * 1e-3), 1),
               "gates_per_s_composition": round(len(steps) / (comp_ms * 1e-3), 1),
               "host_synchronisations_device_decided": counts["device"], "host_synchronisations_composition": counts["composition"],
               "host_synchronisations_note": "composition: counted, one per reduced_density call made; device_decided: derived from the "
                                             "library's rule (one wait per 256 general channel calls, one for the log read), not observed",
               "composition_over_device_decided": round(comp_ms / dev_ms, 3), "device_decided_is_faster": bool(dev_ms < comp_ms)}
        result["circuits"][f"n{m}"] = row
        print(f"n={m}: {len(steps)} noisy gates: device-decided {dev_ms:.2f} ms ({counts['device']} waits), composition {comp_ms:.2f} ms "
              f"({counts['composition']} waits)", flush=True)
        save()
        reg.close()

    # ---- density registers ---------------------------------------------------------------------------------------------------
    for m in args.density_sizes:
        flat = DeviceState.random(2 * m, seed=5)                         # any 4^m numbers will do for a timing
        rho = DensityState(flat._h, device=flat.device)
        flat._h = None
        dense = random_unitary(4, 9)
        row = {}
        for q in (0, m // 2, m - 1):
            got = contest(rho, channel=lambda: rho.apply_channel(ad, [q]),
                          dense_4x4_gate=lambda: DeviceState.apply_matrix(rho, dense, [q, m + q]))
            row[f"qubit_{q}"] = {**got, "channel_over_gate": round(got["channel"]["median_ms"] / got["dense_4x4_gate"]["median_ms"], 3),
                                 "kernel": rho.last_kernel()}
            print(f"density n={m} qubit {q}: channel {got['channel']['median_ms']:.3f} ms, dense 4x4 {got['dense_4x4_gate']['median_ms']:.3f} ms", flush=True)
        result["density"][f"n{m}"] = {"register_GB": round(16 * 4 ** m / 1e9, 4), **row}
        save()
        rho.close()


if __name__ == "__main__":
    main()
