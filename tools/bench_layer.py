#!/usr/bin/env python3
"""Product layers on one MI355X, everything in one process.

* points per second of ``qaoa.energies`` (3-regular MaxCut, ``p = 4``, ``batch = 256``) at 12, 16 and 20 qubits:
  ``mixer="layer"`` against ``mixer="rotations"``, the code path this keyword leaves untouched.
* on a register of 2^28 amplitudes read as members of 16 and of 20 qubits: one per-member layer pass (twelve stages, index
  bits 0..11) and the same pass with shared matrices, against a dense 1-qubit gate, a plain copy and a ``k_qft_tile`` pass on
  the same register; the full per-member wall against the ``n`` per-member rotation passes it replaces.
* single registers, a full wall of random unitaries: 28 qubits against 28 ``apply_matrix`` calls through the deferred queue
  and with deferral off; 16 and 20 qubits against the (non-deferring) default.

Timing: host clock around whole calls that end in a synchronisation; every contender warmed first, contenders alternated
inside one repetition loop; medians over ``--reps`` repetitions, minima and maxima alongside; every ratio carries the
(max - min) / median of its yardstick from the same loop.  Every section has a time limit of its own: a case that would start
after it is recorded as "not measured", and nothing is ever tried twice.

    python tools/bench_layer.py [--reps 7] [--out profiles/r22_layer.json]
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

from quantum_computations_amd import DiagonalOperator, _lib, layers, qaoa  # noqa: E402
from quantum_computations_amd import workloads as W  # noqa: E402
from quantum_computations_amd.device import DeviceState  # noqa: E402
from quantum_computations_amd.ensemble import Ensemble  # noqa: E402


def random_unitaries(shape, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(tuple(shape) + (2, 2)) + 1j * rng.standard_normal(tuple(shape) + (2, 2))
    q, r = np.linalg.qr(g)
    d = np.diagonal(r, axis1=-2, axis2=-1)
    return np.ascontiguousarray(q * (d / np.abs(d))[..., None, :])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--total", type=int, default=28, help="qubits of the large register")
    ap.add_argument("--sizes", type=int, nargs="*", default=[12, 16, 20])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--member-sizes", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--single-sizes", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--section-seconds", type=float, default=120.0, help="time limit of each of the three sections")
    ap.add_argument("--out", default="profiles/r22_layer.json")
    args = ap.parse_args()
    reps = args.reps
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    result = {"tool": "tools/bench_layer.py", "reps": reps, "batch": args.batch,
              "timing": "host clock around whole calls that end in a synchronisation; medians; contenders alternated per repetition; "
                        "spread = (max - min) / median of the yardstick",
              "qaoa_points": {}, "passes": {}, "single": {}}

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
        """ratio of `mine` to each yardstick (below 1: the layer is faster), with the yardstick's own spread"""
        return {f"{mine}_over_{y}": {"ratio": round(got[mine]["median_ms"] / got[y]["median_ms"], 3), "yardstick_spread": spread(got[y]),
                                     "own_spread": spread(got[mine])} for y in yardsticks}

    rng = np.random.default_rng(0)
    batch = args.batch

    # ---- points per second: QAOA ---------------------------------------------------------------------------------------------------
    deadline = time.perf_counter() + args.section_seconds
    for n in args.sizes:
        if time.perf_counter() > deadline:
            result["qaoa_points"][f"n{n}"] = "not measured"
            continue
        op = DiagonalOperator.from_terms(n, W.maxcut_terms(n, W.ring_chord_edges(n)))
        gammas, betas = rng.uniform(-0.6, 0.6, (batch, args.layers)), rng.uniform(-0.6, 0.6, (batch, args.layers))
        got = contest(lambda: None, rotations=lambda: qaoa.energies(op, gammas, betas, batch=batch, mixer="rotations"),
                      layer=lambda: qaoa.energies(op, gammas, betas, batch=batch, mixer="layer"))
        row = {name: {**s, "points_per_s": round(batch / (s["median_ms"] * 1e-3), 1)} for name, s in got.items()}
        row.update(against(got, "layer", ["rotations"]))
        row["layers"] = args.layers
        row["whole_call"] = "register allocation, |+>^n and read-out included on both sides"
        result["qaoa_points"][f"n{n}"] = row
        print(f"qaoa n={n}: rotations {row['rotations']['points_per_s']:.1f} points/s, layer {row['layer']['points_per_s']:.1f}; time ratio "
              f"{row['layer_over_rotations']['ratio']:.3f} (yardstick spread {row['layer_over_rotations']['yardstick_spread']:.3f})", flush=True)
        op.close()
        save()

    # ---- passes on one large register ------------------------------------------------------------------------------------------------
    deadline = time.perf_counter() + args.section_seconds
    total = args.total
    reg_gb = 16 * (1 << total) / 1e9
    result["register_qubits"] = total
    result["register_GB"] = round(reg_gb, 4)
    state = DeviceState.random(total, seed=1)
    state.set_option(_lib.OPT_DEFER, 0)                                     # the dense gate runs as its own kernel
    other = DeviceState.zeros(total)
    u1 = random_unitaries((), 1)
    for n in args.member_sizes:
        if n > total:
            continue
        if time.perf_counter() > deadline:
            result["passes"][f"n{n}"] = "not measured"
            continue
        ens = Ensemble(state, n)
        shift = total - n
        low12 = [n - 1 - b for b in range(12)]                              # member qubits of index bits 0..11: one pass
        table12 = random_unitaries((ens.members, 12), n)
        def sync_both():
            state.sync()
            other.sync()

        got = contest(sync_both,
                      layer_pass_per_member=lambda: ens.apply_layer(table12, low12),
                      layer_pass_shared=lambda: ens.apply_layer(table12[0], low12),
                      dense_1q=lambda: state.apply_matrix(u1, [shift]),
                      copy=lambda: state.copy_into(other),
                      qft_pass=lambda: state._apply_qft([q + shift for q in low12], swaps=False))
        row = {"one_pass": {**got, **against(got, "layer_pass_per_member", ["dense_1q", "copy", "qft_pass", "layer_pass_shared"]),
                            **against(got, "layer_pass_shared", ["dense_1q", "copy", "qft_pass"]),
                            "per_member_GB_per_s": round(2 * reg_gb / (got["layer_pass_per_member"]["median_ms"] * 1e-3), 1),
                            "shared_GB_per_s": round(2 * reg_gb / (got["layer_pass_shared"]["median_ms"] * 1e-3), 1)}}
        ens.apply_layer(table12, low12)
        row["one_pass"]["kernel"] = state.last_kernel()
        print(f"members of {n}: one pass per member {got['layer_pass_per_member']['median_ms']:.3f} ms, shared {got['layer_pass_shared']['median_ms']:.3f}, "
              f"dense 1q {got['dense_1q']['median_ms']:.3f}, copy {got['copy']['median_ms']:.3f}, qft pass {got['qft_pass']['median_ms']:.3f}", flush=True)
        if time.perf_counter() < deadline:
            wall = random_unitaries((ens.members, n), 100 + n)
            thetas = rng.uniform(-1.0, 1.0, (ens.members, n))
            x_rotations = [(0.0, "X", [q]) for q in range(n)]
            got = contest(state.sync, layer_wall=lambda: ens.apply_layer(wall), rotation_passes=lambda: ens.apply_pauli_rotations(x_rotations, thetas))
            row["full_wall"] = {**got, **against(got, "layer_wall", ["rotation_passes"]), "layer_passes": ens.apply_layer(wall).last_passes,
                                "rotation_passes_count": ens.apply_pauli_rotations(x_rotations, thetas).last_passes}
            print(f"members of {n}: full wall {got['layer_wall']['median_ms']:.3f} ms against {n} rotation passes {got['rotation_passes']['median_ms']:.3f} ms", flush=True)
        else:
            row["full_wall"] = "not measured"
        result["passes"][f"n{n}_members{ens.members}"] = row
        save()
    other.close()
    state.close()

    # ---- single registers: a full wall of random unitaries -------------------------------------------------------------------------------
    deadline = time.perf_counter() + args.section_seconds
    for n in [total] + list(args.single_sizes):
        if time.perf_counter() > deadline:
            result["single"][f"n{n}"] = "not measured"
            continue
        wall = random_unitaries((n,), 200 + n)
        layer_state, default_state = DeviceState.random(n, seed=2), DeviceState.random(n, seed=2)

        def gates(register):
            for q in range(n):
                register.apply_matrix(wall[q], [q])

        contenders = {"layer": lambda: layer_state.apply_layer(wall), "apply_matrix_default": lambda: gates(default_state)}
        undeferred = None
        if n == total:
            undeferred = DeviceState.random(n, seed=2)
            undeferred.set_option(_lib.OPT_DEFER, 0)
            contenders["apply_matrix_defer_off"] = lambda: gates(undeferred)

        def sync_all():
            layer_state.sync()
            default_state.sync()
            if undeferred is not None:
                undeferred.sync()

        got = contest(sync_all, **contenders)
        queued, launches = default_state.defer_stats()
        row = {**got, **against(got, "layer", [name for name in contenders if name != "layer"]), "layer_passes": layer_state._apply_layer(wall, range(n)),
               "default_path_defers": bool(queued), "layer_kernel": layer_state.last_kernel()}
        result["single"][f"n{n}"] = row
        print(f"single n={n}: " + ", ".join(f"{name} {s['median_ms']:.3f} ms" for name, s in got.items()), flush=True)
        for register in (layer_state, default_state, undeferred):
            if register is not None:
                register.close()
        save()


if __name__ == "__main__":
    main()
