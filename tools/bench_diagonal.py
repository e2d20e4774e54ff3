#!/usr/bin/env python3
"""Diagonal operators on one MI355X: every new call next to an existing call of the library in the
same process.

For the 42 ZZ terms of ``maxcut_terms(n, ring_chord_edges(n))`` and the 378 of ``sk_terms(n, 0)``:

* ``apply_diagonal_phase`` against ``apply_pauli_rotations`` of the same terms and 1.25 x ``copy_into`` (2.5 streams
  against 2); ``apply_diagonal_operator`` against the same copy;
* ``expect_diagonal`` (with and without a threshold) against ``expect_pauli_sum`` of the same terms and ``norm2``;
* ``transition_diagonal`` against ``inner``;
* ``diagonal_phase_adjoint`` against the three separate new calls (two phases and a transition) and against
  ``pauli_rotations_adjoint`` on the same terms;
* ``qaoa.energy_and_gradient`` at ``--layers`` layers against ``DeviceState.energy_and_gradient`` on the equivalent
  rotation list (ZZ rotations plus RX spelled as X rotations), host clock around whole calls, ``--walk-reps`` repetitions;
* the time of ``DiagonalOperator.from_terms`` (allocation, table upload and the one write pass; no yardstick).

Timing of the passes: HIP events on the stream that carries the launches around whole calls, every call warmed first,
the contenders alternated inside one repetition loop; medians over ``--reps`` repetitions, minima alongside.

    python tools/bench_diagonal.py [--n 28] [--reps 9] [--out profiles/r13_diagonal.json]
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

from quantum_computations_amd import DiagonalOperator, _lib, qaoa  # noqa: E402
from quantum_computations_amd import workloads as W  # noqa: E402
from quantum_computations_amd.device import DeviceState  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--walk-reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--skip-walk", action="store_true")
    ap.add_argument("--out", default="profiles/r13_diagonal.json")
    args = ap.parse_args()
    n, reps, p = args.n, args.reps, args.layers
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    reg_gb = 16 * (1 << n) / 1e9
    result = {"tool": "tools/bench_diagonal.py", "n_qubits": n, "reps": reps, "register_GB": round(reg_gb, 4),
              "diagonal_GB": round(reg_gb / 2, 4),
              "timing": "HIP events around whole calls on the stream that carries the launches; medians; contenders alternated per repetition",
              "traffic": "not measured: no counter run was made; stream counts are those of the kernels' loads and stores "
                         "(a register stream is 16 bytes per amplitude, the diagonal half a stream)",
              "cases": {}}

    def save():
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1) + "\n")
        print(f"wrote {path}", flush=True)

    def timed(clock, fn):
        clock.timer_start()
        fn()
        return clock.timer_stop()

    def stats(samples):
        return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4)}

    def contest(clock, everyone, **contenders):
        for fn in contenders.values():
            fn()
        for dev in everyone:
            dev.sync()
        samples = {name: [] for name in contenders}
        for _ in range(reps):
            for name, fn in contenders.items():
                samples[name].append(timed(clock, fn))
        return {name: stats(values) for name, values in samples.items()}

    def rate(streams, ms):
        return round(streams * reg_gb / (ms * 1e-3), 1)

    psi, lam, y = DeviceState.random(n, seed=1), DeviceState.random(n, seed=2), DeviceState.random(n, seed=3)
    everyone = [psi, lam, y]
    gamma = 0.37
    rng = np.random.default_rng(0)
    gammas, betas = rng.uniform(-0.5, 0.5, p), rng.uniform(-0.5, 0.5, p)

    for name, terms in (("maxcut", W.maxcut_terms(n, W.ring_chord_edges(n))), ("sk", W.sk_terms(n, 0))):
        row = {"terms": len(terms)}
        result["cases"][name] = row
        # ---- construction: wall clock, the diagonal's stream drained by a one-element download ------------------------------
        build = []
        for _ in range(3):
            start = time.perf_counter()
            op = DiagonalOperator.from_terms(n, terms)
            op.download(0, 1)
            build.append((time.perf_counter() - start) * 1e3)
            if len(build) < 3:
                op.close()
        start = time.perf_counter()
        op.add_terms(terms[:1])
        op.download(0, 1)
        one_term_ms = (time.perf_counter() - start) * 1e3
        op.add_terms([(-terms[0][0], terms[0][1], terms[0][2])])
        row["from_terms_ms"] = {"first": round(build[0], 3), "later_median": round(statistics.median(build[1:]), 3),
                                "add_one_term_ms": round(one_term_ms, 3),
                                "note": "host clock: allocation and zero-fill of 2^n doubles, table upload, one write pass"}
        print(f"{name}: from_terms of {len(terms)} terms {build} ms, add_terms of one term {one_term_ms:.2f} ms", flush=True)
        rotations = [(2 * gamma * c, letters, qubits) for c, letters, qubits in terms]
        back = [(-theta, letters, qubits) for theta, letters, qubits in rotations]
        rot_passes = psi._pauli_rotations(rotations)
        psi._pauli_rotations(back)

        # ---- phase and mul ----------------------------------------------------------------------------------------------------
        got = contest(psi, everyone,
                      diagonal_phase=lambda: psi.apply_diagonal_phase(op, gamma),
                      pauli_rotations=lambda: psi.apply_pauli_rotations(rotations),
                      diagonal_operator=lambda: psi.apply_diagonal_operator(op, out=lam),
                      copy=lambda: y.copy_into(lam))
        copy_ms = got["copy"]["median_ms"]
        row["phase"] = {**got, "pauli_rotation_passes": rot_passes, "streams": 2.5,
                        "phase_over_1.25_copy": round(got["diagonal_phase"]["median_ms"] / (1.25 * copy_ms), 3),
                        "operator_over_1.25_copy": round(got["diagonal_operator"]["median_ms"] / (1.25 * copy_ms), 3),
                        "rotations_over_phase": round(got["pauli_rotations"]["median_ms"] / got["diagonal_phase"]["median_ms"], 2),
                        "phase_GB_per_s": rate(2.5, got["diagonal_phase"]["median_ms"]),
                        "operator_GB_per_s": rate(2.5, got["diagonal_operator"]["median_ms"]), "copy_GB_per_s": rate(2, copy_ms)}
        print(f"{name}: phase {got['diagonal_phase']['median_ms']:.3f} ms ({row['phase']['phase_over_1.25_copy']:.2f} x of 1.25 copies), "
              f"rotations in {rot_passes} passes {got['pauli_rotations']['median_ms']:.3f} ms, D psi {got['diagonal_operator']['median_ms']:.3f} ms, "
              f"copy {copy_ms:.3f} ms", flush=True)
        save()

        # ---- read-only reductions ---------------------------------------------------------------------------------------------
        threshold = op.extrema()[0] / 2
        got = contest(psi, everyone,
                      expect_diagonal=lambda: psi.expect_diagonal(op),
                      expect_diagonal_threshold=lambda: psi.expect_diagonal(op, threshold),
                      expect_pauli_sum=lambda: psi.expect_pauli_sum(terms),
                      norm2=lambda: psi.norm2(),
                      transition_diagonal=lambda: psi.transition_diagonal(op, lam),
                      inner=lambda: psi.inner(lam),
                      extrema=lambda: op.extrema())
        row["reductions"] = {**got, "expect_streams": 1.5, "transition_streams": 2.5,
                             "expect_over_1.5_norm2": round(got["expect_diagonal"]["median_ms"] / (1.5 * got["norm2"]["median_ms"]), 3),
                             "pauli_sum_over_expect": round(got["expect_pauli_sum"]["median_ms"] / got["expect_diagonal"]["median_ms"], 2),
                             "transition_over_1.25_inner": round(got["transition_diagonal"]["median_ms"] / (1.25 * got["inner"]["median_ms"]), 3),
                             "expect_GB_per_s": rate(1.5, got["expect_diagonal"]["median_ms"]),
                             "transition_GB_per_s": rate(2.5, got["transition_diagonal"]["median_ms"]),
                             "extrema_GB_per_s": rate(0.5, got["extrema"]["median_ms"]),
                             "note": "extrema runs on the diagonal's stream (the null stream, as the register's here)"}
        print(f"{name}: expect {got['expect_diagonal']['median_ms']:.3f} ms, with threshold {got['expect_diagonal_threshold']['median_ms']:.3f}, "
              f"expect_pauli_sum {got['expect_pauli_sum']['median_ms']:.3f}, norm2 {got['norm2']['median_ms']:.3f}; transition "
              f"{got['transition_diagonal']['median_ms']:.3f}, inner {got['inner']['median_ms']:.3f}; extrema {got['extrema']['median_ms']:.3f}", flush=True)
        save()

        # ---- the fused adjoint step -------------------------------------------------------------------------------------------
        def separate():
            psi.apply_diagonal_phase(op, -gamma)
            lam.apply_diagonal_phase(op, -gamma)
            lam.transition_diagonal(op, psi)

        got = contest(psi, everyone,
                      phase_adjoint=lambda: psi.diagonal_phase_adjoint(op, lam, -gamma),
                      three_separate_calls=separate,
                      pauli_rotations_adjoint=lambda: psi.pauli_rotations_adjoint(rotations, lam))
        row["phase_adjoint"] = {**got, "streams": 4.5, "separate_streams": 7.5,
                                "separate_over_fused": round(got["three_separate_calls"]["median_ms"] / got["phase_adjoint"]["median_ms"], 3),
                                "pauli_adjoint_over_fused": round(got["pauli_rotations_adjoint"]["median_ms"] / got["phase_adjoint"]["median_ms"], 2),
                                "fused_over_2.25_copy": round(got["phase_adjoint"]["median_ms"] / (2.25 * copy_ms), 3),
                                "GB_per_s": rate(4.5, got["phase_adjoint"]["median_ms"])}
        print(f"{name}: phase_adjoint {got['phase_adjoint']['median_ms']:.3f} ms, three calls {got['three_separate_calls']['median_ms']:.3f}, "
              f"pauli_rotations_adjoint {got['pauli_rotations_adjoint']['median_ms']:.3f}", flush=True)
        save()

        # ---- the whole walk ---------------------------------------------------------------------------------------------------
        if not args.skip_walk:
            walk_rotations = []
            for g, b in zip(gammas, betas):
                walk_rotations += [(2 * g * c, letters, qubits) for c, letters, qubits in terms] + [(2 * b, "X", [q]) for q in range(n)]
            plus = qaoa.plus_state(n)
            samples = {"qaoa": [], "rotation_list": []}
            values = {}
            for rep in range(args.walk_reps + 1):                     # the first round warms
                for which in samples:
                    plus.sync()
                    start = time.perf_counter()
                    if which == "qaoa":
                        values[which] = qaoa.energy_and_gradient(op, gammas, betas, plus)[0]
                    else:
                        values[which] = plus.energy_and_gradient(walk_rotations, terms)[0]
                    plus.sync()
                    if rep:
                        samples[which].append((time.perf_counter() - start) * 1e3)
            plus.close()
            row["energy_and_gradient"] = {"layers": p, "rotations": len(walk_rotations), "qaoa": stats(samples["qaoa"]),
                                          "rotation_list": stats(samples["rotation_list"]),
                                          "rotation_list_over_qaoa": round(statistics.median(samples["rotation_list"]) / statistics.median(samples["qaoa"]), 2),
                                          "energies": values, "timing": "host clock around whole calls, register synchronised"}
            print(f"{name}: energy_and_gradient p={p}: qaoa {row['energy_and_gradient']['qaoa']['median_ms']:.1f} ms, rotation list "
                  f"{row['energy_and_gradient']['rotation_list']['median_ms']:.1f} ms, energies {values}", flush=True)
            save()
        op.close()
    for dev in everyone:
        dev.close()


if __name__ == "__main__":
    main()
