#!/usr/bin/env python3
"""The multi-register BLAS-1 passes and the Krylov methods built on them, on one MI355X.

(a) Single passes.  ``lincomb`` with K = 1, 2, 4, 8 sources, with and without ``beta`` and with and without ``norm2``
    (and, to tell the norm from the grid it runs on, without the norm under QSV_OPT_GRID_CAP = 1024);
    yardstick ``copy_into`` (two streams) times ``(K + 1 + [beta != 0]) / 2``.  ``inner_many`` with K = 1, 2, 4, 8;
    yardstick ``inner`` (two read streams) times ``(K + 1) / 2``.
(b) One Lanczos step without reorthogonalisation on ``heisenberg_chain_terms(n)``: the vector part through the new calls
    (``inner_many`` + ``lincomb`` with the norm + ``apply_scale``, 8 streams) against the same recurrence through the calls
    the library had before (``inner``, two identity-term ``apply_pauli_sum(..., accumulate=True)``, ``norm2``,
    ``apply_scale``, 11 streams), and the ``H v`` passes next to them.
(c) Whole runs on the Heisenberg chain: ``ground_state`` and ``evolve_krylov(t)``, wall time (host clock around the call,
    register synchronised), H applications and kernel passes.  Next to the evolution the Trotter route ``evolve(order=2)``:
    its error against ``evolve_krylov`` is taken at ``--small-n`` qubits for a ladder of step counts, the time of one
    step at ``n`` qubits, and the cost of each rung is their product.

Timing of (a) and (b): HIP events on the stream that carries the launches around whole calls, every shape warmed first,
the contenders alternated inside one repetition loop; medians over ``--reps`` repetitions, minima alongside.

    python tools/bench_krylov.py [--n 28] [--reps 9] [--out profiles/r12_krylov.json]
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

from quantum_computations_amd import _lib, krylov  # noqa: E402
from quantum_computations_amd import workloads as W  # noqa: E402
from quantum_computations_amd.device import DeviceState  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=28)
    ap.add_argument("--small-n", type=int, default=12)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--t", type=float, default=1.0)
    ap.add_argument("--ground-m", type=int, default=30)
    ap.add_argument("--ground-tol", type=float, default=1e-6)
    ap.add_argument("--ground-restarts", type=int, default=20)
    ap.add_argument("--evolve-m", type=int, default=20)
    ap.add_argument("--skip-runs", action="store_true")
    ap.add_argument("--out", default="profiles/r12_krylov.json")
    args = ap.parse_args()
    n, reps = args.n, args.reps
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    reg_gb = 16 * (1 << n) / 1e9
    result = {"tool": "tools/bench_krylov.py", "n_qubits": n, "reps": reps, "register_GB": round(reg_gb, 4),
              "timing": "HIP events around whole calls on the stream that carries the launches; medians; contenders alternated per repetition",
              "traffic": "not measured: no counter run was made; stream counts are those of the kernels' loads and stores"}

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

    # ---- (a) single passes --------------------------------------------------------------------------------------------------------
    sources = [DeviceState.random(n, seed=k + 1) for k in range(8)]
    dst, y = DeviceState.random(n, seed=20), DeviceState.random(n, seed=21)
    everyone = sources + [dst, y]
    result["lincomb"], result["inner_many"] = [], []

    def capped(fn):
        """``fn`` on the grid of a pass that forms the norm (QSV_OPT_GRID_CAP = 1024 workgroups), without the norm."""
        dst.set_option(_lib.OPT_GRID_CAP, 1024)
        fn()
        dst.set_option(_lib.OPT_GRID_CAP, 0)
    for count in (1, 2, 4, 8):
        coeffs = [0.25 / count * (1 - 0.5j)] * count
        srcs = sources[:count]
        got = contest(dst, everyone,
                      plain=lambda: dst.lincomb(coeffs, srcs),
                      norm=lambda: dst.lincomb(coeffs, srcs, return_norm2=True),
                      beta=lambda: dst.lincomb(coeffs, srcs, beta=0.5j),
                      beta_norm=lambda: dst.lincomb(coeffs, srcs, beta=0.5j, return_norm2=True),
                      plain_capped=lambda: capped(lambda: dst.lincomb(coeffs, srcs)),
                      copy=lambda: y.copy_into(dst))
        copy_ms = got["copy"]["median_ms"]
        row = {"sources": count, **got}
        for name, streams in (("plain", count + 1), ("plain_capped", count + 1), ("norm", count + 1), ("beta", count + 2), ("beta_norm", count + 2)):
            row[f"{name}_streams"] = streams
            row[f"{name}_over_yardstick"] = round(got[name]["median_ms"] / (copy_ms * streams / 2), 3)
            row[f"{name}_GB_per_s"] = round(streams * reg_gb / (got[name]["median_ms"] * 1e-3), 1)
        result["lincomb"].append(row)
        print(f"(a) lincomb K={count}: plain {got['plain']['median_ms']:.3f} ms ({row['plain_over_yardstick']:.2f} x), on 1024 workgroups "
              f"{got['plain_capped']['median_ms']:.3f} ({row['plain_capped_over_yardstick']:.2f} x), norm {got['norm']['median_ms']:.3f} "
              f"({row['norm_over_yardstick']:.2f} x), beta {got['beta']['median_ms']:.3f} ({row['beta_over_yardstick']:.2f} x), beta+norm "
              f"{got['beta_norm']['median_ms']:.3f} ({row['beta_norm_over_yardstick']:.2f} x), copy {copy_ms:.3f} ms", flush=True)
        got = contest(y, everyone, inner_many=lambda: y.inner_many(srcs), inner=lambda: y.inner(dst))
        inner_ms = got["inner"]["median_ms"]
        row = {"x": count, "streams": count + 1, **got,
               "over_yardstick": round(got["inner_many"]["median_ms"] / (inner_ms * (count + 1) / 2), 3),
               "GB_per_s": round((count + 1) * reg_gb / (got["inner_many"]["median_ms"] * 1e-3), 1)}
        result["inner_many"].append(row)
        print(f"(a) inner_many K={count}: {got['inner_many']['median_ms']:.3f} ms ({row['over_yardstick']:.2f} x of (K+1)/2 inner), inner {inner_ms:.3f} ms", flush=True)

    # ---- (b) one Lanczos step without reorthogonalisation -----------------------------------------------------------------------
    terms = W.heisenberg_chain_terms(n)
    v_prev, v, w = sources[0], sources[1], dst
    flat = krylov._flat_terms(krylov._real_terms(terms, "bench"))
    count = krylov._Counter()
    krylov._apply(flat, v, w, count)
    a, b = -1e-3, -2e-3                      # fixed small coefficients: the registers stay bounded over the repetitions

    def new_route():
        w.inner_many([v])
        w.lincomb([a, b], [v, v_prev], beta=1.0, return_norm2=True)
        w.apply_scale(1.0)

    def old_route():
        w.inner(v)
        v.apply_pauli_sum([(a, "", [])], out=w, accumulate=True)
        v_prev.apply_pauli_sum([(b, "", [])], out=w, accumulate=True)
        w.norm2()
        w.apply_scale(1.0)

    got = contest(w, everyone, new_vector_part=new_route, old_vector_part=old_route, h_passes=lambda: v.apply_pauli_sum(terms, out=w),
                  copy=lambda: y.copy_into(w))
    new_ms, old_ms, h_ms = (got[k]["median_ms"] for k in ("new_vector_part", "old_vector_part", "h_passes"))
    result["lanczos_step"] = {"terms": len(terms), "h_passes_count": count.passes, **got, "new_streams": 8, "old_streams": 11,
                              "old_over_new": round(old_ms / new_ms, 3), "new_over_4_copies": round(new_ms / (4 * got["copy"]["median_ms"]), 3),
                              "h_share_of_new_step": round(h_ms / (h_ms + new_ms), 3), "h_share_of_old_step": round(h_ms / (h_ms + old_ms), 3),
                              "step_old_over_new": round((h_ms + old_ms) / (h_ms + new_ms), 3)}
    print(f"(b) Lanczos step: H in {count.passes} passes {h_ms:.2f} ms; vector part new {new_ms:.3f} ms, old {old_ms:.3f} ms "
          f"({old_ms / new_ms:.2f} x); H share {result['lanczos_step']['h_share_of_new_step']:.2f}", flush=True)

    def save():
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1) + "\n")
        print(f"wrote {path}", flush=True)
    save()
    for dev in everyone:
        dev.close()
    if args.skip_runs:
        return

    # ---- (c) whole runs ---------------------------------------------------------------------------------------------------------
    def wall(fn):
        start = time.perf_counter()
        out = fn()
        return out, time.perf_counter() - start

    state = DeviceState.random(n, seed=3)
    info, seconds = wall(lambda: (state.evolve_krylov(terms, args.t, m=args.evolve_m), state.sync())[0])
    result["evolve_krylov"] = {"t": args.t, "m": args.evolve_m, "tol": 1e-10, "registers": args.evolve_m + 2, "wall_s": round(seconds, 3), **info}
    print(f"(c) evolve_krylov t={args.t}: {seconds:.2f} s, {info}", flush=True)
    save()

    # Trotter: errors at small n against evolve_krylov, the time of a step at n
    small = args.small_n
    small_terms = W.heisenberg_chain_terms(small)
    exact = DeviceState.random(small, seed=3)
    small_info = exact.evolve_krylov(small_terms, args.t, m=args.evolve_m)
    want = exact.to_numpy()
    ladder = []
    for steps in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096):
        trial = DeviceState.random(small, seed=3)
        trial.evolve(small_terms, args.t, steps=steps, order=2)
        ladder.append({"steps": steps, "error_at_small_n": float(np.linalg.norm(trial.to_numpy() - want))})
    state.evolve(terms, args.t / 1024, steps=1, order=2)               # warm
    state.sync()
    step_samples = []
    for _ in range(3):
        state.timer_start()
        state.evolve(terms, args.t / 1024, steps=4, order=2)
        step_samples.append(state.timer_stop() / 4)
    step_ms = statistics.median(step_samples)
    for rung in ladder:
        rung["ms_at_n"] = round(rung["steps"] * step_ms, 1)
    closest = min(ladder, key=lambda rung: abs(np.log(rung["error_at_small_n"]) - np.log(max(small_info["error_estimate"], 1e-16))))
    result["trotter_order_2"] = {"small_n": small, "krylov_error_estimate_at_small_n": small_info["error_estimate"], "step_ms_at_n": round(step_ms, 3),
                                 "ladder": ladder, "closest_in_error": closest,
                                 "note": "the error of a rung is its distance from evolve_krylov at small_n qubits; its cost is steps x the time of one step at n qubits"}
    print(f"(c) Trotter order 2: {step_ms:.1f} ms per step at n={n}; closest in error to Krylov: {closest}", flush=True)
    state.close()
    save()

    try:
        def run():
            found = krylov.ground_state(terms, n, m=args.ground_m, tol=args.ground_tol, max_restarts=args.ground_restarts, seed=3)
            found[1].sync()
            return found
        (energy, ground, info), seconds = wall(run)
        info = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in info.items()}
        info["ritz_values"] = info["ritz_values"][:4]
        result["ground_state"] = {"m": args.ground_m, "tol": args.ground_tol, "registers": args.ground_m + 2, "wall_s": round(seconds, 3), "energy": energy, **info}
        ground.close()
    except RuntimeError as error:
        result["ground_state"] = {"m": args.ground_m, "tol": args.ground_tol, "max_restarts": args.ground_restarts, "not_converged": str(error)}
    print(f"(c) ground_state: {result['ground_state']}", flush=True)
    save()


if __name__ == "__main__":
    main()
