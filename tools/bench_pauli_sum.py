#!/usr/bin/env python3
"""Pauli-sum expectation values on one MI355X: ``DeviceState.expect_pauli_sum`` (terms that flip the same qubits share
passes, each pass reads the register once) against a loop of ``DeviceState.expect_pauli`` over the same terms (two reads
of the register and one synchronisation per term), on a random ket, for ``heisenberg_chain_terms(n)`` and
``ising_terms(n, 1.0)``.  Also timed in the same process: ``norm2`` (one read of the register with one accumulator:
the floor a pass is judged against) and single passes of every kernel width (1, 2, 4, 8 terms) for the diagonal group
and for a low and a high pivot bit.

Timing: HIP events on the register's stream around whole calls (tools/sweep_readout.py), every shape warmed first, the
two contenders alternated inside one repetition loop; medians over ``--reps`` repetitions, minima alongside.

    python tools/bench_pauli_sum.py [--n 28] [--reps 9] [--out profiles/r08_pauli_sum.json]
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


def passes_of(dev, terms) -> int:
    offsets, qubits, letters = [0], [], ""
    for _, paulis, qs in terms:
        qubits += list(qs)
        letters += paulis
        offsets.append(len(qubits))
    re, im, passes = C.c_double(), C.c_double(), C.c_uint64()
    _lib.call("qsv_expect_pauli_sum", dev._h, len(terms), (C.c_int * len(offsets))(*offsets), (C.c_int * len(qubits))(*qubits),
              letters.encode(), None, None, C.byref(re), C.byref(im), C.byref(passes))
    return passes.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="profiles/r08_pauli_sum.json")
    args = ap.parse_args()
    n, reps = args.n, args.reps
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    dev = DeviceState.random(n, seed=1)
    reg_gb = 16 * (1 << n) / 1e9

    def timed(fn):
        dev.timer_start()
        out = fn()
        return dev.timer_stop(), out

    def stats(samples):
        return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4)}

    result = {"tool": "tools/bench_pauli_sum.py", "n_qubits": n, "reps": reps, "register_GB": round(reg_gb, 4),
              "timing": "HIP events around whole calls on the register's stream; medians; contenders alternated per repetition",
              "terms_per_pass_cap": 8}

    dev.norm2()
    floor = [timed(dev.norm2)[0] for _ in range(max(reps, 9))]
    floor_ms = statistics.median(floor)
    result["norm2"] = {**stats(floor), "GB_per_s": round(reg_gb / (floor_ms * 1e-3), 1), "bytes": "one read of the register"}
    print(f"norm2: {floor_ms:.3f} ms  {reg_gb / (floor_ms * 1e-3):.0f} GB/s", flush=True)

    result["hamiltonians"] = {}
    for name, terms in (("heisenberg_chain", W.heisenberg_chain_terms(n)), ("ising", W.ising_terms(n, 1.0))):
        def grouped():
            return dev.expect_pauli_sum(terms)

        def loop():
            return sum(c * dev.expect_pauli(letters, qubits) for c, letters, qubits in terms)

        passes = passes_of(dev, terms)
        a, b = grouped(), loop()                                  # warm both, and the two must agree
        scale = sum(abs(c) for c, _, _ in terms)
        assert abs(a - b) <= 1e-12 * scale, (a, b)
        t_grouped, t_loop = [], []
        for _ in range(reps):
            t_grouped.append(timed(grouped)[0])
            t_loop.append(timed(loop)[0])
        g_ms, l_ms = statistics.median(t_grouped), statistics.median(t_loop)
        per_pass = g_ms / passes
        row = {"terms": len(terms), "passes": passes, "value": [a.real, a.imag], "abs_diff_grouped_vs_loop": abs(a - b),
               "grouped": stats(t_grouped), "per_term_loop": stats(t_loop), "speedup": round(l_ms / g_ms, 3),
               "ms_per_pass": round(per_pass, 4), "GB_per_s_per_pass": round(reg_gb / (per_pass * 1e-3), 1),
               "pass_rate_over_norm2_rate": round(floor_ms / per_pass, 3),
               "ms_per_term_loop": round(l_ms / len(terms), 4),
               "algorithmic_GB_per_s_per_term_loop": round(2 * reg_gb / (l_ms / len(terms) * 1e-3), 1),
               "note": "the per-term figure counts two reads of the register per term, as k_expect_pauli issues them; "
                       "partner reads that hit a cache are not HBM traffic, so it is no HBM rate"}
        result["hamiltonians"][name] = row
        print(f"{name}: {len(terms)} terms, {passes} passes: grouped {g_ms:.2f} ms ({per_pass:.3f} ms/pass, "
              f"{row['GB_per_s_per_pass']:.0f} GB/s, {row['pass_rate_over_norm2_rate']:.2f} of the norm2 rate), "
              f"per-term loop {l_ms:.2f} ms, speed-up {row['speedup']:.2f}", flush=True)

    # single passes of every width: is the widest instantiation slower per term than a narrower one?
    result["single_passes"] = []
    rest = list(range(1, n - 1))
    for label, flip in (("diagonal", None), ("pivot bit 0", n - 1), (f"pivot bit {n - 1}", 0)):
        for width in (1, 2, 4, 8):
            terms = []
            for t in range(width):
                zs = [rest[(3 * t + 5 * j) % len(rest)] for j in range(1 + t % 3)]
                zs = sorted(set(zs))
                terms.append((1.0, ("" if flip is None else "XY"[t % 2]) + "Z" * len(zs), ([] if flip is None else [flip]) + zs))
            assert passes_of(dev, terms) == 1
            samples = [timed(lambda: dev.expect_pauli_sum(terms))[0] for _ in range(reps)]
            ms = statistics.median(samples)
            result["single_passes"].append({"group": label, "terms": width, **stats(samples), "ms_per_term": round(ms / width, 4),
                                            "GB_per_s": round(reg_gb / (ms * 1e-3), 1),
                                            "rate_over_norm2_rate": round(floor_ms / ms, 3)})
            print(f"single pass, {label}, {width} terms: {ms:.3f} ms ({ms / width:.3f} ms/term, {floor_ms / ms:.2f} of the norm2 rate)",
                  flush=True)

    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
