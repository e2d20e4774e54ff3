#!/usr/bin/env python3
"""Subsystem read-out on one MI355X: reduced states of k = 7 .. 12 qubits and marginals of an n-qubit
register, timed in the same process against

  (a) ``norm2``, the read-pass floor -- the yardstick for the marginals and for small k;
  (b) ``3 * 2^(n+k)`` real flops expressed as TFLOP/s, next to the k = 6 dense kernel (``reduced_density``, k_rdm_tile<4>);
  (c) ``torch`` computing ``M @ M.conj().T`` (rocBLAS) on the one placement where M is a contiguous row-major view of the
      register: the kept qubits on the top bits, in order;
  (d) the download of the whole ket that the feature makes unnecessary.

Kept qubits sit on the lowest bits, the highest bits and scattered over the register.  Reduced states are timed with HIP
events on the register's stream (the call does not wait); everything that ends in a synchronisation of its own (marginals,
``norm2``, the download) with the host clock around the call.  Every contender is warmed first; medians over ``--reps``.

    python tools/bench_subsystem.py [--n 28] [--reps 7] [--out profiles/r15_subsystem.json]
    rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d DIR -- python tools/bench_subsystem.py --one-call 10
    python tools/bench_subsystem.py --counters DIR        # adds the byte ratio of that call to the JSON

``--one-call K`` makes a single reduced-state call of K scattered qubits and nothing else: the run counters are collected in
(one counter per run: FETCH_SIZE and WRITE_SIZE together exceed what the hardware collects in one pass).
"""
from __future__ import annotations

import argparse
import csv
import json
import re
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from quantum_computations_amd import _lib  # noqa: E402
from quantum_computations_amd.device import DeviceState, _ints  # noqa: E402


def placements(n, k):
    """Qubit q sits on bit n-1-q.  ``top`` lists the top bits in order: M is then a row-major view of the register."""
    step = (n - 1) / (k - 1) if k > 1 else 0
    scattered = sorted({int(round(j * step)) for j in range(k)})
    scattered += [q for q in range(n) if q not in scattered][:k - len(scattered)]      # where rounding made two legs meet
    return {"low": [n - 1 - b for b in range(k)][::-1], "top": list(range(k)), "scattered": scattered}


def stats(samples):
    return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4)}


def counters(directory, n, k):
    """FETCH_SIZE per kernel of the ``--one-call`` run, in bytes, against the register's bytes.  The counter is in KiB and, on
    gfx950, counts a wide read once: it is doubled, as profiles/r05_pmc_traffic.md does.  ``k_scale`` of the same run (the
    normalisation of the random ket: one read of the register) is the check of that factor: its ratio must come out as 1."""
    sums = {}
    for f in Path(directory).rglob("*_counter_collection.csv"):
        for row in csv.DictReader(f.open()):
            m = re.search(r"(k_\w+)", row["Kernel_Name"])
            name = m.group(1) if m else row["Kernel_Name"]
            if name.startswith(("k_subsys", "k_marginal", "k_scale")) and row["Counter_Name"] == "FETCH_SIZE":
                sums[name] = sums.get(name, 0.0) + 2.0 * 1024.0 * float(row["Counter_Value"])
    register = 16.0 * (1 << n)
    out = {"n_qubits": n, "k": k, "register_bytes": register, "fetch_bytes": {name: round(v) for name, v in sums.items()},
           "fetch_over_register": {name: round(v / register, 3) for name, v in sums.items()},
           "model_rows_read_over_register": (1 << k) // 64,
           "note": "FETCH_SIZE in KiB, doubled (gfx950 wide reads); k_scale reads the register once and calibrates the factor"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="profiles/r15_subsystem.json")
    ap.add_argument("--one-call", type=int, default=0, metavar="K")
    ap.add_argument("--counters", default="", metavar="DIR")
    args = ap.parse_args()
    n, reps = args.n, args.reps
    path = Path(args.out)
    if args.counters:
        result = json.loads(path.read_text()) if path.exists() else {"tool": "tools/bench_subsystem.py"}
        k = int(result.get("pmc_call_k", 10))
        result["pmc_one_call"] = counters(args.counters, int(result.get("n_qubits", n)), k)
        path.write_text(json.dumps(result, indent=1) + "\n")
        print(json.dumps(result["pmc_one_call"], indent=1))
        return
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    psi = DeviceState.random(n, seed=1)
    if args.one_call:
        rho = psi.reduced_density_state(placements(n, args.one_call)["scattered"])
        psi.sync()
        print(f"one call: n={n} k={args.one_call} {psi.last_kernel()} trace {rho.trace():.15f}")
        return

    reg_gb = 16 * (1 << n) / 1e9
    result = {"tool": "tools/bench_subsystem.py", "n_qubits": n, "register_GB": round(reg_gb, 4), "reps": reps, "pmc_call_k": 10,
              "timing": "reduced states: HIP events on the register's stream; marginals, norm2, download: host clock around the "
                        "synchronising call; medians over reps, every contender warmed first",
              "reduced_state": {}, "marginals": {}}

    def save():
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1) + "\n")

    def host_timed(fn):
        fn()
        samples = []
        for _ in range(reps):
            psi.sync()
            start = time.perf_counter()
            fn()
            samples.append((time.perf_counter() - start) * 1e3)
        return stats(samples)

    def event_timed(fn):
        fn()
        samples = []
        for _ in range(reps):
            psi.timer_start()
            fn()
            samples.append(psi.timer_stop())
        return stats(samples)

    # (a) the read-pass floor, and the k = 6 dense kernel for (b)
    floor = host_timed(psi.norm2)
    result["norm2_floor"] = {**floor, "GB_per_s": round(reg_gb / (floor["median_ms"] * 1e-3), 1)}
    print(f"norm2: {floor['median_ms']:.3f} ms ({result['norm2_floor']['GB_per_s']} GB/s)", flush=True)
    dense = {}
    for name, qubits in placements(n, 6).items():
        got = host_timed(lambda: psi.reduced_density(qubits))
        dense[name] = {**got, "kernel": psi.last_kernel(), "TFLOP_per_s": round(3 * 2.0 ** (n + 6) / (got["median_ms"] * 1e-3) / 1e12, 2)}
        print(f"k=6 dense {name}: {got['median_ms']:.3f} ms, {dense[name]['TFLOP_per_s']} TFLOP/s ({psi.last_kernel()})", flush=True)
    result["dense_k6_reduced_density"] = dense
    save()

    # reduced states, k = 7 .. 12
    for k in range(7, 13):
        row = {}
        rho = DeviceState.zeros(2 * k)               # allocated once: the calls below are the library's work alone
        for name, qubits in placements(n, k).items():
            got = event_timed(lambda: _lib.call("qsv_reduced_density_state", psi._h, k, _ints(qubits), rho._h))
            ms = got["median_ms"]
            row[name] = {**got, "kernel": psi.last_kernel(), "TFLOP_per_s": round(3 * 2.0 ** (n + k) / (ms * 1e-3) / 1e12, 2),
                         "over_norm2_floor": round(ms / floor["median_ms"], 2),
                         "model_traffic_GB": round(reg_gb * (1 << k) / 64, 1)}
            print(f"k={k} {name}: {ms:.3f} ms, {row[name]['TFLOP_per_s']} TFLOP/s, {row[name]['over_norm2_floor']} x norm2", flush=True)
        rho.close()
        result["reduced_state"][f"k{k}"] = row
        save()

    # marginals
    for k in (1, 3, 6, 10, 12, 16, 20):
        row = {}
        for name, qubits in placements(n, k).items():
            got = host_timed(lambda: psi.marginal_probabilities(qubits))
            row[name] = {**got, "kernel": psi.last_kernel(), "over_norm2_floor": round(got["median_ms"] / floor["median_ms"], 2),
                         "GB_per_s": round(reg_gb / (got["median_ms"] * 1e-3), 1)}
            print(f"marginal k={k} {name}: {got['median_ms']:.3f} ms ({psi.last_kernel()})", flush=True)
        result["marginals"][f"k{k}"] = row
        save()

    # (d) the download the feature replaces
    start = time.perf_counter()
    host = psi.to_numpy()
    result["download_whole_ket_ms"] = round((time.perf_counter() - start) * 1e3, 1)
    print(f"download of the ket: {result['download_whole_ket_ms']} ms", flush=True)
    del host
    save()

    # (c) rocBLAS through torch on the contiguous placement
    try:
        import torch
    except ImportError:
        result["torch_rocblas"] = "torch not installed"
        save()
        return
    t = torch.view_as_complex(torch.randn((1 << n, 2), dtype=torch.float64, device="cuda"))
    t /= torch.linalg.vector_norm(t)
    rows = {}
    for k in range(7, 13):
        m = t.view(1 << k, -1)
        torch.matmul(m, m.conj().T)
        torch.cuda.synchronize()
        samples = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = torch.matmul(m, m.conj().T)
            b.record()
            torch.cuda.synchronize()
            samples.append(a.elapsed_time(b))
        got = stats(samples)
        ours = result["reduced_state"][f"k{k}"]["top"]["median_ms"]
        rows[f"k{k}"] = {**got, "TFLOP_per_s_3M_convention": round(3 * 2.0 ** (n + k) / (got["median_ms"] * 1e-3) / 1e12, 2),
                         "tiled_kernel_top_ms": ours, "tiled_over_torch": round(ours / got["median_ms"], 2),
                         "tiled_is_slower": bool(ours > got["median_ms"])}
        print(f"torch M M^H k={k}: {got['median_ms']:.3f} ms (tiled kernel, top placement: {ours:.3f} ms)", flush=True)
        del out
    result["torch_rocblas"] = rows
    save()


if __name__ == "__main__":
    main()
