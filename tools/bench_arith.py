#!/usr/bin/env python3
"""Reversible register arithmetic on one MI355X: ``DeviceState.apply_register_map`` (one gather pass of ``k_arith``) next to
the plain copy of the register and a qubit permutation (bit reversal), all timed in one process.

On a 28-qubit register:

* every kind of map with the target on index bits 8 and up (the LINE form), with ``M = 2^m`` and with an odd modulus, with and
  without a control;
* the four coalescing cases: lowest target bit 0, 1, 2 (the ELEMENT form: reads in runs of 16 / 32 / 64 bytes) and 3, and a random
  value permutation on the lowest bits;
* scattered and reversed operands (one segment per bit);
* ``--items`` : the LINE and ELEMENT rows again with 1, 2 and 4 amplitudes per lane, each in a fresh child process
  (``QSV_ARITH_ITEMS`` is read once per process), the copy timed in each child as its yardstick.

And order finding at full size (``m = 9``, ``t = 18``: 27 qubits): the modular exponentiation in one pass, the 18 controlled
multiplications it replaces, and the inverse Fourier transform, each on its own.

Timing: HIP events on the register's stream around whole calls (``timer_start`` / ``timer_stop``), every shape warmed first,
copy and permutation re-timed next to every group; min / median / max over ``--reps`` repetitions.  A pass reads and writes the
register once: GB/s = 2 x 16 x 2^n bytes over the median.  Before anything is timed every kind is applied and undone at 20
qubits and compared bit for bit.

    python tools/bench_arith.py [--n 28] [--reps 7] [--items] [--out profiles/r20_arith.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from quantum_computations_amd import _lib  # noqa: E402
from quantum_computations_amd import workloads as W  # noqa: E402
from quantum_computations_amd.arithmetic import RegisterMap  # noqa: E402
from quantum_computations_amd.device import DeviceState  # noqa: E402

M_BITS, MX_BITS = 9, 10
ODD = 509              # prime below 2^9


def kinds(odd: bool) -> dict:
    M = ODD if odd else None
    rng = np.random.default_rng(20)
    out = {"add": RegisterMap.add(M_BITS, 123, M), "multiply": RegisterMap.multiply(M_BITS, 7, M),
           "add_register": RegisterMap.add_register(M_BITS, MX_BITS, 5, 3, M), "modexp": RegisterMap.modexp(M_BITS, MX_BITS, 7, M)}
    if not odd:
        out["xor_lookup"] = RegisterMap.xor_lookup(M_BITS, MX_BITS, rng.integers(0, 1 << M_BITS, size=1 << MX_BITS))
        out["permutation"] = RegisterMap.permutation(M_BITS, rng.permutation(1 << M_BITS))
    return out


def qubits_of(n: int, bits) -> list[int]:
    return [n - 1 - b for b in bits]


def self_check() -> None:
    n = 20
    dev = DeviceState.random(n, seed=3)
    before = dev.to_numpy()
    for odd in (False, True):
        for name, op in kinds(odd).items():
            target, source = qubits_of(n, range(M_BITS - 1, -1, -1)), qubits_of(n, range(n - 1, n - 1 - op.mx, -1))
            dev.apply_register_map(op, target[:op.m], source)
            moved = dev.to_numpy()
            assert not np.array_equal(moved, before), name
            dev.apply_register_map(op, target[:op.m], source, inverse=True)
            assert np.array_equal(dev.to_numpy(), before), name
            op.close()
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--items", action="store_true", help="also sweep the amplitudes per lane in child processes")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="profiles/r20_arith.json")
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    n = args.n
    result = {"tool": "tools/bench_arith.py", "reps": args.reps, "n_qubits": n, "register_GB": round(16 * (1 << n) / 1e9, 4),
              "timing": "HIP events around whole calls on the register's stream; min / median / max; copy and permutation re-timed with every group",
              "traffic": "not measured: no counter run was made; a pass is one read and one write of the register",
              "amplitudes_per_lane_cap": 1 << int(os.environ.get("QSV_ARITH_ITEMS", "0"))}
    sweep = []
    if args.items and not args.child:     # children first: they need the memory this process takes below
        for items_log2 in (0, 1, 2):
            env = dict(os.environ, QSV_ARITH_ITEMS=str(items_log2))
            proc = subprocess.run([sys.executable, __file__, "--child", "--n", str(n), "--reps", str(args.reps), "--out", "-"], env=env,
                                  capture_output=True, text=True, timeout=600)
            if proc.returncode != 0:
                raise SystemExit(f"child with QSV_ARITH_ITEMS={items_log2} failed:\n{proc.stderr[-3000:]}")
            sweep.append(json.loads(proc.stdout.strip().splitlines()[-1]))
            print(f"amplitudes per lane <= {1 << items_log2}: " + ", ".join(f"{r['case']} {r['over_copy']}" for r in sweep[-1]["rows"]), flush=True)
    if not args.child:
        self_check()

    dev = DeviceState.random(n, seed=1)
    twin = DeviceState.zeros(n)
    pass_bytes = 2 * 16 * (1 << n)
    reversal = list(range(n))[::-1]

    def timed(fn):
        dev.timer_start()
        fn()
        return dev.timer_stop()

    def stats(samples):
        med = statistics.median(samples)
        return {"min_ms": round(min(samples), 4), "median_ms": round(med, 4), "max_ms": round(max(samples), 4), "GB_per_s": round(pass_bytes / med / 1e6, 1)}

    def contest(contenders: dict) -> dict:
        for fn in contenders.values():
            fn()
        dev.sync()
        samples = {name: [] for name in contenders}
        for _ in range(args.reps):
            for name, fn in contenders.items():
                samples[name].append(timed(fn))
        return {name: stats(values) for name, values in samples.items()}

    yardsticks = {"copy": lambda: dev.copy_into(twin), "permute_bit_reversal": lambda: dev.permute(reversal)}

    def group(title: str, cases: dict) -> dict:
        """cases: label -> (map, target bits, source bits, control bits), bits most significant first"""
        fns = dict(yardsticks)
        kernels = {}
        for label, (op, tbits, sbits, cbits) in cases.items():
            call = (lambda op=op, t=qubits_of(n, tbits), s=qubits_of(n, sbits), c=qubits_of(n, cbits): dev.apply_register_map(op, t, s, c))
            call()
            kernels[label] = dev.last_kernel()
            fns[label] = call
        got = contest(fns)
        copy_ms, perm_ms = got["copy"]["median_ms"], got["permute_bit_reversal"]["median_ms"]
        rows = []
        for label in cases:
            t = got[label]["median_ms"]
            rows.append({"case": label, "kernel": kernels[label], **got[label], "over_copy": round(t / copy_ms, 3), "over_permute": round(t / perm_ms, 3)})
            print(f"{title} | {label}: {t:.3f} ms = {got[label]['GB_per_s']:.0f} GB/s, {t / copy_ms:.2f} x copy, {t / perm_ms:.2f} x permute  [{kernels[label]}]", flush=True)
        return {"group": title, "copy": got["copy"], "permute_bit_reversal": got["permute_bit_reversal"], "rows": rows}

    line_t = list(range(8 + M_BITS - 1, 7, -1))                  # target on bits 8 .. 16
    src_hi = list(range(n - 1, n - 1 - MX_BITS, -1))             # source on the top bits
    pow2, odd = kinds(False), kinds(True)

    def sbits_of(op):
        return src_hi[:op.mx]

    if args.child:
        cases = {"multiply odd M, line": (odd["multiply"], line_t, [], []), "modexp odd M, line": (odd["modexp"], line_t, src_hi, []),
                 "multiply odd M, t0=0": (odd["multiply"], list(range(M_BITS - 1, -1, -1)), [], []),
                 "add 2^m, line": (pow2["add"], line_t, [], [])}
        out = group(f"amplitudes per lane <= {result['amplitudes_per_lane_cap']}", cases)
        out["amplitudes_per_lane_cap"] = result["amplitudes_per_lane_cap"]
        print(json.dumps(out))
        return

    groups = []
    groups.append(group("line form, M = 2^m", {name: (op, line_t, sbits_of(op), []) for name, op in pow2.items()}))
    groups.append(group("line form, odd M", {name: (op, line_t, sbits_of(op), []) for name, op in odd.items()}))
    groups.append(group("line form, one control (bit 7 / bit 0)", {
        "multiply odd M, control bit 7": (odd["multiply"], line_t, [], [7]), "multiply odd M, control bit 0": (odd["multiply"], line_t, [], [0]),
        "modexp odd M, control bit 7": (odd["modexp"], line_t, src_hi, [7]), "add 2^m, control bit 7": (pow2["add"], line_t, [], [7]),
        "xor_lookup, two controls": (pow2["xor_lookup"], line_t, src_hi, [7, 0])}))
    low = {}
    for t0 in (0, 1, 2, 3):
        tbits = list(range(t0 + M_BITS - 1, t0 - 1, -1))
        low[f"multiply odd M, lowest target bit {t0}"] = (odd["multiply"], tbits, [], [])
        low[f"add 2^m, lowest target bit {t0}"] = (pow2["add"], tbits, [], [])
    low["permutation (random table), lowest target bit 0"] = (pow2["permutation"], list(range(M_BITS - 1, -1, -1)), [], [])
    groups.append(group("the four coalescing cases", low))
    scattered = [int(b) for b in np.random.default_rng(21).permutation(np.arange(8, 8 + 2 * M_BITS, 2))]
    groups.append(group("operands of one segment per bit", {
        "multiply odd M, scattered target": (odd["multiply"], scattered, [], []), "multiply odd M, reversed target": (odd["multiply"], line_t[::-1], [], []),
        "modexp odd M, reversed source": (odd["modexp"], line_t, src_hi[::-1], []),
        "add_register odd M, source on bits 0 .. 9": (odd["add_register"], list(range(10 + M_BITS - 1, 9, -1)), list(range(MX_BITS - 1, -1, -1)), [])}))
    result["groups"] = groups
    result["amplitudes_per_lane_sweep"] = sweep
    for op in list(pow2.values()) + list(odd.values()):
        op.close()
    dev.close()
    twin.close()

    # ---- order finding at full size ---------------------------------------------------------------------------------------
    t_bits, N, a = 18, ODD, 2
    nq = t_bits + M_BITS
    dev = DeviceState.zeros(nq)
    twin = DeviceState.zeros(nq)
    gates = {spelled: W.to_gates(W.order_finding_ops(a, N, t_bits, spelled=spelled)) for spelled in (False, True)}
    for gate in gates[False][:t_bits + 1]:       # the Hadamards and the X: a state of the right kind under the timed maps
        gate.apply(dev)
    one_pass, spelled, qft = gates[False][t_bits + 1], gates[True][t_bits + 1:-1], gates[False][-1]
    assert len(spelled) == t_bits
    pass_bytes = 2 * 16 * (1 << nq)
    got = contest({"copy": lambda: dev.copy_into(twin), "modexp_one_pass": lambda: one_pass.apply(dev),
                   "controlled_multiplications": lambda: [g.apply(dev) for g in spelled], "inverse_qft": lambda: qft.apply(dev)})
    one_pass.apply(dev)
    kernel = dev.last_kernel()
    for name in ("controlled_multiplications", "inverse_qft"):      # several passes each: no single-pass rate
        del got[name]["GB_per_s"]
    result["order_finding"] = {"a": a, "N": N, "t": t_bits, "m": M_BITS, "n_qubits": nq, "kernel_of_the_one_pass": kernel, **got,
                               "multiplications_over_one_pass": round(got["controlled_multiplications"]["median_ms"] / got["modexp_one_pass"]["median_ms"], 2),
                               "one_pass_over_copy": round(got["modexp_one_pass"]["median_ms"] / got["copy"]["median_ms"], 3)}
    print(f"order finding n={nq}: modexp in one pass {got['modexp_one_pass']['median_ms']:.3f} ms [{kernel}], {t_bits} controlled multiplications "
          f"{got['controlled_multiplications']['median_ms']:.3f} ms, inverse QFT {got['inverse_qft']['median_ms']:.3f} ms, copy {got['copy']['median_ms']:.3f} ms", flush=True)
    dev.close()
    twin.close()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
