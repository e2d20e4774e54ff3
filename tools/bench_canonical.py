#!/usr/bin/env python3
"""Time ``SiteRegister.canonicalise(0)`` and ``compress(max_bond_dim = chi / 2)`` on random registers (d = 1000, 8 modes,
bonds 16 / 64 / 100; median of 3 after a warm-up) next to the same sweeps done with ``torch.linalg.qr`` /
``torch.linalg.svd`` + ``torch.matmul`` on the same device tensors, and record the accuracy figures of
tests/test_gpu_canonical.py's checks.  Writes profiles/r07_canonical.json (or ``--out``).

    python tools/bench_canonical.py [--out FILE] [--bonds 16 64 100] [--modes 8] [--d 1000]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import canonical_reference as ref  # noqa: E402
from quantum_computations_amd.cv_simulator.site_register import SiteRegister, _torch, kept_rank  # noqa: E402


def timed(fn, repeats=3):
    torch = _torch()
    fn()                                   # warm-up
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def torch_canonicalise(sites):
    """All the way right with QR, back to site 0 with SVD: the sweep of ``canonicalise(0)`` on torch operators."""
    torch = _torch()
    sites = list(sites)
    for k in range(len(sites) - 1):
        cl, d, cr = sites[k].shape
        q, r = torch.linalg.qr(sites[k].reshape(cl * d, cr))
        sites[k] = q.reshape(cl, d, -1)
        sites[k + 1] = torch.matmul(r, sites[k + 1].reshape(cr, -1)).reshape(r.shape[0], d, -1)
    return sites


def torch_back_sweep(sites, cap=None):
    torch = _torch()
    for k in range(len(sites) - 1, 0, -1):
        cl, d, cr = sites[k].shape
        u, s, vh = torch.linalg.svd(sites[k].reshape(cl, d * cr), full_matrices=False)
        keep = len(s) if cap is None else min(cap, len(s))
        sites[k] = vh[:keep].reshape(keep, d, cr)
        carry = u[:, :keep] * s[:keep]
        pl, pd, _ = sites[k - 1].shape
        sites[k - 1] = torch.matmul(sites[k - 1].reshape(pl * pd, cl), carry).reshape(pl, pd, keep)
    return sites


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "r07_canonical.json"))
    ap.add_argument("--bonds", type=int, nargs="+", default=[16, 64, 100])
    ap.add_argument("--modes", type=int, default=8)
    ap.add_argument("--d", type=int, default=1000)
    args = ap.parse_args()
    torch = _torch()
    record = {"device": torch.cuda.get_device_name(0), "d": args.d, "modes": args.modes, "timings": []}
    try:
        torch.linalg.qr(torch.zeros(8, 4, dtype=torch.complex128, device="cuda"))
        record["torch_qr_complex128"] = True
    except Exception as exc:  # noqa: BLE001
        record["torch_qr_complex128"] = False
        record["torch_qr_error"] = str(exc)
    for chi in args.bonds:
        rng = np.random.default_rng(chi)
        host = ref.random_register(rng, args.d, [chi] * (args.modes - 1))
        reg = SiteRegister(host, args.d)
        base = [t.clone() for t in reg.sites]

        def ours_canonicalise():
            reg.sites = [t.clone() for t in base]
            reg.canonicalise(0)

        def ours_compress():
            reg.sites = [t.clone() for t in base]
            reg.compress(0, max_bond_dim=chi // 2)

        row = {"bond": chi, "canonicalise_s": timed(ours_canonicalise), "compress_s": timed(ours_compress)}
        if record["torch_qr_complex128"]:
            row["torch_canonicalise_s"] = timed(lambda: torch_back_sweep(torch_canonicalise(base)))
            row["torch_compress_s"] = timed(lambda: torch_back_sweep(torch_canonicalise(base), cap=chi // 2))
        record["timings"].append(row)
        print(json.dumps(row), flush=True)
        Path(args.out).write_text(json.dumps(record, indent=1) + "\n")      # rows survive a run that is cut short
    # accuracy: the figures of checks 1-3 of tests/test_gpu_canonical.py (GPU route next to the NumPy restatement on the
    # same input) for the reference's registers of tests/golden/mps_canonical.npz and one random register
    golden = np.load(REPO / "tests" / "golden" / "mps_canonical.npz", allow_pickle=False)
    cases = {name: [np.array(golden[f"{name}_site_{i}"]) for i in range(int(golden[f"{name}_modes"]))]
             for name in ("gates", "bell", "tight")}
    cases["random d=64 bonds [10, 40]"] = ref.random_register(np.random.default_rng(1), 64, [10, 40])
    record["accuracy"] = {}
    for name, host in cases.items():
        psi = ref.contract(host)
        top = float(np.max(np.abs(psi)))
        dense = ref.dense_schmidt(psi) if psi.size <= 64 ** 3 else None
        rows = []
        for centre in range(len(host)):
            reg = SiteRegister(host, host[0].shape[1])
            values = reg.canonicalise(centre)
            got = reg.site_arrays()
            want_sites, want_values = ref.canonicalise(host, centre)
            row = {"centre": centre,
                   "gauge_defect": ref.gauge_defect(got, centre), "gauge_defect_restatement": ref.gauge_defect(want_sites, centre),
                   "state_change": float(np.max(np.abs(reg.to_numpy() - psi))) / top,
                   "state_change_restatement": float(np.max(np.abs(ref.contract(want_sites) - psi))) / top}
            if dense is not None:
                row["schmidt_abs_over_s0"] = max(float(np.max(np.abs(a - b[: len(a)])) / b[0]) for a, b in zip(values, dense))
                row["schmidt_abs_over_s0_restatement"] = max(float(np.max(np.abs(a - b[: len(a)])) / b[0])
                                                            for a, b in zip(want_values, dense))
            else:
                row["schmidt_abs_over_s0_vs_restatement"] = max(float(np.max(np.abs(a - b[: len(a)])) / b[0])
                                                               for a, b in zip(values, want_values))
            rows.append(row)
        record["accuracy"][name] = rows
    Path(args.out).write_text(json.dumps(record, indent=1) + "\n")
    print(args.out)


if __name__ == "__main__":
    main()
