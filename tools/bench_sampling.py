#!/usr/bin/env python3
"""Multi-shot MPS sampling (``MPS.sample``) on the d = 1000 grid: one JSON line per configuration.

    python tools/bench_sampling.py [--bonds 16 64 100] [--modes 3 8] [--shots 10000 100000] [--chain-shots 200]

Per configuration (random complex sites, bond ``chi`` throughout): wall time of ``MPS.sample`` (median of ``--repeats``
runs after one warm-up), shots per second, the time of every ``qsv_tensor_sample_site`` call (weights + pick + advance,
the call ends with a stream synchronisation), and ``8 S L d R`` flops of the weights product over that time for the
widest site -- a LOWER bound of the weights kernel's own rate (the environment route does two such products per site,
so the MFMA rate of the kernel is up to twice the figure; ``rocprofv3 --kernel-trace --stats`` has the split).

``--chain-shots N`` times the only way to get the same shots without this feature -- ``copy()`` plus the ``Mq(0)`` chain
per shot -- on the same register for N shots and reports the per-shot ratio (an N-shot extrapolation).
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from quantum_computations_amd import _lib  # noqa: E402
from quantum_computations_amd.cv_simulator import gates as G  # noqa: E402
from quantum_computations_amd.cv_simulator.mps import MPS  # noqa: E402

X = np.linspace(-20, 20, 1000)


def random_sites(seed: int, d: int, m: int, chi: int):
    rng = np.random.default_rng(seed)
    dims = [1] + [chi] * (m - 1) + [1]
    return [(rng.normal(size=(l, d, r)) + 1j * rng.normal(size=(l, d, r))) / np.sqrt(l * d) for l, r in zip(dims, dims[1:])]


def timed_site_calls(mps: MPS, uniforms: np.ndarray):
    """``SiteRegister.sample`` with every library call timed: wraps ``_lib.call`` for the duration of one run."""
    per_call = []
    original = _lib.call

    def call(name, *args):
        if name != "qsv_tensor_sample_site":
            return original(name, *args)
        mps.reg.sync()
        t0 = time.perf_counter()
        original(name, *args)
        per_call.append(time.perf_counter() - t0)

    _lib.call = call
    try:
        mps.reg.sample(uniforms, measure=mps.diff)
    finally:
        _lib.call = original
    return per_call


def chain_seconds_per_shot(mps: MPS, shots: int) -> float:
    rng = np.random.default_rng(1)
    mps.reg.sync()
    t0 = time.perf_counter()
    for _ in range(shots):
        work = mps.copy()
        for _ in range(len(mps)):
            G.Mq(0).apply(work, rng=rng)
    mps.reg.sync()
    return (time.perf_counter() - t0) / shots


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bonds", type=int, nargs="+", default=[16, 64, 100])
    ap.add_argument("--modes", type=int, nargs="+", default=[3, 8])
    ap.add_argument("--shots", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chain-shots", type=int, default=200)
    args = ap.parse_args()
    d = len(X)
    for chi in args.bonds:
        for m in args.modes:
            mps = MPS(X, random_sites(chi + m, d, m, chi))
            chain = chain_seconds_per_shot(mps, args.chain_shots) if args.chain_shots > 0 else None
            for shots in args.shots:
                mps.sample(min(shots, 10_000), rng=0)          # warm-up: pools, operators, code objects
                walls = []
                for rep in range(args.repeats):
                    mps.reg.sync()
                    t0 = time.perf_counter()
                    mps.sample(shots, rng=rep)
                    walls.append(time.perf_counter() - t0)
                wall = float(np.median(walls))
                calls = timed_site_calls(mps, np.random.default_rng(9).random((shots, m)))
                widest = max(range(m), key=lambda k: mps.reg.sites[k].shape[0] * mps.reg.sites[k].shape[2])
                l, _, r = (int(v) for v in mps.reg.sites[widest].shape)
                flops = 8.0 * shots * l * d * r
                line = {"bench": "mps_sampling", "d": d, "bond": chi, "modes": m, "shots": shots,
                        "wall_s": round(wall, 4), "shots_per_s": round(shots / wall, 1),
                        "site_call_ms": [round(1e3 * t, 3) for t in calls],
                        "widest_site": {"L": l, "R": r, "products": 2 if r > 1 else 1,
                                        "weights_tflops_lower_bound": round(flops / calls[widest] / 1e12, 2)}}
                if chain is not None:
                    line["mq_chain_s_per_shot"] = round(chain, 5)
                    line["mq_chain_shots_timed"] = args.chain_shots
                    line["per_shot_ratio_chain_over_sample"] = round(chain / (wall / shots), 1)
                print(json.dumps(line), flush=True)
            mps.reg.close()


if __name__ == "__main__":
    main()
