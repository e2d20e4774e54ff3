#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (development time): regenerate tests/golden/mps_sampling.npz.

    python tests/golden/generate_sampling_golden.py <checkout of the reference>

Imports the reference's ``simulators`` package by path and RUNS it; what is written are inputs (site tensors, grid,
seeds) and the reference's outputs (picks, densities) -- data, no reference code.  The tests only read the ``.npz``.

One 4-mode register on a d = 64 grid, bonds capped at 12, built by the reference's own gates, and two cases of 64
seeded chains each on copies of it: ``Mq(0), Mq(0), ...`` (case ``q``) and ``Mp(0), Homodyne(0, pi), Homodyne(0, 0.4),
Mq(0)`` (case ``rot``); the last mode's weights come from ``partial_density_mps(0)`` because the reference returns a bare value
there (gates.py:104-105).  ``rng.choice`` consumes one uniform per measurement, so chain ``s`` seeded with ``seed``
uses row ``s`` of ``default_rng(seed).random((64, 4))`` when the generator is shared by all chains in order.

The generator ASSERTS that every uniform lies at least 1e-6 from every CDF edge of its step (it re-seeds otherwise):
that margin is what makes exact agreement of the picks a fair demand on an implementation that sums in another order.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
SHOTS, MARGIN = 64, 1e-6
ANGLES = (0.4, np.pi)          # Homodyne angles of case "rot": a generic one and one that reduces to -q


def build_register(cv, State, MPS, qs):
    opts = {"max_bond_dim": 12}
    mps = MPS(qs, [])
    rng = np.random.default_rng(5)
    for gate in [cv.Insert(0, State.VACUUM), cv.Insert(1, State.GKP_PLUS, gkp_epsilon=0.3),
                 cv.Insert(2, State.GKP_ZERO, gkp_epsilon=0.35), cv.Insert(3, State.VACUUM), cv.X(0, 0.7), cv.Z(1, 0.5),
                 cv.X(3, -0.4), cv.BS(0, 1, np.pi / 4, **opts), cv.CZ(1, 2, 0.6, **opts), cv.BS(2, 3, 0.5, **opts),
                 cv.BS(1, 2, 0.3, **opts)]:
        gate.apply(mps, rng=rng)
    return mps


def chain_gates(cv, kind: str):
    if kind == "q":
        return [cv.Mq(0) for _ in range(4)]
    # the angle of pi is not last: on the last mode the reference's Homodyne would flip the sign of a bare float
    return [cv.Mp(0), cv.Homodyne(0, ANGLES[1]), cv.Homodyne(0, ANGLES[0]), cv.Mq(0)]


def run_chains(cv, mps, kind: str, seed: int):
    """64 chains sharing one generator; returns values, picks, densities and the smallest CDF margin."""
    rng = np.random.default_rng(seed)
    shadow = np.random.default_rng(seed)          # the same stream, to know which uniform each choice consumed
    qs, dq = mps.domain, mps.diff
    values, picks, densities = (np.zeros((SHOTS, 4)) for _ in range(3))
    margin = np.inf
    for s in range(SHOTS):
        work = mps.copy()
        for k, gate in enumerate(chain_gates(cv, kind)):
            u = shadow.random()
            last = len(work) == 1
            before = work.copy()
            out = gate.apply(work, rng=rng)
            # the distribution the gate drew from: `before` after the gate's own pre-rotation
            if isinstance(gate, cv.Mp):
                before[0] = cv.fourier(qs, before[0], axis=1, inv=True)
            elif isinstance(gate, cv.Homodyne) and not np.isclose(np.sin(gate.arg), 0):
                before[0] = cv.rotation(qs, before[0], -gate.arg, axis=1)
            w = np.real(np.diag(before.partial_density_mps(0))) * dq
            cdf = np.cumsum(w / w.sum())
            cdf /= cdf[-1]
            margin = min(margin, float(np.min(np.abs(cdf - u))))
            pick = int(np.searchsorted(cdf, u, side="right"))
            value = out if last else out.result
            sign = np.round(np.cos(gate.arg)) if isinstance(gate, cv.Homodyne) and np.isclose(np.sin(gate.arg), 0) else 1.0
            assert np.isclose(value, sign * qs[pick]), (s, k, value, qs[pick])
            values[s, k], picks[s, k] = value, pick
            densities[s, k] = w[pick] / dq if last else out.probability
    return values, picks.astype(np.int64), densities, margin


def main(reference: Path) -> None:
    sys.path.insert(0, str(reference))
    from simulators.cv_simulator import gates as cv
    from simulators.cv_simulator.mps import MPS
    from simulators.cv_simulator.states import State

    qs = np.linspace(-8.0, 8.0, 64)
    mps = build_register(cv, State, MPS, qs)
    arrays = {"domain": qs, "angles": np.array(ANGLES), "shapes": np.array([t.shape for t in mps.tensors])}
    for i, t in enumerate(mps.tensors):
        arrays[f"site_{i}"] = np.asarray(t, dtype=np.complex128)
    for kind in ("q", "rot"):
        seed = 11
        while True:
            values, picks, densities, margin = run_chains(cv, mps, kind, seed)
            if margin >= MARGIN:
                break
            seed += 1
        print(f"{kind}: seed {seed}, smallest CDF margin {margin:.3e}, bonds {[t.shape[2] for t in mps.tensors[:-1]]}")
        arrays.update({f"{kind}_seed": np.array(seed), f"{kind}_values": values, f"{kind}_picks": picks,
                       f"{kind}_densities": densities, f"{kind}_margin": np.array(margin)})
    np.savez_compressed(HERE / "mps_sampling.npz", **arrays)
    print(HERE / "mps_sampling.npz", (HERE / "mps_sampling.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(Path(sys.argv[1]))
