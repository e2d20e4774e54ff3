#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (development time): regenerate tests/golden/mps_canonical.npz.

    python tests/golden/generate_canonical_golden.py <checkout of the reference>

Imports the reference's ``simulators`` package by path and RUNS it; what is written are arrays only -- the site tensors
of registers the reference's own gates produced, its ``norm()``, amplitudes of its ``contract()`` and the Schmidt values
of every bond, computed here by ``numpy.linalg.svd`` of the reference's contracted tensor reshaped at that bond.  The
tests only read the ``.npz``.

Registers (grid of d = 64 points on [-8, 8]):
  ``gates``  3 modes, BS / CZ / CX with ``max_bond_dim = 10``;
  ``bell``   a GKP Bell pair (``InsertBell``) and a vacuum mode mixed into it by a beam splitter, ``max_bond_dim = 8``;
  ``tight``  4 modes, BS / CZ / CX with ``rel_err = 1e-2``: the bonds are as narrow as that tolerance lets them be.
The whole ``contract()`` of a d = 64 register is 4 MB (3 modes) or 268 MB (4 modes), beyond what a committed file may
hold: the file keeps the amplitudes at every ``stride``-th grid point of every mode (stride 4 / 8: 4096 amplitudes), which
is what the state checks compare; the Schmidt values are those of the whole tensor.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent


def build(cv, gkp_bell, State, MPS, qs, name):
    rng = np.random.default_rng(7)
    mps = MPS(qs, [])
    if name == "gates":
        o = {"max_bond_dim": 10}
        gates = [cv.Insert(0, State.VACUUM), cv.Insert(1, State.GKP_PLUS, gkp_epsilon=0.3),
                 cv.Insert(2, State.GKP_ZERO, gkp_epsilon=0.35), cv.X(0, 0.7), cv.Z(1, 0.5),
                 cv.BS(0, 1, np.pi / 4, **o), cv.CZ(1, 2, 0.6, **o), cv.CX(0, 1, 0.4, **o), cv.BS(1, 2, 0.5, **o)]
    elif name == "bell":
        o = {"max_bond_dim": 8}
        gates = [gkp_bell.InsertBell(0, gkp_bell.GKPBellState.PLUS, gkp_epsilon=0.3), cv.Insert(2, State.VACUUM),
                 cv.X(2, 0.5), cv.BS(1, 2, np.pi / 5, **o)]
    else:
        o = {"rel_err": 1e-2}
        gates = [cv.Insert(0, State.VACUUM), cv.Insert(1, State.GKP_PLUS, gkp_epsilon=0.3),
                 cv.Insert(2, State.GKP_ZERO, gkp_epsilon=0.35), cv.Insert(3, State.VACUUM), cv.X(0, 0.7), cv.X(3, -0.4),
                 cv.BS(0, 1, np.pi / 4, **o), cv.CZ(1, 2, 0.6, **o), cv.BS(2, 3, 0.5, **o), cv.CX(1, 2, 0.3, **o)]
    for gate in gates:
        gate.apply(mps, rng=rng)
    return mps


def main(reference: Path) -> None:
    sys.path.insert(0, str(reference))
    from simulators.cv_simulator import gates as cv
    from simulators.cv_simulator.mps import MPS
    from simulators.cv_simulator.states import State
    from simulators.gkp_simulator import insert_bell as gkp_bell

    qs = np.linspace(-8.0, 8.0, 64)
    arrays = {"domain": qs, "names": np.array(["gates", "bell", "tight"])}
    for name in ("gates", "bell", "tight"):
        mps = build(cv, gkp_bell, State, MPS, qs, name)
        m = len(mps)
        psi = np.asarray(mps.contract(), dtype=np.complex128)
        stride = 4 if m == 3 else 8
        arrays[f"{name}_modes"] = np.array(m)
        arrays[f"{name}_stride"] = np.array(stride)
        arrays[f"{name}_norm"] = np.array(mps.norm())
        arrays[f"{name}_contract_strided"] = psi[(slice(None, None, stride),) * m]
        arrays[f"{name}_max_amplitude"] = np.array(np.max(np.abs(psi)))
        for i, t in enumerate(mps.tensors):
            arrays[f"{name}_site_{i}"] = np.asarray(t, dtype=np.complex128)
        for b in range(m - 1):
            arrays[f"{name}_schmidt_{b}"] = np.linalg.svd(psi.reshape(64 ** (b + 1), -1), compute_uv=False)
        print(name, [t.shape for t in mps.tensors], "norm", mps.norm(), flush=True)
    np.savez_compressed(HERE / "mps_canonical.npz", **arrays)
    print(HERE / "mps_canonical.npz", (HERE / "mps_canonical.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(Path(sys.argv[1]))
