#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (development time): regenerate tests/golden/ensemble_control.npz.

    python tests/golden/generate_ensemble_control_golden.py <checkout of the reference>

Imports the reference's ``simulators`` package by path and RUNS its ``Simulator``, ``M(result=)``, ``Insert`` and
``ClassicalControl`` on the CPU; what is written are arrays only -- input kets, forced outcomes, eigenvectors, the kets its
gates returned and its result lists.  The tests only read the ``.npz``.

The reference's ``M`` removes the measured qubit.  A measurement that keeps it is stated as
``keep = Insert(q, conj(e_s))(M(q, ...)(psi))``: the generator runs exactly that pair, with ``Insert`` given an object whose
``get()`` returns ``conj(e_s)`` (all ``Insert`` asks of its ``state``), and stores both the removed and the kept ket.

Cases:
  ``teleport_ab``  3-qubit teleportation for the four forced outcome pairs (a, b);
  ``general_s``    one ``M(theta, phi)`` with complex eigenvectors on qubit 1 of a random 3-qubit ket, outcome s forced;
  ``mx_s``         one ``MX`` on qubit 2 of a random 3-qubit ket, outcome s forced;
  ``rep_e``        a distance-3 bit-flip repetition-code cycle on 5 qubits with an X error on data qubit e (e = 3: none): two
                   syndrome measurements, not forced (their outcomes are certain), three corrections that each use positive
                   and negative result indices.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
THETA, PHI = 1.1, 0.7


class Vec:
    """What ``Insert`` asks of its ``state``: ``get()``."""

    def __init__(self, v):
        self._v = np.asarray(v, dtype=np.complex128)

    def get(self):
        return self._v

    def __repr__(self):
        return "Vec"


def random_ket(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    return v / np.linalg.norm(v)


def main(reference: Path) -> None:
    sys.path.insert(0, str(reference))
    from simulators.dv_simulator import gates as G
    from simulators.dv_simulator import numpy_quantum as npq
    from simulators.dv_simulator.simulator import ClassicalControl, Simulator

    def eigs(theta, phi):
        rotation = npq.axis_rotation(phi, [0, 0, 1]) @ npq.axis_rotation(theta, [0, 1, 0])       # as M.apply forms them
        return rotation @ npq.ZERO, rotation @ npq.ONE

    def kept(q, theta, phi, s):
        """``[M(q, result=s), Insert(q, conj(e_s))]``"""
        return [G.M(q, theta, phi, result=s), G.Insert(q, Vec(np.conj(eigs(theta, phi)[s])))]

    arrays = {}

    # ---- teleportation ------------------------------------------------------------------------------------------------------
    message = random_ket(1, 1)
    start = npq.tensor(message, npq.ZERO, npq.ZERO)
    arrays["teleport_message"] = message
    arrays["teleport_in"] = start
    for a in (0, 1):
        for b in (0, 1):
            sim = Simulator([G.H(1), G.CX(1, 2), G.CX(0, 1), G.H(0)] + kept(0, 0.0, 0.0, a) + kept(1, 0.0, 0.0, b) +
                            [ClassicalControl(G.X(2), [1]), ClassicalControl(G.Z(2), [0])])
            arrays[f"teleport_{a}{b}_out"] = sim.run(start)
            arrays[f"teleport_{a}{b}_results"] = np.array(sim.results, dtype=np.int8)

    # ---- single measurements: the removed ket and the kept one ----------------------------------------------------------------------
    for name, q, theta, phi, seed in (("general", 1, THETA, PHI, 2), ("mx", 2, np.pi / 2, 0.0, 3)):
        psi = random_ket(3, seed)
        e0, e1 = eigs(theta, phi)
        arrays[f"{name}_in"] = psi
        arrays[f"{name}_qubit"] = np.array(q)
        arrays[f"{name}_angles"] = np.array([theta, phi])
        arrays[f"{name}_eigs"] = np.stack([e0, e1])
        for s in (0, 1):
            measure, insert = kept(q, theta, phi, s)
            removed, outcome = measure.apply(psi)
            assert outcome == s
            arrays[f"{name}_{s}_removed"] = removed
            arrays[f"{name}_{s}_kept"] = insert.apply(removed)

    # ---- repetition code ----------------------------------------------------------------------------------------------------------
    logical = np.zeros(32, dtype=np.complex128)
    logical[0b00000], logical[0b11100] = 0.6, 0.8j
    arrays["rep_in"] = logical
    for e in (0, 1, 2, 3):
        np.random.seed(100 + e)
        error = [G.X(e)] if e < 3 else []
        syndrome = [G.CX(0, 3), G.CX(1, 3), G.CX(1, 4), G.CX(2, 4)]
        # not forced: M draws with the probabilities (1, 0) or (0, 1); the qubit goes back in the eigenvector it was found in
        results_so_far = []

        class Keep:
            """M followed by the Insert of the outcome M reported: ``Simulator.run`` appends the outcome."""

            def __init__(self, q):
                self.indices = [q]
                self.q = q

            def apply(self, state):
                removed, s = G.MZ(self.q).apply(state)
                results_so_far.append(s)
                return G.Insert(self.q, Vec(np.conj(eigs(0.0, 0.0)[s]))).apply(removed), s

        corrections = [ClassicalControl(G.X(0), [0], [1]), ClassicalControl(G.X(1), [0, 1], []), ClassicalControl(G.X(2), [1], [0])]
        sim = Simulator(error + syndrome + [Keep(3), Keep(4)] + corrections)
        arrays[f"rep_{e}_out"] = sim.run(logical)
        arrays[f"rep_{e}_results"] = np.array(sim.results, dtype=np.int8)

    np.savez(HERE / "ensemble_control.npz", **arrays)
    print(HERE / "ensemble_control.npz", sum(v.nbytes for v in arrays.values()), "bytes of arrays")


if __name__ == "__main__":
    main(Path(sys.argv[1]))
