"""TEST INFRASTRUCTURE: NumPy statement of a trajectory ensemble (quantum_computations_amd/ensemble.py).

Built on ``noise_reference`` one member at a time, so everything that file pins -- the branch rule, the order of the sums, what
a zero-weight branch gives -- holds here by construction.  An ensemble is a list of kets; nothing is shared between members.
"""
from __future__ import annotations

import numpy as np

import noise_reference as R


def block_draws(seed, shots: int, n_channels: int) -> np.ndarray:
    """``draws[s, c]``: what channel ``c`` of shot ``s`` draws.  One block call of NumPy's default generator gives the numbers
    its scalar calls give, in row-major order (test_ensemble_reference_host.py checks that)."""
    return np.random.default_rng(seed).random((int(shots), int(n_channels)))


def ensemble_step(kraus, kets, qubits, n: int, u, forced=None):
    """One member-wise step: ``(new kets, branches, probabilities)``; ``forced[m] = -1`` or ``forced=None``: draw."""
    out, branches, probs = [], [], []
    for m, psi in enumerate(kets):
        f = None if forced is None or int(forced[m]) < 0 else int(forced[m])
        new, j, p = R.trajectory_step(kraus, psi, qubits, n, float(u[m]), f)
        out.append(new)
        branches.append(j)
        probs.append(p)
    return out, np.array(branches, dtype=np.int32), np.array(probs, dtype=np.float64)


class _Fixed:
    """The one method ``R.run_trajectory`` calls on its generator, fed from a row of the block."""

    def __init__(self, row):
        self._row = [float(x) for x in row]
        self._next = 0

    def random(self):
        self._next += 1
        return self._row[self._next - 1]


def n_channels(circuit) -> int:
    return sum(1 for step in circuit if step[0] == "channel")


def run_batched(circuit, ket, n: int, shots: int, seed, batch: int, terms=None):
    """``shots`` trajectories in chunks of ``batch`` members, shot ``s`` and channel ``c`` taking entry ``[s, c]`` of the block;
    the surplus members of the last chunk take ``u = 0`` and are discarded.  Returns ``(final kets, branches, values or None,
    smallest boundary distance)`` -- per shot, in shot order."""
    draws = block_draws(seed, shots, n_channels(circuit))
    full = R.full_matrices(circuit, n)
    finals, branches, closest = [], [], 1.0
    for first in range(0, shots, batch):
        count = min(batch, shots - first)
        rows = np.zeros((batch, draws.shape[1]))
        rows[:count] = draws[first:first + count]
        chunk = [R.run_trajectory(circuit, ket, n, _Fixed(rows[m]), full) for m in range(batch)]
        for final, taken, _, near in chunk[:count]:
            finals.append(final)
            branches.append(taken)
            closest = min(closest, near)
    values = None if terms is None else np.array([R.expect_terms_ket(terms, psi, n) for psi in finals])
    return finals, branches, values, closest
