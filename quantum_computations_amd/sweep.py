"""Parameter sweeps: one Pauli-rotation circuit at many parameter points, ``batch`` points per register.

``M`` points are cut into chunks of a power of two of members, at most ``batch`` each; a chunk is one :class:`Ensemble`
whose members take their own row of angles through ``apply_pauli_rotations`` and read their own energy through
``expect_pauli_sum``.  Below about ``2^22`` amplitudes a launch costs more than the data it moves, so one launch per gate for
``batch`` points is what makes a landscape, a parameter-shift gradient or a line search cheap.
"""
from __future__ import annotations

from typing import Iterator

import numpy as np

from .ensemble import Ensemble


def chunks(points: int, batch: int) -> Iterator[tuple[int, int, int]]:
    """``(first, count, members)`` for every chunk of ``points`` parameter points: the chunks cover ``0 .. points - 1`` in
    order and exactly once, ``members`` is the power of two at or above ``count`` and at most ``batch`` rounded down to a
    power of two.  Pure host logic."""
    points, batch = int(points), int(batch)
    if points < 0:
        raise ValueError("a negative number of points")
    if batch < 1:
        raise ValueError("batch must be at least 1")
    cap = 1 << (batch.bit_length() - 1)
    first = 0
    while first < points:
        count = min(cap, points - first)
        members = 1 << (count - 1).bit_length()
        yield first, count, members
        first += count


def _default_ket(rotations, terms, ket) -> np.ndarray:
    if ket is not None:
        return np.ascontiguousarray(ket, dtype=np.complex128)
    top = max((int(q) for _, _, qs in list(rotations) + list(terms) for q in qs), default=0)
    out = np.zeros(1 << (top + 1), dtype=np.complex128)
    out[0] = 1.0
    return out


def energies(rotations, thetas, terms, ket=None, batch: int = 256, device: int = 0) -> np.ndarray:
    """``E[m] = <psi_m| H |psi_m>`` with ``psi_m = U(thetas[m]) ket`` for ``rotations = [(theta, letters, qubits), ...]`` (the
    list's own angles are overridden), ``thetas[M, R]`` and ``H = terms`` (real coefficients).  ``ket``: ``|0...0>`` on the
    qubits the lists mention when None.  Surplus members of the last chunk take rows of zeros and are dropped."""
    rotations = [(0.0, str(paulis), [int(q) for q in qs]) for _, paulis, qs in rotations]
    terms = list(terms)
    thetas = np.asarray(thetas, dtype=np.float64)
    if thetas.ndim != 2 or thetas.shape[1] != len(rotations):
        raise ValueError("thetas must have shape [points, rotations]")
    ket = _default_ket(rotations, terms, ket)
    out = np.zeros(thetas.shape[0], dtype=np.float64)
    ens = None
    try:
        for first, count, members in chunks(thetas.shape[0], batch):
            if ens is None or ens.members != members:
                if ens is not None:
                    ens.close()
                ens = Ensemble.from_ket(ket, members, device)
            else:
                ens.reset(ket)
            rows = np.zeros((members, len(rotations)), dtype=np.float64)
            rows[:count] = thetas[first:first + count]
            ens.apply_pauli_rotations(rotations, rows)
            out[first:first + count] = ens.expect_pauli_sum(terms)[:count]
    finally:
        if ens is not None:
            ens.close()
    return out


def energies_and_gradients(rotations, thetas, terms, ket=None, batch: int = 256, device: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """``(E[M], G[M, R])`` with ``E[m]`` as in ``energies`` and ``G[m, r] = dE[m] / dtheta[m, r]`` by the adjoint method, every
    point a member: per chunk the rotations forward, ``lambda_m = H psi_m``, ``E_m = Re <psi_m|lambda_m>``
    and one backward walk whose values give ``G = Im <lambda_m|P_r|psi_m>`` -- about three forward walks per chunk, where
    ``parameter_shift`` spends ``2 R + 1`` members on one point.  ``H`` must be hermitian (real coefficients).  Surplus
    members of the last chunk take rows of zeros and are dropped."""
    from .device import DeviceState, _check_terms, _real_terms

    rotations = [(0.0, str(paulis), [int(q) for q in qs]) for _, paulis, qs in rotations]
    terms = _real_terms(terms, "the gradient")
    thetas = np.asarray(thetas, dtype=np.float64)
    if thetas.ndim != 2 or thetas.shape[1] != len(rotations):
        raise ValueError("thetas must have shape [points, rotations]")
    ket = _default_ket(rotations, terms, ket)
    n = ket.shape[0].bit_length() - 1
    _check_terms(terms, n)
    _check_terms(rotations, n)
    energy = np.zeros(thetas.shape[0], dtype=np.float64)
    gradient = np.zeros(thetas.shape, dtype=np.float64)
    ens = lam = None
    try:
        for first, count, members in chunks(thetas.shape[0], batch):
            if ens is None or ens.members != members:      # both ensembles of a chunk before anything is touched
                for old in (ens, lam):
                    if old is not None:
                        old.close()
                ens = lam = None
                ens = Ensemble.from_ket(ket, members, device)
                lam = Ensemble(DeviceState.zeros(n + members.bit_length() - 1, device), n)
            else:
                ens.reset(ket)
            rows = np.zeros((members, len(rotations)), dtype=np.float64)
            rows[:count] = thetas[first:first + count]
            ens.apply_pauli_rotations(rotations, rows)
            ens.apply_pauli_sum(terms, out=lam)
            energy[first:first + count] = ens.inner(lam).real[:count]
            gradient[first:first + count] = ens.pauli_rotations_adjoint(rotations, lam, rows).imag[:count]
    finally:
        for old in (ens, lam):
            if old is not None:
                old.close()
    return energy, gradient


def parameter_shift(rotations, theta, terms, ket=None, batch: int = 256, device: int = 0) -> tuple[float, np.ndarray]:
    """``(E(theta), dE/dtheta)`` by the parameter-shift rule, exact for Pauli rotations ``exp(-i theta_r / 2 P_r)``:
    ``dE/dtheta_r = (E(theta + pi/2 e_r) - E(theta - pi/2 e_r)) / 2``.  The ``2 R + 1`` circuits run as one sweep."""
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    count = theta.shape[0]
    rows = np.tile(theta, (2 * count + 1, 1))
    for r in range(count):
        rows[1 + 2 * r, r] += 0.5 * np.pi
        rows[2 + 2 * r, r] -= 0.5 * np.pi
    values = energies(rotations, rows, terms, ket=ket, batch=batch, device=device)
    return float(values[0]), 0.5 * (values[1::2] - values[2::2])
