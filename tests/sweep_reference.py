"""TEST INFRASTRUCTURE: the NumPy statement of the per-member parameter calls of an ensemble, member by
member on the references the single-register calls are tested against: ``pauli_rotation_reference.rotate_list``,
``diagonal_reference.phase`` / ``moments`` / ``qaoa_state`` and a plain ``apply_kq``.  Nothing here touches the device or the
library.  tests/test_sweep_reference_host.py pins the parameter-shift rule of this model against the adjoint gradients.

Index convention of the project: qubit q of n is bit n - 1 - q of the amplitude index.
"""
from __future__ import annotations

import numpy as np

import diagonal_reference as D
import pauli_rotation_reference as P


def with_angles(rotations, row) -> list:
    """The list with its angles replaced by ``row``."""
    assert len(row) == len(rotations)
    return [(float(theta), letters, list(qubits)) for theta, (_, letters, qubits) in zip(row, rotations)]


def rotate_members(kets, rotations, thetas) -> list[np.ndarray]:
    """Member m becomes ``rotate_list(kets[m], rotations with row m of thetas)``."""
    return [P.rotate_list(ket, with_angles(rotations, row)) for ket, row in zip(kets, thetas)]


def phase_members(kets, d, gammas) -> list[np.ndarray]:
    return [D.phase(np.asarray(ket, dtype=complex), d, float(gamma)) for ket, gamma in zip(kets, gammas)]


def moments_members(kets, d, threshold=None) -> np.ndarray:
    """``[members, 4]``: sum p, sum p d, sum p d^2, sum_{d <= threshold} p."""
    return np.array([D.moments(np.asarray(ket, dtype=complex), d, threshold) for ket in kets])


def apply_kq(ket, n: int, qubits, matrix) -> np.ndarray:
    """``matrix`` (2^k x 2^k, ``qubits[0]`` the most significant bit of its indices) on ``qubits`` of an n-qubit ket."""
    k = len(qubits)
    t = np.asarray(ket, dtype=complex).reshape((2,) * n)
    t = np.moveaxis(t, [int(q) for q in qubits], range(k)).reshape(1 << k, -1)
    t = (np.asarray(matrix, dtype=complex) @ t).reshape((2,) * n)
    return np.moveaxis(t, range(k), [int(q) for q in qubits]).reshape(-1)


def matrices_members(kets, n: int, qubits, matrices) -> list[np.ndarray]:
    return [apply_kq(ket, n, qubits, m) for ket, m in zip(kets, matrices)]


def pauli_energy(ket, terms) -> float:
    """``<ket| sum_t c_t P_t |ket>`` for real c_t (not divided by the norm)."""
    ket = np.asarray(ket, dtype=complex)
    return float(sum(float(np.real(c)) * np.vdot(ket, P.apply_string(ket, letters, qubits)).real for c, letters, qubits in terms))


def energies(rotations, thetas, terms, ket) -> np.ndarray:
    return np.array([pauli_energy(P.rotate_list(ket, with_angles(rotations, row)), terms) for row in thetas])


def shifted_rows(theta) -> np.ndarray:
    """``theta``, then ``theta + pi/2 e_r`` and ``theta - pi/2 e_r`` for every r: the 2 R + 1 rows of a parameter-shift sweep."""
    theta = np.asarray(theta, dtype=float).reshape(-1)
    rows = np.tile(theta, (2 * theta.size + 1, 1))
    for r in range(theta.size):
        rows[1 + 2 * r, r] += 0.5 * np.pi
        rows[2 + 2 * r, r] -= 0.5 * np.pi
    return rows


def parameter_shift(rotations, theta, terms, ket) -> tuple[float, np.ndarray]:
    """``(E, dE/dtheta)``: exact for Pauli rotations, ``dE/dtheta_r = (E_+ - E_-) / 2``."""
    values = energies(rotations, shifted_rows(theta), terms, ket)
    return float(values[0]), 0.5 * (values[1::2] - values[2::2])


def qaoa_energies(d, gammas, betas) -> np.ndarray:
    return np.array([D.qaoa_energy(d, g, b) for g, b in zip(np.atleast_2d(gammas), np.atleast_2d(betas))])
