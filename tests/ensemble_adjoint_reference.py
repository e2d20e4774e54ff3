"""TEST INFRASTRUCTURE: the NumPy statement of the per-member adjoint calls of an ensemble, member by
member on the references the single-register calls are tested against: ``pauli_operator_reference.adjoint_values``,
``diagonal_reference.phase_adjoint`` and ``np.vdot``.  Nothing here touches the device or the library.
tests/test_ensemble_adjoint_reference_host.py pins the gradients of this model against the parameter-shift rule of
``sweep_reference`` and the QAOA form against ``diagonal_reference.qaoa_energy_and_gradient``.

Index convention of the project: qubit q of n is bit n - 1 - q of the amplitude index.
"""
from __future__ import annotations

import numpy as np

import diagonal_reference as D
import pauli_operator_reference as O
import pauli_rotation_reference as P
import sweep_reference as S


def inner_members(a, b) -> np.ndarray:
    """``values[m] = <a_m|b_m>``."""
    return np.array([np.vdot(x, y) for x, y in zip(a, b)], dtype=complex)


def rotations_adjoint_members(rotations, thetas, psis, lams):
    """``(values[members, R], rewound psis, rewound lams)``: ``adjoint_values`` per member with row m of ``thetas``."""
    values, out_psi, out_lam = [], [], []
    for row, psi, lam in zip(thetas, psis, lams):
        v, p, l = O.adjoint_values(S.with_angles(rotations, row), psi, lam)
        values.append(v)
        out_psi.append(p)
        out_lam.append(l)
    return np.array(values, dtype=complex).reshape(len(psis), len(rotations)), out_psi, out_lam


def diag_phase_adjoint_members(d, gammas, psis, lams):
    """``(values[members], psis', lams')``: ``<lam_m|D|psi_m>`` of the inputs, then both take ``exp(-i gammas[m] d)``."""
    out = [D.phase_adjoint(np.asarray(psi, dtype=complex), np.asarray(lam, dtype=complex), d, float(g)) for g, psi, lam in zip(gammas, psis, lams)]
    return np.array([v for v, _, _ in out], dtype=complex), [p for _, p, _ in out], [l for _, _, l in out]


def apply_sum_members(terms, kets) -> list[np.ndarray]:
    return [O.apply_sum(terms, ket) for ket in kets]


def energies_and_gradients(rotations, thetas, terms, ket):
    """``sweep.energies_and_gradients`` step for step: forward, ``lambda = H psi``, ``E = Re <psi|lambda>``, one walk, ``G = Im``."""
    thetas = np.asarray(thetas, dtype=float)
    psis = S.rotate_members([ket] * len(thetas), rotations, thetas)
    lams = apply_sum_members(terms, psis)
    energy = inner_members(psis, lams).real
    values, _, _ = rotations_adjoint_members(rotations, thetas, psis, lams)
    return energy, np.ascontiguousarray(values.imag)


def qaoa_energies_and_gradients(d, gammas, betas):
    """``qaoa.energies_and_gradients`` step for step, the mixer as ``n`` X rotations of angle ``2 beta``."""
    gammas, betas = np.atleast_2d(np.asarray(gammas, dtype=float)), np.atleast_2d(np.asarray(betas, dtype=float))
    points, layers = gammas.shape
    n = int(d.size).bit_length() - 1
    x_rotations = [(0.0, "X", [q]) for q in range(n)]
    psis = [D.plus_state(n) for _ in range(points)]
    for layer in range(layers):
        psis = S.phase_members(psis, d, gammas[:, layer])
        psis = S.rotate_members(psis, x_rotations, np.repeat(2.0 * betas[:, layer, None], n, axis=1))
    energy = S.moments_members(psis, d)[:, 1]
    lams = [d * psi for psi in psis]
    d_gamma, d_beta = np.zeros((points, layers)), np.zeros((points, layers))
    for layer in range(layers - 1, -1, -1):
        values, psis, lams = rotations_adjoint_members(x_rotations, np.repeat(2.0 * betas[:, layer, None], n, axis=1), psis, lams)
        d_beta[:, layer] = 2.0 * values.imag.sum(axis=1)
        values, psis, lams = diag_phase_adjoint_members(d, -gammas[:, layer], psis, lams)
        d_gamma[:, layer] = 2.0 * values.imag
    return energy, d_gamma, d_beta


def heisenberg_terms(n: int, jx: float = 1.0, jy: float = 0.8, jz: float = 0.6, field: float = 0.3) -> list:
    """An open Heisenberg chain with a field: XX, YY, ZZ on neighbours and Z on every qubit."""
    terms = []
    for q in range(n - 1):
        terms += [(jx, "XX", [q, q + 1]), (jy, "YY", [q, q + 1]), (jz, "ZZ", [q, q + 1])]
    terms += [(field, "Z", [q]) for q in range(n)]
    return terms


def trotter_step(terms, t: float = 0.4) -> list:
    """One first-order Trotter step of ``exp(-i t H)`` as a rotation list: ``theta = 2 t c`` per term."""
    return P.trotter_rotations(terms, t, 1, 1)
