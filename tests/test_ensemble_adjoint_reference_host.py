"""The NumPy model of the per-member adjoint calls (tests/ensemble_adjoint_reference.py) pinned on the host, no GPU and no
library: ``energies_and_gradients`` against the parameter-shift rule of ``sweep_reference`` (exact for Pauli rotations), the
QAOA form against ``diagonal_reference.qaoa_energy_and_gradient``, and the three per-member calls against their
single-register references, on 3 to 5 qubits.

Bounds: every figure is a sum of at most a few hundred products of numbers of modulus at most ``sum|c_t|``, each rounded
to eps = 2.2e-16, so model and pin agree within ``1e-12 sum|c_t|``.
"""
from __future__ import annotations

import numpy as np
import pytest

import diagonal_reference as D
import ensemble_adjoint_reference as A
import pauli_operator_reference as O
import sweep_reference as S

TOL = 1e-12


def weight(terms) -> float:
    return float(sum(abs(complex(c)) for c, _, _ in terms))


@pytest.mark.parametrize("n", (3, 4, 5))
def test_energies_and_gradients_against_the_parameter_shift_rule(n):
    terms = A.heisenberg_terms(n)
    rotations = A.trotter_step(terms)
    rng = np.random.default_rng(100 + n)
    thetas = rng.uniform(-3.0, 3.0, (5, len(rotations)))
    thetas[0] = 0.0
    thetas[1, ::2] = np.pi
    ket = D.random_ket(n, 7 + n)
    energy, gradient = A.energies_and_gradients(rotations, thetas, terms, ket)
    assert energy.shape == (5,) and gradient.shape == thetas.shape
    for m, row in enumerate(thetas):
        e, g = S.parameter_shift(rotations, row, terms, ket)
        assert abs(energy[m] - e) <= TOL * weight(terms)
        assert np.max(np.abs(gradient[m] - g)) <= TOL * weight(terms)


@pytest.mark.parametrize("n", (3, 4, 5))
def test_qaoa_form_against_the_single_register_walk(n):
    d = D.diagonal_from_terms(n, D.random_z_terms(n, 6, 40 + n))
    rng = np.random.default_rng(200 + n)
    gammas, betas = rng.uniform(-1.0, 1.0, (4, 2)), rng.uniform(-1.0, 1.0, (4, 2))
    gammas[0], betas[0] = 0.0, 0.0
    energy, d_gamma, d_beta = A.qaoa_energies_and_gradients(d, gammas, betas)
    scale = float(np.max(np.abs(d)))
    for m in range(4):
        e, dg, db, _ = D.qaoa_energy_and_gradient(d, gammas[m], betas[m])
        assert abs(energy[m] - e) <= TOL * scale
        assert np.max(np.abs(d_gamma[m] - dg)) <= TOL * scale * scale * n
        assert np.max(np.abs(d_beta[m] - db)) <= TOL * scale * n


def test_the_three_calls_member_by_member():
    n, members = 4, 3
    psis = [(1.0 + 0.5 * m) * D.random_ket(n, 300 + m) for m in range(members)]
    lams = [D.random_ket(n, 400 + m) for m in range(members)]
    rotations = [(0.0, "XY", [0, 3]), (0.0, "Z", [1]), (0.0, "", []), (0.0, "YYXZ", [0, 1, 2, 3])]
    thetas = np.random.default_rng(5).uniform(-3.0, 3.0, (members, len(rotations)))
    values, out_psi, out_lam = A.rotations_adjoint_members(rotations, thetas, psis, lams)
    assert values.shape == (members, len(rotations))
    for m in range(members):
        v, p, l = O.adjoint_values(S.with_angles(rotations, thetas[m]), psis[m], lams[m])
        assert np.array_equal(values[m], v) and np.array_equal(out_psi[m], p) and np.array_equal(out_lam[m], l)
    # the identity string: the value is the inner product, wherever it stands in the list
    assert abs(values[1, 2] - np.vdot(out_lam[1], out_psi[1])) <= TOL * np.linalg.norm(psis[1])
    d = np.random.default_rng(6).uniform(-2.0, 2.0, 1 << n)
    gammas = np.array([0.0, 0.7, -1.3])
    values, out_psi, out_lam = A.diag_phase_adjoint_members(d, gammas, psis, lams)
    for m in range(members):
        assert values[m] == np.vdot(lams[m], d * psis[m])
        assert np.allclose(out_psi[m], psis[m] * np.exp(-1j * gammas[m] * d), rtol=0, atol=1e-15 * 2)
        assert np.allclose(out_lam[m], lams[m] * np.exp(-1j * gammas[m] * d), rtol=0, atol=1e-15 * 2)
    assert np.array_equal(out_psi[0], psis[0])                                      # gamma = 0
    inner = A.inner_members(psis, psis)
    assert np.all(np.abs(inner.imag) <= 1e-15 * inner.real) and np.allclose(inner.real, [np.linalg.norm(p) ** 2 for p in psis], rtol=1e-14)
