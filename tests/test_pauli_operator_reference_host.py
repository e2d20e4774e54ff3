"""The NumPy model of tests/pauli_operator_reference.py against independent roads (CPU only): the dense matrix
``npq.PauliSum(...).matrix()`` for n <= 6, the exact parameter-shift rule, and a central finite difference.
"""
from __future__ import annotations

import numpy as np
import pytest

import pauli_operator_reference as P
import pauli_rotation_reference as R
from quantum_computations_amd.dv_simulator import numpy_quantum as npq


def random_ket(n, seed):
    rng = np.random.default_rng(100 * n + seed)
    ket = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return ket / np.linalg.norm(ket)


def random_terms(n, count, rng, real=False):
    terms = []
    for _ in range(count):
        k = int(rng.integers(0, n + 1))
        letters = "".join(rng.choice(list("IXYZ"), size=k))
        qubits = [int(q) for q in rng.permutation(n)[:k]]
        c = float(rng.standard_normal()) if real else complex(rng.standard_normal(), rng.standard_normal())
        terms.append((c, letters, qubits))
    return terms


@pytest.mark.parametrize("n", (1, 2, 3, 5, 6))
def test_apply_and_transition_against_the_dense_matrix(n):
    rng = np.random.default_rng(n)
    terms = random_terms(n, 12, rng) + [(0.5 - 0.25j, "", [])]
    dense = npq.PauliSum(n, terms).matrix()
    bra, ket = random_ket(n, 1), random_ket(n, 2)
    assert np.allclose(P.apply_sum(terms, ket), dense @ ket, atol=1e-13)
    total, values = P.transition(terms, bra, ket)
    assert abs(total - np.vdot(bra, dense @ ket)) < 1e-13
    for (_, letters, qubits), value in zip(terms, values):
        assert abs(value - np.vdot(bra, npq.PauliSum(n, [(1.0, letters, qubits)]).matrix() @ ket)) < 1e-13
    assert P.apply_sum([], ket).tolist() == [0.0] * (1 << n)


@pytest.mark.parametrize("n", (1, 3, 6))
def test_mask_forms_are_the_letter_forms(n):
    rng = np.random.default_rng(10 + n)
    psi, lam = random_ket(n, 3), 2.5 * random_ket(n, 4)
    rotations = [(float(rng.uniform(-3, 3)), letters, qubits) for _, letters, qubits in random_terms(n, 9, rng)]
    for theta, letters, qubits in rotations:
        x, z = R.masks(n, letters, qubits)
        assert np.allclose(P.apply_string_masks(psi, x, z), R.apply_string(psi, letters, qubits), atol=1e-15)
        assert np.allclose(P.rotate_masks(psi, theta, x, z), R.rotate(psi, theta, letters, qubits), atol=1e-15)
    want = P.adjoint_values(rotations, psi, lam)
    got = P.adjoint_values_masks(n, rotations, psi, lam)
    for a, b in zip(want, got):
        assert np.allclose(a, b, atol=1e-13)


@pytest.mark.parametrize("n", (2, 4, 6))
def test_walk_rewinds_and_gradient_is_parameter_shift_and_finite_difference(n):
    rng = np.random.default_rng(20 + n)
    terms = random_terms(n, 7, rng, real=True)
    rotations = [(float(rng.uniform(-3, 3)), letters, qubits) for _, letters, qubits in random_terms(n, 11, rng)]
    rotations += [(0.7, "X", [0]), (-0.4, "Y", [0]), (1.1, "Z" * n, list(range(n)))]
    psi0 = random_ket(n, 5)
    psi = R.rotate_list(psi0, rotations)
    lam = P.apply_sum(terms, psi)
    values, back_psi, back_lam = P.adjoint_values(rotations, psi, lam)
    assert np.allclose(back_psi, psi0, atol=1e-13)
    want_lam = lam
    for theta, letters, qubits in rotations[::-1]:
        want_lam = R.rotate(want_lam, -theta, letters, qubits)
    assert np.allclose(back_lam, want_lam, atol=1e-13)
    e, grad = P.energy_gradient(rotations, terms, psi0)
    dense = npq.PauliSum(n, terms).matrix()
    assert abs(e - np.vdot(psi, dense @ psi).real) < 1e-12
    assert abs(e - P.energy(rotations, terms, psi0)) < 1e-12
    shift = P.parameter_shift(rotations, terms, psi0)
    print(f"n={n}: adjoint against parameter shift {np.max(np.abs(grad - shift)):.3e}")
    assert np.max(np.abs(grad - shift)) < 1e-12
    h = 1e-5
    for k in range(len(rotations)):
        theta, letters, qubits = rotations[k]
        up = rotations[:k] + [(theta + h, letters, qubits)] + rotations[k + 1:]
        down = rotations[:k] + [(theta - h, letters, qubits)] + rotations[k + 1:]
        central = (P.energy(up, terms, psi0) - P.energy(down, terms, psi0)) / (2 * h)
        assert abs(central - grad[k]) < 1e-8, (k, central, grad[k])       # O(h^2) truncation plus eps / h rounding


def test_order_inside_a_shared_xmask_matters():
    n = 3
    psi0, terms = random_ket(n, 6), [(1.0, "ZZ", [0, 1]), (0.5, "X", [2]), (0.3, "Y", [0])]
    rotations = [(0.9, "X", [0]), (1.3, "Y", [0])]
    _, forward = P.energy_gradient(rotations, terms, psi0)
    _, backward = P.energy_gradient(rotations[::-1], terms, psi0)
    assert np.max(np.abs(forward - backward[::-1])) > 1e-3


def test_plan_models():
    terms = [(0b110, 0b010), (0, 0b1), (0b110, 0b100), (0b001, 0)] + [(0, z) for z in range(9)]
    passes = P.sum_plan(terms)
    assert [p["index"] for p in passes] == [[0, 2], [1, 4, 5, 6, 7, 8, 9, 10], [11, 12], [3]]
    coeffs = [1.0 + 0.5j * t for t in range(len(terms))]
    launches = P.apply_launches(terms, coeffs, 8, accumulate=False)
    assert [l["first"] for l in launches] == [True, False, False, False]
    assert not any(l["first"] for l in P.apply_launches(terms, coeffs, 8, accumulate=True))
    assert launches[0]["pivot"] == 2 and launches[0]["items"] == 4 and launches[1]["items"] == 8
    assert launches[0]["odd"] == 0b11 and launches[0]["d"] == [1j * coeffs[0], 1j * coeffs[2]]
    assert [l["width"] for l in launches] == [2, 8, 2, 1]
    walk = P.adjoint_launches(terms[:4], [0.9, 0.8, 0.7, 0.6], [0.1, 0.2, 0.3, 0.4], 8)
    assert [l["index"] for l in walk] == [[3], [2, 1, 0]]
    assert walk[1]["sn"] == [-0.3, -0.2, -0.1] and walk[1]["cs"] == [0.7, 0.8, 0.9] and walk[1]["diag"] == [False, True, False]
