"""Host tests of tests/sweep_reference.py and of the pure host logic of quantum_computations_amd/sweep.py: the
parameter-shift rule of the reference against the adjoint gradients that tests/test_diagonal_reference_host.py pins
(``ADJOINT_TOL sum|c_t|``, ADJOINT_TOL = 1e-12 as in tests/test_gpu_qaoa.py), ``apply_kq`` against Kronecker products, and
``sweep.chunks``.  No device, no library.
"""
from __future__ import annotations

import numpy as np
import pytest

import diagonal_reference as D
import pauli_rotation_reference as P
import sweep_reference as S
from quantum_computations_amd import sweep
from quantum_computations_amd import workloads as W

ADJOINT_TOL = 1e-12


@pytest.mark.parametrize("n,p", [(4, 1), (6, 2)])
def test_parameter_shift_equals_the_adjoint_gradient_of_qaoa(n, p):
    terms = W.maxcut_terms(n, W.ring_chord_edges(n))
    weight = sum(abs(c) for c, _, _ in terms)
    d = D.diagonal_from_terms(n, terms)
    rng = np.random.default_rng(n + p)
    gammas, betas = rng.uniform(-0.6, 0.6, p), rng.uniform(-0.6, 0.6, p)
    rotations = D.qaoa_rotations(terms, n, gammas, betas)
    theta = np.array([t for t, _, _ in rotations])
    energy, d_theta = S.parameter_shift(rotations, theta, terms, D.plus_state(n))
    d_gamma, d_beta = D.gradient_from_rotations(terms, n, p, d_theta)
    want_e, want_g, want_b, _ = D.qaoa_energy_and_gradient(d, gammas, betas)
    print(f"n={n} p={p}: energy {abs(energy - want_e):.3e}, dgamma {np.max(np.abs(d_gamma - want_g)):.3e}, "
          f"dbeta {np.max(np.abs(d_beta - want_b)):.3e} (bound {ADJOINT_TOL * weight:.3e})")
    assert abs(energy - want_e) <= ADJOINT_TOL * weight
    assert np.max(np.abs(d_gamma - want_g)) <= ADJOINT_TOL * weight
    assert np.max(np.abs(d_beta - want_b)) <= ADJOINT_TOL * weight
    assert max(np.max(np.abs(want_g)), np.max(np.abs(want_b))) > 1e-3          # not a comparison of zeros
    # the energies of the sweep are those of the QAOA reference
    assert abs(S.qaoa_energies(d, [gammas], [betas])[0] - want_e) <= ADJOINT_TOL * weight


def test_rows_of_a_parameter_shift_sweep():
    rows = S.shifted_rows([0.1, -0.2, 0.3])
    assert rows.shape == (7, 3) and np.array_equal(rows[0], [0.1, -0.2, 0.3])
    for r in range(3):
        delta_plus, delta_minus = rows[1 + 2 * r] - rows[0], rows[2 + 2 * r] - rows[0]
        assert np.count_nonzero(delta_plus) == 1 and np.count_nonzero(delta_minus) == 1
        assert delta_plus[r] == pytest.approx(np.pi / 2, abs=1e-15) and delta_minus[r] == pytest.approx(-np.pi / 2, abs=1e-15)


@pytest.mark.parametrize("qubits", [[0], [2], [3], [0, 1], [3, 1], [2, 3]])
def test_apply_kq_against_kronecker_products(qubits):
    n = 4
    rng = np.random.default_rng(7)
    ket = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    k = len(qubits)
    m = rng.standard_normal((1 << k, 1 << k)) + 1j * rng.standard_normal((1 << k, 1 << k))      # not unitary
    # the full operator from its matrix elements: <r|M|c> on the target bits, identity elsewhere
    full = np.zeros((1 << n, 1 << n), dtype=complex)
    for col in range(1 << n):
        c = sum(((col >> (n - 1 - q)) & 1) << (k - 1 - j) for j, q in enumerate(qubits))
        for r in range(1 << k):
            row = col
            for j, q in enumerate(qubits):
                bit = (r >> (k - 1 - j)) & 1
                row = (row & ~(1 << (n - 1 - q))) | (bit << (n - 1 - q))
            full[row, col] += m[r, c]
    assert np.max(np.abs(S.apply_kq(ket, n, qubits, m) - full @ ket)) < 1e-13


def test_member_wise_statements_are_the_single_register_ones():
    n = 3
    kets = [D.random_ket(n, s) * (1.0 + 0.5 * s) for s in range(4)]
    rotations = [(0.0, "XY", [0, 2]), (0.0, "Z", [1]), (0.0, "", [])]
    thetas = np.random.default_rng(1).uniform(-3, 3, (4, 3))
    got = S.rotate_members(kets, rotations, thetas)
    for m in range(4):
        want = kets[m]
        for theta, (_, letters, qubits) in zip(thetas[m], rotations):
            want = P.rotate(want, theta, letters, qubits)
        assert np.array_equal(got[m], want)
    d = np.arange(1 << n, dtype=float) - 3.0
    sums = S.moments_members(kets, d, threshold=0.5)
    for m in range(4):
        p = np.abs(kets[m]) ** 2
        assert sums[m, 0] == pytest.approx(p.sum()) and sums[m, 3] == pytest.approx(p[d <= 0.5].sum())
        assert np.allclose(S.phase_members(kets, d, [0.1 * m] * 4)[m], kets[m] * np.exp(-0.1j * m * d))


@pytest.mark.parametrize("batch", (1, 2, 256))
def test_chunks_cover_every_point_exactly_once(batch):
    for points in range(1, 601):
        seen = np.zeros(points, dtype=int)
        expect_first = 0
        for first, count, members in sweep.chunks(points, batch):
            assert first == expect_first and count >= 1
            assert members >= count and members <= batch and members & (members - 1) == 0
            assert members < 2 * count                                    # never more than twice the points it carries
            seen[first:first + count] += 1
            expect_first = first + count
        assert expect_first == points and np.all(seen == 1)


def test_chunks_refuse_nonsense_and_round_the_batch_down():
    assert list(sweep.chunks(0, 8)) == []
    assert list(sweep.chunks(13, 6)) == [(0, 4, 4), (4, 4, 4), (8, 4, 4), (12, 1, 1)]
    assert list(sweep.chunks(37, 8))[-1] == (32, 5, 8)
    with pytest.raises(ValueError):
        list(sweep.chunks(3, 0))
    with pytest.raises(ValueError):
        list(sweep.chunks(-1, 4))
