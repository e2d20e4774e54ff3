"""tests/layer_adjoint_reference.py, the statement the GPU tests of the adjoint walk through a product layer compare with
(DESIGN.md section 29), pinned on the CPU for up to 6 qubits against dense matrices; and the host formulas built on it --
``layers.generator`` / ``layers.gradient``, the walk of ``ansatz.Ansatz.energy_and_gradient`` and the fused ``dE/dbeta`` of
``qaoa.energy_and_gradient`` -- against central differences of the dense-matrix energy.  No GPU.

The central differences use step 1e-5 and tolerance 1e-7 * sum |c_t|: the truncation of a central difference (h^2 / 6 times a
third derivative of size sum |c_t|, plus eps / h rounding), not a device tolerance.
"""
from __future__ import annotations

import numpy as np
import pytest

import layer_adjoint_reference as A
import layer_reference as L
from quantum_computations_amd import ansatz, layers
from quantum_computations_amd.dv_simulator import numpy_quantum as npq

STEP, FD_TOL = 1e-5, 1e-7


def subsets(n):
    rng = np.random.default_rng(40 + n)
    out = [list(range(n)), [n - 1], [0]]
    for _ in range(4):
        out.append([int(q) for q in rng.permutation(n)[:int(rng.integers(1, n + 1))]])
    return out


def dense_on(n, m, q):
    """The 2^n x 2^n matrix of the 2x2 ``m`` on qubit ``q``."""
    return np.kron(np.kron(np.eye(1 << q), m), np.eye(1 << (n - 1 - q)))


def apply_gate(ket, n, matrix, qubits):
    """A 2^k x 2^k matrix on ``qubits`` (the first the most significant leg) of a host ket."""
    k = len(qubits)
    t = np.tensordot(np.asarray(matrix).reshape([2] * (2 * k)), ket.reshape([2] * n), axes=(list(range(k, 2 * k)), list(qubits)))
    return np.moveaxis(t, list(range(k)), list(qubits)).reshape(-1)


@pytest.mark.parametrize("n", range(1, 7))
def test_the_values_are_the_dense_matrix_elements(n):
    psi, lam = 1.3 * L.random_ket(n, n), 0.8 * L.random_ket(n, 20 + n)
    for qubits in subsets(n):
        T = A.layer_transition(lam, psi, qubits)
        for j, q in enumerate(qubits):
            for a in range(2):
                for b in range(2):
                    e = np.zeros((2, 2))
                    e[a, b] = 1.0
                    want = np.vdot(lam, dense_on(n, e, q) @ psi)
                    assert abs(T[j, a, b] - want) <= A.value_bound(n, np.linalg.norm(psi), np.linalg.norm(lam)), (n, qubits, q, a, b)
        # non-unitary matrices: the first stage sees the entry registers, and the operational definition gives the rest
        mats = 1.5 * L.random_unitaries((len(qubits),), 7 * n) + 0.1
        walked, _, _ = A.layer_adjoint(psi, lam, mats, qubits)
        lowest = int(np.argmax(qubits))                      # the highest qubit is the lowest index bit: the first stage
        assert np.array_equal(walked[lowest], T[lowest])


@pytest.mark.parametrize("n", range(1, 7))
def test_unitary_layers_leave_the_values_of_the_entry_registers(n):
    psi, lam = L.random_ket(n, 3 * n), L.random_ket(n, 3 * n + 1)
    for number, qubits in enumerate(subsets(n)):
        mats = L.random_unitaries((len(qubits),), 100 * n + number)
        walked, _, _ = A.layer_adjoint(psi, lam, mats, qubits)
        entry = A.layer_transition(lam, psi, qubits)
        assert np.max(np.abs(walked - entry)) <= 2 * L.bound(mats, len(qubits), 1.0) + A.value_bound(n, 1.0, 1.0), (n, qubits)


@pytest.mark.parametrize("n", range(1, 7))
def test_the_registers_take_the_product_of_the_inverses(n):
    psi, lam = 1.2 * L.random_ket(n, 5 * n), L.random_ket(n, 5 * n + 1)
    for number, qubits in enumerate(subsets(n)):
        k = len(qubits)
        for mats in (L.random_unitaries((k,), 200 * n + number), 1.7 * L.random_unitaries((k,), 300 * n + number) - 0.2):
            _, psi_out, lam_out = A.layer_adjoint(psi, lam, mats, qubits)
            assert np.array_equal(psi_out, L.apply_layer(psi, mats, qubits)) and np.array_equal(lam_out, L.apply_layer(lam, mats, qubits))
            order = sorted(range(k), key=lambda j: qubits[j])
            full = [np.eye(2, dtype=complex)] * n
            for j in order:
                full[qubits[j]] = mats[j]
            dense = layers.product_matrix(np.array(full))
            for got, ket in ((psi_out, psi), (lam_out, lam)):
                assert np.linalg.norm(got - dense @ ket) <= L.bound(mats, k, np.linalg.norm(ket)), (n, qubits)


@pytest.mark.parametrize("n", range(1, 7))
def test_one_qubit_densities_are_the_reduced_density_matrices(n):
    ket = 1.1 * L.random_ket(n, 9 * n)
    bound = A.value_bound(n, np.linalg.norm(ket), np.linalg.norm(ket))
    rho = A.one_qubit_densities(ket)
    host = npq.one_qubit_densities(ket)
    assert rho.shape == host.shape == (n, 2, 2)
    for q in range(n):
        want = npq.reduced_density(ket, [q])
        assert np.max(np.abs(rho[q] - want)) <= bound and np.max(np.abs(host[q] - want)) <= bound, (n, q)
        assert abs(np.trace(rho[q]) - np.vdot(ket, ket)) <= bound
    some = [n - 1, 0] if n > 1 else [0]
    assert np.array_equal(npq.one_qubit_densities(ket, some), host[some])
    with pytest.raises(ValueError):
        npq.one_qubit_densities(ket, [n])


def test_generators_and_the_gradient_contraction():
    theta, h = 0.37, 1e-6
    for kind, fn in (("rx", layers.rx), ("ry", layers.ry), ("rz", layers.rz)):
        derivative = (fn(theta + h) - fn(theta - h)) / (2 * h)
        assert np.max(np.abs(derivative @ fn(theta).conj().T - layers.generator(kind))) <= 1e-9, kind
        assert np.array_equal(layers.rotation(kind, theta), fn(theta))
    with pytest.raises(ValueError):
        layers.generator("rw")
    T = np.arange(8, dtype=float).reshape(2, 2, 2) * (1 + 0.5j) + 1j * np.arange(8, 0, -1).reshape(2, 2, 2) ** 2
    pauli_y = np.array([[0, -1j], [1j, 0]])
    want = [np.imag(np.sum(pauli_y * T[j])) for j in range(2)]          # Im <lam|P|psi> = Im sum_ab P[a][b] T[a][b]
    assert np.allclose(layers.gradient(T, layers.generator("ry")), want, rtol=0, atol=1e-13)
    assert np.allclose(layers.gradient(T, np.array([layers.generator("ry")] * 2)), want, rtol=0, atol=1e-13)
    with pytest.raises(ValueError):
        layers.gradient(T[0], layers.generator("rx"))


# ---- the walk of Ansatz.energy_and_gradient, on the host ------------------------------------------------------------------------
def host_run(circuit, params, ket):
    n, first = circuit.num_qubits, 0
    for block in circuit.blocks:
        if block[0] == "rotation":
            _, kind, qubits = block
            ket = L.apply_layer(ket, layers.rotation(kind, params[first:first + len(qubits)]), qubits)
            first += len(qubits)
        else:
            for matrix, qubits in block[1]:
                ket = apply_gate(ket, n, matrix, qubits)
    return ket


def host_energy_and_gradient(circuit, params, terms, ket):
    """``Ansatz.energy_and_gradient`` step for step, with the reference in place of the device calls."""
    n = circuit.num_qubits
    psi = host_run(circuit, params, ket)
    lam = A.apply_terms(psi, terms)
    energy = np.vdot(psi, lam).real
    grad, last = np.zeros(circuit.num_parameters), circuit.num_parameters
    for block in reversed(circuit.blocks):
        if block[0] == "rotation":
            _, kind, qubits = block
            first = last - len(qubits)
            inverse = np.conjugate(np.swapaxes(layers.rotation(kind, params[first:last]), 1, 2))
            T, psi, lam = A.layer_adjoint(psi, lam, inverse, qubits)
            grad[first:last] = layers.gradient(T, layers.generator(kind))
            last = first
        else:
            for matrix, qubits in reversed(block[1]):
                psi, lam = apply_gate(psi, n, matrix.conj().T, qubits), apply_gate(lam, n, matrix.conj().T, qubits)
    return energy, grad, psi


def test_the_ansatz_gradient_against_central_differences():
    n = 4
    circuit = ansatz.Ansatz(n)
    for _ in range(2):
        circuit.rotation_layer("ry").rotation_layer("rz", [3, 0, 2]).fixed(ansatz.cz_ring(n)).rotation_layer("rx", [1, 2])
    assert circuit.num_parameters == 2 * (4 + 3 + 2) and circuit.num_gates() == 2 * (9 + 4)
    terms = A.heisenberg_chain(n) + [(0.3, "X", [1]), (-0.2, "Z", [3])]
    scale = sum(abs(c) for c, _, _ in terms)
    dense = A.dense_terms(n, terms)
    params = np.random.default_rng(11).uniform(-np.pi, np.pi, circuit.num_parameters)
    ket = L.random_ket(n, 12)

    def energy(x):
        out = host_run(circuit, x, ket)
        return np.vdot(out, dense @ out).real

    got_energy, grad, rewound = host_energy_and_gradient(circuit, params, terms, ket)
    assert abs(got_energy - energy(params)) <= 64 * L.EPS * scale
    assert np.linalg.norm(rewound - ket) <= 16 * circuit.num_gates() * L.EPS
    for p in range(circuit.num_parameters):
        step = np.zeros_like(params)
        step[p] = STEP
        difference = (energy(params + step) - energy(params - step)) / (2 * STEP)
        assert abs(grad[p] - difference) <= FD_TOL * scale, (p, grad[p], difference)
    # the rotation spelling of the same circuit: same energy (CZ up to a global phase), parameters where they are said to be
    rotations = circuit.rotations(params)
    positions = circuit.parameter_positions()
    assert [rotations[i][0] for i in positions] == list(params)
    spelled = ket
    pauli = {"X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0])}
    for theta, letters, qubits in rotations:
        p = np.ones((1, 1))
        for letter in letters:
            p = np.kron(p, pauli[letter])
        spelled = apply_gate(spelled, n, np.cos(theta / 2) * np.eye(p.shape[0]) - 1j * np.sin(theta / 2) * p, qubits)
    assert abs(np.vdot(spelled, dense @ spelled).real - got_energy) <= 64 * circuit.num_gates() * L.EPS * scale
    with pytest.raises(ValueError):
        ansatz.Ansatz(2).fixed([(np.eye(4)[::-1], [0, 1])]).rotations([])
    with pytest.raises(ValueError):
        circuit.run(params[:-1])
    with pytest.raises(ValueError):
        ansatz.Ansatz(3).rotation_layer("ry", [0, 0])


def test_the_fused_qaoa_beta_derivative_against_central_differences():
    n, p = 4, 2
    rng = np.random.default_rng(5)
    cost = rng.uniform(-1.0, 1.0, 1 << n)
    # the cost's own size.  |d^3 E / dbeta^3| <= (2 n)^3 scale (the mixer's generator has norm n), so the truncation of the
    # central difference is at most h^2 / 6 * 512 scale = 8.6e-9 scale at n = 4: inside 1e-7 * n * scale
    scale = float(np.max(np.abs(cost)))
    gammas, betas = rng.uniform(-1, 1, p), rng.uniform(-1, 1, p)
    plus = np.full(1 << n, 2.0 ** (-0.5 * n), dtype=np.complex128)

    def forward(g, b):
        ket = plus
        for gamma, beta in zip(g, b):
            ket = np.exp(-1j * gamma * cost) * ket
            ket = L.apply_layer(ket, layers.rx(2.0 * beta))
        return ket

    def energy(g, b):
        ket = forward(g, b)
        return float(np.sum(cost * np.abs(ket) ** 2))

    psi = forward(gammas, betas)
    lam = cost * psi
    d_beta = np.zeros(p)
    for layer in range(p - 1, -1, -1):
        inverse = layers.rx(2.0 * betas[layer]).conj().T
        T, psi, lam = A.layer_adjoint(psi, lam, inverse)
        d_beta[layer] = np.sum(layers.gradient(T, 2.0 * layers.generator("rx")))
        x_sum = sum(T[q, 0, 1] + T[q, 1, 0] for q in range(n))             # sum_q <lam|X_q|psi>
        assert abs(d_beta[layer] - 2.0 * x_sum.imag) <= 64 * L.EPS * n * scale
        psi, lam = np.exp(1j * gammas[layer] * cost) * psi, np.exp(1j * gammas[layer] * cost) * lam
    assert np.linalg.norm(psi - plus) <= 16 * p * (n + 1) * L.EPS
    for layer in range(p):
        step = np.zeros(p)
        step[layer] = STEP
        difference = (energy(gammas, betas + step) - energy(gammas, betas - step)) / (2 * STEP)
        assert abs(d_beta[layer] - difference) <= FD_TOL * n * scale, (layer, d_beta[layer], difference)
