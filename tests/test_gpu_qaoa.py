"""quantum_computations_amd/qaoa.py on the device against tests/diagonal_reference.py (pinned against dense matrices and
central differences in tests/test_diagonal_reference_host.py), against the device's own adjoint gradient of the
equivalent Pauli rotation list, and a Grover search whose oracle is one diagonal phase.

Tolerances: states within CIRCUIT_TOL = 1e-12; energies and gradients within ``ADJOINT_TOL sum|c_t|`` with ADJOINT_TOL =
1e-12, the bound the existing gradient tests (tests/test_gpu_pauli_operator.py) use for the same number of passes, and
twice that where two device results are compared; the rewound register within 2 CIRCUIT_TOL of ``|+>^n``.

Worst observed errors are printed with their bounds (run with -s).
"""
from __future__ import annotations

import numpy as np
import pytest

import diagonal_reference as R
from quantum_computations_amd import DiagonalOperator, qaoa
from quantum_computations_amd import workloads as W
from quantum_computations_amd.device import DeviceState
from quantum_computations_amd.dv_simulator import gates as G

pytestmark = pytest.mark.gpu

CIRCUIT_TOL = 1e-12
ADJOINT_TOL = 1e-12


def maxabs(a):
    return float(np.max(np.abs(a)))


def report(what, err, bound):
    print(f"{what}: {err:.3e} (bound {bound:.3e})")
    assert err <= bound, what


def instance(name, n):
    terms = W.maxcut_terms(n, W.ring_chord_edges(n)) if name == "maxcut" else W.sk_terms(n, 3)
    return terms, sum(abs(c) for c, _, _ in terms)


def angles(p, seed=0):
    rng = np.random.default_rng(seed + p)
    return rng.uniform(-0.6, 0.6, p), rng.uniform(-0.6, 0.6, p)


@pytest.fixture(scope="module")
def references():
    """(terms, weight, host diagonal, reference walk) per case, computed once."""
    out = {}
    for name in ("maxcut", "sk"):
        for n in (8, 12):
            terms, weight = instance(name, n)
            d = R.diagonal_from_terms(n, terms)
            for p in (1, 3):
                gammas, betas = angles(p)
                out[name, n, p] = terms, weight, d, gammas, betas, R.qaoa_energy_and_gradient(d, gammas, betas)
    return out


CASES = [(name, n, p) for name in ("maxcut", "sk") for n in (8, 12) for p in (1, 3)]


@pytest.mark.parametrize("name,n,p", CASES)
def test_run_against_the_reference(references, name, n, p):
    terms, weight, d, gammas, betas, _ = references[name, n, p]
    op = DiagonalOperator.from_terms(n, terms)
    state = qaoa.run(op, gammas, betas)
    report(f"{name} n={n} p={p} state", maxabs(state.to_numpy() - R.qaoa_state(d, gammas, betas)), CIRCUIT_TOL)
    given = DeviceState.from_numpy(R.plus_state(n))
    assert qaoa.run(op, gammas, betas, given) is given
    report(f"{name} n={n} p={p} state, register given", maxabs(given.to_numpy() - R.qaoa_state(d, gammas, betas)), CIRCUIT_TOL)
    report(f"{name} n={n} plus_state", maxabs(qaoa.plus_state(n).to_numpy() - R.plus_state(n)), CIRCUIT_TOL)
    one = DeviceState.from_numpy(R.random_ket(n, 1))
    report(f"{name} n={n} mixer", maxabs(qaoa.mixer(one, 0.3).to_numpy() - R.mixer(R.random_ket(n, 1), n, 0.3)), CIRCUIT_TOL)


@pytest.mark.parametrize("name,n,p", CASES)
def test_energy_and_gradient(references, name, n, p):
    terms, weight, d, gammas, betas, (energy, d_gamma, d_beta, _) = references[name, n, p]
    op = DiagonalOperator.from_terms(n, terms)
    bound = ADJOINT_TOL * weight
    psi = qaoa.plus_state(n)
    got_e, got_g, got_b = qaoa.energy_and_gradient(op, gammas, betas, psi)
    report(f"{name} n={n} p={p} energy", abs(got_e - energy), bound)
    report(f"{name} n={n} p={p} dE/dgamma", maxabs(got_g - d_gamma), bound)
    report(f"{name} n={n} p={p} dE/dbeta", maxabs(got_b - d_beta), bound)
    assert max(maxabs(got_g), maxabs(got_b)) > 1e-3                              # not a comparison of zeros
    report(f"{name} n={n} p={p} register rewound to |+>", maxabs(psi.to_numpy() - R.plus_state(n)), 2 * CIRCUIT_TOL)
    # without a register of the caller's: the same numbers
    again = qaoa.energy_and_gradient(op, gammas, betas)
    assert again[0] == got_e and np.array_equal(again[1], got_g) and np.array_equal(again[2], got_b)
    # the device's own adjoint gradient of the same circuit spelled as Pauli rotations
    rotations = R.qaoa_rotations(terms, n, gammas, betas)
    e_rot, d_theta = qaoa.plus_state(n).energy_and_gradient(rotations, terms)
    rot_g, rot_b = R.gradient_from_rotations(terms, n, p, d_theta)
    report(f"{name} n={n} p={p} energy against the rotation list", abs(got_e - e_rot), 2 * bound)
    report(f"{name} n={n} p={p} dE/dgamma against the rotation list", maxabs(got_g - rot_g), 2 * bound)
    report(f"{name} n={n} p={p} dE/dbeta against the rotation list", maxabs(got_b - rot_b), 2 * bound)


def test_minimise():
    n, p = 8, 2
    terms, weight = instance("maxcut", n)
    op = DiagonalOperator.from_terms(n, terms)
    x0 = np.array([0.2, 0.3, 0.25, 0.1])
    start = qaoa.energy_and_gradient(op, x0[:p], x0[p:])[0]
    x, energy, result = qaoa.minimise(op, p, x0=x0, options={"maxiter": 30})
    print(f"minimise: {start:.6f} -> {energy:.6f} in {result.nit} iterations ({result.nfev} evaluations), min C = {op.extrema()[0]}")
    assert x.shape == (2 * p,) and energy <= start
    state = qaoa.run(op, x[:p], x[p:])
    report("minimise: energy at the returned angles", abs(state.expect_diagonal(op).mean - energy), ADJOINT_TOL * weight)
    assert energy >= op.extrema()[0]
    with pytest.raises(ValueError):
        qaoa.minimise(op, p, x0=np.zeros(3))
    with pytest.raises(ValueError):
        qaoa.energy_and_gradient(op, [0.1, 0.2], [0.3])


def test_grover_with_an_indicator_oracle():
    n, marked = 10, [5, 377, 1000]
    indicator = np.zeros(1 << n)
    indicator[marked] = 1.0
    oracle = DiagonalOperator.from_numpy(indicator)
    h, x = G.H(0).matrix, G.X(0).matrix
    state = qaoa.plus_state(n)
    for k in range(1, 15):
        state.apply_diagonal_phase(oracle, np.pi)                      # exp(-i pi) = -1 on the marked set, one pass
        for gate in (h, x):                                            # the diffuser of workloads.grover_iteration
            for q in range(n):
                state.apply_matrix(gate, [q])
        state.apply_mcphase(list(range(n)), -1.0)
        for gate in (x, h):
            for q in range(n):
                state.apply_matrix(gate, [q])
        moments = state.expect_diagonal(oracle, 0.5)                   # no download: d <= 0.5 is the unmarked set
        want = W.grover_success_probability(n, k, len(marked))
        report(f"Grover k={k} marked probability (mean)", abs(moments.mean - want), CIRCUIT_TOL)
        report(f"Grover k={k} marked probability (threshold)", abs(moments.norm2 - moments.probability_below - want), CIRCUIT_TOL)
    assert want > 0.99                                                 # k = 14 is the optimum for 3 marked of 1024
