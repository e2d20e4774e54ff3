"""tests/krylov_reference.py -- the NumPy restatement of quantum_computations_amd/krylov.py -- against dense matrices, on
the host only.  H is built column by column with ``apply_sum``; the yardsticks are ``numpy.linalg.eigvalsh`` and
``scipy.linalg.expm``.

Bounds.  On the 10-qubit chains used here the restatement was measured at: max|V^H V - I| <= 1.2e-15 and the Lanczos
relation to 9e-16 (m = 10 / 20 / 30, with reorthogonalisation); ground-energy error <= 4e-14 in at most 4 restarts
(m = 20 / 30 / 40, tol = 1e-10); evolution error against expm <= 2.5e-13 for tol = 1e-10 at t = 1 and t = 5 and <= 8e-9
for tol = 1e-6 (m = 20).  The assertions are: orthogonality and relation 1e-13, |E - E0| <= 1e-12 sum|c_t|, evolution
error <= tol -- each a factor 80 or more above the measurement.
"""
from __future__ import annotations

import numpy as np
import pytest
import scipy.linalg

import krylov_reference as K
from quantum_computations_amd import workloads as W

N = 10


def start_vector(n, seed=5):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    return v / np.linalg.norm(v)


@pytest.fixture(scope="module", params=["heisenberg", "ising"])
def model(request):
    terms = W.heisenberg_chain_terms(N) if request.param == "heisenberg" else W.ising_terms(N, 1.0)
    H = K.dense(terms, N)
    assert np.array_equal(H, H.conj().T)
    return terms, H, np.linalg.eigvalsh(H), K.scale_of(terms)


@pytest.mark.parametrize("m", [10, 20, 30])
def test_lanczos_basis_is_orthonormal_and_satisfies_the_relation(model, m):
    terms, H, _, scale = model
    alphas, betas, V, breakdown, norm = K.lanczos(terms, 1.7 * start_vector(N), m)
    assert not breakdown and len(alphas) == len(betas) == len(V) == m and abs(norm - 1.7) < 1e-14
    orth = np.abs(V.conj() @ V.T - np.eye(m)).max()
    # H V = V T + beta_m v_{m+1} e_m^T: every column but the last closes inside the basis
    R = H @ V.T - V.T @ K.tridiagonal(alphas, betas)
    relation = np.abs(R[:, :-1]).max() / scale
    last = abs(np.linalg.norm(R[:, -1]) - betas[-1]) / scale
    print(f"m={m}: orthogonality {orth:.2e}, relation {relation:.2e}, last column {last:.2e} (bound 1e-13)")
    assert orth <= 1e-13 and relation <= 1e-13 and last <= 1e-13


def test_recurrence_without_reorthogonalisation_agrees_for_ten_steps(model):
    terms, _, _, scale = model
    a1, b1, *_ = K.lanczos(terms, start_vector(N), 10, True)
    a2, b2, *_ = K.lanczos(terms, start_vector(N), 10, False)
    worst = max(np.abs(a1 - a2).max(), np.abs(b1 - b2).max()) / scale
    print(f"three-term recurrence against full reorthogonalisation: {worst:.2e} (bound 1e-13)")
    assert worst <= 1e-13


@pytest.mark.parametrize("m", [20, 30, 40])
def test_ground_state(model, m):
    terms, H, eigenvalues, scale = model
    energy, state, info = K.ground_state(terms, start_vector(N), m=m, tol=1e-10)
    error = abs(energy - eigenvalues[0])
    residual = np.linalg.norm(H @ state - energy * state)
    print(f"m={m}: |E - E0| = {error:.2e} (bound {1e-12 * scale:.2e}), residual {residual:.2e}, restarts {info['restarts']}, "
          f"applications {info['applications']}")
    assert error <= 1e-12 * scale
    assert residual <= 10 * 1e-10 * scale and abs(np.linalg.norm(state) - 1.0) <= 1e-12
    assert info["restarts"] <= 50 and info["applications"] <= (info["restarts"] + 1) * m


@pytest.mark.parametrize("t, tol", [(1.0, 1e-10), (5.0, 1e-10), (-2.0, 1e-10), (1.0, 1e-6)])
def test_evolve_krylov_against_expm(model, t, tol):
    terms, H, _, _ = model
    psi = 1.7 * start_vector(N)
    want = scipy.linalg.expm(-1j * t * H) @ psi
    got, info = K.evolve_krylov(terms, psi, t, m=20, tol=tol)
    error = np.linalg.norm(got - want) / 1.7
    print(f"t={t}, tol={tol}: error {error:.2e}, estimate {info['error_estimate']:.2e}, substeps {info['substeps']}, "
          f"applications {info['applications']}")
    assert error <= tol
    assert abs(np.linalg.norm(got) - 1.7) <= 1e-12


def test_invariant_subspace_breaks_down_after_three_steps():
    """The open 3-qubit Heisenberg chain has three distinct eigenvalues: the Krylov space of any start closes at k = 3."""
    terms = W.heisenberg_chain_terms(3)
    H = K.dense(terms, 3)
    psi = start_vector(3)
    alphas, betas, V, breakdown, _ = K.lanczos(terms, psi, 20)
    assert breakdown and len(alphas) == 3 and len(V) == 3 and betas[-1] <= 1e-12 * K.scale_of(terms)
    assert np.all(np.isfinite(alphas)) and np.all(np.isfinite(betas))
    got, info = K.evolve_krylov(terms, psi, 1.0, m=20)
    error = np.linalg.norm(got - scipy.linalg.expm(-1j * H) @ psi)
    print(f"3-qubit chain: evolution error {error:.2e} (bound 1e-14), substeps {info['substeps']}")
    assert info["substeps"] == 1 and error <= 1e-14
    energy, state, ginfo = K.ground_state(terms, psi, m=20)
    assert ginfo["breakdown"] and ginfo["restarts"] == 0 and abs(energy - np.linalg.eigvalsh(H)[0]) <= 1e-12 * K.scale_of(terms)
