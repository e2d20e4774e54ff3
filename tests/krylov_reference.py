"""TEST INFRASTRUCTURE: a NumPy restatement of quantum_computations_amd/krylov.py -- ``lanczos``, ``ground_state`` and
``evolve_krylov`` with the same recurrences, stopping rules and step-halving rule -- on top of
``pauli_operator_reference.apply_sum``.  tests/test_krylov_reference_host.py pins it against dense matrices; the GPU
tests compare the library with it.
"""
from __future__ import annotations

import numpy as np

import pauli_operator_reference as P

BREAKDOWN = 1e-12
TAU_UNDERFLOW = 1e-12


def scale_of(terms) -> float:
    return float(sum(abs(complex(c)) for c, _, _ in terms))


def dense(terms, n: int) -> np.ndarray:
    """H column by column through ``apply_sum``."""
    dim = 1 << n
    H = np.zeros((dim, dim), dtype=complex)
    for j in range(dim):
        e = np.zeros(dim, dtype=complex)
        e[j] = 1.0
        H[:, j] = P.apply_sum(terms, e)
    return H


def tridiagonal(alphas, betas) -> np.ndarray:
    k = len(alphas)
    return np.diag(alphas) + np.diag(betas[:k - 1], 1) + np.diag(betas[:k - 1], -1)


def lanczos(terms, start: np.ndarray, m: int, reorthogonalise: bool = True, counter: dict | None = None):
    """(alphas[k], betas[k], V[k, dim], breakdown, ||start||): betas[k-1] is the norm of the last residual."""
    scale = scale_of(terms)
    start = np.asarray(start, dtype=complex)
    norm = float(np.sqrt(np.vdot(start, start).real))
    V = [start / norm]
    alphas, betas, breakdown = [], [], False
    for j in range(m):
        w = P.apply_sum(terms, V[j])
        if counter is not None:
            counter["applications"] = counter.get("applications", 0) + 1
        if reorthogonalise:
            alpha = 0.0
            for _ in range(2):
                basis = np.array(V)
                h = basis.conj() @ w
                w = w - h @ basis
                alpha += h[j].real
        else:
            alpha = np.vdot(V[j], w).real
            w = w - alpha * V[j] - (betas[j - 1] * V[j - 1] if j > 0 else 0.0)
        beta = float(np.sqrt(np.vdot(w, w).real))
        alphas.append(float(alpha))
        betas.append(beta)
        if beta <= BREAKDOWN * scale:
            breakdown = True
            break
        if j + 1 < m:
            V.append(w / beta)
    return np.array(alphas), np.array(betas), np.array(V), breakdown, norm


def ground_state(terms, start: np.ndarray, m: int = 30, tol: float = 1e-10, max_restarts: int = 50):
    """(energy, state, info) by restarted Lanczos."""
    scale = scale_of(terms)
    state = np.asarray(start, dtype=complex)
    counter: dict = {}
    for restarts in range(max_restarts + 1):
        alphas, betas, V, breakdown, _ = lanczos(terms, state, m, True, counter)
        ritz, vectors = np.linalg.eigh(tridiagonal(alphas, betas))
        y = vectors[:, 0]
        residual = float(betas[-1] * abs(y[-1]))
        state = y @ V
        if breakdown or residual <= tol * scale:
            return float(ritz[0]), state, {"restarts": restarts, "residual": residual, "ritz_values": ritz,
                                           "applications": counter["applications"], "breakdown": breakdown}
    raise RuntimeError("ground_state did not converge")


def evolve_krylov(terms, state: np.ndarray, t: float, m: int = 20, tol: float = 1e-10):
    """(exp(-i t H) state, info)."""
    state = np.asarray(state, dtype=complex)
    counter: dict = {}
    remaining, substeps, estimate = float(t), 0, 0.0
    while remaining != 0.0:
        alphas, betas, V, breakdown, norm = lanczos(terms, state, m, True, counter)
        w, Y = np.linalg.eigh(tridiagonal(alphas, betas))

        def err(tau):
            return float(betas[-1] * abs(np.sum(Y[-1] * np.exp(-1j * tau * w) * Y[0])))
        tau = remaining
        if not breakdown:
            while err(tau) > tol * abs(tau) / abs(t):
                tau *= 0.5
                if abs(tau) < TAU_UNDERFLOW * abs(t):
                    raise RuntimeError("the substep underflowed")
            estimate += err(tau)
        state = norm * ((Y @ (np.exp(-1j * tau * w) * Y[0])) @ V)
        remaining -= tau
        substeps += 1
    return state, {"substeps": substeps, "error_estimate": estimate, "applications": counter.get("applications", 0)}
