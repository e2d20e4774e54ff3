"""TEST INFRASTRUCTURE: NumPy statements of the diagonal-operator calls and of the QAOA adjoint walk (DESIGN.md section
20).  Everything here is dense host arithmetic on small registers; tests/test_diagonal_reference_host.py pins it against
Kronecker products, ``scipy.linalg.expm`` and central differences, and the GPU tests compare the device against it.

Index convention of the project: qubit q of n is bit n - 1 - q of the amplitude index.
"""
from __future__ import annotations

import numpy as np


def term_signs(n: int, letters: str, qubits) -> np.ndarray:
    """``(-1)^popcount(i & zmask)`` for every index i, as +-1.0."""
    index = np.arange(1 << n, dtype=np.uint64)
    parity = np.zeros(1 << n, dtype=np.uint64)
    for letter, q in zip(letters, qubits):
        if letter in "Zz":
            parity ^= (index >> np.uint64(n - 1 - int(q))) & np.uint64(1)
        elif letter not in "Ii":
            raise ValueError("a diagonal operator takes the letters I and Z only")
    return 1.0 - 2.0 * parity.astype(np.float64)


def diagonal_from_terms(n: int, terms, start: np.ndarray | None = None) -> np.ndarray:
    """``start + sum_t c_t sign_t`` added term by term in float64, in the caller's order (start: zeros)."""
    values = np.zeros(1 << n, dtype=np.float64) if start is None else np.array(start, dtype=np.float64)
    for c, letters, qubits in terms:
        values += float(np.real(c)) * term_signs(n, letters, qubits)      # c * (+-1) is exact
    return values


def extrema(values: np.ndarray):
    return float(values.min()), int(values.argmin()), float(values.max()), int(values.argmax())


def phase(psi: np.ndarray, d: np.ndarray, gamma: float) -> np.ndarray:
    return psi * np.exp(-1j * gamma * d)


def mul(src: np.ndarray, d: np.ndarray, coeff: complex = 1.0, dst: np.ndarray | None = None) -> np.ndarray:
    out = coeff * d * src
    return out if dst is None else dst + out


def moments(psi: np.ndarray, d: np.ndarray, threshold: float | None = None):
    p = np.abs(psi) ** 2
    below = float(p[d <= threshold].sum()) if threshold is not None else 0.0
    return float(p.sum()), float((p * d).sum()), float((p * d * d).sum()), below


def transition(bra: np.ndarray, ket: np.ndarray, d: np.ndarray) -> complex:
    return complex(np.vdot(bra, d * ket))


def phase_adjoint(psi: np.ndarray, lam: np.ndarray, d: np.ndarray, gamma: float):
    """(value, psi', lambda'): <lambda|D|psi>, then both registers take exp(-i gamma d)."""
    return transition(lam, psi, d), phase(psi, d, gamma), phase(lam, d, gamma)


# ---- QAOA ------------------------------------------------------------------------------------------------------------------
def plus_state(n: int) -> np.ndarray:
    return np.full(1 << n, 2.0 ** (-n / 2.0), dtype=complex)


def apply_1q(psi: np.ndarray, n: int, q: int, m: np.ndarray) -> np.ndarray:
    t = psi.reshape(1 << q, 2, 1 << (n - 1 - q))
    return np.einsum("ab,xby->xay", m, t).reshape(-1)


def mixer(psi: np.ndarray, n: int, beta: float) -> np.ndarray:
    """exp(-i beta sum_q X_q) psi: RX(2 beta) on every qubit."""
    c, s = np.cos(beta), np.sin(beta)
    rx = np.array([[c, -1j * s], [-1j * s, c]])
    for q in range(n):
        psi = apply_1q(psi, n, q, rx)
    return psi


def apply_b(psi: np.ndarray, n: int) -> np.ndarray:
    """B psi, B = sum_q X_q."""
    x = np.array([[0.0, 1.0], [1.0, 0.0]])
    return sum(apply_1q(psi, n, q, x) for q in range(n))


def qaoa_state(d: np.ndarray, gammas, betas, psi: np.ndarray | None = None) -> np.ndarray:
    n = int(d.size).bit_length() - 1
    psi = plus_state(n) if psi is None else np.array(psi, dtype=complex)
    for gamma, beta in zip(gammas, betas):
        psi = mixer(phase(psi, d, gamma), n, beta)
    return psi


def qaoa_energy(d: np.ndarray, gammas, betas) -> float:
    psi = qaoa_state(d, gammas, betas)
    return float(np.real(np.vdot(psi, d * psi)))


def qaoa_energy_and_gradient(d: np.ndarray, gammas, betas):
    """(E, dE/dgamma, dE/dbeta, the rewound register) by the adjoint walk of ``qaoa.energy_and_gradient``."""
    gammas, betas = np.asarray(gammas, dtype=float), np.asarray(betas, dtype=float)
    n = int(d.size).bit_length() - 1
    psi = qaoa_state(d, gammas, betas)
    energy = float(np.real(np.vdot(psi, d * psi)))
    lam = d * psi
    d_gamma, d_beta = np.zeros_like(gammas), np.zeros_like(betas)
    for layer in range(len(gammas) - 1, -1, -1):
        d_beta[layer] = 2.0 * np.vdot(lam, apply_b(psi, n)).imag
        psi, lam = mixer(psi, n, -betas[layer]), mixer(lam, n, -betas[layer])
        value, psi, lam = phase_adjoint(psi, lam, d, -gammas[layer])
        d_gamma[layer] = 2.0 * value.imag
    return energy, d_gamma, d_beta, psi


def qaoa_rotations(terms, n: int, gammas, betas) -> list:
    """The same circuit as a Pauli rotation list ``[(theta, letters, qubits), ...]`` for ``apply_pauli_rotations``:
    ``exp(-i gamma c P) = exp(-i theta / 2 P)`` with ``theta = 2 gamma c``, and ``RX(2 beta)`` as an X rotation."""
    out = []
    for gamma, beta in zip(gammas, betas):
        out += [(2.0 * gamma * float(np.real(c)), letters, list(qubits)) for c, letters, qubits in terms]
        out += [(2.0 * beta, "X", [q]) for q in range(n)]
    return out


def gradient_from_rotations(terms, n: int, p: int, d_theta: np.ndarray):
    """(dE/dgamma, dE/dbeta) from the per-rotation gradient of the list ``qaoa_rotations`` made."""
    per_layer = len(terms) + n
    coeffs = np.array([float(np.real(c)) for c, _, _ in terms])
    d_theta = np.asarray(d_theta).reshape(p, per_layer)
    return 2.0 * d_theta[:, :len(terms)] @ coeffs, 2.0 * d_theta[:, len(terms):].sum(axis=1)


def random_z_terms(n: int, count: int, seed: int, identity: bool = True) -> list:
    """``count`` random Z-only terms of weight 1 to min(n, 4), every qubit equally likely, coefficients in (-1, 1); the
    first touches qubit 0, the second qubit n - 1, and (with ``identity``) the third is the empty term."""
    rng = np.random.default_rng(seed)
    terms = []
    for t in range(count):
        weight = int(rng.integers(1, min(n, 4) + 1)) if n else 0
        qubits = sorted(int(q) for q in rng.choice(n, size=weight, replace=False)) if n else []
        if n and t == 0 and 0 not in qubits:
            qubits[0] = 0
        if n and t == 1 and n - 1 not in qubits:
            qubits[-1] = n - 1
        if identity and t == 2:
            qubits = []
        terms.append((float(rng.uniform(-1.0, 1.0)), "Z" * len(qubits), sorted(set(qubits))))
    return [(c, "Z" * len(qs), qs) for c, _, qs in terms]


def random_ket(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return psi / np.linalg.norm(psi)
