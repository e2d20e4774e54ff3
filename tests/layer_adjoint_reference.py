"""TEST INFRASTRUCTURE: the NumPy statement of the adjoint walk through a product layer.  The stages go
in ASCENDING INDEX-BIT order, as in tests/layer_reference.py; for each, ``T[a][b] = sum_rest conj(lambda[a, rest]) psi[b, rest]``
is taken on the registers as they stand, by reshaping both kets to ``[.., 2, ..]`` and contracting, and then the stage's matrix
goes onto both through ``layer_reference.stage``.  Nothing here touches the device or the library.
tests/test_layer_adjoint_reference_host.py pins it against dense matrices.

Index convention of the project: qubit q of n is bit n - 1 - q of the amplitude index.
"""
from __future__ import annotations

import numpy as np

import layer_reference as L

EPS = L.EPS


def transition(lam: np.ndarray, psi: np.ndarray, n: int, bit: int) -> np.ndarray:
    """``T[a][b] = sum_rest conj(lam[a, rest]) psi[b, rest]`` for index bit ``bit``."""
    l = np.asarray(lam, dtype=np.complex128).reshape(1 << (n - 1 - bit), 2, 1 << bit)
    p = np.asarray(psi, dtype=np.complex128).reshape(1 << (n - 1 - bit), 2, 1 << bit)
    return np.einsum("xay,xby->ab", l.conj(), p)


def _qubits(n: int, qubits) -> list[int]:
    qubits = list(range(n)) if qubits is None else [int(q) for q in qubits]
    assert len(set(qubits)) == len(qubits) and all(0 <= q < n for q in qubits)
    return qubits


def layer_adjoint(psi, lam, inverse, qubits=None):
    """``(T[k, 2, 2], psi', lam')``: for the stages in ascending bit order ``T`` of the stage on the registers as they stand,
    then ``inverse[j]`` on both.  ``inverse``: (2, 2) or (k, 2, 2), indexed as ``qubits`` is, and so is ``T``."""
    psi, lam = np.asarray(psi, dtype=np.complex128), np.asarray(lam, dtype=np.complex128)
    n = psi.size.bit_length() - 1
    qubits = _qubits(n, qubits)
    mats = L.table(inverse, len(qubits))
    T = np.zeros((len(qubits), 2, 2), dtype=np.complex128)
    for bit, j in sorted((n - 1 - q, j) for j, q in enumerate(qubits)):
        T[j] = transition(lam, psi, n, bit)
        psi = L.stage(psi, n, bit, mats[j])
        lam = L.stage(lam, n, bit, mats[j])
    return T, psi, lam


def layer_transition(bra, ket, qubits=None) -> np.ndarray:
    """``T`` of every listed qubit with nothing applied."""
    ket = np.asarray(ket, dtype=np.complex128)
    n = ket.size.bit_length() - 1
    return np.array([transition(bra, ket, n, n - 1 - q) for q in _qubits(n, qubits)], dtype=np.complex128).reshape(-1, 2, 2)


def one_qubit_densities(ket, qubits=None) -> np.ndarray:
    """``rho_q[b][a] = T_q[a][b]`` with bra = ket."""
    return np.swapaxes(layer_transition(ket, ket, qubits), 1, 2)


def value_bound(n: int, norm_psi: float, norm_lam: float) -> float:
    """``4 * 2^n * eps * ||psi|| ||lambda||``: the any-order bound on a sum of 2^n rounded products, with a factor 4 for the
    complex arithmetic and the reference's own rounding."""
    return 4.0 * (1 << n) * EPS * norm_psi * norm_lam


def heisenberg_chain(n: int) -> list[tuple]:
    """``sum_q X_q X_q+1 + Y_q Y_q+1 + Z_q Z_q+1`` on an open chain, with unequal real coefficients."""
    terms = []
    for q in range(n - 1):
        terms += [(1.0, "XX", [q, q + 1]), (0.75, "YY", [q, q + 1]), (-0.5, "ZZ", [q, q + 1])]
    return terms


_P = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0])}


def apply_terms(ket: np.ndarray, terms) -> np.ndarray:
    """``H ket`` for a Pauli term list, factor by factor through ``layer_reference.stage``."""
    ket = np.asarray(ket, dtype=np.complex128)
    n = ket.size.bit_length() - 1
    out = np.zeros_like(ket)
    for c, letters, qubits in terms:
        v = ket
        for letter, q in zip(letters, qubits):
            v = L.stage(v, n, n - 1 - q, _P[letter.upper()].astype(np.complex128))
        out = out + c * v
    return out


def dense_terms(n: int, terms) -> np.ndarray:
    """The 2^n x 2^n matrix of a Pauli term list (small n)."""
    h = np.zeros((1 << n, 1 << n), dtype=np.complex128)
    for c, letters, qubits in terms:
        factors = [np.eye(2, dtype=np.complex128)] * n
        for letter, q in zip(letters, qubits):
            factors[q] = _P[letter.upper()].astype(np.complex128)
        m = np.ones((1, 1), dtype=np.complex128)
        for f in factors:
            m = np.kron(m, f)
        h += c * m
    return h
