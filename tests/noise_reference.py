"""TEST INFRASTRUCTURE: NumPy statements of what the noise entry points compute (tests/test_noise_reference_host.py pins
them on the CPU; tests/test_gpu_noise.py compares the device against them).

Qubit q of n is bit n-1-q of the flat index; ``qubits[0]`` is the most significant leg of a Kraus operator -- the
conventions of include/qsv.h.  Branch weights are formed as ``||K_j psi||^2`` directly, not through a reduced density
matrix, so that the device's route (``Re tr(E_j rho_q)``) is checked against something else.
"""
from __future__ import annotations

import numpy as np


def embed(op: np.ndarray, qubits, n: int) -> np.ndarray:
    """The 2^n x 2^n matrix of ``op`` on ``qubits`` (first = most significant leg) of an n-qubit register."""
    k = len(qubits)
    rest = [q for q in range(n) if q not in qubits]
    full = np.kron(np.asarray(op, dtype=np.complex128), np.eye(1 << (n - k)))
    # kron order is qubits + rest; bring axis i of that order to its own place
    order = list(qubits) + rest
    t = full.reshape((2,) * (2 * n))
    perm = [order.index(q) for q in range(n)]
    t = t.transpose(perm + [n + p for p in perm])
    return np.ascontiguousarray(t).reshape(1 << n, 1 << n)


def apply_op(op: np.ndarray, psi: np.ndarray, qubits, n: int) -> np.ndarray:
    """``op`` on ``qubits`` of the ket ``psi`` without the full matrix."""
    k = len(qubits)
    t = np.asarray(psi, dtype=np.complex128).reshape((2,) * n)
    g = np.asarray(op, dtype=np.complex128).reshape((2,) * (2 * k))
    t = np.tensordot(g, t, axes=(list(range(k, 2 * k)), list(qubits)))
    t = np.moveaxis(t, list(range(k)), list(qubits))
    return np.ascontiguousarray(t).reshape(-1)


def channel_on_density(kraus, rho: np.ndarray, qubits, n: int) -> np.ndarray:
    """``sum_j K_j rho K_j^dagger`` with K_j on ``qubits``."""
    out = np.zeros_like(np.asarray(rho, dtype=np.complex128))
    for K in kraus:
        full = embed(K, qubits, n)
        out += full @ rho @ full.conj().T
    return out


def branch_weights(kraus, psi: np.ndarray, qubits, n: int) -> np.ndarray:
    """``w_j = ||K_j psi||^2``."""
    return np.array([float(np.vdot(v, v).real) for v in (apply_op(K, psi, qubits, n) for K in kraus)])


def pick_branch(weights, u: float) -> int:
    """The first j with w_0 + ... + w_j > u * total; the last j with w_j > 0 if rounding leaves none; 0 if all are 0.
    Sums run in index order."""
    total = 0.0
    for w in weights:
        total += float(w)
    target = u * total
    run, last = 0.0, -1
    for j, w in enumerate(weights):
        run += float(w)
        if w > 0.0:
            last = j
        if run > target and w > 0.0:
            return j
    return max(last, 0)


def branch_intervals(weights) -> list:
    """``[(lo_j, hi_j)]`` of ``u`` for which ``pick_branch`` gives j (as fractions of the total, exact arithmetic aside)."""
    total = float(np.sum(weights))
    edges = np.concatenate([[0.0], np.cumsum(weights) / total]) if total > 0.0 else np.zeros(len(weights) + 1)
    return [(float(edges[j]), float(edges[j + 1])) for j in range(len(weights))]


def boundary_distance(weights, u: float) -> float:
    """How far ``u`` is from the nearest interior branch boundary, relative to the total."""
    total = float(np.sum(weights))
    if not total > 0.0 or len(weights) < 2:
        return 1.0
    edges = np.cumsum(weights)[:-1] / total
    return float(np.min(np.abs(edges - u)))


def trajectory_step(kraus, psi: np.ndarray, qubits, n: int, u: float = 0.0, forced=None):
    """One step: ``(new ket, j, w_j / total)``.  The new ket is ``K_j psi sqrt(total / w_j)``, zeros if ``w_j`` is 0."""
    w = branch_weights(kraus, psi, qubits, n)
    total = 0.0
    for x in w:
        total += float(x)
    j = int(forced) if forced is not None else pick_branch(w, u)
    if not (w[j] > 0.0 and total > 0.0):
        return np.zeros_like(np.asarray(psi, dtype=np.complex128)), j, 0.0
    return apply_op(kraus[j], psi, qubits, n) * np.sqrt(total / w[j]), j, float(w[j] / total)


def full_matrices(circuit, n: int) -> list:
    """The circuit with every operator embedded in the whole register once: ``("gate", M)`` / ``("channel", stack of M_j)``.
    What a run of many shots on a few qubits walks instead of the tensor contractions."""
    return [(kind, embed(op, qubits, n)) if kind == "gate" else (kind, np.stack([embed(K, qubits, n) for K in op]))
            for kind, op, qubits in circuit]


def run_trajectory(circuit, psi: np.ndarray, n: int, rng, full=None):
    """``circuit``: a list of ``("gate", matrix, qubits)`` and ``("channel", kraus, qubits)``.  One uniform number from
    ``rng`` per channel, in order.  Returns ``(final ket, branches, draws, smallest boundary distance)``.  ``full``:
    ``full_matrices(circuit, n)``, to save a caller with many shots the embedding."""
    psi = np.asarray(psi, dtype=np.complex128)
    full = full if full is not None else full_matrices(circuit, n)
    branches, draws, closest = [], [], 1.0
    for kind, op in full:
        if kind == "gate":
            psi = op @ psi
            continue
        u = float(rng.random())
        images = op @ psi                                           # K_j psi, one row per branch
        w = np.array([float(np.vdot(v, v).real) for v in images])   # ||K_j psi||^2, directly
        closest = min(closest, boundary_distance(w, u))
        total = 0.0
        for x in w:
            total += float(x)
        j = pick_branch(w, u)
        psi = images[j] * np.sqrt(total / w[j]) if w[j] > 0.0 and total > 0.0 else np.zeros_like(psi)
        branches.append(j)
        draws.append(u)
    return psi, branches, draws, closest


def run_exact(circuit, rho: np.ndarray, n: int) -> np.ndarray:
    rho = np.asarray(rho, dtype=np.complex128)
    for kind, op, qubits in circuit:
        if kind == "gate":
            full = embed(op, qubits, n)
            rho = full @ rho @ full.conj().T
        else:
            rho = channel_on_density(op, rho, qubits, n)
    return rho


PAULI = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]]), "Y": np.array([[0, -1j], [1j, 0]]), "Z": np.diag([1.0, -1.0])}


def pauli_matrix(letters: str, qubits, n: int) -> np.ndarray:
    out = np.eye(1 << n, dtype=np.complex128)
    for letter, q in zip(letters, qubits):
        out = embed(PAULI[letter.upper()], [q], n) @ out
    return out


def expect_terms_ket(terms, psi: np.ndarray, n: int) -> float:
    total = 0.0
    for c, letters, qubits in terms:
        v = np.asarray(psi, dtype=np.complex128)
        for letter, q in zip(letters, qubits):
            v = apply_op(PAULI[letter.upper()], v, [q], n)
        total += float((complex(c) * np.vdot(psi, v)).real)
    return total


def random_ket(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    v = rng.normal(size=1 << n) + 1j * rng.normal(size=1 << n)
    return v / np.linalg.norm(v)


def random_density(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(1 << n, 1 << n)) + 1j * rng.normal(size=(1 << n, 1 << n))
    rho = a @ a.conj().T
    return rho / np.trace(rho).real


def compose_minimal(first, second) -> list:
    """The channel ``second o first`` (both on the same qubits) with as few Kraus operators as it needs: the eigenvectors of
    its Choi matrix ``sum_ij vec(K_i K_j) vec(K_i K_j)^dagger``, at most dim^2 of them."""
    products = [np.asarray(b, dtype=np.complex128) @ np.asarray(a, dtype=np.complex128) for a in first for b in second]
    dim = products[0].shape[0]
    choi = sum(np.outer(K.reshape(-1), K.reshape(-1).conj()) for K in products)
    values, vectors = np.linalg.eigh(choi)
    return [np.sqrt(v) * vectors[:, i].reshape(dim, dim) for i, v in enumerate(values) if v > 1e-14]


def random_kraus(dim: int, count: int, seed: int) -> list:
    """``count`` Kraus operators of a trace-preserving channel: blocks of a random isometry."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(dim * count, dim)) + 1j * rng.normal(size=(dim * count, dim))
    q, _ = np.linalg.qr(a)
    return [np.ascontiguousarray(q[j * dim:(j + 1) * dim, :]) for j in range(count)]
