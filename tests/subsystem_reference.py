"""TEST INFRASTRUCTURE: the NumPy statements of the subsystem read-out, the reference of
tests/test_gpu_subsystem.py.  Pinned on the CPU by tests/test_subsystem_reference_host.py.

Qubit 0 is the most significant bit of the flat index; ``qubits[0]`` is the most significant bit of a subsystem index.
"""
from __future__ import annotations

import numpy as np


def kept_first(ket: np.ndarray, qubits) -> np.ndarray:
    """M: the ket as a ``(2^k, 2^(n-k))`` matrix, rows = settings of ``qubits``, columns = settings of the rest."""
    ket = np.asarray(ket, dtype=np.complex128)
    n = ket.shape[0].bit_length() - 1
    qubits = list(qubits)
    rest = [q for q in range(n) if q not in qubits]
    return ket.reshape((2,) * n).transpose(qubits + rest).reshape(1 << len(qubits), -1)


def reduced_density(ket: np.ndarray, qubits) -> np.ndarray:
    """``rho_A = M M^dagger``."""
    m = kept_first(ket, qubits)
    return m @ m.conj().T


def marginal_probabilities(ket: np.ndarray, qubits) -> np.ndarray:
    """Squared row norms of M."""
    m = kept_first(ket, qubits)
    return np.sum(m.real ** 2 + m.imag ** 2, axis=1)


def schmidt_values(ket: np.ndarray, qubits) -> np.ndarray:
    """Singular values of M, descending: more accurate than the square roots of the spectrum of ``M M^dagger``."""
    return np.linalg.svd(kept_first(ket, qubits), compute_uv=False)


def entropy(probabilities: np.ndarray, alpha: float = 1.0) -> float:
    """Von Neumann / Renyi entropy of a spectrum, in nats."""
    p = np.asarray(probabilities, dtype=np.float64)
    p = p[p > 0.0]
    if alpha == 1.0:
        return float(-np.sum(p * np.log(p)))
    return float(np.log(np.sum(p ** alpha)) / (1.0 - alpha))


def entanglement_entropy(ket: np.ndarray, qubits, alpha: float = 1.0) -> float:
    return entropy(schmidt_values(ket, qubits) ** 2, alpha)


def subsystem_purity(ket: np.ndarray, qubits) -> float:
    return float(np.sum(schmidt_values(ket, qubits) ** 4))


def mutual_information(ket: np.ndarray, a, b) -> float:
    return entanglement_entropy(ket, a) + entanglement_entropy(ket, b) - entanglement_entropy(ket, list(a) + list(b))


# ---- named states -------------------------------------------------------------------------------------------------
def ghz(n: int) -> np.ndarray:
    ket = np.zeros(1 << n, dtype=np.complex128)
    ket[0] = ket[-1] = np.sqrt(0.5)
    return ket


def product_state(n: int, seed: int) -> np.ndarray:
    """A tensor product of n random one-qubit kets."""
    rng = np.random.default_rng(seed)
    ket = np.ones(1, dtype=np.complex128)
    for _ in range(n):
        q = rng.normal(size=2) + 1j * rng.normal(size=2)
        ket = np.kron(ket, q / np.linalg.norm(q))
    return ket


def bell_pairs(n: int, pairs) -> np.ndarray:
    """``(|00> + |11>) / sqrt 2`` on every (a, b) of ``pairs``, |0> elsewhere."""
    ket = np.zeros(1 << n, dtype=np.complex128)
    pairs = list(pairs)
    for setting in range(1 << len(pairs)):
        index = 0
        for j, (a, b) in enumerate(pairs):
            if (setting >> j) & 1:
                index |= (1 << (n - 1 - a)) | (1 << (n - 1 - b))
        ket[index] = 2.0 ** (-0.5 * len(pairs))
    return ket


def placements(n: int, k: int, seed: int) -> dict:
    """The qubit lists the tests place a subsystem on, by name.  Qubit q sits on bit n-1-q of the flat index:
    ``low`` = the lowest k bits, ``top`` = the top k bits listed in reverse, ``from6`` = bits 6 .. 6+k-1 (where they fit),
    ``random0..2`` = unsorted random choices."""
    out = {"low": [n - 1 - b for b in range(k)], "top": list(range(k))[::-1]}
    if n - 6 >= k:
        out["from6"] = [n - 1 - b for b in range(6, 6 + k)]
    rng = np.random.default_rng(seed)
    for r in range(3):
        out[f"random{r}"] = [int(q) for q in rng.permutation(n)[:k]]
    return out
