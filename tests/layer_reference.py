"""TEST INFRASTRUCTURE: the NumPy statement of a product layer -- a 2x2 matrix on each of k distinct
qubits -- applied stage by stage in ASCENDING INDEX-BIT order, whatever order the caller lists the qubits in, and member by
member for ensembles.  Nothing here touches the device or the library.  tests/test_layer_reference_host.py pins it against
``layers.product_matrix``.

Index convention of the project: qubit q of n is bit n - 1 - q of the amplitude index.
"""
from __future__ import annotations

import numpy as np

EPS = float(np.finfo(np.float64).eps)


def stage(ket: np.ndarray, n: int, bit: int, m: np.ndarray) -> np.ndarray:
    """``m`` on index bit ``bit``: for the pair (a, b) with the bit 0 / 1, a' = m00 a + m01 b, b' = m10 a + m11 b."""
    t = np.asarray(ket, dtype=np.complex128).reshape(1 << (n - 1 - bit), 2, 1 << bit)
    a, b = t[:, 0, :], t[:, 1, :]
    out = np.empty_like(t)
    out[:, 0, :] = m[0, 0] * a + m[0, 1] * b
    out[:, 1, :] = m[1, 0] * a + m[1, 1] * b
    return out.reshape(-1)


def table(matrices, k: int) -> np.ndarray:
    m = np.asarray(matrices, dtype=np.complex128)
    if m.shape == (2, 2):
        m = np.broadcast_to(m, (k, 2, 2))
    assert m.shape == (k, 2, 2), m.shape
    return m


def apply_layer(ket, matrices, qubits=None) -> np.ndarray:
    """The layer on an n-qubit ket: ``matrices`` of shape (2, 2) or (k, 2, 2), ``qubits`` None = all."""
    ket = np.asarray(ket, dtype=np.complex128)
    n = ket.size.bit_length() - 1
    qubits = list(range(n)) if qubits is None else [int(q) for q in qubits]
    assert len(set(qubits)) == len(qubits) and all(0 <= q < n for q in qubits)
    mats = table(matrices, len(qubits))
    for bit, j in sorted((n - 1 - q, j) for j, q in enumerate(qubits)):
        ket = stage(ket, n, bit, mats[j])
    return ket


def apply_layer_members(kets, matrices, qubits=None) -> list[np.ndarray]:
    """Member m takes ``matrices[m]`` ([members, k, 2, 2]), or every member the same (2, 2) / (k, 2, 2)."""
    per_member = np.ndim(matrices) == 4
    return [apply_layer(ket, matrices[m] if per_member else matrices, qubits) for m, ket in enumerate(kets)]


def apply_layer_density(rho, matrices, qubits=None) -> np.ndarray:
    """``U rho U^dagger`` as the device does it: one layer of 2k stages on the flattened matrix, U on the row qubits and
    conj(U) on the column qubits n + q."""
    rho = np.asarray(rho, dtype=np.complex128)
    n = rho.shape[0].bit_length() - 1
    qubits = list(range(n)) if qubits is None else [int(q) for q in qubits]
    mats = table(matrices, len(qubits))
    flat = apply_layer(rho.reshape(-1), np.concatenate([mats, mats.conj()]), qubits + [n + q for q in qubits])
    return flat.reshape(rho.shape)


def pass_count(n: int, qubits) -> int:
    """max(1, ceil(h / 6)), h = listed qubits with index bit >= 6; one pass up to 12 qubits; none for an empty list."""
    qubits = list(qubits)
    if not qubits:
        return 0
    if n <= 12:
        return 1
    h = sum(1 for q in qubits if n - 1 - q >= 6)
    return max(1, -(-h // 6))


def spectral_norm_product(matrices, k: int) -> float:
    """prod_q max(1, ||U_q||_2)."""
    return float(np.prod([max(1.0, np.linalg.norm(m, 2)) for m in table(matrices, k)]))


def bound(matrices, k: int, norm: float, stages: int | None = None) -> float:
    """16 k eps prod_q max(1, ||U_q||_2) ||psi||: about 4.3 eps ||psi|| per stage for the device's cmul + cfma and the same
    again for the complex128 reference, with a factor of two to spare."""
    return 16.0 * (k if stages is None else stages) * EPS * spectral_norm_product(matrices, k) * norm


def random_unitaries(shape, seed: int) -> np.ndarray:
    """Haar-ish 2x2 unitaries of shape ``shape + (2, 2)``: QR of complex normal matrices."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(tuple(shape) + (2, 2)) + 1j * rng.standard_normal(tuple(shape) + (2, 2))
    q, r = np.linalg.qr(g)
    d = np.diagonal(r, axis1=-2, axis2=-1)
    return q * (d / np.abs(d))[..., None, :]


def random_ket(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    ket = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return ket / np.linalg.norm(ket)


def flip_bits(ket: np.ndarray, n: int, qubits) -> np.ndarray:
    """The ket with the index bits of ``qubits`` flipped: X on every listed qubit, exactly."""
    mask = sum(1 << (n - 1 - int(q)) for q in qubits)
    return np.asarray(ket)[np.arange(1 << n) ^ mask]
