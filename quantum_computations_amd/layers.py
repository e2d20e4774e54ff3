"""Product layers: a one-qubit gate on each of many qubits, applied in a few tile passes.

The helpers here build the ``(..., 2, 2)`` arrays that ``DeviceState.apply_layer``, ``DensityState.apply_layer`` and
``TrajectoryEnsemble.apply_layer`` take; they broadcast over their angle, so ``rx(betas[:, None] * np.ones(n))`` is the
``[members, n, 2, 2]`` table of a per-member mixer.  Conventions are the project's: ``rz(t) = exp(-i t/2 Z)``.
"""
from __future__ import annotations

import numpy as np


def _half(theta) -> np.ndarray:
    return 0.5 * np.asarray(theta, dtype=np.float64)


def rx(theta) -> np.ndarray:
    """``[[cos t/2, -i sin t/2], [-i sin t/2, cos t/2]]`` for every entry of ``theta``."""
    h = _half(theta)
    c, s = np.cos(h), np.sin(h)
    out = np.empty(h.shape + (2, 2), dtype=np.complex128)
    out[..., 0, 0] = out[..., 1, 1] = c
    out[..., 0, 1] = out[..., 1, 0] = -1j * s
    return out


def ry(theta) -> np.ndarray:
    """``[[cos t/2, -sin t/2], [sin t/2, cos t/2]]`` for every entry of ``theta``."""
    h = _half(theta)
    c, s = np.cos(h), np.sin(h)
    out = np.empty(h.shape + (2, 2), dtype=np.complex128)
    out[..., 0, 0] = out[..., 1, 1] = c
    out[..., 0, 1] = -s
    out[..., 1, 0] = s
    return out


def rz(theta) -> np.ndarray:
    """``diag(exp(-i t/2), exp(+i t/2))`` for every entry of ``theta``."""
    h = _half(theta)
    out = np.zeros(h.shape + (2, 2), dtype=np.complex128)
    out[..., 0, 0] = np.cos(h) - 1j * np.sin(h)
    out[..., 1, 1] = np.cos(h) + 1j * np.sin(h)
    return out


def hadamard() -> np.ndarray:
    return np.array([[1.0, 1.0], [1.0, -1.0]], dtype=np.complex128) / np.sqrt(2.0)


_PAULI = {"rx": np.array([[0.0, 1.0], [1.0, 0.0]], dtype=np.complex128),
          "ry": np.array([[0.0, -1.0j], [1.0j, 0.0]], dtype=np.complex128),
          "rz": np.array([[1.0, 0.0], [0.0, -1.0]], dtype=np.complex128)}
_ROTATION = {"rx": rx, "ry": ry, "rz": rz}


def rotation(kind: str, theta) -> np.ndarray:
    """``rx`` / ``ry`` / ``rz`` by name, for every entry of ``theta``."""
    if kind not in _ROTATION:
        raise ValueError(f"kind must be one of {tuple(_ROTATION)}, not {kind!r}")
    return _ROTATION[kind](theta)


def generator(kind: str) -> np.ndarray:
    """The constant ``G = (dU/dtheta) U^dagger = -i/2 P`` of ``U = exp(-i theta/2 P)`` for ``kind`` in ``rx`` / ``ry`` /
    ``rz`` (``P = X`` / ``Y`` / ``Z``): what ``gradient`` contracts with the transition matrices of ``layer_adjoint``."""
    if kind not in _PAULI:
        raise ValueError(f"kind must be one of {tuple(_PAULI)}, not {kind!r}")
    return -0.5j * _PAULI[kind]


def gradient(T, generators) -> np.ndarray:
    """``2 Re sum_ab G[a][b] T[a][b]`` per stage: ``dE/dtheta`` of every factor of a layer from ``T[k, 2, 2]``
    (``DeviceState.layer_adjoint`` with ``lam = H psi``) and the factors' generators, ``(2, 2)`` for all or ``(k, 2, 2)``.
    For ``generator(kind)`` this is ``Im <lam|P|psi>``."""
    T = np.asarray(T, dtype=np.complex128)
    if T.ndim != 3 or T.shape[1:] != (2, 2):
        raise ValueError("T must have shape [k, 2, 2]")
    G = layer_table(generators, T.shape[0], "generators")
    return 2.0 * np.real(np.sum(G * T, axis=(1, 2)))


def product_matrix(matrices) -> np.ndarray:
    """``matrices[0] (x) matrices[1] (x) ...``: the ``2^k x 2^k`` matrix of a layer whose first listed qubit is the most
    significant leg, as ``apply_matrix`` takes it.  For tests and small hosts."""
    matrices = np.asarray(matrices, dtype=np.complex128)
    if matrices.ndim != 3 or matrices.shape[1:] != (2, 2):
        raise ValueError("matrices must have shape [k, 2, 2]")
    out = np.ones((1, 1), dtype=np.complex128)
    for m in matrices:
        out = np.kron(out, m)
    return out


def layer_table(matrices, k: int, what: str = "matrices") -> np.ndarray:
    """``matrices`` of shape ``(2, 2)`` (the same gate on each of the ``k`` qubits) or ``(k, 2, 2)`` as a contiguous
    ``[k, 2, 2]`` complex128 array; ``ValueError`` for any other shape."""
    m = np.asarray(matrices, dtype=np.complex128)
    if m.shape == (2, 2):
        m = np.broadcast_to(m, (k, 2, 2))
    if m.shape != (k, 2, 2):
        raise ValueError(f"{what} must have shape (2, 2) or (k, 2, 2) = ({k}, 2, 2), not {np.shape(matrices)}")
    return np.ascontiguousarray(m)
