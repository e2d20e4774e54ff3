"""TEST INFRASTRUCTURE: the NumPy model of Pauli-string rotations, of the greedy pass planner
(quantum_computations_amd/csrc/qsv_pauli_rotation_plan.h) and of ``npq.trotter_rotations``.

``P psi`` is built letter by letter with ``oracle.dv_oracle.apply_gate`` (as ``term_truth`` does in
tests/test_gpu_pauli_sum.py); the rotated ket is ``cos(theta/2) psi - i sin(theta/2) P psi``.  Nothing here touches the
device or the library.  tests/test_pauli_rotation_reference_host.py pins this model against ``scipy.linalg.expm``.
"""
from __future__ import annotations

import numpy as np

from oracle import dv_oracle as O

ROTATIONS_PER_PASS = 8
MATS = {"I": np.eye(2), "X": np.array([[0, 1], [1, 0]], dtype=complex), "Y": np.array([[0, -1j], [1j, 0]]),
        "Z": np.array([[1, 0], [0, -1]], dtype=complex)}


def apply_string(ket: np.ndarray, letters: str, qubits) -> np.ndarray:
    """``P ket`` for the Pauli string ``letters[j]`` on ``qubits[j]`` (qubit 0 is the leftmost factor)."""
    phi = np.asarray(ket, dtype=complex)
    for letter, q in zip(letters.upper(), qubits):
        if letter != "I":
            phi = O.apply_gate(phi, MATS[letter], [int(q)])
    return phi


def rotate(ket: np.ndarray, theta: float, letters: str, qubits) -> np.ndarray:
    """``exp(-i theta/2 P) ket``."""
    ket = np.asarray(ket, dtype=complex)
    return np.cos(theta / 2) * ket - 1j * np.sin(theta / 2) * apply_string(ket, letters, qubits)


def rotate_list(ket: np.ndarray, rotations) -> np.ndarray:
    """The ordered list ``[(theta, letters, qubits), ...]``, the first applied first."""
    for theta, letters, qubits in rotations:
        ket = rotate(ket, theta, letters, qubits)
    return np.asarray(ket, dtype=complex)


def rotate_density(rho: np.ndarray, rotations) -> np.ndarray:
    """``U rho U^dagger`` for the ordered list: ``U`` on every column of ``rho``, then ``conj(U)`` on every row."""
    rho = np.asarray(rho, dtype=complex)
    left = np.stack([rotate_list(rho[:, j], rotations) for j in range(rho.shape[1])], axis=1)       # U rho
    return np.stack([np.conj(rotate_list(np.conj(left[i, :]), rotations)) for i in range(left.shape[0])], axis=0)


def masks(n: int, letters: str, qubits) -> tuple[int, int]:
    """(xmask, zmask) in register bits: qubit q is bit n - 1 - q; X and Y flip, Z and Y give a sign."""
    x = sum(1 << (n - 1 - int(q)) for letter, q in zip(letters.upper(), qubits) if letter in "XY")
    z = sum(1 << (n - 1 - int(q)) for letter, q in zip(letters.upper(), qubits) if letter in "ZY")
    return x, z


def plan(terms, cap: int = ROTATIONS_PER_PASS) -> list[dict]:
    """The greedy planner on ``[(xmask, zmask), ...]``: never reorders; the open pass takes the next term if it holds
    fewer than ``cap`` terms and the term is diagonal, the pass still is, or both flip the same bits.  A pass that was
    diagonal takes the xmask of the first flipping term.  The pivot is the HIGHEST set bit of the xmask (-1: none)."""
    passes: list[dict] = []
    for t, (x, z) in enumerate(terms):
        last = passes[-1] if passes else None
        if last is None or len(last["index"]) >= cap or not (x == 0 or last["xmask"] == 0 or x == last["xmask"]):
            last = {"xmask": 0, "pivot": -1, "index": [], "term_xmask": [], "zmask": [], "n_y": []}
            passes.append(last)
        if last["xmask"] == 0 and x:
            last["xmask"], last["pivot"] = x, x.bit_length() - 1
        last["index"].append(t)
        last["term_xmask"].append(x)
        last["zmask"].append(z)
        last["n_y"].append(bin(x & z).count("1"))
    return passes


def pass_count(n: int, rotations) -> int:
    return len(plan([masks(n, letters, qubits) for _, letters, qubits in rotations]))


def trotter_rotations(terms, t: float, steps: int = 1, order: int = 1) -> list:
    """The model of ``npq.trotter_rotations`` on a term list ``[(coefficient, letters, qubits), ...]``."""
    if order not in (1, 2):
        raise ValueError("Trotter order must be 1 or 2")
    out = []
    for _ in range(steps):
        if order == 1:
            out += [(2.0 * complex(c).real * t / steps, letters, list(qubits)) for c, letters, qubits in terms]
        else:
            half = [(complex(c).real * t / steps, letters, list(qubits)) for c, letters, qubits in terms]
            out += half + half[::-1]
    return out
