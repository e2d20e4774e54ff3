"""Subsystem read-out of a qubit register: reduced states, marginals and entanglement measures.

The reduced state of up to 12 qubits stays on the device as a ``DensityState`` (``qsv_reduced_density_state``: a Hermitian
rank update on the f64 matrix cores), so ``purity``, ``trace``, ``expect_terms`` and ``apply_channel`` apply to it without a
download.  Spectra go through the host: ``numpy.linalg.eigvalsh`` on the downloaded matrix -- at 12 qubits that is a
256 MiB download and several seconds, and a device eigensolver is out of scope.

A cut is taken on its smaller side: a pure state's two sides share their non-zero spectrum, so any bipartition works
while ``min(k, n - k) <= 12``.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .device import DensityState, DeviceState, _dbl, _ints

MAX_KEPT = 12          # qsv_reduced_density_state
MAX_MARGINAL = 26      # qsv_marginal_probabilities


def check_qubits(qubits, n_qubits: int, limit: int, what: str) -> list[int]:
    """The qubit list as ints; ``ValueError`` for an empty or too long list, repeats and indices out of range."""
    qubits = [int(q) for q in qubits]
    if not 1 <= len(qubits) <= min(limit, n_qubits):
        raise ValueError(f"{what}: keep between 1 and {min(limit, n_qubits)} qubits, not {len(qubits)}")
    if len(set(qubits)) != len(qubits):
        raise ValueError("Indices must be distinct.")
    if any(not 0 <= q < n_qubits for q in qubits):
        raise ValueError(f"qubit index out of range for a {n_qubits}-qubit register")
    return qubits


def smaller_side(qubits, n_qubits: int, limit: int = MAX_KEPT) -> tuple[list[int], bool]:
    """The side of the cut ``qubits | rest`` that is reduced: ``(side, complemented)``.  The complement where it is the
    smaller one; ``ValueError`` where both sides are wider than ``limit``."""
    qubits = check_qubits(qubits, n_qubits, n_qubits, "cut")
    k = len(qubits)
    if min(k, n_qubits - k) > limit:
        raise ValueError(f"a cut of {k} against {n_qubits - k} qubits needs the reduced state of {min(k, n_qubits - k)} qubits: "
                         f"both sides are wider than the {limit} that fit on the device as a density register")
    if k > n_qubits - k:
        kept = set(qubits)
        return [q for q in range(n_qubits) if q not in kept], True
    return qubits, False


def reduced_density_state(state: DeviceState, qubits) -> DensityState:
    """The reduced state of ``qubits`` (at most 12) as a ``DensityState`` on the ket's device; nothing is downloaded and
    the call does not wait.  ``qubits[0]`` is the most significant bit of both indices, as in ``reduced_density``."""
    if state.ndim != 1:
        raise ValueError("the reduced state is taken of a ket: the partial trace of a density register is out of scope")
    qubits = check_qubits(qubits, state.num_qubits, MAX_KEPT, "reduced state")
    flat = DeviceState.zeros(2 * len(qubits), state.device)
    rho = DensityState(flat._h, device=flat.device)
    flat._h = None
    _lib.call("qsv_reduced_density_state", state._h, len(qubits), _ints(qubits), rho._h)
    return rho


def marginal_probabilities(state: DeviceState, qubits) -> np.ndarray:
    """``2^k`` probabilities of the outcomes of ``qubits`` (at most 26), every other qubit summed over; ``qubits[0]`` is
    the most significant bit of the index.  One read pass over the register."""
    if state.ndim != 1:
        raise ValueError("marginal probabilities are taken of a ket")
    qubits = check_qubits(qubits, state.num_qubits, MAX_MARGINAL, "marginal probabilities")
    out = np.empty(1 << len(qubits), dtype=np.float64)
    _lib.call("qsv_marginal_probabilities", state._h, len(qubits), _ints(qubits), _dbl(out))
    return out


def subsystem_purity(state: DeviceState, qubits) -> float:
    """``tr(rho_A^2)``: the reduced state of the smaller side and one pass over it; no spectrum, no download."""
    side, _ = smaller_side(qubits, state.num_qubits)
    if not side:                       # the whole register against nothing: a pure state
        return 1.0
    rho = reduced_density_state(state, side)
    try:
        return rho.purity()
    finally:
        rho.close()


def renyi2_entropy(state: DeviceState, qubits, base: float = np.e) -> float:
    """``-log tr(rho_A^2)`` from ``subsystem_purity``."""
    return float(-np.log(subsystem_purity(state, qubits)) / np.log(base))


def spectrum_of(matrix: np.ndarray) -> np.ndarray:
    """Eigenvalues of a Hermitian matrix, ascending, clipped at 0."""
    return np.linalg.eigvalsh(matrix).clip(min=0.0)


def entropy_of(spectrum: np.ndarray, alpha: float = 1.0, base: float = np.e) -> float:
    """Von Neumann (``alpha = 1``) or Renyi entropy of a probability spectrum."""
    p = np.asarray(spectrum, dtype=np.float64)
    p = p[p > 0.0]
    if alpha == 1.0:
        value = -np.sum(p * np.log(p))
    elif alpha == np.inf:
        value = -np.log(p.max())
    else:
        if alpha <= 0.0:
            raise ValueError("the Renyi order must be positive")
        value = np.log(np.sum(p ** alpha)) / (1.0 - alpha)
    return float(value / np.log(base))


def schmidt_values(state: DeviceState, qubits) -> np.ndarray:
    """Schmidt coefficients of the cut ``qubits | rest``, descending: square roots of the spectrum of the smaller side's
    reduced state (``2^min(k, n-k)`` values)."""
    side, _ = smaller_side(qubits, state.num_qubits)
    if not side:
        return np.ones(1)
    rho = reduced_density_state(state, side)
    try:
        return np.sqrt(rho.eigenvalues()[::-1])
    finally:
        rho.close()


def entanglement_entropy(state: DeviceState, qubits, alpha: float = 1.0, base: float = np.e, *, return_info: bool = False):
    """Entanglement entropy of the cut ``qubits | rest`` (von Neumann for ``alpha = 1``, else Renyi of that order).
    ``alpha = 2`` needs no spectrum and goes through ``renyi2_entropy``.  With ``return_info`` also a dict telling which
    side was reduced (``side``, ``complemented``) and by which kernel."""
    side, complemented = smaller_side(qubits, state.num_qubits)
    if not side:
        value = 0.0
    elif alpha == 2.0:
        value = renyi2_entropy(state, side, base)
    else:
        rho = reduced_density_state(state, side)
        try:
            value = entropy_of(rho.eigenvalues(), alpha, base)
        finally:
            rho.close()
    if return_info:
        return value, {"side": side, "complemented": complemented, "kernel": state.last_kernel()}
    return value


def mutual_information(state: DeviceState, a, b, base: float = np.e) -> float:
    """``S(A) + S(B) - S(AB)`` for two disjoint qubit sets."""
    a, b = [int(q) for q in a], [int(q) for q in b]
    if set(a) & set(b):
        raise ValueError("the two sets must be disjoint")
    return (entanglement_entropy(state, a, base=base) + entanglement_entropy(state, b, base=base)
            - entanglement_entropy(state, a + b, base=base))
