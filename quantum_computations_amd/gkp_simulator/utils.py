"""Conversions and logical read-out of GKP registers (``simulators/gkp_simulator/utils.py:1-106``).

``full_logical_density_mps`` is the expensive one: ``4^N`` Pauli strings, each an environment contraction through the
chain.  Here the four read-out operators are uploaded once, each site is dressed with them by one GEMM each
(``qsv_tensor_apply_axis_dev``), and a depth-first walk over the strings shares the environments of common prefixes, so
the device does ``(4^(N+1) - 4) / 3`` small GEMM pairs instead of ``N 4^N`` einsums.
"""
from __future__ import annotations

import threading
from functools import reduce
from itertools import product

import numpy as np

from ..cv_simulator.mps import MPS, tensor_svd  # noqa: F401  (re-exported, as upstream)
from ..cv_simulator.utils import *  # noqa: F401,F403
from ..dv_simulator import numpy_quantum as npq

PI = np.pi
SQPI = np.sqrt(np.pi)

_LOGICAL_PAULIS = (np.array([[1, 0], [0, 1]]), np.array([[0, 1], [1, 0]]), np.array([[0, -1j], [1j, 0]]),
                   np.array([[1, 0], [0, -1]]))


def eps2db(epsilon: float) -> float:
    """GKP damping parameter -> squeezing in dB."""
    return -10.0 * np.log10(2.0 * np.tanh(epsilon / 2.0))


def db2eps(db_squeezing: float) -> float:
    """Squeezing in dB -> GKP damping parameter (inverse of :func:`eps2db`)."""
    return 2.0 * np.arctanh(np.float_power(10.0, -db_squeezing / 10.0) / 2.0)


def decomp_result(s: float) -> tuple[int, float]:
    """``s = (n + r) sqrt(pi)`` with ``n`` the nearest integer."""
    in_units = s / SQPI
    n = np.round(in_units).astype(int)
    return n, in_units - n


def format_result(s: float, dec: int = 4) -> str:
    n, r = decomp_result(s * 2 ** 0.5)
    return f"({n}{r:+.{dec}f})√π"


def cv2dv_information(s: float) -> bool:
    """Logical bit carried by a homodyne value: parity of the nearest multiple of sqrt(pi)."""
    return np.round(s / SQPI) % 2 == 1


def syndrome_matrix(syndromes: list[tuple[int, int]]) -> np.ndarray:
    """Tensor product of ``Z^z X^x`` over the qubits, one ``(x, z)`` pair each."""
    factors = []
    for x, z in syndromes:
        m = npq.IDTY
        if x:
            m = npq.X @ m
        if z:
            m = npq.Z @ m
        factors.append(m)
    return npq.tensor(*factors)


_READOUT_OPERATORS: dict = {}      # grid -> [I, X, Y, Z] read-out operators, see pauli_readout_operators
_READOUT_LOCK = threading.Lock()   # held for lookup and insertion (simulations on worker threads share the cache)


def pauli_readout_operators(qs: np.ndarray) -> list[np.ndarray]:
    """Grid operators ``[I, X, Y, Z]`` whose expectation values are the logical Bloch components: truncated Fourier
    series of the sqrt(pi)-periodic sign functions -- odd multiples ``m`` of sqrt(pi), coefficients ``±2/(m pi)``,
    displacements realised by sinc interpolation and the momentum-like ones by cosines (utils.py:48-71; appendix D
    of Shaw et al., arXiv:2403.02396).  The quirks are kept: the spacing here is ``(q_max - q_min) / len(qs)``."""
    # the operators depend on the grid alone (0.2 s of sinc evaluations at d = 1000): one set per grid is kept, read-only,
    # which also lets a register keep ONE device copy of each (SiteRegister._keep goes by array identity)
    key = (qs.shape[0], qs.dtype.str, qs.tobytes()) if isinstance(qs, np.ndarray) and qs.ndim == 1 and qs.shape[0] <= 4096 else None
    if key is not None:
        with _READOUT_LOCK:
            hit = _READOUT_OPERATORS.get(key)
        if hit is not None:
            return hit
    d = len(qs)
    dq = (qs[-1] - qs[0]) / d
    offsets = qs[:, None] - qs[None, :]
    shift, phase = np.zeros((d, d)), np.zeros((d, d))
    for n, m in enumerate(range(1, int((qs[-1] - qs[0]) / SQPI) + 1, 2)):
        weight = (-1) ** (n % 2) * 2 / (m * PI)
        shift += weight * (np.sinc((offsets - m * SQPI) / dq) + np.sinc((offsets + m * SQPI) / dq))
        phase += weight * np.diag(2 * np.cos(SQPI * m * qs))
    operators = [np.identity(d), shift, 1j * shift @ phase, phase]
    if key is not None:
        for op in operators:
            op.setflags(write=False)
        with _READOUT_LOCK:
            hit = _READOUT_OPERATORS.get(key)
            if hit is not None:         # another thread was quicker: hand out its arrays (one device copy per register)
                return hit
            if len(_READOUT_OPERATORS) >= 2:
                _READOUT_OPERATORS.clear()
            _READOUT_OPERATORS[key] = operators
    return operators


def full_logical_density_mps(mps: MPS, normalised: bool = False) -> np.ndarray:
    """Logical ``2^N x 2^N`` density matrix of an N-mode GKP register: ``sum_P <P_readout> P_logical / 2^N`` with
    the grid measure ``(dq/2)^N`` of the reference (utils.py:82-96)."""
    qs, n = mps.domain, len(mps)
    dq = (qs[-1] - qs[0]) / len(qs)
    operators = pauli_readout_operators(qs)
    if mps.layout == "sites":
        coefficients = mps.reg.operator_string_coefficients(operators)
    else:  # dense register: contract on the host (small registers only)
        psi = mps.contract().reshape((len(qs),) * n)
        coefficients = np.zeros((4,) * n, dtype=np.complex128)
        for index in product(range(4), repeat=n):
            dressed = psi
            for axis, i in enumerate(index):
                dressed = np.moveaxis(np.tensordot(operators[i], dressed, [1, axis]), 0, axis)
            coefficients[index] = np.vdot(psi, dressed)
    rho = np.zeros((2 ** n, 2 ** n), dtype=complex)
    for index in product(range(4), repeat=n):
        rho += coefficients[index] * (dq / 2) ** n * reduce(np.kron, [_LOGICAL_PAULIS[i] for i in index], 1)
    if normalised:
        rho /= np.trace(rho)
    return rho


def full_logical_density(qs: np.ndarray, state: np.ndarray, normalised: bool = False, device: int = 0) -> np.ndarray:
    """Logical density matrix of a dense wavefunction ``state[q_0, ..., q_{N-1}]``.  (Upstream this helper stops after
    splitting the tensor into sites and returns nothing, utils.py:98-106; here it finishes the job.)"""
    rest = np.reshape(state, (1, *np.shape(state), 1))
    sites = []
    while rest.ndim > 3:
        head, rest = tensor_svd(rest, (0, 1), tuple(range(2, rest.ndim)), device=device)
        sites.append(head)
    sites.append(rest)
    return full_logical_density_mps(MPS(qs, sites, device=device, layout="sites"), normalised)


def sample_logical(mps: MPS, shots: int, basis="Z", rng=None) -> np.ndarray:
    """Logical bit strings of an N-mode GKP register as the experiment reads them: ``shots`` homodyne outcomes of every
    mode (``MPS.sample``), each binned to the nearest multiple of sqrt(pi) by :func:`cv2dv_information`.  ``basis``:
    ``"Z"`` (q outcomes) or ``"X"`` (p outcomes) for the whole register, or one character per mode (``"ZXZ"`` or a
    sequence).  Returns ``uint8 (shots, N)``; the register is not modified.  No upstream counterpart."""
    n = len(mps)
    letters = [basis] * n if isinstance(basis, str) and len(basis) == 1 else list(basis)
    if len(letters) != n:
        raise IndexError(f"basis must be one character or one per mode ({n}), got {basis!r}")
    if any(letter not in ("Z", "X") for letter in letters):
        raise ValueError(f"basis characters must be 'Z' or 'X', got {basis!r}")
    values = mps.sample(shots, quadratures=["q" if letter == "Z" else "p" for letter in letters], rng=rng)
    return cv2dv_information(values).astype(np.uint8)


def logical_distribution(bits: np.ndarray) -> np.ndarray:
    """Frequencies of the ``2^N`` logical basis states in ``bits`` (``(shots, N)`` zeros and ones, as
    :func:`sample_logical` returns them), qubit 0 the most significant bit of the index."""
    bits = np.asarray(bits)
    if bits.ndim != 2 or bits.shape[0] < 1:
        raise ValueError(f"bits must have shape (shots >= 1, N), got {bits.shape}")
    if not np.all((bits == 0) | (bits == 1)):
        raise ValueError("bits must be zeros and ones")
    n = bits.shape[1]
    index = bits.astype(np.int64) @ (1 << np.arange(n - 1, -1, -1, dtype=np.int64))
    return np.bincount(index, minlength=2 ** n) / bits.shape[0]
