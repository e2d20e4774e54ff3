"""Krylov methods on a Pauli sum ``H = sum_t c_t P_t`` held as a term list: Lanczos, a restarted Lanczos ground-state
solver and a Krylov (Lanczos-exponential) time evolution with step-size control.

Everything that touches a register is a pass of the library: ``H v`` by ``qsv_apply_pauli_sum``, the projections by
``DeviceState.inner_many``, the updates and the Ritz / evolved vectors by ``DeviceState.lincomb``.  The host only sees the
``k x k`` tridiagonal matrix.

Memory: a run holds ``m + 2`` registers of the state's size -- the ``m`` basis vectors, the work vector and the state
itself (n = 28, m = 20: 22 x 4 GiB = 88 GiB).  A two-pass variant that does not store the basis, thick restarts, excited
states and sharded registers are out of scope.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .device import DensityState, DeviceState, _check_terms, _dbl, _flat_terms, _real_terms

BREAKDOWN = 1e-12          # beta_j <= BREAKDOWN * sum|c_t|: the Krylov space is invariant
TAU_UNDERFLOW = 1e-12      # evolve_krylov gives up when a substep falls below this fraction of |t|


class _Counter:
    """H applications and kernel launches of a run."""

    def __init__(self):
        self.applications = 0
        self.passes = 0


def _prepare(terms, register: DeviceState, what: str):
    if isinstance(register, DensityState):
        raise ValueError(f"{what} is not defined for a density register")
    terms = _real_terms(terms, what)
    _check_terms(terms, register.num_qubits)
    return terms, float(sum(abs(c) for c, _, _ in terms))


def _apply(flat, src: DeviceState, dst: DeviceState, count: _Counter) -> None:
    """dst = H src (qsv_apply_pauli_sum), counted."""
    n_terms, offsets, qubits, letters, cbuf = flat
    passes = C.c_uint64()
    _lib.call("qsv_apply_pauli_sum", dst._h, src._h, n_terms, offsets, qubits, letters, _dbl(cbuf), 0, C.byref(passes))
    count.applications += 1
    count.passes += passes.value


def _close(registers) -> None:
    for register in registers:
        register.close()


def _lanczos(terms, scale: float, start: DeviceState, m: int, reorthogonalise: bool, count: _Counter):
    """``lanczos`` on checked terms; also returns ``||start||``."""
    if m < 1:
        raise ValueError("the Krylov dimension m must be at least 1")
    flat = _flat_terms(terms)
    n, device = start.num_qubits, start.device
    alphas, betas, basis, breakdown = [], [], [], False
    w = None
    try:
        v0 = DeviceState.zeros(n, device)
        basis.append(v0)
        norm2, passes = v0._lincomb([1.0], [start], 0.0, True)          # the copy and ||start||^2 in one pass
        count.passes += passes
        if not norm2 > 0.0:
            raise ValueError("the start vector has no norm")
        norm = float(np.sqrt(norm2))
        v0.apply_scale(1.0 / norm)
        count.passes += 1
        for j in range(m):
            if w is None:
                w = DeviceState.zeros(n, device)
            _apply(flat, basis[j], w, count)
            if reorthogonalise:
                # two rounds of classical Gram-Schmidt against the whole basis; v_j's coefficients add up to alpha_j
                alpha = 0.0
                for _ in range(2):
                    h, passes = w._inner_many(basis)
                    count.passes += passes
                    beta2, passes = w._lincomb(-h, basis, 1.0, True)
                    count.passes += passes
                    alpha += h[j].real
            else:
                h, passes = w._inner_many([basis[j]])
                count.passes += passes
                alpha = h[0].real
                sources, coeffs = [basis[j]], [-alpha]
                if j > 0:
                    sources.append(basis[j - 1])
                    coeffs.append(-betas[j - 1])
                beta2, passes = w._lincomb(coeffs, sources, 1.0, True)
                count.passes += passes
            beta = float(np.sqrt(max(beta2, 0.0)))
            alphas.append(float(alpha))
            betas.append(beta)
            if beta <= BREAKDOWN * scale:
                breakdown = True
                break
            if j + 1 < m:
                w.apply_scale(1.0 / beta)
                count.passes += 1
                basis.append(w)
                w = None
    except BaseException:
        _close(basis)
        raise
    finally:
        if w is not None:
            w.close()
    return np.array(alphas), np.array(betas), basis, breakdown, norm


def lanczos(terms, start: DeviceState, m: int, *, reorthogonalise: bool = True):
    """``m`` Lanczos steps on ``H = sum_t c_t P_t`` (``terms`` as for ``expect_pauli_sum``, real coefficients) from the
    register ``start``, which is not changed.  Returns ``(alphas, betas, basis, breakdown)``: the diagonal
    ``alphas[0..k-1]`` and the off-diagonal ``betas[0..k-2]`` of the tridiagonal ``T_k = V^H H V``, ``betas[k-1]`` the
    norm of the last residual (``H V = V T_k + betas[k-1] v_k e_k^T``), and the ``k <= m`` orthonormal basis vectors as
    ``DeviceState`` registers the caller closes.  Step ``j`` is ``w = H v_j`` followed, with ``reorthogonalise`` (the
    default), by two rounds of classical Gram-Schmidt against the whole basis (``inner_many``, then ``lincomb``), or
    without it by the three-term recurrence (one ``inner_many``, one ``lincomb``); ``beta_j`` comes out of the last
    ``lincomb`` of the step.  ``breakdown`` is set, and the run stops with ``k < m`` or ``k = m`` vectors, when
    ``beta_j <= 1e-12 sum|c_t|``: the Krylov space is invariant under ``H``.

    Memory: up to ``m + 1`` registers of ``start``'s size next to ``start`` itself."""
    terms, scale = _prepare(terms, start, "lanczos")
    return _lanczos(terms, scale, start, int(m), bool(reorthogonalise), _Counter())[:4]


def _tridiagonal(alphas, betas) -> np.ndarray:
    k = len(alphas)
    return np.diag(alphas) + np.diag(betas[:k - 1], 1) + np.diag(betas[:k - 1], -1)


def ground_state(terms, start_or_n_qubits, *, m: int = 30, tol: float = 1e-10, max_restarts: int = 50, seed: int = 0,
                 device: int = 0):
    """Lowest eigenpair of ``H = sum_t c_t P_t`` by restarted Lanczos.  A cycle builds ``T_k`` (``k <= m``, full
    reorthogonalisation), diagonalises it on the host and assembles the lowest Ritz vector with ``lincomb`` over the basis
    in ``ceil(k / 8)`` passes; it stops when the residual estimate ``beta_k |y_k|`` is at most ``tol sum|c_t|`` or the
    Krylov space is invariant, and otherwise restarts from the Ritz vector.  ``start_or_n_qubits``: a register (not
    changed), or a number of qubits for a random ket from ``DeviceState.random(n, seed)``.

    Returns ``(energy, state, info)``; ``state`` is a new register the caller closes, ``info`` has ``restarts``,
    ``residual``, ``ritz_values`` (of the last cycle), ``applications`` (of ``H``), ``passes`` (kernel launches) and
    ``breakdown``.  ``RuntimeError`` when ``max_restarts`` restarts did not converge.

    Memory: ``m + 2`` registers of the state's size (n = 28, m = 20: 88 GiB)."""
    if isinstance(start_or_n_qubits, DeviceState):
        terms, scale = _prepare(terms, start_or_n_qubits, "ground_state")
        state = start_or_n_qubits.copy()
    else:
        state = DeviceState.random(int(start_or_n_qubits), int(seed), int(device))
    count = _Counter()
    try:
        terms, scale = _prepare(terms, state, "ground_state")
        for restarts in range(int(max_restarts) + 1):
            alphas, betas, basis, breakdown, _ = _lanczos(terms, scale, state, int(m), True, count)
            try:
                ritz, vectors = np.linalg.eigh(_tridiagonal(alphas, betas))
                y = vectors[:, 0]
                residual = float(betas[-1] * abs(y[-1]))
                count.passes += state._lincomb(y, basis, 0.0)[1]
            finally:
                _close(basis)
            if breakdown or residual <= tol * scale:
                info = {"restarts": restarts, "residual": residual, "ritz_values": ritz, "applications": count.applications,
                        "passes": count.passes, "breakdown": breakdown}
                return float(ritz[0]), state, info
        raise RuntimeError(f"ground_state: residual estimate {residual:.3e} above {tol * scale:.3e} after {max_restarts} restarts")
    except BaseException:
        state.close()
        raise


def evolve_krylov(state: DeviceState, terms, t: float, *, m: int = 20, tol: float = 1e-10) -> dict:
    """In place ``state <- exp(-i t H) state`` for ``H = sum_t c_t P_t`` (real coefficients), without Trotter error.  Per
    substep, with ``r`` the time that remains: Lanczos from the current state (its norm is kept), ``T_k = Y diag(w) Y^T``
    on the host, the error estimate ``err(tau) = beta_k |sum_i Y[k-1, i] exp(-i tau w_i) Y[0, i]|``, and ``tau = r``
    halved until ``err(tau) <= tol tau / |t|`` (``tau = r`` at once when the Krylov space is invariant); the new state is
    ``norm sum_j c_j v_j`` with ``c = Y exp(-i tau w) Y[0]``, formed by ``lincomb``.  A negative ``t`` runs backwards.

    Returns ``info`` with ``substeps``, ``error_estimate`` (the summed estimates: a bound of the order of ``tol`` on the
    error relative to the state's norm), ``applications`` and ``passes``.  ``RuntimeError`` when a substep falls below
    ``1e-12 |t|``.

    Memory: ``m + 2`` registers of the state's size (n = 28, m = 20: 88 GiB)."""
    terms, scale = _prepare(terms, state, "evolve_krylov")
    t = float(t)
    count = _Counter()
    remaining, substeps, estimate = t, 0, 0.0
    while remaining != 0.0:
        alphas, betas, basis, breakdown, norm = _lanczos(terms, scale, state, int(m), True, count)
        try:
            w, Y = np.linalg.eigh(_tridiagonal(alphas, betas))

            def err(tau):
                return float(betas[-1] * abs(np.sum(Y[-1] * np.exp(-1j * tau * w) * Y[0])))
            tau = remaining
            if not breakdown:
                while err(tau) > tol * abs(tau) / abs(t):
                    tau *= 0.5
                    if abs(tau) < TAU_UNDERFLOW * abs(t):
                        raise RuntimeError("evolve_krylov: the substep underflowed; raise m or tol")
                estimate += err(tau)
            coeffs = norm * (Y @ (np.exp(-1j * tau * w) * Y[0]))
            count.passes += state._lincomb(coeffs, basis, 0.0)[1]
        finally:
            _close(basis)
        remaining -= tau
        substeps += 1
    return {"substeps": substeps, "error_estimate": estimate, "applications": count.applications, "passes": count.passes}
