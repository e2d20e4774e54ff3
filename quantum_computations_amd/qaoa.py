"""QAOA on a ``DiagonalOperator`` cost: layers ``exp(-i beta_l B) exp(-i gamma_l D)`` on
``|+>^n`` with the mixer ``B = sum_q X_q``, the energy ``<D>`` and its gradient in all ``2 p`` angles by one adjoint walk.

The cost layer is one pass over the register whatever ``D`` was built from (``DeviceState.apply_diagonal_phase``); the
mixer is ``RX(2 beta)`` on every qubit through ``apply_matrix``, which the deferred queue batches into shared passes, or
-- ``mixer="layer"`` -- one product layer (``apply_layer``): ``max(1, ceil((n - 6) / 6))`` passes.
"""
from __future__ import annotations

import numpy as np

from . import layers
from .device import DeviceState
from .diagonal import DiagonalOperator

_H = np.array([[1.0, 1.0], [1.0, -1.0]], dtype=complex) / np.sqrt(2.0)


def _angles(gammas, betas) -> tuple[np.ndarray, np.ndarray]:
    gammas = np.atleast_1d(np.asarray(gammas, dtype=np.float64))
    betas = np.atleast_1d(np.asarray(betas, dtype=np.float64))
    if gammas.ndim != 1 or gammas.shape != betas.shape:
        raise ValueError("one gamma and one beta per layer")
    return gammas, betas


def plus_state(n_qubits: int, device: int = 0) -> DeviceState:
    """``|+>^n`` made on the device: H on every qubit of ``|0...0>``."""
    state = DeviceState.zeros(n_qubits, device)
    for q in range(n_qubits):
        state.apply_matrix(_H, [q])
    return state


def _mixer_kind(mixer: str, kinds: tuple) -> str:
    if mixer not in kinds:
        raise ValueError(f"mixer must be one of {kinds}, not {mixer!r}")
    return mixer


def mixer(state: DeviceState, beta: float, mixer: str = "gates") -> DeviceState:
    """In place ``exp(-i beta sum_q X_q) state``: ``RX(2 beta)`` on every qubit -- ``mixer="gates"``: one ``apply_matrix``
    per qubit; ``"layer"``: one ``apply_layer``."""
    if _mixer_kind(mixer, ("gates", "layer")) == "layer":
        return state.apply_layer(layers.rx(2.0 * float(beta)))
    c, s = np.cos(beta), np.sin(beta)
    rx = np.array([[c, -1j * s], [-1j * s, c]], dtype=complex)
    for q in range(state.num_qubits):
        state.apply_matrix(rx, [q])
    return state


_apply_mixer = mixer      # for the functions below, whose ``mixer`` keyword hides the function

def mixer_terms(n_qubits: int) -> list[tuple]:
    """``B = sum_q X_q`` as a Pauli term list."""
    return [(1.0, "X", [q]) for q in range(n_qubits)]


def run(diag: DiagonalOperator, gammas, betas, state: DeviceState | None = None, mixer: str = "gates") -> DeviceState:
    """The QAOA state: for every layer the cost phase ``exp(-i gamma_l D)`` and then the mixer ``exp(-i beta_l B)``, on
    ``state`` in place (``|+>^n`` on the diagonal's device when None).  ``mixer``: as in ``mixer()``.  Returns the register."""
    gammas, betas = _angles(gammas, betas)
    kind = _mixer_kind(mixer, ("gates", "layer"))
    if state is None:
        state = plus_state(diag.num_qubits, diag.device)
    for gamma, beta in zip(gammas, betas):
        state.apply_diagonal_phase(diag, gamma)
        _apply_mixer(state, beta, kind)
    return state


def energy_and_gradient(diag: DiagonalOperator, gammas, betas, state: DeviceState | None = None, mixer: str = "gates",
                        walk: str = "calls"):
    """``(E, dE/dgamma, dE/dbeta)`` of ``E = <psi_p| D |psi_p>`` by one adjoint walk: the layers forward, ``E`` and
    ``lambda = D psi``, then for the last layer first ``dE/dbeta_l = 2 Im <lambda| B |psi>``, the mixer undone on both
    registers, and ``dE/dgamma_l = 2 Im <lambda| D |psi>`` from ``qsv_diag_phase_adjoint``, which undoes the cost phase
    on both in the same pass.  ``state`` (``|+>^n`` when None) holds its input again on return, up to rounding.
    ``mixer``: as in ``mixer()``, for the walk forward and the walk back.  ``walk="fused"`` (needs ``mixer="layer"``) takes
    ``dE/dbeta_l`` and the undone mixer on both registers from one ``layer_adjoint``:
    ``dE/dbeta_l = sum_q 2 Im <lambda|X_q|psi>`` from the transition matrices, ``RX(2 beta)`` having the generator ``-i X``
    in ``beta``; ``walk="calls"`` is the transition sum and the two mixer calls."""
    gammas, betas = _angles(gammas, betas)
    kind = _mixer_kind(mixer, ("gates", "layer"))
    if walk not in ("calls", "fused"):
        raise ValueError(f"walk must be one of ('calls', 'fused'), not {walk!r}")
    if walk == "fused" and kind != "layer":
        raise ValueError('walk="fused" needs mixer="layer"')
    own = state is None
    psi = plus_state(diag.num_qubits, diag.device) if own else state
    lam = DeviceState.zeros(psi.num_qubits, psi.device)
    try:
        run(diag, gammas, betas, psi, kind)
        energy = psi.expect_diagonal(diag).mean
        psi.apply_diagonal_operator(diag, out=lam)
        b_terms = mixer_terms(psi.num_qubits)
        d_gamma, d_beta = np.zeros_like(gammas), np.zeros_like(betas)
        for layer in range(len(gammas) - 1, -1, -1):
            if walk == "fused":
                T = psi.layer_adjoint(layers.rx(2.0 * float(betas[layer])), lam)
                d_beta[layer] = float(np.sum(layers.gradient(T, 2.0 * layers.generator("rx"))))
            else:
                d_beta[layer] = 2.0 * lam.transition_pauli_sum(b_terms, psi).imag
                _apply_mixer(psi, -betas[layer], kind)
                _apply_mixer(lam, -betas[layer], kind)
            d_gamma[layer] = 2.0 * psi.diagonal_phase_adjoint(diag, lam, -gammas[layer]).imag
    finally:
        lam.close()
        if own:
            psi.close()
    return energy, d_gamma, d_beta


def energies(diag: DiagonalOperator, gammas, betas, batch: int = 256, threshold: float | None = None, mixer: str = "rotations"):
    """``<D>`` at ``M`` parameter points, ``gammas[M, p]`` and ``betas[M, p]``, ``batch`` points per register: every point is a
    member of an ``Ensemble``.  Per layer one per-member cost phase, then the mixer as ``n``
    per-member ``X`` rotations of angle ``2 beta_m`` (``mixer="rotations"``) or as one per-member product layer of
    ``layers.rx(2 beta_m)`` on every qubit (``mixer="layer"``).  Returns ``E[M]``; with a ``threshold`` also
    ``P(D <= threshold)[M]``.  Surplus members of the last chunk take angles of zero and are dropped."""
    from . import sweep
    from .ensemble import Ensemble

    gammas = np.atleast_2d(np.asarray(gammas, dtype=np.float64))
    betas = np.atleast_2d(np.asarray(betas, dtype=np.float64))
    if gammas.ndim != 2 or gammas.shape != betas.shape:
        raise ValueError("gammas and betas must both have shape [points, layers]")
    as_layer = _mixer_kind(mixer, ("rotations", "layer")) == "layer"
    points, n_layers = gammas.shape
    n = diag.num_qubits
    plus = np.full(1 << n, 2.0 ** (-0.5 * n), dtype=np.complex128)
    x_rotations = [(0.0, "X", [q]) for q in range(n)]
    energy, below = np.zeros(points), np.zeros(points)
    ens = None
    try:
        for first, count, members in sweep.chunks(points, batch):
            if ens is None or ens.members != members:
                if ens is not None:
                    ens.close()
                ens = Ensemble.from_ket(plus, members, diag.device)
            else:
                ens.reset(plus)
            g, b = np.zeros((members, n_layers)), np.zeros((members, n_layers))
            g[:count], b[:count] = gammas[first:first + count], betas[first:first + count]
            for layer in range(n_layers):
                ens.apply_diagonal_phase(diag, g[:, layer])
                if as_layer:
                    ens.apply_layer(layers.rx(np.repeat(2.0 * b[:, layer, None], n, axis=1)))
                else:
                    ens.apply_pauli_rotations(x_rotations, np.repeat(2.0 * b[:, layer, None], n, axis=1))
            moments = ens.expect_diagonal(diag, threshold)
            energy[first:first + count] = moments.mean[:count]
            below[first:first + count] = moments.probability_below[:count]
    finally:
        if ens is not None:
            ens.close()
    return energy if threshold is None else (energy, below)


def energies_and_gradients(diag: DiagonalOperator, gammas, betas, batch: int = 256):
    """``(E[M], dE/dgamma[M, p], dE/dbeta[M, p])`` at ``M`` parameter points, every point a member of an ``Ensemble`` (DESIGN.md
    section 30): ``energy_and_gradient`` member by member.  Forward as ``energies(mixer="rotations")``; ``E`` from
    ``expect_diagonal`` and ``lambda_m = D psi_m``; then per layer backwards ``dE/dbeta_l[m] = 2 sum_q Im <lambda_m|X_q|psi_m>``
    from one rotation walk over the ``n`` ``X`` rotations of angle ``2 beta_l[m]`` and ``dE/dgamma_l[m] = 2 Im <lambda_m|D|psi_m>``
    from one ``diagonal_phase_adjoint``, which undoes the cost phase on both in the same pass.  Surplus members of the last
    chunk take angles of zero and are dropped."""
    from . import sweep
    from .ensemble import Ensemble

    gammas = np.atleast_2d(np.asarray(gammas, dtype=np.float64))
    betas = np.atleast_2d(np.asarray(betas, dtype=np.float64))
    if gammas.ndim != 2 or gammas.shape != betas.shape:
        raise ValueError("gammas and betas must both have shape [points, layers]")
    points, n_layers = gammas.shape
    n = diag.num_qubits
    plus = np.full(1 << n, 2.0 ** (-0.5 * n), dtype=np.complex128)
    x_rotations = [(0.0, "X", [q]) for q in range(n)]
    energy, d_gamma, d_beta = np.zeros(points), np.zeros((points, n_layers)), np.zeros((points, n_layers))
    ens = lam = None
    try:
        for first, count, members in sweep.chunks(points, batch):
            if ens is None or ens.members != members:      # both ensembles of a chunk before anything is touched
                for old in (ens, lam):
                    if old is not None:
                        old.close()
                ens = lam = None
                ens = Ensemble.from_ket(plus, members, diag.device)
                lam = Ensemble(DeviceState.zeros(n + members.bit_length() - 1, diag.device), n)
            else:
                ens.reset(plus)
            g, b = np.zeros((members, n_layers)), np.zeros((members, n_layers))
            g[:count], b[:count] = gammas[first:first + count], betas[first:first + count]
            for layer in range(n_layers):
                ens.apply_diagonal_phase(diag, g[:, layer])
                ens.apply_pauli_rotations(x_rotations, np.repeat(2.0 * b[:, layer, None], n, axis=1))
            energy[first:first + count] = ens.expect_diagonal(diag).mean[:count]
            ens.apply_diagonal_operator(diag, out=lam)
            for layer in range(n_layers - 1, -1, -1):
                values = ens.pauli_rotations_adjoint(x_rotations, lam, np.repeat(2.0 * b[:, layer, None], n, axis=1))
                d_beta[first:first + count, layer] = 2.0 * values.imag.sum(axis=1)[:count]
                d_gamma[first:first + count, layer] = 2.0 * ens.diagonal_phase_adjoint(diag, lam, -g[:, layer]).imag[:count]
    finally:
        for old in (ens, lam):
            if old is not None:
                old.close()
    return energy, d_gamma, d_beta


def landscape(diag: DiagonalOperator, gamma_grid, beta_grid, batch: int = 256, mixer: str = "rotations") -> np.ndarray:
    """The ``p = 1`` surface ``E[G, B]`` over ``gamma_grid x beta_grid`` through ``energies``."""
    gamma_grid = np.asarray(gamma_grid, dtype=np.float64).reshape(-1)
    beta_grid = np.asarray(beta_grid, dtype=np.float64).reshape(-1)
    g, b = np.meshgrid(gamma_grid, beta_grid, indexing="ij")
    return energies(diag, g.reshape(-1, 1), b.reshape(-1, 1), batch=batch, mixer=mixer).reshape(gamma_grid.size, beta_grid.size)


def minimise(diag: DiagonalOperator, p: int, x0=None, **scipy_options):
    """Minimise ``<D>`` over the ``2 p`` angles ``x = (gammas, betas)`` with L-BFGS-B on ``energy_and_gradient``.
    ``x0``: the starting angles (default: ``gamma_l = 0.1 (l + 1) / p``, ``beta_l = 0.1 (p - l) / p``); keyword options
    go to ``scipy.optimize.minimize``.  Returns ``(angles, energy, result)``, ``angles`` as ``x``."""
    from scipy.optimize import minimize

    p = int(p)
    if p < 1:
        raise ValueError("at least one layer")
    if x0 is None:
        x0 = np.concatenate([0.1 * (np.arange(p) + 1) / p, 0.1 * (p - np.arange(p)) / p])
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1)
    if x0.size != 2 * p:
        raise ValueError("x0 holds p gammas and then p betas")

    def objective(x):      # a fresh |+>^n per evaluation: rounding of the rewound register does not pile up
        energy, d_gamma, d_beta = energy_and_gradient(diag, x[:p], x[p:])
        return energy, np.concatenate([d_gamma, d_beta])

    result = minimize(objective, x0, jac=True, method="L-BFGS-B", **scipy_options)
    return np.asarray(result.x), float(result.fun), result
