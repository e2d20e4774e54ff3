"""Layered variational circuits: walls of one-parameter rotations between fixed gates, with the energy of a Pauli sum
and its gradient in every parameter by one adjoint walk.

A rotation wall is one product layer forward (``DeviceState.apply_layer``) and one ``DeviceState.layer_adjoint`` on the
way back, which returns the transition matrices of all its qubits in the layer's own passes; a fixed block is undone on
both registers by the conjugate transposes of its gates in reverse order.
"""
from __future__ import annotations

import numpy as np

from . import layers
from .device import DeviceState, _check_terms, _ket_operand, _real_terms

CZ = np.diag([1.0, 1.0, 1.0, -1.0]).astype(np.complex128)


def cz_line(n_qubits: int) -> list[tuple]:
    """``CZ`` on ``(0, 1), (1, 2), ... (n - 2, n - 1)`` as a gate list for ``Ansatz.fixed``."""
    return [(CZ, [q, q + 1]) for q in range(int(n_qubits) - 1)]


def cz_ring(n_qubits: int) -> list[tuple]:
    """``cz_line`` closed by ``CZ`` on ``(n - 1, 0)`` (three qubits or more)."""
    n = int(n_qubits)
    return cz_line(n) + ([(CZ, [n - 1, 0])] if n > 2 else [])


class Ansatz:
    """A circuit on ``num_qubits`` qubits made of blocks, first added first applied.  The builders return ``self``."""

    def __init__(self, num_qubits: int):
        self.num_qubits = int(num_qubits)
        if self.num_qubits < 1:
            raise ValueError("at least one qubit")
        self.blocks: list[tuple] = []       # ("rotation", kind, qubits) or ("fixed", [(matrix, qubits), ...])

    def _qubits(self, qubits) -> list[int]:
        qubits = list(range(self.num_qubits)) if qubits is None else [int(q) for q in qubits]
        if any(not 0 <= q < self.num_qubits for q in qubits):
            raise ValueError(f"qubit index out of range for a {self.num_qubits}-qubit register")
        if len(set(qubits)) != len(qubits):
            raise ValueError("Indices must be distinct.")
        return qubits

    def rotation_layer(self, kind: str, qubits=None) -> "Ansatz":
        """``exp(-i theta_q / 2 P)`` on each of ``qubits`` (``None``: all), ``kind`` in ``rx`` / ``ry`` / ``rz``: one
        parameter per listed qubit, in the order of the list."""
        layers.generator(kind)          # refuses an unknown kind
        self.blocks.append(("rotation", kind, self._qubits(qubits)))
        return self

    def fixed(self, gates) -> "Ansatz":
        """One- and two-qubit gates without parameters, ``[(matrix, qubits), ...]``, applied through ``apply_matrix`` in
        order.  The matrices must be unitary for the walk back to restore the register."""
        block = []
        for matrix, qubits in gates:
            qubits = self._qubits(qubits)
            matrix = np.asarray(matrix, dtype=np.complex128)
            if len(qubits) not in (1, 2) or matrix.shape != (1 << len(qubits),) * 2:
                raise ValueError("a fixed gate is a 2x2 or 4x4 matrix on one or two qubits")
            block.append((matrix, qubits))
        self.blocks.append(("fixed", block))
        return self

    @property
    def num_parameters(self) -> int:
        return sum(len(block[2]) for block in self.blocks if block[0] == "rotation")

    def _params(self, params) -> np.ndarray:
        params = np.asarray(params, dtype=np.float64).reshape(-1)
        if params.size != self.num_parameters:
            raise ValueError(f"the circuit has {self.num_parameters} parameters, not {params.size}")
        return params

    def rotations(self, params) -> list[tuple]:
        """The circuit as a Pauli-rotation list for ``apply_pauli_rotations`` / ``DeviceState.energy_and_gradient``, the
        parameters' rotations in parameter order and ``CZ`` spelled, up to a global phase, as the rotations
        ``(pi/2, Z, a), (pi/2, Z, b), (-pi/2, ZZ, ab)``; any other fixed gate is refused.  ``parameter_positions`` says
        where the parameters sit in the list."""
        params, out, first = self._params(params), [], 0
        letter = {"rx": "X", "ry": "Y", "rz": "Z"}
        for block in self.blocks:
            if block[0] == "rotation":
                _, kind, qubits = block
                out += [(float(params[first + j]), letter[kind], [q]) for j, q in enumerate(qubits)]
                first += len(qubits)
            else:
                for matrix, qubits in block[1]:
                    if matrix.shape != (4, 4) or not np.array_equal(matrix, CZ):
                        raise ValueError("only CZ has a rotation spelling here")
                    a, b = qubits
                    out += [(0.5 * np.pi, "Z", [a]), (0.5 * np.pi, "Z", [b]), (-0.5 * np.pi, "ZZ", [a, b])]
        return out

    def parameter_positions(self) -> list[int]:
        """``positions[p]`` = the place of parameter ``p`` in ``rotations(params)``."""
        positions, at = [], 0
        for block in self.blocks:
            if block[0] == "rotation":
                positions += list(range(at, at + len(block[2])))
                at += len(block[2])
            else:
                at += 3 * len(block[1])
        return positions

    def num_gates(self) -> int:
        """Gates of the circuit: one per rotation and one per fixed gate."""
        return sum(len(block[2]) if block[0] == "rotation" else len(block[1]) for block in self.blocks)

    def run(self, params, state: DeviceState | None = None) -> DeviceState:
        """The circuit on ``state`` in place (``|0...0>`` when None).  Returns the register."""
        params = self._params(params)
        if state is None:
            state = DeviceState.zeros(self.num_qubits)
        if state.num_qubits != self.num_qubits:
            raise ValueError(f"the circuit acts on {self.num_qubits} qubits, the register has {state.num_qubits}")
        first = 0
        for block in self.blocks:
            if block[0] == "rotation":
                _, kind, qubits = block
                state.apply_layer(layers.rotation(kind, params[first:first + len(qubits)]), qubits)
                first += len(qubits)
            else:
                for matrix, qubits in block[1]:
                    state.apply_matrix(matrix, qubits)
        return state

    def energy_and_gradient(self, params, terms, state: DeviceState | None = None) -> tuple[float, np.ndarray]:
        """``(E, dE/dparams)`` of ``E = <psi|H|psi>``, ``psi`` = the circuit on ``state`` (``|0...0>`` when None) and
        ``H = sum_t c_t P_t`` with real coefficients: the circuit forward, ``E`` from ``expect_pauli_sum``,
        ``lambda = H psi`` from ``apply_pauli_sum``, then the blocks last first -- ``layer_adjoint`` for a rotation wall
        (its transition matrices contracted with the wall's generator), the inverse gates on both registers for a fixed
        block.  ``state`` holds its input again on return, up to rounding."""
        params = self._params(params)
        terms = _real_terms(terms, "the gradient")
        _check_terms(terms, self.num_qubits)
        own = state is None
        if not own:      # refused before the register is touched
            _ket_operand(state, "state")
            if state.num_qubits != self.num_qubits:
                raise ValueError(f"the circuit acts on {self.num_qubits} qubits, the register has {state.num_qubits}")
        psi = DeviceState.zeros(self.num_qubits) if own else state
        lam = None
        try:
            lam = DeviceState.zeros(self.num_qubits, psi.device)
            self.run(params, psi)
            energy = psi.expect_pauli_sum(terms).real
            psi.apply_pauli_sum(terms, out=lam)
            grad = np.zeros(self.num_parameters)
            last = self.num_parameters
            for block in reversed(self.blocks):
                if block[0] == "rotation":
                    _, kind, qubits = block
                    first = last - len(qubits)
                    T = psi.layer_adjoint(layers.rotation(kind, params[first:last]), lam, qubits)
                    grad[first:last] = layers.gradient(T, layers.generator(kind))
                    last = first
                else:
                    for matrix, qubits in reversed(block[1]):
                        inverse = matrix.conj().T
                        psi.apply_matrix(inverse, qubits)
                        lam.apply_matrix(inverse, qubits)
        finally:
            if lam is not None:
                lam.close()
            if own:
                psi.close()
        return float(energy), grad

    def minimise(self, terms, x0, **scipy_options):
        """Minimise ``<H>`` over the parameters with L-BFGS-B on ``energy_and_gradient`` from ``|0...0>``; keyword
        options go to ``scipy.optimize.minimize``.  Returns ``(params, energy, result)``."""
        from scipy.optimize import minimize

        x0 = self._params(x0)

        def objective(x):      # a fresh |0...0> per evaluation: rounding of the rewound register does not pile up
            return self.energy_and_gradient(x, terms)

        result = minimize(objective, x0, jac=True, method="L-BFGS-B", **scipy_options)
        return np.asarray(result.x), float(result.fun), result
