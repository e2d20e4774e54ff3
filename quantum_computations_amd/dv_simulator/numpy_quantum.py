"""Host-side constants and small linear algebra of the qubit simulator (the ``npq`` namespace).

Keeps the public names, argument meaning and error classes of ``simulators/dv_simulator/numpy_quantum.py`` so code
written against ``npq.*`` runs unchanged.  Everything here is O(small) host work: gate matrices, single-qubit states,
fidelities of kets that have already been downloaded.  The O(2^N) work the reference does in this module for
``Gate.apply`` -- ``expand_gate`` / ``permute_tensor_product`` / ``tensor`` (``numpy_quantum.py:169-170,212-247``) -- is
what the HIP kernels replace; the functions of those names below exist for small-N API compatibility only and are never
on the device path.
"""
from __future__ import annotations

import functools

import numpy as np

_INV_SQRT2 = 1.0 / np.sqrt(2)


def _ket(*amplitudes):
    return np.array(amplitudes)


# ---- single-qubit kets (dtypes as in the reference: integer computational states, float / complex superpositions)
ZERO, ONE = _ket(1, 0), _ket(0, 1)
PLUS, MINUS = _ket(1, 1) / np.sqrt(2), _ket(1, -1) / np.sqrt(2)
IPLUS, IMINUS = _ket(1, 1j) / np.sqrt(2), _ket(1, -1j) / np.sqrt(2)

# ---- gate matrices ----------------------------------------------------------------------------------------------
IDTY = np.eye(2)
X = np.array([[0, 1], [1, 0]])
Y = np.array([[0, -1j], [1j, 0]])
Z = np.array([[1, 0], [0, -1]])
PAULIS = [X, Y, Z]
H = np.array([[1, 1], [1, -1]]) / np.sqrt(2)
CZ = np.diag([1.0, 1.0, 1.0, -1.0])
CX = np.eye(4)[[0, 1, 3, 2]]            # first index controls, second is the target (gates.py:116-126)
SWAP = np.eye(4)[[0, 2, 1, 3]]
P = np.diag([1.0, 1.0j])
T = np.diag([1.0, np.exp(0.25j * np.pi)])


# ---- Pauli bookkeeping --------------------------------------------------------------------------------------------
class PauliError(ValueError):
    """The identifier is not one of I, +-X, +-Y, +-Z (letter, signed number or unit axis)."""


_LETTERS = "ixyz"
_AXES = {(1, 0, 0): 1, (0, 1, 0): 2, (0, 0, 1): 3}


def get_pauli_number(pauli_identifier) -> int:
    """0 for I, +-1 / +-2 / +-3 for +-X / +-Y / +-Z."""
    ident = pauli_identifier
    if isinstance(ident, str) and 1 <= len(ident) <= 2:
        negative, letter = ident[:-1] == "-", ident[-1].lower()
        if letter in _LETTERS and ident[:-1] in ("", "-") and not (negative and letter == "i"):
            return (-1 if negative else 1) * _LETTERS.index(letter)
    elif isinstance(ident, (int, np.integer)) and not isinstance(ident, bool) and abs(int(ident)) <= 3:
        return int(ident)
    elif isinstance(ident, (list, tuple)) and len(ident) == 3:
        flipped = tuple(-c for c in ident)
        if tuple(ident) in _AXES:
            return _AXES[tuple(ident)]
        if flipped in _AXES:
            return -_AXES[flipped]
    raise PauliError(f'"{pauli_identifier}" could not be interpreted as a Pauli operator')


def get_pauli_identifier(pauli_identifier) -> str:
    number = get_pauli_number(pauli_identifier)
    return ("-" if number < 0 else "") + _LETTERS[abs(number)].upper()


def is_pauli(case) -> bool:
    try:
        get_pauli_number(case)
    except PauliError:
        return False
    return True


def get_pauli_operator(pauli_identifier) -> np.ndarray:
    return PAULIS[get_pauli_number(pauli_identifier) - 1]


def get_pauli_states(pauli_identifier):
    eigenbases = ([PLUS, MINUS], [IPLUS, IMINUS], [ZERO, ONE])
    return eigenbases[get_pauli_number(pauli_identifier) - 1]


def get_pauli_state(pauli_identifier, state_index: int) -> np.ndarray:
    return get_pauli_states(pauli_identifier)[state_index]


# ---- states -------------------------------------------------------------------------------------------------------
def basis_state(identifier, N: int = None) -> np.ndarray:
    """Computational basis ket from an index, a bit string or a bit sequence.

    (The reference's list / tuple branch forgets to pass ``N`` on, ``numpy_quantum.py:79``; here a bit sequence gives
    what the equivalent bit string gives.)
    """
    if isinstance(identifier, (list, tuple)):
        identifier = "".join(str(bit) for bit in identifier)
    if isinstance(identifier, str):
        identifier, N = int(identifier, 2), len(identifier)
    if not isinstance(identifier, (int, np.integer)):
        raise NotImplementedError(f"Could not generate basis state from identifier of type {type(identifier)}")
    ket = np.zeros(1 << N)
    ket[identifier] = 1
    return ket


def qubit_from_polar(theta: float, phi: float):
    return np.cos(theta / 2) * ZERO + np.exp(1j * phi) * np.sin(theta / 2) * ONE


def qubit_from_axis(axis) -> np.ndarray:
    length = np.sqrt(sum(component ** 2 for component in axis))
    return qubit_from_polar(np.arccos(axis[-1] / length), np.arctan2(axis[1], axis[0]))


def rand_ket(d=2) -> np.ndarray:
    return normalise(np.random.rand(d) + 1j * np.random.rand(d))


# ---- rotations ----------------------------------------------------------------------------------------------------
def phase_gate(theta: float) -> np.ndarray:
    return np.array([[1, 0], [0, np.exp(1j * theta)]])


def axis_rotation(theta: float, axis) -> np.ndarray:
    """``exp(-i theta/2 (a . sigma))`` for a unit axis ``a``."""
    a_dot_sigma = axis[0] * X + axis[1] * Y + axis[2] * Z
    return IDTY * np.cos(theta / 2) - 1j * a_dot_sigma * np.sin(theta / 2)


def euler_rotation(theta1, theta2, theta3) -> np.ndarray:
    x_axis, z_axis = [1, 0, 0], [0, 0, 1]
    return axis_rotation(theta3, x_axis) @ axis_rotation(theta2, z_axis) @ axis_rotation(theta1, x_axis)


# ---- kets, density matrices, overlaps -----------------------------------------------------------------------------
def dagger(array: np.ndarray) -> np.ndarray:
    return array.conj().T


def ket2dm(ket: np.ndarray) -> np.ndarray:
    if ket.ndim != 1:
        raise TypeError("state is not a ket")
    return np.multiply.outer(ket, ket.conj())


def is_hermitian(oper: np.ndarray) -> bool:
    return np.allclose(oper, dagger(oper))


def norm(ket: np.ndarray) -> float:
    return np.linalg.norm(ket)


def normalise(state: np.ndarray) -> np.ndarray:
    if state.ndim not in (1, 2):
        raise ValueError("State not ket nor density matrix.")
    return state / (np.linalg.norm(state) if state.ndim == 1 else np.trace(state))


def dm2ket(dm: np.ndarray, strict: bool = True) -> np.ndarray:
    """Dominant eigenvector of a density matrix; ``strict`` demands that it is the only one with weight."""
    if not is_hermitian(dm):
        raise TypeError("input is not a density matrix")
    weights, vectors = np.linalg.eigh(dm)
    if strict and not np.allclose(weights[:-1], 0):
        raise TypeError("density matrix does not represent a pure state")
    return normalise(vectors[:, -1])


def compare_kets(a: np.ndarray, b: np.ndarray) -> bool:
    return np.allclose(ket2dm(normalise(a)), ket2dm(normalise(b)))


def fidelity(a, b) -> float:
    """Fidelity between any mix of kets and (hermitian) density matrices (numpy_quantum.py:148-161).  Host arrays
    as in the reference; registers in HBM (``DeviceState`` kets, ``DensityState`` matrices) are reduced on the device
    -- ket/ket by one pass over both, ket/matrix by one pass over the matrix -- and never downloaded.  Two device
    density matrices need the spectrum of ``a @ b`` and go through the host (they are 4^n numbers: small n only)."""
    from ..device import DensityState, DeviceState
    if isinstance(a, DeviceState) or isinstance(b, DeviceState):
        if not (isinstance(a, DeviceState) and isinstance(b, DeviceState)):
            def lift(x, like):
                if isinstance(x, DeviceState):
                    return x
                x = np.asarray(x)
                return (DeviceState if x.ndim == 1 else DensityState).from_numpy(x, like.device)
            a, b = lift(a, b if isinstance(b, DeviceState) else a), lift(b, a if isinstance(a, DeviceState) else b)
        kinds = (a.ndim, b.ndim)
        if kinds == (1, 1):
            return abs(a.inner(b)) ** 2
        if kinds == (1, 2):
            return a.expect_density(b).real
        if kinds == (2, 1):
            return b.expect_density(a).real
        a, b = a.to_numpy(), b.to_numpy()
    kinds = (a.ndim, b.ndim)
    if kinds == (1, 1):
        return np.abs(np.vdot(a, b)).real ** 2
    if kinds == (1, 2):
        return np.vdot(a, b @ a).real
    if kinds == (2, 1):
        return np.vdot(b, a @ b).real
    spectrum = np.linalg.eigvals(a @ b).real.clip(min=0.0)        # (tr sqrt(a b))^2
    return np.sqrt(spectrum).sum() ** 2


def _kept_first(state: np.ndarray, qubits) -> np.ndarray:
    """A host ket as the ``(2^k, 2^(n-k))`` matrix whose row index is the setting of ``qubits`` (``qubits[0]`` the most
    significant bit) and whose column index is the setting of every other qubit."""
    state = np.asarray(state)
    n = state.shape[0].bit_length() - 1
    qubits = [int(q) for q in qubits]
    if state.ndim != 1 or state.shape[0] != 1 << n:
        raise ValueError("State has wrong dimensions.")
    if not qubits or len(set(qubits)) != len(qubits) or any(not 0 <= q < n for q in qubits):
        raise ValueError("Indices must be distinct qubits of the register.")
    rest = [q for q in range(n) if q not in qubits]
    return state.reshape((2,) * n).transpose(qubits + rest).reshape(1 << len(qubits), -1)


def reduced_density(state, qubits):
    """The reduced density matrix of ``qubits``, every other qubit traced out; ``qubits[0]`` is the most significant bit
    of both indices.  A host ket gives a host matrix (``M M^dagger``); a ``DeviceState`` gives a ``DensityState`` on its
    device (at most 12 qubits, ``DeviceState.reduced_density_state``) -- the split ``fidelity`` has."""
    from ..device import DeviceState
    if isinstance(state, DeviceState):
        return state.reduced_density_state(qubits)
    m = _kept_first(state, qubits)
    return m @ m.conj().T


def one_qubit_densities(state, qubits=None) -> np.ndarray:
    """The one-qubit reduced density matrix of each of ``qubits`` (``None``: every qubit, in order) as one ``[k, 2, 2]``
    array: ``rho_q[b][a] = sum_rest conj(state[a, rest]) state[b, rest]``, nothing divided by the norm.  A host ket is
    contracted on the host; a ``DeviceState`` goes to ``DeviceState.one_qubit_densities`` (all of them in the passes of one
    product layer)."""
    from ..device import DeviceState
    if isinstance(state, DeviceState):
        return state.one_qubit_densities(qubits)
    ket = np.asarray(state, dtype=np.complex128).reshape(-1)
    n = ket.size.bit_length() - 1
    qubits = list(range(n)) if qubits is None else [int(q) for q in qubits]
    out = np.zeros((len(qubits), 2, 2), dtype=np.complex128)
    for j, q in enumerate(qubits):
        if not 0 <= q < n:
            raise ValueError(f"qubit index out of range for a {n}-qubit register")
        m = ket.reshape(1 << q, 2, -1)
        out[j] = np.einsum("xby,xay->ba", m, m.conj())
    return out


def marginal_probabilities(state, qubits) -> np.ndarray:
    """Probabilities of the ``2^k`` outcomes of ``qubits`` with every other qubit summed over (host ket or
    ``DeviceState``)."""
    from ..device import DeviceState
    if isinstance(state, DeviceState):
        return state.marginal_probabilities(qubits)
    m = _kept_first(state, qubits)
    return np.sum(m.real ** 2 + m.imag ** 2, axis=1)


def entanglement_entropy(state, qubits, alpha: float = 1.0, base: float = np.e) -> float:
    """Entanglement entropy of the cut ``qubits | rest`` of a pure state: von Neumann for ``alpha = 1``, else Renyi.  A
    host ket goes through the singular values of the reshaped ket; a ``DeviceState`` through its reduced state."""
    from ..device import DeviceState
    from ..entanglement import entropy_of
    if isinstance(state, DeviceState):
        return state.entanglement_entropy(qubits, alpha, base)
    return entropy_of(np.linalg.svd(_kept_first(state, qubits), compute_uv=False) ** 2, alpha, base)


def purity(rho) -> float:
    """``tr(rho rho)`` of a hermitian density matrix (numpy_quantum.py:164-166); a ``DensityState`` is reduced on
    the device."""
    if hasattr(rho, "purity"):
        return rho.purity()
    return np.trace(rho @ rho).real


def expect(oper: np.ndarray, state: np.ndarray):
    if not (is_qubit_operator(oper) and is_qubit_state(state) and oper.shape[0] == state.shape[0]):
        raise TypeError("incompatible operator and state vector")
    return np.vdot(state, oper @ state)


def expecth(oper: np.ndarray, state: np.ndarray):
    return expect(oper, state).real


class PauliSum:
    """``H = sum_t c_t P_t`` on ``n_qubits`` qubits; ``terms`` is a list of ``(coefficient, letters, qubits)`` with one
    letter of I / X / Y / Z per listed qubit (qubit 0 is the leftmost factor, as everywhere in ``npq``)."""

    def __init__(self, n_qubits: int, terms=()):
        self.n_qubits = int(n_qubits)
        self.terms = []
        for coefficient, letters, qubits in terms:
            letters, qubits = str(letters), [int(q) for q in qubits]
            if len(letters) != len(qubits):
                raise ValueError("one Pauli letter per qubit")
            if len(set(qubits)) != len(qubits):
                raise ValueError("Indices must be distinct.")
            if any(q < 0 or q >= self.n_qubits for q in qubits):
                raise ValueError(f"qubit index out of range for a {self.n_qubits}-qubit register")
            if any(not is_pauli(letter) for letter in letters):
                raise PauliError("Pauli letters must be I, X, Y or Z")
            self.terms.append((complex(coefficient), letters, qubits))

    def __add__(self, other: "PauliSum") -> "PauliSum":
        if not isinstance(other, PauliSum):
            return NotImplemented
        if other.n_qubits != self.n_qubits:
            raise ValueError("Pauli sums on registers of different sizes")
        return PauliSum(self.n_qubits, self.terms + other.terms)

    def __mul__(self, scalar) -> "PauliSum":
        if not np.isscalar(scalar):
            return NotImplemented
        return PauliSum(self.n_qubits, [(scalar * c, letters, qubits) for c, letters, qubits in self.terms])

    __rmul__ = __mul__

    def __len__(self) -> int:
        return len(self.terms)

    def matrix(self) -> np.ndarray:
        """The dense ``2^n x 2^n`` operator, by Kronecker products of ``PAULIS``; small n only."""
        dim = 1 << self.n_qubits
        total = np.zeros((dim, dim), dtype=complex)
        for c, letters, qubits in self.terms:
            factors = [IDTY] * self.n_qubits
            for letter, q in zip(letters, qubits):
                number = get_pauli_number(letter)
                factors[q] = IDTY if number == 0 else PAULIS[number - 1]
            total += c * tensor(*factors)
        return total


def expect_pauli_sum(hamiltonian: PauliSum, state) -> complex:
    """``<state| H |state>`` for a ``PauliSum``, computed on the device in passes shared between the terms that flip
    the same qubits (``DeviceState.expect_pauli_sum``).  A host ket is uploaded first: the product path has no CPU
    fallback (``fidelity`` lifts host arrays the same way)."""
    from ..device import DeviceState
    if not isinstance(state, DeviceState):
        state = DeviceState.from_numpy(np.asarray(state))
    if state.num_qubits != hamiltonian.n_qubits:
        raise TypeError("incompatible operator and state vector")
    return state.expect_pauli_sum(hamiltonian.terms)


def trotter_rotations(hamiltonian: PauliSum, t: float, steps: int = 1, order: int = 1) -> list:
    """The Pauli rotations ``[(theta, letters, qubits), ...]`` of a Trotterised ``exp(-i t H)``, first applied first:
    ``exp(-i c t / steps P) = exp(-i theta/2 P)`` with ``theta = 2 c t / steps``.  Order 1: the terms in ``H.terms``
    order, ``steps`` times.  Order 2: per step a forward sweep with half angles, then the reverse sweep with half
    angles.  What ``DeviceState.apply_pauli_rotations`` takes."""
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps must be at least 1")
    if order not in (1, 2):
        raise ValueError("Trotter order must be 1 or 2")
    if any(c.imag != 0.0 for c, _, _ in hamiltonian.terms):
        raise ValueError("time evolution needs real coefficients (a hermitian Pauli sum)")
    sweep = [(2.0 * c.real * t / steps / order, letters, qubits) for c, letters, qubits in hamiltonian.terms]
    return (sweep if order == 1 else sweep + sweep[::-1]) * steps


def evolve(hamiltonian: PauliSum, state, t: float, steps: int = 1, order: int = 1):
    """Trotterised ``exp(-i t H) state`` on the device (``DeviceState.evolve``).  A register is evolved in place and
    returned; a host ket is uploaded first and the evolved ket is downloaded, as ``expect_pauli_sum`` lifts host arrays."""
    from ..device import DeviceState
    host = not isinstance(state, DeviceState)
    if host:
        state = DeviceState.from_numpy(np.asarray(state))
    if state.num_qubits != hamiltonian.n_qubits:
        raise TypeError("incompatible operator and state vector")
    state.apply_pauli_rotations(trotter_rotations(hamiltonian, t, steps, order))
    return state.to_numpy() if host else state


def _lift(hamiltonian: PauliSum, state):
    """(register, whether ``state`` was a host ket that had to be uploaded); sizes checked as ``expect_pauli_sum`` does.
    The caller closes a register that was uploaded for it once its result is on the host."""
    from ..device import DeviceState
    host = not isinstance(state, DeviceState)
    if host:
        state = DeviceState.from_numpy(np.asarray(state))
    if state.num_qubits != hamiltonian.n_qubits:
        if host:
            state.close()
        raise TypeError("incompatible operator and state vector")
    return state, host


def apply_pauli_sum(hamiltonian: PauliSum, state):
    """``H state`` on the device (``DeviceState.apply_pauli_sum``).  A register gives a new register and is left as it
    is; a host ket is uploaded first and ``H ket`` is downloaded, as ``evolve`` lifts host arrays."""
    state, host = _lift(hamiltonian, state)
    if not host:
        return state.apply_pauli_sum(hamiltonian.terms)
    try:
        out = state.apply_pauli_sum(hamiltonian.terms)
        try:
            return out.to_numpy()
        finally:
            out.close()
    finally:
        state.close()


def transition(hamiltonian: PauliSum, bra, ket) -> complex:
    """``<bra| H |ket>`` on the device (``DeviceState.transition_pauli_sum``); host kets are uploaded first, and their
    registers are released once the value is on the host."""
    uploaded = []
    try:
        bra, host = _lift(hamiltonian, bra)
        if host:
            uploaded.append(bra)
        ket, host = _lift(hamiltonian, ket)
        if host:
            uploaded.append(ket)
        return bra.transition_pauli_sum(hamiltonian.terms, ket)
    finally:
        for register in uploaded:
            register.close()


def energy_and_gradient(hamiltonian: PauliSum, rotations, state):
    """``(E, dE/dtheta)`` of ``E(theta) = <state| U(theta)^dagger H U(theta) |state>`` for the rotation list
    ``[(theta, letters, qubits), ...]`` by the adjoint method (``DeviceState.energy_and_gradient``): the cost of about
    three circuit runs whatever the number of angles.  A register holds its input state again afterwards; a host ket is
    uploaded first and left untouched."""
    state, host = _lift(hamiltonian, state)
    try:
        return state.energy_and_gradient(rotations, hamiltonian.terms)
    finally:
        if host:
            state.close()


def ground_state(hamiltonian: PauliSum, state=None, **options):
    """``(energy, ground state, info)`` of a hermitian ``PauliSum`` by restarted Lanczos on the device
    (``krylov.ground_state``, whose keyword options pass through; ``m + 2`` registers of the state's size).  ``state``:
    the start vector -- None for a random ket (``seed``), a register (left as it is; a new register is returned), or a
    host ket, which is uploaded first, left untouched, and answered with a host ket."""
    from .. import krylov
    if state is None:
        return krylov.ground_state(hamiltonian.terms, hamiltonian.n_qubits, **options)
    state, host = _lift(hamiltonian, state)
    try:
        energy, ground, info = krylov.ground_state(hamiltonian.terms, state, **options)
        if not host:
            return energy, ground, info
        try:
            return energy, ground.to_numpy(), info
        finally:
            ground.close()
    finally:
        if host:
            state.close()


def evolve_exact(hamiltonian: PauliSum, state, t: float, **options):
    """``exp(-i t H) state`` by Krylov evolution on the device, without Trotter error (``krylov.evolve_krylov``, whose
    keyword options pass through; ``m + 2`` registers of the state's size).  A register is evolved in place and returned;
    a host ket is uploaded first, left untouched, and the evolved ket is downloaded, as ``evolve`` lifts host arrays."""
    from .. import krylov
    state, host = _lift(hamiltonian, state)
    if not host:
        krylov.evolve_krylov(state, hamiltonian.terms, t, **options)
        return state
    try:
        krylov.evolve_krylov(state, hamiltonian.terms, t, **options)
        return state.to_numpy()
    finally:
        state.close()


# ---- diagonal operators (``DiagonalOperator``) ---------------------------------------------------
def _term_list(pauli_sum_or_terms) -> list:
    terms = pauli_sum_or_terms.terms if isinstance(pauli_sum_or_terms, PauliSum) else pauli_sum_or_terms
    return [(c, str(letters), [int(q) for q in qubits]) for c, letters, qubits in terms]


def split_diagonal(terms) -> tuple[list, list]:
    """``(z_only_terms, other_terms)`` of a term list or ``PauliSum``, each in the caller's order: the first is what a
    ``DiagonalOperator`` holds, the second what stays a Pauli sum."""
    z_only, other = [], []
    for term in _term_list(terms):
        (z_only if all(letter in "IZiz" for letter in term[1]) else other).append(term)
    return z_only, other


def diagonal_of(pauli_sum_or_terms, n: int) -> np.ndarray:
    """The ``2^n`` float64 values of a Z-only Pauli sum, built on the host: ``c_t * sign`` added term by term in the
    caller's order, the additions ``DiagonalOperator.from_terms`` makes on the device (the two agree bit for bit)."""
    n = int(n)
    index = np.arange(1 << n, dtype=np.uint64)
    values = np.zeros(1 << n, dtype=np.float64)
    for c, letters, qubits in _term_list(pauli_sum_or_terms):
        c = complex(c)
        if c.imag != 0.0:
            raise ValueError("a diagonal operator needs real coefficients")
        if len(letters) != len(qubits):
            raise ValueError("one Pauli letter per qubit")
        if any(letter not in "IZiz" for letter in letters):
            raise ValueError("a diagonal operator takes the letters I and Z only")
        if any(not 0 <= q < n for q in qubits):
            raise ValueError(f"qubit index out of range for a {n}-qubit register")
        if len(set(qubits)) != len(qubits):
            raise ValueError("Indices must be distinct.")
        parity = np.zeros(1 << n, dtype=np.uint64)
        for letter, q in zip(letters, qubits):
            if letter in "Zz":
                parity ^= (index >> np.uint64(n - 1 - q)) & np.uint64(1)
        values += np.where(parity == 1, -c.real, c.real)
    return values


def _lift_diagonal(diag, state):
    """(operator, register, which of the two were uploaded here).  ``diag``: a ``DiagonalOperator`` or a host vector;
    ``state``: a ``DeviceState`` or a host ket.  Sizes are checked as ``expect_pauli_sum`` checks them."""
    from ..device import DeviceState
    from ..diagonal import DiagonalOperator
    uploaded = []
    try:
        if not isinstance(state, DeviceState):
            state = DeviceState.from_numpy(np.asarray(state))
            uploaded.append(state)
        if not isinstance(diag, DiagonalOperator):
            diag = DiagonalOperator.from_numpy(np.asarray(diag), state.device)
            uploaded.append(diag)
        if diag.num_qubits != state.num_qubits:
            raise TypeError("incompatible operator and state vector")
    except Exception:
        for handle in uploaded:
            handle.close()
        raise
    return diag, state, uploaded


def apply_diagonal_phase(diag, state, gamma: float):
    """``exp(-i gamma D) state`` on the device (``DeviceState.apply_diagonal_phase``).  A register is changed in place
    and returned; a host ket is uploaded first and the result is downloaded, as ``evolve`` lifts host arrays."""
    from ..device import DeviceState
    host = not isinstance(state, DeviceState)
    diag, state, uploaded = _lift_diagonal(diag, state)
    try:
        state.apply_diagonal_phase(diag, gamma)
        return state.to_numpy() if host else state
    finally:
        for handle in uploaded:
            handle.close()


def expect_diagonal(diag, state, threshold: float | None = None):
    """``(norm2, mean, second_moment, probability_below)`` of a diagonal operator in ``state``, one read pass on the
    device (``DeviceState.expect_diagonal``); host arrays are uploaded first and released afterwards."""
    diag, state, uploaded = _lift_diagonal(diag, state)
    try:
        return state.expect_diagonal(diag, threshold)
    finally:
        for handle in uploaded:
            handle.close()


# ---- sizes ----------------------------------------------------------------------------------------------------------
def is_power_of_two(n: int) -> bool:
    return n > 0 and n & (n - 1) == 0


def is_qubit_operator(oper: np.ndarray) -> bool:
    return oper.ndim == 2 and oper.shape[0] == oper.shape[1] and is_power_of_two(oper.shape[0])


def is_qubit_state(state: np.ndarray) -> bool:
    return state.ndim == 1 and is_power_of_two(len(state))


def num_qubits(arr) -> int:
    return int(np.log2(arr if isinstance(arr, int) else arr.shape[0]))


# ---- small-N tensor-product helpers (host arrays only; Gate.apply does NOT go through these) ------------------------
def tensor(*arrays) -> np.ndarray:
    """Kronecker product of all arguments, left to right."""
    return functools.reduce(np.kron, arrays, 1)


def permute_tensor_product(array: np.ndarray, new_ordering) -> np.ndarray:
    """Re-order the qubit factors of a ket or operator: the factor at position ``j`` moves to ``new_ordering[j]``."""
    dim = array.shape[0]
    if not is_power_of_two(dim):
        raise ValueError("Given array is not a qubit state nor operator")
    n = num_qubits(array)
    if sorted(new_ordering) != list(range(n)):
        raise ValueError("new_ordering must be a permutation of all qubits")
    came_from = list(np.argsort(new_ordering))

    def shuffle_rows(values):
        return values.reshape((2,) * n + (-1,)).transpose(came_from + [n]).reshape(dim, -1)

    if array.ndim == 1:
        return shuffle_rows(array).ravel()
    return shuffle_rows(shuffle_rows(array).T).T


def expand_gate(gate: np.ndarray, N: int, targets) -> np.ndarray:
    """Dense 2^N x 2^N operator of ``gate`` acting on ``targets`` (identity elsewhere); small N only."""
    targets = list(targets)
    spectators = [q for q in range(N) if q not in targets]
    padded = tensor(gate, *[IDTY for _ in spectators])
    return permute_tensor_product(padded, targets + spectators)


def qft_matrix(m: int, inverse: bool = False, swaps: bool = True) -> np.ndarray:
    """Dense quantum Fourier transform on ``m`` qubits (leg 0 most significant): ``F[y, x] = 2^(-m/2) exp(+2 pi i x y /
    2^m)``, ``numpy.fft.ifft(norm="ortho")`` as a matrix.  ``swaps=False`` leaves the final reversal of the qubits out
    (the rows come out bit-reversed); ``inverse`` is the adjoint of either."""
    dim = 1 << m
    index = np.arange(dim, dtype=np.int64)
    turns = np.multiply.outer(index, index) % dim          # x y mod 2^m, exact
    matrix = np.exp(2j * np.pi * turns / dim) / np.sqrt(dim)
    if not swaps:
        reverse = np.array([int(format(y, f"0{m}b")[::-1], 2) if m else 0 for y in range(dim)])
        matrix = matrix[reverse, :]
    return matrix.conj().T if inverse else matrix


def register_map_matrix(op, n_controls: int = 0, inverse: bool = False) -> np.ndarray:
    """Dense permutation matrix of an ``arithmetic.RegisterMap`` on ``m + mx + n_controls`` qubits, legs in the order
    target, source, controls (each most significant first): column ``(y, x, c)`` holds its 1 in row ``(y', x, c)``, with
    ``y' = y`` unless every control is 1.  Small sizes only (at most 12 qubits)."""
    total = op.m + op.mx + int(n_controls)
    if total > 12:
        raise ValueError("register_map_matrix is for at most 12 qubits")
    values = (op.inverse() if inverse else op).index_map()           # [x, y] -> y'
    dim, all_on = 1 << total, (1 << n_controls) - 1
    matrix = np.zeros((dim, dim))
    for y in range(1 << op.m):
        for x in range(1 << op.mx):
            for c in range(1 << n_controls):
                to = int(values[x, y]) if c == all_on else y
                matrix[((to << op.mx | x) << n_controls) | c, ((y << op.mx | x) << n_controls) | c] = 1.0
    return matrix


def apply_register_map(state, op, target, source=None, controls=(), inverse: bool = False) -> np.ndarray:
    """An ``arithmetic.RegisterMap`` on a host ket or density matrix (a new array; one gather pass on a borrowed device
    register, as ``gates.QFT`` does for host arrays)."""
    from . import gates
    return gates.apply_register_map_on_host(state, op, target, source, controls, inverse)


def add_control(gate: np.ndarray) -> np.ndarray:
    """``|0><0| x I + |1><1| x gate``."""
    dim = gate.shape[0]
    controlled = np.eye(2 * dim, dtype=np.result_type(gate, float))
    controlled[dim:, dim:] = gate
    return controlled
