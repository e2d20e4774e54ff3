"""Trajectory ensembles: many shots of a noisy circuit in one register.

``members = 2^b`` independent ``n``-qubit kets sit side by side in one ``(n + b)``-qubit :class:`DeviceState`, member ``m`` at the
amplitudes ``[m 2^n, (m + 1) 2^n)``: the member index is the leading ``b`` qubits of the register, member qubit ``q`` is
register qubit ``q + b``.  A unitary on member qubits is one pass over the register for all members, deferred gates included;
what differs from member to member -- the branch a Kraus channel takes, norms, Pauli values -- goes through the
``qsv_ensemble_*`` entry points.  Qubit indices of this class are MEMBER qubits.

Every member also owns 64 classical bits on the device (section 24): ``measure`` projects a qubit of every member, each
with its own draw, and writes the member's outcome to one of them; ``apply_conditional`` applies a gate to the members
whose bits satisfy a condition and leaves the others untouched -- feed-forward without a host round trip.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .device import DeviceState, DiagonalMoments, _check_terms, _diagonal_operand, _flat_terms, _ints, _real_terms


class TrajectoryEnsemble:
    """``members`` kets of ``member_qubits`` qubits in one register (``.state``)."""

    def __init__(self, state: DeviceState, member_qubits: int):
        total = DeviceState.num_qubits.fget(state)
        if not 0 <= int(member_qubits) <= total:
            raise ValueError("member_qubits must lie between 0 and the register's qubits")
        self.state = state
        self.member_qubits = int(member_qubits)
        self.member_bits = total - self.member_qubits
        self.members = 1 << self.member_bits
        self._measured: list[int] = []        # the classical bit of the k-th measurement since reset(): ClassicalControl's indices
        self.last_passes = 0                  # passes of the last apply_pauli_rotations

    @classmethod
    def from_ket(cls, ket, members: int, device: int = 0) -> "TrajectoryEnsemble":
        """Every member a copy of ``ket``; ``members`` is a power of two."""
        ket = np.asarray(ket)
        if ket.ndim != 1:
            raise ValueError("State has wrong dimensions.")
        size = ket.shape[0]
        if size == 0 or size & (size - 1):
            raise ValueError("Given array is not a qubit state nor operator")
        members = int(members)
        if members < 1 or members & (members - 1):
            raise ValueError("the number of members must be a power of two")
        n = size.bit_length() - 1
        ens = cls(DeviceState.zeros(n + members.bit_length() - 1, device), n)
        try:
            ens.reset(ket)
        except BaseException:
            ens.close()
            raise
        return ens

    def reset(self, ket) -> "TrajectoryEnsemble":
        """Every member becomes ``ket`` again: one upload of a member and a broadcast on the device."""
        ket = np.asarray(ket)
        if ket.shape != (1 << self.member_qubits,):
            raise ValueError("the ket does not have the size of a member")
        self.state.upload(ket, 0)
        _lib.call("qsv_ensemble_broadcast", self.state._h, self.member_qubits)
        self.set_bits(None)
        self._measured = []
        return self

    def close(self) -> None:
        if self.state is not None:
            self.state.close()
        self.state = None

    # ---- circuit elements -------------------------------------------------------------------------------------------------
    def apply(self, gate, *, u=None) -> "TrajectoryEnsemble":
        """A unitary gate on member qubits goes to the register and acts on every member; a ``noise.Channel`` is one
        trajectory step of every member; a ``noise.Measure`` measures every member (the k-th since ``reset()`` writes
        classical bit k unless it names a ``bit``); a ``ClassicalControl`` is taken by the members whose outcomes satisfy it,
        its indices being positions in the list of measurements, as in ``Simulator.run``.  ``u``: the draws of a channel or
        a measurement, one per member."""
        from .dv_simulator.simulator import ClassicalControl
        from .noise import Channel, Measure, _control_masks
        if isinstance(gate, Channel):
            return self.apply_channel(gate.channel, gate.indices, u=u, rng=gate.rng)
        if isinstance(gate, Measure):
            bit = gate.bit
            if bit is None:
                bit = len(self._measured)
                if bit > 63:
                    raise ValueError("a member has 64 classical bits: reuse bits with bit=")
            self.measure(gate.indices[0], gate.theta, gate.phi, u=u, result=gate.result, reset=gate.reset, bit=bit, rng=gate.rng)
            self._measured.append(bit)
            return self
        if isinstance(gate, ClassicalControl):
            positive, negative = _control_masks(gate, self._measured)
            return self.apply_conditional(gate.gate, positive, negative)
        if any(not 0 <= int(q) < self.member_qubits for q in gate.indices):
            raise ValueError(f"qubit index out of range for members of {self.member_qubits} qubits")
        matrix = getattr(gate, "matrix", None)
        if matrix is None or matrix.shape[0] != matrix.shape[1]:
            raise ValueError("an ensemble takes unitary gates and channels; measurements are not supported")
        shifted = gate.copy()
        shifted.indices = [int(q) + self.member_bits for q in gate.indices]
        if getattr(shifted, "sources", None):
            shifted.sources = None            # a fused block's parts carry register indices of their own: apply its matrix
        out = shifted.apply(self.state)
        if isinstance(out, tuple):
            raise ValueError("an ensemble takes unitary gates and channels; measurements are not supported")
        return self

    def apply_channel(self, channel, qubits, *, u=None, forced=None, rng=None) -> "TrajectoryEnsemble":
        """One trajectory step per member.  ``u``: one draw in ``[0, 1)`` per member (default: ``rng.random(members)``, or
        the global ``np.random``); ``forced``: ``None`` or one branch per member, ``-1`` = draw."""
        qubits = [int(q) for q in qubits]
        if len(qubits) != channel.num_qubits:
            raise ValueError(f"the channel acts on {channel.num_qubits} qubits, got {len(qubits)}")
        if u is None:
            u = rng.random(self.members) if rng is not None else np.random.random(self.members)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        if u.shape[0] != self.members:
            raise ValueError("one draw per member")
        fbuf = None
        if forced is not None:
            fbuf = np.ascontiguousarray(forced, dtype=np.int32).reshape(-1)
            if fbuf.shape[0] != self.members:
                raise ValueError("one forced branch per member (-1 = draw)")
        _lib.call("qsv_ensemble_apply_channel", self.state._h, self.member_qubits, channel.handle(self.state.device), _ints(qubits),
                  u.ctypes.data_as(C.POINTER(C.c_double)), None if fbuf is None else fbuf.ctypes.data_as(C.POINTER(C.c_int)))
        return self

    def measure(self, q: int, theta: float = 0.0, phi: float = 0.0, *, u=None, result=None, reset: bool = False, bit=None,
                rng=None) -> "TrajectoryEnsemble":
        """Measure member qubit ``q`` of every member along ``(theta, phi)``; the qubit stays (``reset``: in ``|0>``).
        ``u``: one draw per member (default ``rng.random(members)`` or the global ``np.random``); ``result``: ``None``, one
        forced outcome for all, or one per member with ``-1`` = draw; ``bit``: the classical bit that takes the outcome
        (``None``: it is only logged).  The step is appended to ``channel_log()``."""
        from .noise import Measure
        e0, e1 = Measure(q, theta, phi).eigenvectors()
        if u is None:
            u = rng.random(self.members) if rng is not None else np.random.random(self.members)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        if u.shape[0] != self.members:
            raise ValueError("one draw per member")
        fbuf = None
        if result is not None:
            fbuf = np.ascontiguousarray(np.broadcast_to(np.asarray(result, dtype=np.int32), (self.members,)) if np.ndim(result) == 0
                                        else np.asarray(result, dtype=np.int32).reshape(-1))
            if fbuf.shape[0] != self.members:
                raise ValueError("one forced outcome per member (-1 = draw)")
        eig0 = np.ascontiguousarray(np.asarray(e0, dtype=np.complex128).reshape(2)).view(np.float64)
        eig1 = np.ascontiguousarray(np.asarray(e1, dtype=np.complex128).reshape(2)).view(np.float64)
        _lib.call("qsv_ensemble_measure", self.state._h, self.member_qubits, int(q), eig0.ctypes.data_as(C.POINTER(C.c_double)),
                  eig1.ctypes.data_as(C.POINTER(C.c_double)), 1 if reset else 0, -1 if bit is None else int(bit),
                  u.ctypes.data_as(C.POINTER(C.c_double)), None if fbuf is None else fbuf.ctypes.data_as(C.POINTER(C.c_int)))
        return self

    def apply_conditional(self, gate, positive=(), negative=()) -> "TrajectoryEnsemble":
        """``gate`` (a 1- or 2-qubit unitary on member qubits) on the members whose classical bits ``positive`` are all 1
        and ``negative`` all 0; every other member is left bit-identical."""
        matrix = getattr(gate, "matrix", None)
        indices = [int(q) for q in getattr(gate, "indices", [])]
        if matrix is None or matrix.shape[0] != matrix.shape[1] or len(indices) not in (1, 2) or matrix.shape[0] != 1 << len(indices):
            raise ValueError("a conditional gate of an ensemble is a 1- or 2-qubit unitary")
        all_of = none_of = 0
        for b in positive:
            if not 0 <= int(b) <= 63:
                raise ValueError("a member has the classical bits 0 .. 63")
            all_of |= 1 << int(b)
        for b in negative:
            if not 0 <= int(b) <= 63:
                raise ValueError("a member has the classical bits 0 .. 63")
            none_of |= 1 << int(b)
        buf = np.ascontiguousarray(matrix, dtype=np.complex128).view(np.float64)
        _lib.call("qsv_ensemble_apply_conditional", self.state._h, self.member_qubits, len(indices), _ints(indices),
                  buf.ctypes.data_as(C.POINTER(C.c_double)), C.c_uint64(all_of), C.c_uint64(none_of))
        return self

    # ---- per-member parameters: the same circuit at many parameter points ---------------------------
    def apply_pauli_rotations(self, rotations, thetas=None) -> "TrajectoryEnsemble":
        """``rotations = [(theta, letters, member qubits), ...]`` as in ``DeviceState.apply_pauli_rotations``, the first
        applied first.  ``thetas[members, R]`` gives member ``m`` row ``m`` instead of the list's angles; without it every
        member takes the list's.  The passes are those of the list on one member, whatever the number of members."""
        offsets, qubits, letters, angles = [0], [], [], []
        for theta, paulis, qs in rotations:
            paulis, qs = str(paulis), [int(q) for q in qs]
            if len(paulis) != len(qs):
                raise ValueError("one Pauli letter per qubit")
            qubits += qs
            letters.append(paulis)
            offsets.append(len(qubits))
            angles.append(float(theta))
        count = len(angles)
        if thetas is None:
            table = np.ascontiguousarray(np.broadcast_to(np.asarray(angles, dtype=np.float64), (self.members, count)))
        else:
            table = np.ascontiguousarray(thetas, dtype=np.float64)
            if table.shape != (self.members, count):
                raise ValueError(f"thetas must have shape [members, rotations] = [{self.members}, {count}]")
        passes = C.c_uint64()
        _lib.call("qsv_ensemble_apply_pauli_rotations", self.state._h, self.member_qubits, count, _ints(offsets), _ints(qubits),
                  "".join(letters).encode(), table.ctypes.data_as(C.POINTER(C.c_double)), C.byref(passes))
        self.last_passes = int(passes.value)
        return self

    def apply_matrices(self, matrices, qubits) -> "TrajectoryEnsemble":
        """Member ``m`` takes ``matrices[m]`` (``[members, 2^k, 2^k]``, ``k`` = 1 or 2, ``qubits[0]`` the most significant
        bit of the row index) on member qubits ``qubits``.  Unitarity is not demanded; nothing is logged."""
        qubits = [int(q) for q in qubits]
        if len(qubits) not in (1, 2):
            raise ValueError("per-member matrices act on 1 or 2 qubits")
        dim = 1 << len(qubits)
        buf = np.ascontiguousarray(matrices, dtype=np.complex128)
        if buf.shape != (self.members, dim, dim):
            raise ValueError(f"matrices must have shape [members, 2^k, 2^k] = [{self.members}, {dim}, {dim}]")
        _lib.call("qsv_ensemble_apply_matrices", self.state._h, self.member_qubits, len(qubits), _ints(qubits),
                  buf.view(np.float64).ctypes.data_as(C.POINTER(C.c_double)))
        return self

    def apply_layer(self, matrices, qubits=None) -> "TrajectoryEnsemble":
        """A one-qubit gate on each of the member qubits ``qubits`` (``None``: all of them) of every member, in a few tile
        passes.  ``matrices`` of shape ``(2, 2)`` or ``(k, 2, 2)``: the same gates for every member
        (``DeviceState.apply_layer`` on the member part of the register); ``(members, k, 2, 2)``: member ``m`` takes
        ``matrices[m]`` (``qsv_ensemble_apply_layer``).  Either way a member's amplitudes are bit for bit those of a register
        of its own after ``apply_layer`` with its matrices.  ``last_passes`` holds the passes."""
        from .layers import layer_table
        qubits = list(range(self.member_qubits)) if qubits is None else [int(q) for q in qubits]
        k = len(qubits)
        if np.ndim(matrices) < 4:
            if any(not 0 <= q < self.member_qubits for q in qubits):
                raise ValueError(f"qubit index out of range for members of {self.member_qubits} qubits")
            self.last_passes = self.state._apply_layer(layer_table(matrices, k), [q + self.member_bits for q in qubits])
            return self
        table = np.ascontiguousarray(matrices, dtype=np.complex128)
        if table.shape != (self.members, k, 2, 2):
            raise ValueError(f"per-member matrices must have shape [members, k, 2, 2] = [{self.members}, {k}, 2, 2]")
        passes = C.c_uint64()
        _lib.call("qsv_ensemble_apply_layer", self.state._h, self.member_qubits, k, _ints(qubits),
                  table.view(np.float64).ctypes.data_as(C.POINTER(C.c_double)), C.byref(passes))
        self.last_passes = int(passes.value)
        return self

    def apply_diagonal_phase(self, diag, gammas) -> "TrajectoryEnsemble":
        """``psi_m[i] *= exp(-i gammas[m] d[i])`` for a ``DiagonalOperator`` of ``member_qubits`` qubits: one gamma per member."""
        _diagonal_operand(diag)
        gbuf = np.ascontiguousarray(gammas, dtype=np.float64)
        if gbuf.shape != (self.members,):
            raise ValueError("one gamma per member")
        _lib.call("qsv_ensemble_apply_diag_phase", self.state._h, self.member_qubits, diag._h, gbuf.ctypes.data_as(C.POINTER(C.c_double)))
        return self

    def expect_diagonal(self, diag, threshold: float | None = None) -> DiagonalMoments:
        """The fields of ``DeviceState.expect_diagonal`` as arrays with one entry per member; nothing is divided by a norm."""
        _diagonal_operand(diag)
        out = np.zeros((self.members, 4), dtype=np.float64)
        thr = None if threshold is None else C.byref(C.c_double(float(threshold)))
        _lib.call("qsv_ensemble_expect_diag", self.state._h, self.member_qubits, diag._h, thr, out.ctypes.data_as(C.POINTER(C.c_double)))
        return DiagonalMoments(*(np.ascontiguousarray(out[:, k]) for k in range(4)))

    def bits(self) -> np.ndarray:
        """The classical bits: one ``uint64`` per member."""
        out = np.zeros(self.members, dtype=np.uint64)
        _lib.call("qsv_ensemble_bits_read", self.state._h, self.member_qubits, out.ctypes.data_as(C.POINTER(C.c_uint64)))
        return out

    def set_bits(self, words) -> "TrajectoryEnsemble":
        """One ``uint64`` per member, or ``None``: all bits 0."""
        if words is None:
            _lib.call("qsv_ensemble_bits_write", self.state._h, self.member_qubits, None)
            return self
        buf = np.array(words, dtype=np.uint64).reshape(-1)          # a copy of our own
        if buf.shape[0] != self.members:
            raise ValueError("one word per member")
        _lib.call("qsv_ensemble_bits_write", self.state._h, self.member_qubits, buf.ctypes.data_as(C.POINTER(C.c_uint64)))
        self._bits_source = buf          # the copy is enqueued, not waited for: the words stay alive until the next write
        return self

    def outcomes(self, count: int) -> np.ndarray:
        """``[members, count]`` int8: the classical bits ``0 .. count - 1`` of every member."""
        count = int(count)
        if not 0 <= count <= 64:
            raise ValueError("a member has 64 classical bits")
        words = self.bits()
        return ((words[:, None] >> np.arange(count, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int8)

    def channel_log(self) -> tuple[np.ndarray, np.ndarray]:
        """``(branches[steps, members], probs[steps, members])`` since the last read, in call order; clears the log."""
        steps = C.c_uint64(0)
        _lib.call("qsv_ensemble_log_read", self.state._h, None, None, 0, C.byref(steps))
        branches = np.zeros((steps.value, self.members), dtype=np.int32)
        probs = np.zeros((steps.value, self.members), dtype=np.float64)
        if steps.value:
            _lib.call("qsv_ensemble_log_read", self.state._h, branches.ctypes.data_as(C.POINTER(C.c_int32)),
                      probs.ctypes.data_as(C.POINTER(C.c_double)), steps.value, C.byref(steps))
        return branches, probs

    # ---- read-out -----------------------------------------------------------------------------------------------------------
    def norm2(self) -> np.ndarray:
        out = np.zeros(self.members, dtype=np.float64)
        _lib.call("qsv_ensemble_norm2", self.state._h, self.member_qubits, out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def expect_pauli_sum(self, terms, *, return_terms: bool = False):
        """``values[m] = sum_t c_t <psi_m|P_t|psi_m>`` for ``terms = [(c, letters, member qubits), ...]`` with real ``c``;
        with ``return_terms`` also the ``[members, T]`` values of the single strings."""
        terms = _real_terms(terms, "an ensemble's expect_pauli_sum")
        _check_terms(terms, self.member_qubits)
        count, offsets, qubits, letters, cbuf = _flat_terms(terms)
        coeffs = np.ascontiguousarray(cbuf[0::2])
        values = np.zeros(self.members, dtype=np.float64)
        per_term = np.zeros((self.members, count), dtype=np.float64)
        _lib.call("qsv_ensemble_expect_pauli_sum", self.state._h, self.member_qubits, count, offsets, qubits, letters,
                  coeffs.ctypes.data_as(C.POINTER(C.c_double)), values.ctypes.data_as(C.POINTER(C.c_double)),
                  per_term.ctypes.data_as(C.POINTER(C.c_double)) if return_terms else None)
        return (values, per_term) if return_terms else values

    # ---- two ensembles, member by member: operators, inner products and adjoint walks ----------------
    def _partner(self, other, name: str) -> "TrajectoryEnsemble":
        if not isinstance(other, TrajectoryEnsemble):
            raise ValueError(f"{name} must be an ensemble")
        if other.member_qubits != self.member_qubits or other.members != self.members:
            raise ValueError(f"{name} must have this ensemble's shape: {self.members} members of {self.member_qubits} qubits")
        return other

    def inner(self, other: "TrajectoryEnsemble") -> np.ndarray:
        """``values[m] = <self_m|other_m>``, complex; ``other`` may be ``self`` (then the imaginary parts are exactly 0)."""
        self._partner(other, "other")
        values = np.zeros(self.members, dtype=np.complex128)
        _lib.call("qsv_ensemble_inner", self.state._h, other.state._h, self.member_qubits,
                  values.view(np.float64).ctypes.data_as(C.POINTER(C.c_double)))
        return values

    def apply_pauli_sum(self, terms, out: "TrajectoryEnsemble | None" = None, accumulate: bool = False) -> "TrajectoryEnsemble":
        """``out_m = H self_m`` (``+=`` with ``accumulate``) for ``H = sum_t c_t P_t`` on member qubits: ``DeviceState.apply_pauli_sum``
        on the whole register with the qubits shifted past the member index.  ``out`` is an ensemble of this shape, allocated
        when None; it is returned.  A member's amplitudes are bit for bit those of a register of its own."""
        terms = [(complex(c), str(paulis), [int(q) for q in qs]) for c, paulis, qs in terms]
        _check_terms(terms, self.member_qubits)
        own = out is None
        if own:
            out = TrajectoryEnsemble(DeviceState.zeros(self.member_qubits + self.member_bits, self.state.device), self.member_qubits)
        try:
            self._partner(out, "out")
            self.state.apply_pauli_sum([(c, paulis, [q + self.member_bits for q in qs]) for c, paulis, qs in terms], out=out.state,
                                       accumulate=accumulate)
        except BaseException:
            if own:
                out.close()
            raise
        return out

    def apply_diagonal_operator(self, diag, out: "TrajectoryEnsemble | None" = None) -> "TrajectoryEnsemble":
        """``out_m = D self_m`` for a ``DiagonalOperator`` of ``member_qubits`` qubits.  ``out`` is an ensemble of this shape,
        allocated when None; it may be ``self``.  Returns ``out``."""
        _diagonal_operand(diag)
        own = out is None
        if own:
            out = TrajectoryEnsemble(DeviceState.zeros(self.member_qubits + self.member_bits, self.state.device), self.member_qubits)
        try:
            self._partner(out, "out")
            _lib.call("qsv_ensemble_apply_diag_mul", out.state._h, self.state._h, self.member_qubits, diag._h)
        except BaseException:
            if own:
                out.close()
            raise
        return out

    def pauli_rotations_adjoint(self, rotations, lam: "TrajectoryEnsemble", thetas=None) -> np.ndarray:
        """``DeviceState.pauli_rotations_adjoint`` member by member: for the last rotation first, ``values[m, k] =
        <lam_m|P_k|self_m>``, then both members are rotated back by ``R_k(thetas[m, k])``.  ``thetas[members, R]`` as in
        ``apply_pauli_rotations`` (the list's own angles for every member when None).  Both ensembles are consumed.  Costs
        the passes of the forward list on one member (``last_passes``), whatever the number of members."""
        self._partner(lam, "lam")
        count, offsets, qubits, letters, cbuf = _flat_terms(rotations)
        if thetas is None:
            table = np.ascontiguousarray(np.broadcast_to(cbuf.view(np.complex128).real, (self.members, count)), dtype=np.float64)
        else:
            table = np.ascontiguousarray(thetas, dtype=np.float64)
            if table.shape != (self.members, count):
                raise ValueError(f"thetas must have shape [members, rotations] = [{self.members}, {count}]")
        values = np.zeros((self.members, count), dtype=np.complex128)
        passes = C.c_uint64()
        _lib.call("qsv_ensemble_pauli_rotations_adjoint", self.state._h, lam.state._h, self.member_qubits, count, offsets, qubits, letters,
                  table.ctypes.data_as(C.POINTER(C.c_double)), values.view(np.float64).ctypes.data_as(C.POINTER(C.c_double)), C.byref(passes))
        self.last_passes = int(passes.value)
        return values

    def diagonal_phase_adjoint(self, diag, lam: "TrajectoryEnsemble", gammas) -> np.ndarray:
        """``values[m] = <lam_m| D |self_m>``, then ``exp(-i gammas[m] D)`` on ``self_m`` and on ``lam_m``, in one pass: the
        step of an adjoint walk over a per-member cost layer.  ``D`` has ``member_qubits`` qubits."""
        _diagonal_operand(diag)
        self._partner(lam, "lam")
        gbuf = np.ascontiguousarray(gammas, dtype=np.float64)
        if gbuf.shape != (self.members,):
            raise ValueError("one gamma per member")
        values = np.zeros(self.members, dtype=np.complex128)
        _lib.call("qsv_ensemble_diag_phase_adjoint", self.state._h, lam.state._h, self.member_qubits, diag._h,
                  gbuf.ctypes.data_as(C.POINTER(C.c_double)), values.view(np.float64).ctypes.data_as(C.POINTER(C.c_double)))
        return values

    def member(self, m: int) -> np.ndarray:
        """Member ``m`` as a NumPy ket."""
        m = int(m)
        if not 0 <= m < self.members:
            raise ValueError("no such member")
        size = 1 << self.member_qubits
        return self.state.download(m * size, size)


Ensemble = TrajectoryEnsemble      # the same object when its members differ by parameters instead of draws
