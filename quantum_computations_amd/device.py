"""Device-resident registers: thin Python handles over ``qsv_state`` (include/qsv.h).

``DeviceState`` is what ``Gate.apply`` receives when the caller wants the register to stay in HBM between gates
(the reference passes a NumPy ket to every ``apply`` -- ``simulators/dv_simulator/simulator.py:47`` -- which
would cost one upload and one download per gate here).  Host arrays are only touched by ``from_numpy`` /
``to_numpy``.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple

import numpy as np

from . import _lib

_SEQUENCE_WORK_ENV = int(os.environ.get("QSV_SEQUENCE_WORK", "0") or 0)   # see DeviceState.apply_sequence
_PACKED_SEQUENCES: dict = {}     # id(sources list of a fused block) -> its packed gate list, see DeviceState.apply_sequence
_TILE_SEQUENCE_ENV = int(os.environ.get("QSV_TILE_SEQUENCE_GATES", "12") or 0)     # qsv_api.hip: qsv_apply_sequence


def _cbuf(a, n_complex: int | None = None) -> np.ndarray:
    """Contiguous complex128 copy of ``a`` (the interleaved layout the C ABI wants)."""
    arr = np.ascontiguousarray(np.asarray(a), dtype=np.complex128)
    if n_complex is not None and arr.size != n_complex:
        raise ValueError(f"expected {n_complex} complex entries, got {arr.size}")
    return arr


def _ptr(arr: np.ndarray) -> C.c_void_p:
    # data_as() keeps a reference to the array on the returned pointer object, so a temporary passed as
    # `_ptr(_cbuf(x))` stays alive for the duration of the foreign call (c_void_p(arr.ctypes.data) would not)
    return arr.ctypes.data_as(C.c_void_p)


def _ints(values) -> "C.Array[C.c_int]":
    values = [int(v) for v in values]
    return (C.c_int * max(len(values), 1))(*values)


def _flat_terms(terms):
    """``[(coefficient or angle, letters, qubits), ...]`` as the C ABI takes it: (count, offsets, qubits, letters,
    the first entries as a float64 buffer of interleaved complex numbers)."""
    offsets, qubits, letters, coeffs = [0], [], [], []
    for coefficient, paulis, qs in terms:
        qs = [int(q) for q in qs]
        if len(paulis) != len(qs):
            raise ValueError("one Pauli letter per qubit")
        qubits += qs
        letters.append(str(paulis))
        offsets.append(len(qubits))
        coeffs.append(complex(coefficient))
    cbuf = np.ascontiguousarray(coeffs, dtype=np.complex128).view(np.float64)
    return len(coeffs), _ints(offsets), _ints(qubits), "".join(letters).encode(), cbuf


def _real_terms(terms, what: str) -> list:
    terms = [(complex(c), str(paulis), [int(q) for q in qs]) for c, paulis, qs in terms]
    if any(c.imag != 0.0 for c, _, _ in terms):
        raise ValueError(f"{what} needs real coefficients (a hermitian Pauli sum)")
    return terms


def _check_terms(terms, n_qubits: int) -> None:
    """The refusals of the C term parser, for a caller that has to know the list is good before it changes a register."""
    for _, paulis, qs in terms:
        if len(paulis) != len(qs):
            raise ValueError("one Pauli letter per qubit")
        if len(paulis) > 64:
            raise ValueError("bad Pauli string length")
        if any(letter not in "IXYZixyz" for letter in paulis):
            raise ValueError("Pauli letters must be I, X, Y or Z")
        if any(not 0 <= q < n_qubits for q in qs):
            raise ValueError(f"qubit index out of range for a {n_qubits}-qubit register")
        if len(set(qs)) != len(qs):
            raise ValueError("Indices must be distinct.")


def _ket_operand(register, name: str) -> None:
    if isinstance(register, DensityState):
        raise ValueError(f"{name} must be a ket register, not a density register")


def _dbl(buf: np.ndarray):
    return buf.ctypes.data_as(C.POINTER(C.c_double))


# what DeviceState.expect_diagonal returns: sum p, sum p d, sum p d^2 and sum of p over d <= threshold, p = |amplitude|^2
DiagonalMoments = namedtuple("DiagonalMoments", ["norm2", "mean", "second_moment", "probability_below"])


def _diagonal_operand(diag) -> None:
    from .diagonal import DiagonalOperator
    if not isinstance(diag, DiagonalOperator):
        raise TypeError("expected a DiagonalOperator")


class DeviceState:
    """An n-qubit complex128 register in HBM (qubit 0 = most significant bit, as in the reference)."""

    def __init__(self, handle: C.c_void_p, keepalive=None, device: int = 0):
        self._h = handle
        self._keepalive = keepalive   # e.g. the torch tensor backing a view
        self.device = device          # HIP device ordinal the register lives on

    # ---- construction -------------------------------------------------------------------------
    @classmethod
    def zeros(cls, n_qubits: int, device: int = 0) -> "DeviceState":
        """|0...0> on ``device`` (``n_qubits = 0`` is the empty register ``[1.]``, simulator.py:22)."""
        h = C.c_void_p()
        _lib.call("qsv_create", int(n_qubits), int(device), C.byref(h))
        return cls(h, device=int(device))

    @classmethod
    def from_numpy(cls, ket: np.ndarray, device: int = 0) -> "DeviceState":
        ket = np.asarray(ket)
        if ket.ndim != 1:
            raise ValueError("State has wrong dimensions.")
        size = ket.shape[0]
        if size == 0 or size & (size - 1):
            raise ValueError("Given array is not a qubit state nor operator")
        st = cls.zeros(size.bit_length() - 1, device)
        buf = _cbuf(ket)
        _lib.call("qsv_upload", st._h, _ptr(buf), 0, size)
        return st

    @classmethod
    def view(cls, n_qubits: int, dev_ptr: int, capacity_amps: int, device: int = 0, stream: int = 0,
             keepalive=None) -> "DeviceState":
        """Wrap caller-owned device memory (e.g. ``tensor.data_ptr()``) without copying."""
        h = C.c_void_p()
        _lib.call("qsv_create_view", int(n_qubits), int(device), C.c_void_p(dev_ptr), int(capacity_amps),
                  C.c_void_p(stream), C.byref(h))
        return cls(h, keepalive, int(device))

    def rebind(self, n_qubits: int, dev_ptr: int, capacity_amps: int, keepalive=None) -> "DeviceState":
        """Re-point a view register at another window of caller-owned device memory (``qsv_rebind_view``): no
        allocation, no synchronisation.  The sharded register walks the slices of an exchange with one handle."""
        _lib.call("qsv_rebind_view", self._h, int(n_qubits), C.c_void_p(dev_ptr), int(capacity_amps))
        self._keepalive = keepalive
        return self

    @classmethod
    def random(cls, n_qubits: int, seed: int, device: int = 0) -> "DeviceState":
        """Normalised pseudo-random ket generated on the device (counter-based, reproducible)."""
        st = cls.zeros(n_qubits, device)
        st.fill_random(seed)
        return st

    def fill_random(self, seed: int, index_offset: int = 0, normalise: bool = True) -> float:
        n2 = C.c_double()
        _lib.call("qsv_fill_random", self._h, int(seed), int(index_offset), C.byref(n2))
        if normalise:
            _lib.call("qsv_scale", self._h, 1.0 / np.sqrt(n2.value), 0.0)
        return n2.value

    def close(self) -> None:
        if self._h is not None and self._h.value:
            _lib.load().qsv_destroy(self._h)
        self._h = None
        self._keepalive = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- inspection ---------------------------------------------------------------------------
    @property
    def num_qubits(self) -> int:
        n = C.c_int()
        _lib.call("qsv_num_qubits", self._h, C.byref(n))
        return n.value

    @property
    def num_amps(self) -> int:
        n = C.c_uint64()
        _lib.call("qsv_num_amps", self._h, C.byref(n))
        return n.value

    @property
    def shape(self) -> tuple[int]:
        return (self.num_amps,)

    ndim = 1

    @property
    def device_ptr(self) -> int:
        p = C.c_void_p()
        _lib.call("qsv_device_ptr", self._h, C.byref(p))
        return p.value or 0

    def to_numpy(self) -> np.ndarray:
        out = np.empty(self.num_amps, dtype=np.complex128)
        _lib.call("qsv_download", self._h, _ptr(out), 0, out.size)
        return out

    def download(self, offset: int, count: int) -> np.ndarray:
        out = np.empty(count, dtype=np.complex128)
        _lib.call("qsv_download", self._h, _ptr(out), int(offset), int(count))
        return out

    def upload(self, amplitudes: np.ndarray, offset: int = 0) -> None:
        buf = _cbuf(amplitudes)
        _lib.call("qsv_upload", self._h, _ptr(buf), int(offset), buf.size)

    def copy_into(self, other: "DeviceState") -> "DeviceState":
        """Overwrite ``other`` (a register of at least this size on the same device) with this register."""
        _lib.call("qsv_copy", other._h, self._h)
        return other

    def copy(self) -> "DeviceState":
        other = DeviceState.zeros(DeviceState.num_qubits.fget(self), self.device)     # register qubits, whatever the view
        _lib.call("qsv_copy", other._h, self._h)
        return other

    def sync(self) -> None:
        _lib.call("qsv_sync", self._h)

    def set_option(self, option: int, value: int) -> None:
        _lib.call("qsv_set_option", self._h, int(option), int(value))
        if int(option) == _lib.OPT_SEQUENCE_WORK:
            self._sequence_work = int(value) if int(value) >= 0 else _SEQUENCE_WORK_ENV
        if int(option) == _lib.OPT_TILE_SEQUENCE_GATES:
            self._tile_sequence_gates = int(value) if int(value) >= 0 else None

    def set_stream(self, stream: int) -> None:
        _lib.call("qsv_set_stream", self._h, C.c_void_p(stream))

    def set_basis(self, index: int) -> None:
        _lib.call("qsv_set_basis", self._h, int(index))

    # ---- gates --------------------------------------------------------------------------------
    def apply_matrix(self, matrix: np.ndarray, indices) -> "DeviceState":
        """In-place ``U_full @ ket`` for a 2^k x 2^k matrix on qubits ``indices`` (``Gate.apply``)."""
        indices = [int(i) for i in indices]
        k = len(indices)
        m = _cbuf(matrix, (1 << k) ** 2)
        if k == 1:
            _lib.call("qsv_apply_1q", self._h, indices[0], _ptr(m))
        elif k == 2:
            _lib.call("qsv_apply_2q", self._h, indices[0], indices[1], _ptr(m))
        else:
            _lib.call("qsv_apply_kq", self._h, k, _ints(indices), _ptr(m))
        return self

    def apply_sequence(self, indices, sources, matrix) -> "DeviceState":
        """A fused block (``fusion.fuse_circuit``): ``matrix`` on qubits ``indices`` is the product of the gates
        ``sources``.  6-qubit blocks made of at most 12 one- and two-qubit gates (``OPT_TILE_SEQUENCE_GATES``) are applied
        as that LIST on LDS-resident tiles in one pass over the register (``qsv_apply_sequence`` -> ``k_seq_tile``: a
        fraction of the dense block's arithmetic, 1.7-1.9 ms against 2.0-2.1); 5-qubit blocks only on request (tiles, or
        the register form behind ``OPT_SEQUENCE_WORK``: neither beats their dense product); everything else as the dense
        matrix."""
        indices = [int(i) for i in indices]
        requested = getattr(self, "_tile_sequence_gates", None)        # an explicit limit also admits 5-qubit blocks
        on_tiles = (len(indices) == 6 or (len(indices) == 5 and requested is not None)) and \
            len(sources) <= (_TILE_SEQUENCE_ENV if requested is None else requested)
        in_registers = getattr(self, "_sequence_work", _SEQUENCE_WORK_ENV) > 0 and len(indices) == 5
        if (on_tiles or in_registers) and all(getattr(g, "matrix", None) is not None and 1 <= len(g.indices) <= 2
                                     and np.shape(g.matrix) == (1 << len(g.indices),) * 2 for g in sources):
            packed = _PACKED_SEQUENCES.get(id(sources))
            if packed is None or packed[0] is not sources or packed[1] != indices or packed[6] != len(sources):
                arity = [len(g.indices) for g in sources]
                legs = []
                for g in sources:
                    pos = [indices.index(int(q)) for q in g.indices]
                    legs += pos + [0] * (2 - len(pos))
                mats = np.concatenate([np.ascontiguousarray(g.matrix, dtype=np.complex128).reshape(-1) for g in sources])
                packed = (sources, list(indices), _ints(indices), _ints(arity), _ints(legs), mats, len(sources))
                if len(_PACKED_SEQUENCES) >= 512:
                    _PACKED_SEQUENCES.clear()
                _PACKED_SEQUENCES[id(sources)] = packed       # a fused block is applied many times: pack its list once
            handled = C.c_int(0)
            _lib.call("qsv_apply_sequence", self._h, len(indices), packed[2], len(sources), packed[3], packed[4],
                      _ptr(packed[5]), C.byref(handled))
            if handled.value:
                return self
        return self.apply_matrix(matrix, indices)

    def apply_diagonal(self, diagonal, indices) -> "DeviceState":
        indices = [int(i) for i in indices]
        d = _cbuf(diagonal, 1 << len(indices))
        if len(indices) == 1:
            _lib.call("qsv_apply_diag_1q", self._h, indices[0], _ptr(d))
        elif len(indices) == 2:
            _lib.call("qsv_apply_diag_2q", self._h, indices[0], indices[1], _ptr(d))
        else:
            _lib.call("qsv_apply_kq", self._h, len(indices), _ints(indices), _ptr(_cbuf(np.diag(d))))
        return self

    def apply_cx(self, control: int, target: int) -> "DeviceState":
        _lib.call("qsv_apply_cx", self._h, int(control), int(target))
        return self

    def apply_swap(self, q0: int, q1: int) -> "DeviceState":
        _lib.call("qsv_apply_swap", self._h, int(q0), int(q1))
        return self

    def apply_controlled(self, matrix, controls, target: int) -> "DeviceState":
        m = _cbuf(matrix, 4)
        controls = list(controls)
        _lib.call("qsv_apply_controlled_1q", self._h, len(controls), _ints(controls), int(target), _ptr(m))
        return self

    def apply_mcphase(self, qubits, phase: complex) -> "DeviceState":
        qubits = list(qubits)
        phase = complex(phase)
        _lib.call("qsv_apply_mcphase", self._h, len(qubits), _ints(qubits), phase.real, phase.imag)
        return self

    def apply_scale(self, factor: complex) -> "DeviceState":
        factor = complex(factor)
        _lib.call("qsv_scale", self._h, factor.real, factor.imag)
        return self

    def permute(self, new_ordering) -> "DeviceState":
        _lib.call("qsv_permute", self._h, _ints(new_ordering))
        return self

    # ---- measurement / insertion --------------------------------------------------------------
    def measure(self, index: int, eig0, eig1, forced: int | None = None, u01: float = 0.0):
        """Collapse qubit ``index`` (register shrinks by one).  Returns ``(outcome, p0, p1)``."""
        e0, e1 = _cbuf(eig0, 2), _cbuf(eig1, 2)
        out, p0, p1 = C.c_int(), C.c_double(), C.c_double()
        _lib.call("qsv_measure", self._h, int(index), _ptr(e0), _ptr(e1), -1 if forced is None else int(forced),
                  float(u01), C.byref(out), C.byref(p0), C.byref(p1))
        return out.value, p0.value, p1.value

    def measure_probs(self, index: int, eig0, eig1) -> tuple[float, float]:
        e0, e1 = _cbuf(eig0, 2), _cbuf(eig1, 2)
        p0, p1 = C.c_double(), C.c_double()
        _lib.call("qsv_measure_probs", self._h, int(index), _ptr(e0), _ptr(e1), C.byref(p0), C.byref(p1))
        return p0.value, p1.value

    def collapse(self, index: int, eig, scale: float) -> "DeviceState":
        """Project qubit ``index`` on ``eig`` (unconjugated) and multiply by ``scale``; register shrinks."""
        _lib.call("qsv_collapse", self._h, int(index), _ptr(_cbuf(eig, 2)), float(scale))
        return self

    def insert(self, index: int, amplitudes) -> "DeviceState":
        a = _cbuf(amplitudes, 2)
        _lib.call("qsv_insert", self._h, int(index), _ptr(a))
        return self

    # ---- read-out -----------------------------------------------------------------------------
    def norm2(self) -> float:
        v = C.c_double()
        _lib.call("qsv_norm2", self._h, C.byref(v))
        return v.value

    def probabilities(self, indices) -> np.ndarray:
        idx = np.ascontiguousarray(indices, dtype=np.uint64)
        out = np.empty(idx.size, dtype=np.float64)
        _lib.call("qsv_probabilities", self._h, idx.ctypes.data_as(C.POINTER(C.c_uint64)), idx.size,
                  out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def expect_pauli(self, paulis: str, qubits) -> complex:
        """``<psi| P |psi>`` for the Pauli string ``paulis`` (letters I/X/Y/Z) on ``qubits``, computed on the device."""
        qubits = [int(q) for q in qubits]
        if len(paulis) != len(qubits):
            raise ValueError("one Pauli letter per qubit")
        re, im = C.c_double(), C.c_double()
        _lib.call("qsv_expect_pauli", self._h, len(qubits), _ints(qubits), paulis.encode(), C.byref(re), C.byref(im))
        return complex(re.value, im.value)

    def expect_pauli_sum(self, terms, *, return_terms: bool = False):
        """``<psi| H |psi>`` for ``H = sum_t c_t P_t``; ``terms`` is an iterable of ``(coefficient, letters, qubits)``
        with letters and qubits as in ``expect_pauli``.  Terms that flip the same qubits share passes over the
        register (all Z-only terms need one pass per eight terms; XX and YY on a pair share one), each pass reads
        every amplitude once, and the whole sum costs one synchronisation.  Returns the complex value, or
        ``(value, per-term real expectation values in the caller's order)`` with ``return_terms=True``."""
        count, offsets, qubits, letters, cbuf = _flat_terms(terms)
        values = np.zeros(count, dtype=np.float64)
        re, im = C.c_double(), C.c_double()
        _lib.call("qsv_expect_pauli_sum", self._h, count, offsets, qubits, letters,
                  cbuf.ctypes.data_as(C.POINTER(C.c_double)), values.ctypes.data_as(C.POINTER(C.c_double)),
                  C.byref(re), C.byref(im), None)
        value = complex(re.value, im.value)
        return (value, values) if return_terms else value

    def apply_pauli_rotation(self, theta: float, paulis: str, qubits) -> "DeviceState":
        """In-place ``exp(-i theta/2 P) ket`` for the Pauli string ``P`` = ``paulis[j]`` on ``qubits[j]`` (the sign
        convention of ``RZ``): one pass over the register whatever the weight of the string, no matrix."""
        return self.apply_pauli_rotations([(theta, paulis, qubits)])

    def apply_pauli_rotations(self, rotations) -> "DeviceState":
        """An ordered list ``[(theta, letters, qubits), ...]`` of Pauli rotations, the first applied first.  Consecutive
        rotations that are diagonal or flip the same qubits share a pass of at most eight (``XX``, ``YY``, ``ZZ`` on a
        pair: one pass); the order is never changed.  ``ShardedState`` has no such method: out of scope there."""
        self._pauli_rotations(rotations)
        return self

    def _pauli_rotations(self, rotations, qubit_offset: int = 0, conjugate: bool = False) -> int:
        """Flatten and launch; returns the number of passes.  ``conjugate``: rotate by ``conj(P)`` = ``(-1)^nY P`` in
        the opposite direction, on qubits moved by ``qubit_offset`` (the column side of a density matrix)."""
        offsets, qubits, letters, thetas = [0], [], [], []
        for theta, paulis, qs in rotations:
            paulis, qs = str(paulis), [int(q) + qubit_offset for q in qs]
            if len(paulis) != len(qs):
                raise ValueError("one Pauli letter per qubit")
            theta = float(theta)
            if conjugate:
                theta = -theta if paulis.upper().count("Y") % 2 == 0 else theta
            qubits += qs
            letters.append(paulis)
            offsets.append(len(qubits))
            thetas.append(theta)
        passes = C.c_uint64()
        tbuf = np.ascontiguousarray(thetas, dtype=np.float64)
        _lib.call("qsv_apply_pauli_rotations", self._h, len(thetas), _ints(offsets), _ints(qubits), "".join(letters).encode(),
                  tbuf.ctypes.data_as(C.POINTER(C.c_double)), C.byref(passes))
        return passes.value

    # ---- quantum Fourier transform ---------------------------------------------------------------
    def apply_qft(self, qubits=None, *, inverse: bool = False, swaps: bool = True) -> "DeviceState":
        """In-place quantum Fourier transform on the ordered ``qubits`` (``None``: all of them, in order; the first is the
        most significant leg): ``apply_matrix(npq.qft_matrix(m, inverse, swaps), qubits)`` for any ``m``, in a few tile
        passes over the register (``qsv_apply_qft``) instead of ``m (m + 1) / 2`` gates.  ``swaps=False`` leaves the
        reversal of the qubits out.  ``ShardedState`` has no such method: out of scope there."""
        self._apply_qft(range(self.num_qubits) if qubits is None else qubits, inverse=inverse, swaps=swaps)
        return self

    def _apply_qft(self, qubits, *, inverse: bool = False, swaps: bool = True, qubit_offset: int = 0,
                   conjugate: bool = False) -> int:
        """Launch; returns the number of passes (tile passes plus the permutation).  ``conjugate``: ``conj(F)`` on qubits
        moved by ``qubit_offset`` (the column side of a density matrix)."""
        qubits = [int(q) + qubit_offset for q in qubits]
        flags = (_lib.QFT_INVERSE if inverse else 0) | (0 if swaps else _lib.QFT_NO_SWAPS) | (_lib.QFT_CONJUGATE if conjugate else 0)
        passes = C.c_uint64()
        _lib.call("qsv_apply_qft", self._h, len(qubits), _ints(qubits), flags, C.byref(passes))
        return passes.value

    # ---- product layers ---------------------------------------------------------------------------
    def apply_layer(self, matrices, qubits=None) -> "DeviceState":
        """In-place one-qubit gate on each of ``qubits`` (``None``: all of them): ``matrices`` of shape ``(2, 2)`` is the same
        gate on every listed qubit, ``(k, 2, 2)`` gives ``matrices[j]`` to ``qubits[j]``.  What ``k`` calls of
        ``apply_matrix`` give, to rounding, in ``max(1, ceil(h / 6))`` passes over the register (``qsv_apply_layer``), ``h``
        the listed qubits whose index bit is 6 or above.  The order of the list never changes a bit of the result; any
        finite matrices are taken.  ``ShardedState`` has no such method: out of scope there."""
        self._apply_layer(matrices, range(self.num_qubits) if qubits is None else qubits)
        return self

    def _apply_layer(self, matrices, qubits) -> int:
        """Check the shapes and launch; returns the number of passes."""
        from .layers import layer_table
        qubits = [int(q) for q in qubits]
        table = layer_table(matrices, len(qubits))
        passes = C.c_uint64()
        _lib.call("qsv_apply_layer", self._h, len(qubits), _ints(qubits), _dbl(table.view(np.float64)), C.byref(passes))
        return passes.value

    # ---- adjoint walk through a product layer ------------------------------
    def layer_adjoint(self, matrices, lam: "DeviceState", qubits=None) -> np.ndarray:
        """The backward walk through the layer ``apply_layer(matrices, qubits)`` made ``self`` with: ``matrices`` are the
        FORWARD factors (``(2, 2)`` or ``(k, 2, 2)``), the library is handed their conjugate transposes.  Returns
        ``T[k, 2, 2]`` with ``T[j][a][b] = <lam| (|a><b| on qubits[j]) |self>`` and leaves in both registers, bit for bit,
        what ``apply_layer`` with the conjugate transposes leaves: ``self`` is the register from before the layer (for
        unitary factors, up to rounding) and ``lam`` has gone back with it -- both are consumed.  Costs the passes of the
        forward layer.  ``layers.gradient(T, generators)`` turns ``T`` into derivatives."""
        return self._layer_adjoint(matrices, lam, range(self.num_qubits) if qubits is None else qubits)[0]

    def _layer_adjoint(self, matrices, lam: "DeviceState", qubits) -> tuple[np.ndarray, int]:
        """Check the shapes and launch; returns ``(T, passes)``."""
        from .layers import layer_table
        _ket_operand(lam, "lam")
        qubits = [int(q) for q in qubits]
        inverse = np.ascontiguousarray(np.conjugate(np.swapaxes(layer_table(matrices, len(qubits)), 1, 2)))
        values = np.zeros((len(qubits), 2, 2), dtype=np.complex128)
        passes = C.c_uint64()
        _lib.call("qsv_layer_adjoint", self._h, lam._h, len(qubits), _ints(qubits), _dbl(inverse.view(np.float64)),
                  _dbl(values.view(np.float64)), C.byref(passes))
        return values, passes.value

    def layer_transition(self, ket: "DeviceState", qubits=None) -> np.ndarray:
        """``T[k, 2, 2]`` with ``T[j][a][b] = <self| (|a><b| on qubits[j]) |ket>`` for each of ``qubits`` (``None``: all of
        them); ``self`` is the bra and ``ket`` may be ``self``.  Read-only, in the passes of a product layer on ``qubits``."""
        return self._layer_transition(ket, range(self.num_qubits) if qubits is None else qubits)[0]

    def _layer_transition(self, ket: "DeviceState", qubits) -> tuple[np.ndarray, int]:
        _ket_operand(ket, "ket")
        qubits = [int(q) for q in qubits]
        values = np.zeros((len(qubits), 2, 2), dtype=np.complex128)
        passes = C.c_uint64()
        _lib.call("qsv_layer_transition", self._h, ket._h, len(qubits), _ints(qubits), _dbl(values.view(np.float64)), C.byref(passes))
        return values, passes.value

    def one_qubit_densities(self, qubits=None) -> np.ndarray:
        """The one-qubit reduced density matrix of each of ``qubits`` (``None``: all of them) as ``[k, 2, 2]``:
        ``rho_q[b][a] = T_q[a][b]`` of ``layer_transition`` with ``bra = ket = self``, made exactly hermitian by averaging
        with its conjugate transpose.  The trace of each is ``norm2()`` up to rounding; nothing is divided by it."""
        rho = np.swapaxes(self.layer_transition(self, qubits), 1, 2)
        return 0.5 * (rho + np.conjugate(np.swapaxes(rho, 1, 2)))

    # ---- reversible register arithmetic -------------------------------------------------------
    def apply_register_map(self, op, target, source=None, controls=(), *, inverse: bool = False) -> "DeviceState":
        """In-place classical map on the value of the ``target`` qubits (``arithmetic.RegisterMap``: modular addition and
        multiplication, register-controlled versions of both, xor lookups, value permutations), reading the ``source``
        qubits and acting where every qubit of ``controls`` is 1; the first listed qubit of an operand is its most
        significant bit.  One gather pass over the register (``qsv_apply_arith``), bit-exact.  ``ShardedState`` has no such
        method: out of scope there."""
        self._apply_register_map(op, target, source, controls, inverse=inverse)
        return self

    def _apply_register_map(self, op, target, source=None, controls=(), *, inverse: bool = False, qubit_offset: int = 0) -> int:
        """Launch; returns the number of passes (0 for a map that moves nothing)."""
        target = [int(q) + qubit_offset for q in target]
        source = [int(q) + qubit_offset for q in (source if source is not None else ())]
        controls = [int(q) + qubit_offset for q in controls]
        if len(target) != op.m or len(source) != op.mx:
            raise ValueError(f"{op} needs {op.m} target and {op.mx} source qubits")
        flags = _lib.ARITH_INVERSE if bool(inverse) != bool(op.inverted) else 0
        passes = C.c_uint64()
        _lib.call("qsv_apply_arith", self._h, op._handle(self.device), _ints(target), _ints(source), len(controls), _ints(controls),
                  flags, C.byref(passes))
        return passes.value

    def evolve(self, terms, t: float, steps: int = 1, order: int = 1) -> "DeviceState":
        """Trotterised ``exp(-i t H) ket`` for ``H = sum_t c_t P_t``, ``terms`` as for ``expect_pauli_sum`` (real
        coefficients): ``npq.trotter_rotations`` turned into shared passes by ``apply_pauli_rotations``."""
        from .dv_simulator import numpy_quantum as npq
        return self.apply_pauli_rotations(npq.trotter_rotations(npq.PauliSum(self.num_qubits, terms), t, steps, order))

    # ---- Pauli sums as operators ---------------------------------------------------------------
    def apply_pauli_sum(self, terms, out: "DeviceState | None" = None, accumulate: bool = False) -> "DeviceState":
        """``out = H self`` (``out += H self`` with ``accumulate``) for ``H = sum_t c_t P_t``, ``terms`` as for
        ``expect_pauli_sum``.  ``out`` is another register on the same device, allocated when None; it is returned.
        Terms that flip the same qubits share a pass of at most eight.  ``self`` is not changed."""
        if out is None:
            out = DeviceState.zeros(self.num_qubits, self.device)
        _ket_operand(out, "out")
        count, offsets, qubits, letters, cbuf = _flat_terms(terms)
        _lib.call("qsv_apply_pauli_sum", out._h, self._h, count, offsets, qubits, letters, _dbl(cbuf), int(bool(accumulate)), None)
        return out

    def transition_pauli_sum(self, terms, ket: "DeviceState", *, return_terms: bool = False):
        """``<self| H |ket>`` for ``H = sum_t c_t P_t`` without forming ``H ket``; ``self`` is the bra.  Returns the
        complex value, or ``(value, complex <self|P_t|ket> per term in the caller's order)`` with ``return_terms=True``.
        ``ket`` may be ``self``: then this is ``expect_pauli_sum``."""
        _ket_operand(ket, "ket")
        count, offsets, qubits, letters, cbuf = _flat_terms(terms)
        values = np.zeros(count, dtype=np.complex128)
        re, im = C.c_double(), C.c_double()
        _lib.call("qsv_pauli_transition_sum", self._h, ket._h, count, offsets, qubits, letters, _dbl(cbuf),
                  _dbl(values.view(np.float64)), C.byref(re), C.byref(im), None)
        value = complex(re.value, im.value)
        return (value, values) if return_terms else value

    def variance_pauli_sum(self, terms) -> float:
        """``<H^2> - <H>^2`` of a hermitian ``H`` (real coefficients) on a normalised register: ``||H psi||^2`` from one
        ``apply_pauli_sum`` into a scratch register and ``<H> = <psi|H psi>`` by ``inner``."""
        terms = _real_terms(terms, "the variance")
        h_psi = self.apply_pauli_sum(terms)
        try:
            return h_psi.norm2() - self.inner(h_psi).real ** 2
        finally:
            h_psi.close()

    def pauli_rotations_adjoint(self, rotations, lam: "DeviceState") -> np.ndarray:
        """The backward walk over ``rotations`` (the list ``apply_pauli_rotations`` took to make ``self``): for the last
        rotation first, ``values[k] = <lam|P_k|self>``, then both registers are rotated back by ``R_k``.  On return
        ``self`` is the register from before the rotations (up to rounding) and ``lam`` holds ``U^dagger lam``: both are
        consumed.  Costs the passes of the forward list.  Returns the complex ``values``."""
        _ket_operand(lam, "lam")
        count, offsets, qubits, letters, cbuf = _flat_terms(rotations)
        thetas = np.ascontiguousarray(cbuf.view(np.complex128).real)
        values = np.zeros(count, dtype=np.complex128)
        _lib.call("qsv_pauli_rotations_adjoint", self._h, lam._h, count, offsets, qubits, letters, _dbl(thetas),
                  _dbl(values.view(np.float64)), None)
        return values

    def energy_and_gradient(self, rotations, terms) -> tuple[float, np.ndarray]:
        """``E = <psi|H|psi>`` for ``psi = U(theta) self`` and ``dE/dtheta_k`` for every rotation of the list, by the
        adjoint method: the rotations forward, ``lambda = H psi`` into a scratch register, ``E = Re <psi|lambda>``, then
        one backward walk (``pauli_rotations_adjoint``) whose values give ``dE/dtheta_k = Im <lambda_k|P_k|psi_k>``.
        About three times the passes of the forward list whatever its length, where the parameter-shift rule runs the
        circuit twice per angle.  ``self`` holds the input state again on return (up to rounding).  ``H`` must be
        hermitian: real coefficients.  Both lists are checked, and the scratch register is allocated, before ``self`` is
        touched: a refused call leaves it bit for bit as it was."""
        terms = _real_terms(terms, "the gradient")
        _check_terms(terms, self.num_qubits)
        rotations = [(float(theta), str(paulis), [int(q) for q in qs]) for theta, paulis, qs in rotations]
        lam = DeviceState.zeros(self.num_qubits, self.device)
        try:
            self.apply_pauli_rotations(rotations)          # refuses a bad rotation before its first launch
            self.apply_pauli_sum(terms, out=lam)
            energy = self.inner(lam).real
            values = self.pauli_rotations_adjoint(rotations, lam)
        finally:
            lam.close()
        return energy, np.ascontiguousarray(values.imag)

    # ---- diagonal operators: one pass each, whatever the diagonal was built from ----------
    def apply_diagonal_phase(self, diag, gamma: float) -> "DeviceState":
        """In place ``exp(-i gamma D) self`` for a ``DiagonalOperator`` of this size on this device."""
        _diagonal_operand(diag)
        _lib.call("qsv_apply_diag_phase", self._h, diag._h, float(gamma))
        return self

    def apply_diagonal_operator(self, diag, out: "DeviceState | None" = None, coeff: complex = 1.0,
                                accumulate: bool = False) -> "DeviceState":
        """``out = coeff D self`` (``out += coeff D self`` with ``accumulate``).  ``out`` is a register on the same
        device, allocated when None; it may be ``self`` when not accumulating (``D psi`` in place).  Returns ``out``."""
        _diagonal_operand(diag)
        if out is None:
            if accumulate:
                raise ValueError("accumulate needs a destination register")
            out = DeviceState.zeros(self.num_qubits, self.device)
        _ket_operand(out, "out")
        coeff = complex(coeff)
        _lib.call("qsv_apply_diag_mul", out._h, self._h, diag._h, coeff.real, coeff.imag, int(bool(accumulate)))
        return out

    def expect_diagonal(self, diag, threshold: float | None = None) -> DiagonalMoments:
        """``(norm2, mean, second_moment, probability_below)`` = ``(sum p_i, sum p_i d_i, sum p_i d_i^2,
        sum_{d_i <= threshold} p_i)`` with ``p_i = |amplitude_i|^2`` in one read pass; without a threshold the last
        entry is 0.  Nothing is divided by the norm."""
        _diagonal_operand(diag)
        out = np.zeros(4, dtype=np.float64)
        thr = None if threshold is None else C.byref(C.c_double(float(threshold)))
        _lib.call("qsv_expect_diag", self._h, diag._h, thr, _dbl(out))
        return DiagonalMoments(*(float(v) for v in out))

    def variance_diagonal(self, diag) -> float:
        """``<D^2> - <D>^2`` on a normalised register, from one ``expect_diagonal`` pass."""
        moments = self.expect_diagonal(diag)
        return moments.second_moment - moments.mean ** 2

    def transition_diagonal(self, diag, ket: "DeviceState") -> complex:
        """``<self| D |ket>``; ``self`` is the bra and ``ket`` may be ``self``.  Read-only."""
        _diagonal_operand(diag)
        _ket_operand(ket, "ket")
        re, im = C.c_double(), C.c_double()
        _lib.call("qsv_diag_transition", self._h, ket._h, diag._h, C.byref(re), C.byref(im))
        return complex(re.value, im.value)

    def diagonal_phase_adjoint(self, diag, lam: "DeviceState", gamma: float) -> complex:
        """``<lam| D |self>``, then ``exp(-i gamma D)`` on ``self`` and on ``lam``, all in one pass
        (``qsv_diag_phase_adjoint``): the step of an adjoint walk over a cost layer (``qaoa.energy_and_gradient``)."""
        _diagonal_operand(diag)
        _ket_operand(lam, "lam")
        re, im = C.c_double(), C.c_double()
        _lib.call("qsv_diag_phase_adjoint", self._h, lam._h, diag._h, float(gamma), C.byref(re), C.byref(im))
        return complex(re.value, im.value)

    def sample(self, shots: int, rng=None) -> np.ndarray:
        """``shots`` computational-basis outcomes drawn from |amplitude|^2 (inverse-CDF on the device; the uniforms
        come from ``rng``, a ``numpy.random.Generator``, default the global ``np.random`` state).  No collapse."""
        u = np.ascontiguousarray(rng.random(shots) if rng is not None else np.random.random_sample(shots))
        out = np.empty(shots, dtype=np.uint64)
        _lib.call("qsv_sample", self._h, int(shots), _ptr(u), out.ctypes.data_as(C.c_void_p))
        return out

    def inner(self, other: "DeviceState") -> complex:
        re, im = C.c_double(), C.c_double()
        _lib.call("qsv_inner", self._h, other._h, C.byref(re), C.byref(im))
        return complex(re.value, im.value)

    # ---- several registers in one pass -----------------------------------
    def lincomb(self, coeffs, sources, beta: complex = 0.0, return_norm2: bool = False):
        """In place ``self = beta self + sum_k coeffs[k] sources[k]`` (``qsv_lincomb``): up to eight sources per pass,
        each read once, ``self`` read only where ``beta != 0`` and written once per pass.  ``self`` may not be among
        the sources (fold its coefficient into ``beta``); with ``beta == 0`` its old contents are never read and it
        takes the sources' size.  Returns ``self``, or ``(self, ||self||^2)`` with ``return_norm2`` -- the norm comes
        out of the last pass, from the values it stores, at the price of one synchronisation."""
        norm2, _ = self._lincomb(coeffs, sources, beta, return_norm2)
        return (self, norm2) if return_norm2 else self

    def _lincomb(self, coeffs, sources, beta: complex = 0.0, want_norm2: bool = False) -> tuple[float | None, int]:
        """``lincomb``; returns (||self||^2 or None, kernel launches)."""
        sources = list(sources)
        cbuf = np.ascontiguousarray(coeffs, dtype=np.complex128).reshape(-1)
        if cbuf.size != len(sources):
            raise ValueError("one coefficient per source register")
        beta = complex(beta)
        handles = (C.c_void_p * max(len(sources), 1))(*[s._h for s in sources])
        norm2, passes = C.c_double(), C.c_uint64()
        _lib.call("qsv_lincomb", self._h, beta.real, beta.imag, len(sources), handles, _dbl(cbuf.view(np.float64)),
                  C.byref(norm2) if want_norm2 else None, C.byref(passes))
        return (norm2.value if want_norm2 else None), passes.value

    def inner_many(self, others) -> np.ndarray:
        """Complex array of ``<others[k]|self>`` (``qsv_inner_many``): ``self`` is read once per eight ``others``, each
        of them once; one synchronisation per call.  ``others[k]`` may be ``self``."""
        return self._inner_many(others)[0]

    def _inner_many(self, others) -> tuple[np.ndarray, int]:
        """``inner_many``; returns (values, kernel launches)."""
        others = list(others)
        handles = (C.c_void_p * max(len(others), 1))(*[o._h for o in others])
        values = np.zeros(len(others), dtype=np.complex128)
        passes = C.c_uint64()
        _lib.call("qsv_inner_many", self._h, len(others), handles, _dbl(values.view(np.float64)), C.byref(passes))
        return values, passes.value

    def ground_state_of(self, terms, **options):
        """Ground state of ``H = sum_t c_t P_t`` by restarted Lanczos started from this register (``krylov.ground_state``;
        holds ``m + 2`` registers of this size).  Returns ``(energy, state, info)``; ``self`` is not changed."""
        from . import krylov
        return krylov.ground_state(terms, self, **options)

    def evolve_krylov(self, terms, t: float, **options) -> dict:
        """In place ``exp(-i t H) self`` without Trotter error (``krylov.evolve_krylov``; holds ``m + 2`` registers of
        this size).  Returns ``info``."""
        from . import krylov
        return krylov.evolve_krylov(self, terms, t, **options)

    # ---- noise (noise.py) ---------------------------------------------------
    def apply_channel(self, channel, qubits, *, u=None, forced=None, rng=None) -> "DeviceState":
        """One quantum-trajectory step of the ``noise.KrausChannel`` on ``qubits``: a Kraus branch taken with its Born
        weight replaces the ket, renormalised.  ``u`` in [0, 1) decides (default: one draw from ``rng``, else from the
        global ``np.random``, where ``M`` draws); ``forced`` names the branch instead.  Weights, choice and update happen
        on the device and nothing is downloaded; ``channel_log()`` tells what was taken."""
        from . import noise
        return noise._apply_to_ket(self, channel, qubits, u=u, forced=forced, rng=rng)

    def channel_log(self) -> tuple[np.ndarray, np.ndarray]:
        """``(branches, probabilities)`` of the ``apply_channel`` calls since the last read, in call order."""
        from . import noise
        return noise._channel_log(self)

    def reduced_density(self, qubits) -> np.ndarray:
        """Reduced density matrix of ``qubits`` (at most six; everything else traced out) as a host
        ``(2^k, 2^k)`` array, ``qubits[0]`` the most significant bit of both indices.  One read pass on the device."""
        qubits = [int(q) for q in qubits]
        if not 1 <= len(qubits) <= 6:
            raise ValueError("keep between 1 and 6 qubits")
        dim = 1 << len(qubits)
        out = np.empty((dim, dim), dtype=np.complex128)
        _lib.call("qsv_reduced_density", self._h, len(qubits), _ints(qubits), _ptr(out))
        return out

    # ---- subsystems (entanglement.py) ---------------------------------------
    def reduced_density_state(self, qubits) -> "DensityState":
        """The reduced state of ``qubits`` (at most 12; everything else traced out) as a ``DensityState`` on this device:
        ``M M^dagger`` on the matrix cores, nothing downloaded.  Bit order as in ``reduced_density``."""
        from . import entanglement
        return entanglement.reduced_density_state(self, qubits)

    def marginal_probabilities(self, qubits) -> np.ndarray:
        """Probabilities of the ``2^k`` outcomes of ``qubits`` (at most 26), ``qubits[0]`` the most significant bit."""
        from . import entanglement
        return entanglement.marginal_probabilities(self, qubits)

    def subsystem_purity(self, qubits) -> float:
        """``tr(rho_A^2)`` of the cut ``qubits | rest``, taken on its smaller side; no spectrum and no download."""
        from . import entanglement
        return entanglement.subsystem_purity(self, qubits)

    def renyi2_entropy(self, qubits, base: float = np.e) -> float:
        """``-log tr(rho_A^2)`` (``subsystem_purity``)."""
        from . import entanglement
        return entanglement.renyi2_entropy(self, qubits, base)

    def schmidt_values(self, qubits) -> np.ndarray:
        """Schmidt coefficients of the cut ``qubits | rest``, descending (``min(k, n - k) <= 12``)."""
        from . import entanglement
        return entanglement.schmidt_values(self, qubits)

    def entanglement_entropy(self, qubits, alpha: float = 1.0, base: float = np.e, *, return_info: bool = False):
        """Entanglement entropy of the cut ``qubits | rest``: von Neumann for ``alpha = 1``, else Renyi.  The cut is taken
        on its smaller side, so any bipartition works while ``min(k, n - k) <= 12``; a wider one raises ``ValueError``."""
        from . import entanglement
        return entanglement.entanglement_entropy(self, qubits, alpha, base, return_info=return_info)

    def mutual_information(self, a, b, base: float = np.e) -> float:
        """``S(A) + S(B) - S(AB)`` for two disjoint qubit sets."""
        from . import entanglement
        return entanglement.mutual_information(self, a, b, base)

    def expect_density(self, rho: "DensityState") -> complex:
        """``<self| rho |self>`` for a density matrix held on the device (the ket / matrix branch of ``npq.fidelity``)."""
        re, im = C.c_double(), C.c_double()
        _lib.call("qsv_expect_density", self._h, rho._h, C.byref(re), C.byref(im))
        return complex(re.value, im.value)

    # ---- timing (HIP events on the register's stream) -----------------------------------------
    def timer_start(self) -> None:
        _lib.call("qsv_timer_start", self._h)

    def timer_stop(self) -> float:
        ms = C.c_float()
        _lib.call("qsv_timer_stop", self._h, C.byref(ms))
        return ms.value


    def flush(self) -> None:
        """Apply the gates the register has queued (QSV_OPT_DEFER); every read-out does this by itself."""
        _lib.call("qsv_flush", self._h)

    def defer_stats(self) -> tuple[int, int]:
        """(gates that went through the deferred queue, launches that applied them)."""
        g, n = C.c_uint64(), C.c_uint64()
        _lib.call("qsv_defer_stats", self._h, C.byref(g), C.byref(n))
        return g.value, n.value

    def last_kernel(self) -> str:
        """Name of the gate kernel the most recent apply launched, as rocprofv3 spells it."""
        buf = C.create_string_buffer(128)
        _lib.call("qsv_last_kernel", self._h, buf, 128)
        return buf.value.decode()

    def event_record(self, slot: int) -> None:
        """Non-blocking HIP event mark number ``slot`` on the register's stream."""
        _lib.call("qsv_event_record", self._h, int(slot))

    def event_elapsed_ms(self, slot_a: int, slot_b: int) -> float:
        ms = C.c_float()
        _lib.call("qsv_event_elapsed_ms", self._h, int(slot_a), int(slot_b), C.byref(ms))
        return ms.value


class DensityState(DeviceState):
    """An n-qubit density matrix in HBM: ``rho`` flattened row-major is a 2n-qubit register whose first n qubits index
    the row and whose last n the column -- the layout ``Gate.apply`` uses for ``U rho U^dagger`` (gates.py:51-52), kept
    on the device between gates.  ``ndim == 2`` like the ndarray it stands for."""

    ndim = 2

    @classmethod
    def from_numpy(cls, rho: np.ndarray, device: int = 0) -> "DensityState":
        rho = np.asarray(rho)
        if rho.ndim != 2 or rho.shape[0] != rho.shape[1]:
            raise ValueError("State has wrong dimensions.")
        flat = DeviceState.from_numpy(np.ascontiguousarray(rho).reshape(-1), device)
        out = cls(flat._h, device=flat.device)
        flat._h = None
        return out

    @classmethod
    def from_ket(cls, ket: np.ndarray, device: int = 0) -> "DensityState":
        ket = np.asarray(ket)
        return cls.from_numpy(np.multiply.outer(ket, ket.conj()), device)

    @property
    def num_qubits(self) -> int:
        return super().num_qubits // 2

    @property
    def shape(self) -> tuple[int, int]:
        dim = 1 << self.num_qubits
        return (dim, dim)

    def to_numpy(self) -> np.ndarray:
        return super().to_numpy().reshape(self.shape)

    def copy(self) -> "DensityState":
        twin = DeviceState.copy(self)
        out = DensityState(twin._h, device=twin.device)
        twin._h = None
        return out

    def apply_matrix(self, matrix: np.ndarray, indices) -> "DensityState":
        """``U rho U^dagger``: ``U`` on the row qubits, ``conj(U)`` on the column qubits."""
        n = self.num_qubits
        indices = [int(i) for i in indices]
        if any(not 0 <= q < n for q in indices):
            raise ValueError(f"qubit index out of range for a {n}-qubit register")
        DeviceState.apply_matrix(self, matrix, indices)
        DeviceState.apply_matrix(self, np.conjugate(matrix), [n + q for q in indices])
        return self

    def apply_sequence(self, indices, sources, matrix) -> "DensityState":
        return self.apply_matrix(matrix, indices)       # U rho U^dagger: both sides, as the dense block

    def apply_pauli_rotations(self, rotations) -> "DensityState":
        """``U rho U^dagger`` for the ordered rotation list: the list on the row qubits, then the same letters on the
        column qubits ``n + q`` with angle ``-(-1)^nY theta`` (``conj(P) = (-1)^nY P``)."""
        n = self.num_qubits
        rotations = [(theta, str(paulis), [int(q) for q in qs]) for theta, paulis, qs in rotations]
        if any(not 0 <= q < n for _, _, qs in rotations for q in qs):
            raise ValueError(f"qubit index out of range for a {n}-qubit register")
        self._pauli_rotations(rotations)
        self._pauli_rotations(rotations, qubit_offset=n, conjugate=True)
        return self

    def apply_qft(self, qubits=None, *, inverse: bool = False, swaps: bool = True) -> "DensityState":
        """``F rho F^dagger``: the transform on the row qubits, its complex conjugate on the column qubits ``n + q``
        (with and without the reversal: ``conj(F)``, not the adjoint)."""
        n = self.num_qubits
        qubits = list(range(n)) if qubits is None else [int(q) for q in qubits]
        if any(not 0 <= q < n for q in qubits):
            raise ValueError(f"qubit index out of range for a {n}-qubit register")
        self._apply_qft(qubits, inverse=inverse, swaps=swaps)
        self._apply_qft(qubits, inverse=inverse, swaps=swaps, qubit_offset=n, conjugate=True)
        return self

    def apply_layer(self, matrices, qubits=None) -> "DensityState":
        """``U rho U^dagger`` for the product ``U`` of the layer: ``matrices[j]`` on the row qubit ``qubits[j]`` and its complex
        conjugate on the column qubit ``n + qubits[j]``, in ONE layer of ``2 k`` stages."""
        from .layers import layer_table
        n = self.num_qubits
        qubits = list(range(n)) if qubits is None else [int(q) for q in qubits]
        if any(not 0 <= q < n for q in qubits):
            raise ValueError(f"qubit index out of range for a {n}-qubit register")
        table = layer_table(matrices, len(qubits))
        self._apply_layer(np.concatenate([table, np.conjugate(table)]), qubits + [n + q for q in qubits])
        return self

    def apply_register_map(self, op, target, source=None, controls=(), *, inverse: bool = False) -> "DensityState":
        """``P rho P^T`` for the permutation matrix ``P`` of the map: the map on the row qubits, then on the column qubits
        ``n + q`` (``P`` is real: there is no conjugate form)."""
        n = self.num_qubits
        listed = [int(q) for group in (target, source or (), controls) for q in group]
        if any(not 0 <= q < n for q in listed):
            raise ValueError(f"qubit index out of range for a {n}-qubit register")
        self._apply_register_map(op, target, source, controls, inverse=inverse)
        self._apply_register_map(op, target, source, controls, inverse=inverse, qubit_offset=n)
        return self

    def apply_pauli_sum(self, terms, out=None, accumulate: bool = False):
        raise ValueError("apply_pauli_sum is not defined for a density register: H rho is out of scope")

    def transition_pauli_sum(self, terms, ket, *, return_terms: bool = False):
        raise ValueError("transition_pauli_sum is not defined for a density register")

    def variance_pauli_sum(self, terms):
        raise ValueError("variance_pauli_sum is not defined for a density register")

    def pauli_rotations_adjoint(self, rotations, lam):
        raise ValueError("pauli_rotations_adjoint is not defined for a density register")

    def layer_adjoint(self, matrices, lam, qubits=None):
        raise ValueError("layer_adjoint is not defined for a density register")

    def layer_transition(self, ket, qubits=None):
        raise ValueError("layer_transition is not defined for a density register")

    def one_qubit_densities(self, qubits=None):
        raise ValueError("one_qubit_densities is not defined for a density register: use reduced_density")

    def energy_and_gradient(self, rotations, terms):
        raise ValueError("energy_and_gradient is not defined for a density register")

    def apply_diagonal_phase(self, diag, gamma):
        raise ValueError("apply_diagonal_phase is not defined for a density register")

    def apply_diagonal_operator(self, diag, out=None, coeff=1.0, accumulate: bool = False):
        raise ValueError("apply_diagonal_operator is not defined for a density register")

    def expect_diagonal(self, diag, threshold=None):
        raise ValueError("expect_diagonal is not defined for a density register")

    def variance_diagonal(self, diag):
        raise ValueError("variance_diagonal is not defined for a density register")

    def transition_diagonal(self, diag, ket):
        raise ValueError("transition_diagonal is not defined for a density register")

    def diagonal_phase_adjoint(self, diag, lam, gamma):
        raise ValueError("diagonal_phase_adjoint is not defined for a density register")

    def ground_state_of(self, terms, **options):
        raise ValueError("ground_state_of is not defined for a density register")

    def evolve_krylov(self, terms, t, **options):
        raise ValueError("evolve_krylov is not defined for a density register")

    def apply_channel(self, channel, qubits) -> "DensityState":
        """``rho <- sum_j K_j rho K_j^dagger`` exactly: one pass with the channel's superoperator on the row and column
        legs of ``qubits``."""
        from . import noise
        return noise._apply_to_density(self, channel, qubits)

    def channel_log(self):
        raise ValueError("channel_log is not defined for a density register: its channels are exact")

    def trace(self) -> float:
        """``tr(rho)``: the all-identity term of ``expect_terms``."""
        return self.expect_terms([(1.0, "", [])]).real

    def expect_terms(self, terms, *, return_terms: bool = False):
        """``tr(H rho)`` for ``H = sum_t c_t P_t``, terms as in ``expect_pauli_sum``: one launch for all terms, one
        workgroup per term reading 2^n of the 4^n entries (``qsv_density_expect_paulis``).  Returns the complex value, or
        ``(value, complex per-term traces in the caller's order)`` with ``return_terms=True``."""
        from . import noise
        return noise._density_terms(self, terms, return_terms)

    def purity(self) -> float:
        """``tr(rho rho)`` for a hermitian ``rho`` (``npq.purity``): the squared norm of the flattened register."""
        return self.norm2()

    def eigenvalues(self) -> np.ndarray:
        """The spectrum of ``rho``, ascending and clipped at 0: ``numpy.linalg.eigvalsh`` on the downloaded matrix.  Not
        a device computation -- 12 qubits cost a 256 MiB download and several seconds on the host."""
        from . import entanglement
        return entanglement.spectrum_of(self.to_numpy())

    def von_neumann_entropy(self, base: float = np.e) -> float:
        """``-tr(rho log rho)`` from ``eigenvalues`` (the same host cost)."""
        from . import entanglement
        return entanglement.entropy_of(self.eigenvalues(), 1.0, base)

    def reduced_density_state(self, qubits):
        raise ValueError("reduced_density_state is not defined for a density register: its partial trace is out of scope")

    def marginal_probabilities(self, qubits):
        raise ValueError("marginal_probabilities is not defined for a density register")

    def fidelity_with_ket(self, ket: DeviceState) -> float:
        return ket.expect_density(self).real


class QuditState:
    """``n_modes`` d-level modes, dense complex128, mode 0 slowest (cv_simulator-style mode indices)."""

    def __init__(self, handle: C.c_void_p, device: int = 0):
        self._h = handle
        self.device = device          # HIP device ordinal the register lives on

    @classmethod
    def zeros(cls, n_modes: int, d: int, device: int = 0) -> "QuditState":
        """All modes in level 0 (vacuum in a Fock basis)."""
        h = C.c_void_p()
        _lib.call("qsv_create_qudit", int(n_modes), int(d), int(device), C.byref(h))
        return cls(h, int(device))

    @classmethod
    def from_numpy(cls, tensor: np.ndarray, device: int = 0) -> "QuditState":
        tensor = np.asarray(tensor)
        d = tensor.shape[0]
        if any(s != d for s in tensor.shape):
            raise ValueError("all modes must share one local dimension")
        st = cls.zeros(tensor.ndim, d, device)
        buf = _cbuf(tensor)
        _lib.call("qsv_upload", st._h, _ptr(buf), 0, buf.size)
        return st

    def close(self) -> None:
        if self._h is not None and self._h.value:
            _lib.load().qsv_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def dims(self) -> tuple[int, int]:
        n, d = C.c_int(), C.c_int()
        _lib.call("qsv_qudit_shape", self._h, C.byref(n), C.byref(d))
        return n.value, d.value

    def to_numpy(self) -> np.ndarray:
        n, d = self.dims
        out = np.empty(d ** n, dtype=np.complex128)
        _lib.call("qsv_download", self._h, _ptr(out), 0, out.size)
        return out.reshape((d,) * n)

    def download(self, offset: int, count: int) -> np.ndarray:
        """``count`` consecutive amplitudes starting at flat index ``offset`` (mode 0 slowest)."""
        out = np.empty(count, dtype=np.complex128)
        _lib.call("qsv_download", self._h, _ptr(out), int(offset), int(count))
        return out

    def fill_random(self, seed: int) -> float:
        """Normalised pseudo-random amplitudes generated on the device (counter-based); returns the raw squared norm."""
        n2 = C.c_double()
        _lib.call("qsv_fill_random", self._h, int(seed), 0, C.byref(n2))
        _lib.call("qsv_scale", self._h, 1.0 / np.sqrt(n2.value), 0.0)
        return n2.value

    def upload(self, tensor: np.ndarray) -> None:
        """Overwrite the register with ``tensor`` (shape ``(d,) * n_modes`` or flat, mode 0 slowest)."""
        n, d = self.dims
        buf = _cbuf(tensor, d ** n)
        _lib.call("qsv_upload", self._h, _ptr(buf), 0, buf.size)

    def sync(self) -> None:
        _lib.call("qsv_sync", self._h)

    def apply_mode(self, matrix, mode: int) -> "QuditState":
        _, d = self.dims
        m = np.asarray(matrix)
        if m.ndim == 1:
            _lib.call("qsv_apply_mode1_diag", self._h, int(mode), _ptr(_cbuf(m, d)))
        else:
            _lib.call("qsv_apply_mode1", self._h, int(mode), _ptr(_cbuf(m, d * d)))
        return self

    def apply_two_mode(self, matrix, mode0: int, mode1: int) -> "QuditState":
        _, d = self.dims
        m = np.asarray(matrix)
        if m.ndim == 1 or m.shape == (d, d):   # diagonal given flat or as the (d, d) plane
            _lib.call("qsv_apply_mode2_diag", self._h, int(mode0), int(mode1), _ptr(_cbuf(m, d * d)))
        else:
            _lib.call("qsv_apply_mode2", self._h, int(mode0), int(mode1), _ptr(_cbuf(m, d ** 4)))
        return self

    def apply_two_mode_gather(self, cols, vals, mode0: int, mode1: int) -> "QuditState":
        """Sparse plane map: ``cols`` / ``vals`` of shape ``(d*d, nnz)`` (negative column = unused slot)."""
        _, d = self.dims
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        vals = _cbuf(vals)
        if cols.ndim != 2 or cols.shape[0] != d * d or vals.size != cols.size:
            raise ValueError("cols and vals must both have shape (d*d, nnz)")
        _lib.call("qsv_apply_mode2_gather", self._h, int(mode0), int(mode1), int(cols.shape[1]),
                  C.c_void_p(cols.ctypes.data), _ptr(vals))
        return self

    def apply_two_mode_blocks(self, blocks, mode0: int, mode1: int) -> "QuditState":
        """Block-diagonal plane operator: ``blocks`` = list of ``(plane_indices, matrix)`` with disjoint index sets
        (``j0 * d + j1`` in (mode0, mode1) order) and a dense ``s x s`` matrix each (s <= 32).  In place."""
        sizes = np.array([len(idx) for idx, _ in blocks], dtype=np.int32)
        indices = np.ascontiguousarray(np.concatenate([np.asarray(idx, dtype=np.int32) for idx, _ in blocks]))
        mats = np.ascontiguousarray(np.concatenate([_cbuf(m, len(idx) ** 2).reshape(-1) for idx, m in blocks]))
        _lib.call("qsv_apply_mode2_blocks", self._h, int(mode0), int(mode1), len(blocks),
                  sizes.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p), _ptr(mats))
        return self

    def marginal(self, mode: int) -> np.ndarray:
        """Sum of |amplitude|^2 over every other mode, per level of ``mode``."""
        _, d = self.dims
        out = np.empty(d, dtype=np.float64)
        _lib.call("qsv_mode_marginal", self._h, int(mode), C.c_void_p(out.ctypes.data))
        return out

    def project(self, mode: int, level: int, scale: float) -> "QuditState":
        """Keep level ``level`` of ``mode`` (times ``scale``) and remove the mode."""
        _lib.call("qsv_mode_project", self._h, int(mode), int(level), float(scale))
        return self

    def insert(self, mode: int, amplitudes) -> "QuditState":
        """New mode with the given ``d`` amplitudes at position ``mode`` (product with the rest)."""
        _, d = self.dims
        _lib.call("qsv_mode_insert", self._h, int(mode), _ptr(_cbuf(amplitudes, d)))
        return self

    def scale(self, factor: complex) -> "QuditState":
        factor = complex(factor)
        _lib.call("qsv_scale", self._h, factor.real, factor.imag)
        return self

    def copy(self) -> "QuditState":
        n, d = self.dims
        other = QuditState.zeros(n, d, self.device)
        _lib.call("qsv_copy", other._h, self._h)
        return other

    def norm2(self) -> float:
        v = C.c_double()
        _lib.call("qsv_norm2", self._h, C.byref(v))
        return v.value

    def timer_start(self) -> None:
        _lib.call("qsv_timer_start", self._h)

    def timer_stop(self) -> float:
        ms = C.c_float()
        _lib.call("qsv_timer_stop", self._h, C.byref(ms))
        return ms.value

    def set_option(self, option: int, value: int) -> None:
        _lib.call("qsv_set_option", self._h, int(option), int(value))

    def last_kernel(self) -> str:
        buf = C.create_string_buffer(128)
        _lib.call("qsv_last_kernel", self._h, buf, 128)
        return buf.value.decode()


def tensor_apply_axis(dev_in: int, dev_out: int, L: int, d_in: int, d_out: int, R: int, matrix, device: int = 0,
                      stream: int = 0) -> None:
    """``out[l, :, r] = M @ in[l, :, r]`` on raw device tensors (an MPS site: L = chi_l, R = chi_r).

    ``matrix`` is a host array (uploaded on every call) or, to keep an operator resident the way the reference's
    gates keep ``self.matrix``, the integer device address of a row-major complex128 ``(d_out, d_in)`` buffer
    (e.g. ``torch_tensor.data_ptr()``): then nothing is copied and the call is asynchronous on ``stream``."""
    if isinstance(matrix, (int, np.integer)):
        _lib.call("qsv_tensor_apply_axis_dev", int(device), C.c_void_p(stream), C.c_void_p(dev_in),
                  C.c_void_p(dev_out), int(L), int(d_in), int(d_out), int(R), C.c_void_p(int(matrix)))
        return
    m = _cbuf(matrix, d_in * d_out)
    _lib.call("qsv_tensor_apply_axis", int(device), C.c_void_p(stream), C.c_void_p(dev_in), C.c_void_p(dev_out),
              int(L), int(d_in), int(d_out), int(R), _ptr(m))
