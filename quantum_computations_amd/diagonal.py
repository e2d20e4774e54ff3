"""Real diagonal operators held on the device: thin Python handle over ``qsv_diag`` (include/qsv.h).

A ``DiagonalOperator`` is ``2^n`` doubles in HBM, indexed exactly like a ``DeviceState`` (qubit 0 = most significant
bit): a classical cost function, an oracle on any marked set, the ZZ part of an Ising or MaxCut Hamiltonian.  It is built
from a NumPy vector or, in one write pass for any number of terms, from a Z-only Pauli sum; ``DeviceState`` takes it in
``apply_diagonal_phase``, ``apply_diagonal_operator``, ``expect_diagonal``, ``variance_diagonal`` and
``transition_diagonal``, each one pass over the register.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def _dbl(buf: np.ndarray):
    return buf.ctypes.data_as(C.POINTER(C.c_double))


def flat_diagonal_terms(terms):
    """``[(coefficient, letters, qubits), ...]`` as ``qsv_diag_set_pauli_sum`` takes it: (count, offsets, qubits,
    letters, float64 coefficients).  ``ValueError`` for a coefficient that is not real or a letter other than I or Z."""
    offsets, qubits, letters, coeffs = [0], [], [], []
    for coefficient, paulis, qs in terms:
        paulis, qs = str(paulis), [int(q) for q in qs]
        if len(paulis) != len(qs):
            raise ValueError("one Pauli letter per qubit")
        if len(paulis) > 64:
            raise ValueError("bad Pauli string length")
        if any(letter not in "IZiz" for letter in paulis):
            raise ValueError("a diagonal operator takes the letters I and Z only")
        coefficient = complex(coefficient)
        if coefficient.imag != 0.0:
            raise ValueError("a diagonal operator needs real coefficients")
        qubits += qs
        letters.append(paulis)
        offsets.append(len(qubits))
        coeffs.append(coefficient.real)
    ints = lambda values: (C.c_int * max(len(values), 1))(*values)
    return len(coeffs), ints(offsets), ints(qubits), "".join(letters).encode(), np.ascontiguousarray(coeffs, dtype=np.float64)


class DiagonalOperator:
    """``2^n`` float64 values in HBM; ``values[i]`` multiplies (or weighs) amplitude ``i`` of an n-qubit register."""

    def __init__(self, handle: C.c_void_p, device: int = 0):
        self._h = handle
        self.device = device

    # ---- construction -------------------------------------------------------------------------
    @classmethod
    def zeros(cls, n_qubits: int, device: int = 0) -> "DiagonalOperator":
        h = C.c_void_p()
        _lib.call("qsv_diag_create", int(n_qubits), int(device), C.byref(h))
        return cls(h, int(device))

    @classmethod
    def from_numpy(cls, values, device: int = 0) -> "DiagonalOperator":
        values = np.asarray(values)
        if values.ndim != 1 or values.size == 0 or values.size & (values.size - 1):
            raise ValueError("a diagonal operator needs a vector of 2^n values")
        if np.iscomplexobj(values):
            raise ValueError("a diagonal operator needs real values")
        out = cls.zeros(values.size.bit_length() - 1, device)
        out.upload(values)
        return out

    @classmethod
    def from_terms(cls, n_qubits: int, terms, device: int = 0) -> "DiagonalOperator":
        """``sum_t c_t P_t`` for Z-only strings ``P_t``; ``terms`` as for ``DeviceState.expect_pauli_sum``.  One write
        pass whatever the number of terms, bit-equal to adding ``c_t * sign`` term by term in float64."""
        flat = flat_diagonal_terms(terms)       # refuses before anything is allocated
        out = cls.zeros(n_qubits, device)
        try:
            out._set_terms(flat, accumulate=False)
        except Exception:
            out.close()
            raise
        return out

    def add_terms(self, terms) -> "DiagonalOperator":
        """``self += sum_t c_t P_t`` in one read-and-write pass."""
        self._set_terms(flat_diagonal_terms(terms), accumulate=True)
        return self

    def _set_terms(self, flat, accumulate: bool) -> int:
        count, offsets, qubits, letters, coeffs = flat
        passes = C.c_uint64()
        _lib.call("qsv_diag_set_pauli_sum", self._h, count, offsets, qubits, letters, _dbl(coeffs), int(bool(accumulate)),
                  C.byref(passes))
        return passes.value

    def close(self) -> None:
        if self._h is not None and self._h.value:
            _lib.load().qsv_diag_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- inspection ---------------------------------------------------------------------------
    @property
    def num_qubits(self) -> int:
        n = C.c_int()
        _lib.call("qsv_diag_num_qubits", self._h, C.byref(n))
        return n.value

    def __len__(self) -> int:
        return 1 << self.num_qubits

    def upload(self, values, offset: int = 0) -> None:
        buf = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        _lib.call("qsv_diag_upload", self._h, _dbl(buf), int(offset), buf.size)

    def download(self, offset: int, count: int) -> np.ndarray:
        out = np.empty(int(count), dtype=np.float64)
        _lib.call("qsv_diag_download", self._h, _dbl(out), int(offset), int(count))
        return out

    def to_numpy(self) -> np.ndarray:
        return self.download(0, len(self))

    def extrema(self) -> tuple[float, int, float, int]:
        """``(min, argmin, max, argmax)`` in one read pass; ties go to the lowest index, as ``numpy.argmin`` does."""
        lo, hi = C.c_double(), C.c_double()
        arg_lo, arg_hi = C.c_uint64(), C.c_uint64()
        _lib.call("qsv_diag_extrema", self._h, C.byref(lo), C.byref(arg_lo), C.byref(hi), C.byref(arg_hi))
        return lo.value, arg_lo.value, hi.value, arg_hi.value

    def set_stream(self, stream: int) -> None:
        _lib.call("qsv_diag_set_stream", self._h, C.c_void_p(stream))

    def set_option(self, option: int, value: int) -> None:
        """Only ``_lib.OPT_GRID_CAP``: the most workgroups the diagonal's own kernels (build, extrema) may launch."""
        _lib.call("qsv_diag_set_option", self._h, int(option), int(value))

    def last_kernel(self) -> str:
        buf = C.create_string_buffer(128)
        _lib.call("qsv_diag_last_kernel", self._h, buf, 128)
        return buf.value.decode()
