"""Reversible register arithmetic: classical maps on the value of a qubit register (``qsv_arith``, include/qsv.h, DESIGN.md
section 26).

A ``RegisterMap`` acts on the integer ``y`` that ``m`` *target* qubits spell (the first listed qubit the most significant,
as in ``apply_qft``), may read the integer ``x`` of ``mx`` *source* qubits, and acts only where every control qubit is 1.
``M`` is the modulus (``None``: ``2^m``); values ``y >= M`` stay where they are, which makes the modular maps permutations:

===============  ======================================  =====================
constructor      forward map                             limits
===============  ======================================  =====================
``add``          ``y -> (y + c) mod M``                  ``m <= 32``
``multiply``     ``y -> (a y) mod M``, gcd(a, M) = 1     ``m <= 32``
``add_register`` ``y -> (y + a x + c) mod M``            ``m, mx <= 32``
``modexp``       ``y -> (y a^x) mod M``, gcd(a, M) = 1   ``m <= 32, mx <= 24``
``xor_lookup``   ``y -> y xor T[x]``                     ``m <= 32, mx <= 24``
``permutation``  ``y -> T[y]``, ``T`` a bijection        ``m <= 24``
===============  ======================================  =====================

On a state vector such a map is a permutation of amplitudes: ``DeviceState.apply_register_map`` is ONE gather pass over the
register, bit-exact.  The map object holds the parameters on the host; the device handle (both the map and its inverse) is
made on first use, one per device, and shared with ``inverse()``.  ``distributed.ShardedState`` is out of scope.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib

ADD, MUL, ADD_REG, MUL_POW, XOR_LOOKUP, PERMUTE = range(6)
KIND_NAMES = ("add", "multiply", "add_register", "modexp", "xor_lookup", "permutation")
MAX_BITS, MAX_TABLE_BITS = 32, 24


class _Handles(dict):
    """device -> ``qsv_arith*``; shared by a map and every ``inverse()`` made from it, freed with the last of them."""

    def close(self) -> None:
        while self:
            _, h = self.popitem()
            _lib.call("qsv_arith_destroy", h)

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown: the library may be gone already
            pass


class RegisterMap:
    """One of the maps of the module's table; make it with the class methods."""

    def __init__(self, kind: int, m: int, mx: int = 0, a: int = 0, c: int = 0, modulus: int | None = None, table=None, *,
                 _inverse: bool = False, _shared: "_Handles | None" = None):
        kind, m, mx, a, c = int(kind), int(m), int(mx), int(a), int(c)
        if kind not in range(6):
            raise ValueError("unknown kind of register map")
        if not 1 <= m <= (MAX_TABLE_BITS if kind == PERMUTE else MAX_BITS):
            raise ValueError("target width m out of range")
        if kind in (ADD_REG, MUL_POW, XOR_LOOKUP):
            if not 1 <= mx <= (MAX_BITS if kind == ADD_REG else MAX_TABLE_BITS):
                raise ValueError("source width mx out of range")
        elif mx != 0:
            raise ValueError("this kind of map reads no source register")
        M = 1 << m if modulus in (None, 0) else int(modulus)
        if not 2 <= M <= 1 << m:
            raise ValueError("modulus must be in 2 .. 2^m")
        if kind in (XOR_LOOKUP, PERMUTE) and M != 1 << m:
            raise ValueError("this kind of map has no modulus")
        if not 0 <= a < M or not 0 <= c < M:
            raise ValueError("a and c must be below the modulus")
        if kind in (MUL, MUL_POW) and math.gcd(a, M) != 1:
            raise ValueError("multiplier a must be coprime to the modulus")
        if kind in (XOR_LOOKUP, PERMUTE):
            table = np.array(table, dtype=np.uint64).reshape(-1)
            if table.size != 1 << (m if kind == PERMUTE else mx):
                raise ValueError("wrong table length")
            if table.size and int(table.max()) >= 1 << m:
                raise ValueError("table entry out of range")
            if kind == PERMUTE and np.unique(table).size != table.size:
                raise ValueError("the table is not a bijection")
        elif table is not None:
            raise ValueError("this kind of map takes no table")
        self.kind, self.m, self.mx, self.a, self.c, self.modulus, self.table = kind, m, mx, a, c, M, table
        self.inverted = bool(_inverse)
        self._shared = _Handles() if _shared is None else _shared

    # ---- constructors -----------------------------------------------------------------------------
    @classmethod
    def add(cls, m: int, c: int, modulus: int | None = None) -> "RegisterMap":
        return cls(ADD, m, c=c, modulus=modulus)

    @classmethod
    def multiply(cls, m: int, a: int, modulus: int | None = None) -> "RegisterMap":
        return cls(MUL, m, a=a, modulus=modulus)

    @classmethod
    def add_register(cls, m: int, mx: int, a: int = 1, c: int = 0, modulus: int | None = None) -> "RegisterMap":
        return cls(ADD_REG, m, mx, a=a, c=c, modulus=modulus)

    @classmethod
    def modexp(cls, m: int, mx: int, a: int, modulus: int | None = None) -> "RegisterMap":
        return cls(MUL_POW, m, mx, a=a, modulus=modulus)

    @classmethod
    def xor_lookup(cls, m: int, mx: int, table) -> "RegisterMap":
        """``table``: ``2^mx`` values below ``2^m``, or a callable evaluated on ``range(2**mx)``."""
        if callable(table):
            table = [int(table(x)) for x in range(1 << int(mx))]
        return cls(XOR_LOOKUP, m, mx, table=table)

    @classmethod
    def permutation(cls, m: int, table) -> "RegisterMap":
        return cls(PERMUTE, m, table=table)

    # ---- host side -----------------------------------------------------------------------------------
    def inverse(self) -> "RegisterMap":
        """The inverse map; it shares this map's device handles (which hold both directions)."""
        return RegisterMap(self.kind, self.m, self.mx, self.a, self.c, self.modulus, self.table, _inverse=not self.inverted,
                           _shared=self._shared)

    def index_map(self) -> np.ndarray:
        """The map as integers, host only: ``out[x, y]`` = the value ``y`` becomes when the source reads ``x`` (one row
        when the map reads no source).  Python integers underneath, so nothing overflows."""
        M, size = self.modulus, 1 << self.m
        out = np.empty((1 << self.mx, size), dtype=np.int64)
        for x in range(1 << self.mx):
            for y in range(size):
                out[x, y] = self._value(y, x)
        return out

    def _value(self, y: int, x: int) -> int:
        M, inv = self.modulus, self.inverted
        if self.kind in (ADD, ADD_REG):
            s = self.c + self.a * x
            return y if y >= M else (y - s if inv else y + s) % M
        if self.kind in (MUL, MUL_POW):
            f = pow(self.a, x if self.kind == MUL_POW else 1, M)
            return y if y >= M else y * (pow(f, -1, M) if inv else f) % M
        if self.kind == XOR_LOOKUP:
            return y ^ int(self.table[x])
        if inv:
            return int(np.flatnonzero(self.table == y)[0])
        return int(self.table[y])

    def __repr__(self):
        bits = f"m={self.m}" + (f", mx={self.mx}" if self.mx else "")
        params = {ADD: f", c={self.c}", MUL: f", a={self.a}", ADD_REG: f", a={self.a}, c={self.c}", MUL_POW: f", a={self.a}"}.get(self.kind, "")
        mod = f", M={self.modulus}" if self.modulus != 1 << self.m else ""
        return f"RegisterMap.{KIND_NAMES[self.kind]}({bits}{params}{mod})" + ("^-1" if self.inverted else "")

    # ---- device side ---------------------------------------------------------------------------------
    def _handle(self, device: int) -> C.c_void_p:
        handles = self._shared
        if device not in handles:
            h = C.c_void_p()
            if self.table is None:
                table, length = None, 0
            else:
                buf = np.ascontiguousarray(self.table, dtype=np.uint64)
                table, length = buf.ctypes.data_as(C.POINTER(C.c_uint64)), buf.size
            modular = self.kind not in (XOR_LOOKUP, PERMUTE)
            _lib.call("qsv_arith_create", self.kind, self.m, self.mx, self.a, self.c, self.modulus if modular else 0, table, length,
                      int(device), C.byref(h))
            handles[device] = h
        return handles[device]

    def close(self) -> None:
        """Free the device handles (of this map and of every ``inverse()`` made from it)."""
        self._shared.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
