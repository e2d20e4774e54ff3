"""TEST REFERENCE: the statement of reversible register arithmetic, in Python / NumPy integer arithmetic only.

For every basis index ``i`` of an n-qubit ket (qubit q = bit n-1-q of the index): split ``i`` into the target value ``y``
(first listed qubit most significant), the source value ``x``, the controls and the spectators; where every control is 1
apply the FORWARD map to ``y``; scatter ``out[j(i)] = ket[i]``.  The inverse is stated through the same forward map, as the
gather ``out[i] = ket[j(i)]``.  Nothing here is shared with the product: no import of the package, no modular inverse, no
inverted table.  Also here: the list of maps, the placements (``cases``), the seeded kets and the order-finding statement.

A map is a dict ``{"kind", "m", "mx", "a", "c", "M", "table"}`` with ``M`` spelled out (``2^m`` where the map has no other).
"""
from __future__ import annotations

import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
KINDS = ("add", "multiply", "add_register", "modexp", "xor_lookup", "permutation")
HAS_SOURCE = ("add_register", "modexp", "xor_lookup")
MODULAR = ("add", "multiply", "add_register", "modexp")
SIZES = (3, 5, 7, 13, 14, 18)          # below a wave, either side of the stream threshold (14), many workgroups


def random_ket(n: int, seed: int) -> np.ndarray:
    """Every amplitude non-zero, so the values y >= M are visibly left where they are."""
    rng = np.random.default_rng(seed)
    ket = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return ket / np.linalg.norm(ket)


_KETS: dict[int, np.ndarray] = {}


def ket_of(n: int) -> np.ndarray:
    """One ket per size, shared by every test and never written to."""
    if n not in _KETS:
        _KETS[n] = random_ket(n, 2600 + n)
        _KETS[n].setflags(write=False)
    return _KETS[n]


# ---- the forward map on integers -------------------------------------------------------------------------------------
def forward_value(spec: dict, y: int, x: int = 0) -> int:
    """Python integers: nothing overflows, whatever the widths."""
    kind, M = spec["kind"], spec["M"]
    if kind in MODULAR and y >= M:
        return y
    if kind == "add":
        return (y + spec["c"]) % M
    if kind == "multiply":
        return (spec["a"] * y) % M
    if kind == "add_register":
        return (y + spec["a"] * x + spec["c"]) % M
    if kind == "modexp":
        return (y * pow(spec["a"], x, M)) % M
    if kind == "xor_lookup":
        return y ^ int(spec["table"][x])
    return int(spec["table"][y])


def forward_values(spec: dict, y: np.ndarray, x: np.ndarray) -> np.ndarray:
    """The same on int64 arrays; the widths of the test maps keep every product below 2^62."""
    kind, M = spec["kind"], spec["M"]
    assert spec["m"] + max(spec["mx"], spec["m"]) <= 60
    if kind == "add":
        out = (y + spec["c"]) % M
    elif kind == "multiply":
        out = (spec["a"] * y) % M
    elif kind == "add_register":
        out = (y + (spec["a"] * x) % M + spec["c"]) % M
    elif kind == "modexp":
        powers = np.array([pow(spec["a"], k, M) for k in range(1 << spec["mx"])], dtype=np.int64)
        out = (y * powers[x]) % M
    elif kind == "xor_lookup":
        return y ^ np.asarray(spec["table"], dtype=np.int64)[x]
    else:
        return np.asarray(spec["table"], dtype=np.int64)[y]
    return np.where(y < M, out, y)


def operand(index: np.ndarray, n: int, qubits) -> np.ndarray:
    value = np.zeros_like(index)
    for r, q in enumerate(qubits):
        value |= ((index >> (n - 1 - q)) & 1) << (len(qubits) - 1 - r)
    return value


def destination(n: int, spec: dict, target, source=(), controls=()) -> np.ndarray:
    """``j(i)`` for every basis index: where the forward map sends amplitude ``i``."""
    index = np.arange(1 << n, dtype=np.int64)
    y, x = operand(index, n, target), operand(index, n, source)
    active = np.ones(1 << n, dtype=bool)
    for q in controls:
        active &= ((index >> (n - 1 - q)) & 1) == 1
    new = np.where(active, forward_values(spec, y, x), y)
    out = index.copy()
    for r, q in enumerate(target):
        bit = n - 1 - q
        out &= ~(np.int64(1) << bit)
        out |= ((new >> (len(target) - 1 - r)) & 1) << bit
    return out


def statement(ket: np.ndarray, spec: dict, target, source=(), controls=(), inverse: bool = False) -> np.ndarray:
    n = ket.size.bit_length() - 1
    j = destination(n, spec, target, source, controls)
    if inverse:
        return ket[j]
    out = np.empty_like(ket)
    out[j] = ket
    return out


def is_identity(spec: dict) -> bool:
    return all(forward_value(spec, y, x) == y for x in range(1 << spec["mx"]) for y in range(1 << spec["m"]))


# ---- the maps and where they are placed --------------------------------------------------------------------------------
def make_spec(kind: str, m: int, mx: int, M: int, rng: np.random.Generator) -> dict:
    spec = {"kind": kind, "m": m, "mx": mx if kind in HAS_SOURCE else 0, "a": 0, "c": 0, "M": M if kind in MODULAR else 1 << m, "table": None}
    M = spec["M"]
    if kind in ("add", "add_register"):
        spec["c"] = int(rng.integers(1, M))
    if kind in ("multiply", "modexp", "add_register"):
        units = [a for a in range(2, M) if math.gcd(a, M) == 1] or [1]
        spec["a"] = int(units[int(rng.integers(len(units)))])
    if kind == "xor_lookup":
        spec["table"] = [int(v) for v in rng.integers(0, 1 << m, size=1 << spec["mx"])]
    if kind == "permutation":
        spec["table"] = [int(v) for v in rng.permutation(1 << m)]
    return spec


def moduli(m: int) -> list[int]:
    """2^m, an odd modulus, 2^m - 1 and 2 (fewer where they coincide)."""
    full = 1 << m
    odd = full - 3 if m >= 3 else 3
    return [M for M in dict.fromkeys([full, odd, full - 1, 2]) if 2 <= M <= full]


PLACEMENTS = ("high", "low0", "low1", "low2", "low3", "scattered", "reversed", "one_bit", "whole")


def target_bits(n: int, m: int, placement: str, rng: np.random.Generator):
    """Index bits of the target, most significant value bit first; None where the placement does not fit."""
    if placement == "whole":
        return list(range(n - 1, -1, -1))
    if placement == "one_bit":
        return [int(rng.integers(n))]
    if placement == "high":
        return list(range(n - 1, n - 1 - m, -1))
    if placement.startswith("low"):
        t0 = int(placement[3:])
        return list(range(t0 + m - 1, t0 - 1, -1)) if t0 + m <= n else None
    if placement == "reversed":
        return list(range(1, 1 + m)) if 1 + m <= n else None
    if 2 * m > n:
        return None
    return [int(b) for b in rng.permutation(np.arange(1, 2 * m, 2))]       # scattered: every other bit, in any order


def cases() -> list[dict]:
    """Every GPU case: ``{"id", "n", "spec", "target", "source", "controls"}`` with qubit lists.  All placements for every kind
    at n = 7 and 14, a rotating third of them at 13 and 18, what fits at 3 and 5."""
    rng = np.random.default_rng(26)
    out = []
    for n in SIZES:
        m0 = {3: 1, 5: 2, 7: 3}.get(n, 4)
        mx0 = {3: 1, 5: 2, 7: 2}.get(n, 3)
        for k, kind in enumerate(KINDS):
            for p, placement in enumerate(PLACEMENTS):
                if n in (13, 18) and (p + k) % 3:
                    continue
                if placement == "whole" and kind in HAS_SOURCE:
                    continue
                m = n if placement == "whole" else 1 if placement == "one_bit" else m0
                tbits = target_bits(n, m, placement, rng)
                if tbits is None:
                    continue
                free = [b for b in range(n) if b not in tbits]
                mx = min(mx0, len(free)) if kind in HAS_SOURCE else 0
                if kind in HAS_SOURCE and mx == 0:
                    continue
                sbits = (free[:mx] if (p + k) % 2 else free[-mx:])[::-1] if mx else []        # low bits / high bits
                free = [b for b in free if b not in sbits]
                n_controls = min((p + k) % 3, len(free))
                cbits = free[:n_controls]                                                   # bit 0 first where it is free
                Ms = moduli(m)
                M = Ms[(p + k) % len(Ms)]
                spec = make_spec(kind, m, mx, M, rng)
                name = f"n{n}-{kind}-{placement}-M{spec['M']}-s{'lo' if (p + k) % 2 else 'hi'}{mx}-c{n_controls}"
                out.append({"id": name, "n": n, "spec": spec, "placement": placement, "tbits": tbits, "sbits": sbits, "cbits": cbits,
                            "target": [n - 1 - b for b in tbits], "source": [n - 1 - b for b in sbits],
                            "controls": [n - 1 - b for b in cbits]})
    return out


# ---- order finding -----------------------------------------------------------------------------------------------------
def modexp_ket(a: int, N: int, t: int) -> np.ndarray:
    """``2^(-t/2) sum_x |x>|a^x mod N>``: counting qubits first, then a work register of ``N.bit_length()`` qubits."""
    m = N.bit_length()
    psi = np.zeros((1 << t, 1 << m), dtype=np.complex128)
    psi[np.arange(1 << t), [pow(a, x, N) for x in range(1 << t)]] = 2.0 ** (-t / 2)
    return psi.reshape(-1)


def order_finding_statement(a: int, N: int, t: int) -> np.ndarray:
    """... followed by the inverse Fourier transform of the counting register (``numpy.fft.fft(norm="ortho")``: the
    transform of ``qft_reference`` is ``ifft``)."""
    psi = modexp_ket(a, N, t).reshape(1 << t, -1)
    return np.fft.fft(psi, axis=0, norm="ortho").reshape(-1)
