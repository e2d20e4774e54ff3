"""TEST HELPER: the quantum Fourier transform stated in NumPy, and a NumPy executor of the pass records of
``csrc/qsv_qft_plan.h`` as ``tests/layout/qft_plan_driver.cpp`` prints them.

The statement is ``numpy.fft`` along the flattened legs of the chosen qubits (``qubits[0]`` the most significant): the forward
transform is ``F[y, x] = 2^(-m/2) exp(+2 pi i x y / 2^m)`` = ``ifft(norm="ortho")``.  Without swaps the rows come out
bit-reversed (forward) or go in bit-reversed (adjoint); ``conjugate`` is the elementwise conjugate of the operator.
"""
from __future__ import annotations

import numpy as np

EPS = np.finfo(np.float64).eps
INVERSE, NO_SWAPS, CONJUGATE = 1, 2, 4
ALL_FLAGS = list(range(8))

# (n, qubits) of the parity table of tests/test_gpu_qft.py; the plan tests walk the same shapes
SCATTERED_14 = [13, 0, 7, 3, 9, 1, 12, 5]
CUT_18 = [17 - b for b in (17, 3, 12, 9, 0, 15, 7, 10, 5, 14, 2, 8, 16, 4)]   # 9 index bits >= 6; the cut falls after bit 5
SHAPES = [
    (1, [0]), (2, [1, 0]), (5, list(range(5))), (11, [10, 2, 7, 0, 5, 9, 3]),     # the small-register kernel
    (12, list(range(12))), (13, list(range(13))), (14, [13, 12, 11, 10, 9, 8]), (14, [0, 1, 2]), (14, SCATTERED_14),
    (18, CUT_18), (16, list(range(16))), (20, list(range(20))),
]


def flags_of(inverse: bool = False, swaps: bool = True, conjugate: bool = False) -> int:
    return (INVERSE if inverse else 0) | (0 if swaps else NO_SWAPS) | (CONJUGATE if conjugate else 0)


def greedy_counts(n: int, bits, flags: int) -> list[int]:
    """Stages per pass, the planner's rule restated: consecutive ranks, in the order they are applied, while at most six
    distinct index bits >= 6 are among them.  ``bits[r]`` = index bit of the transform's qubit r."""
    order = list(bits)[::-1] if flags & INVERSE else list(bits)
    counts, high = [], set()
    for b in order:
        if not counts or (b >= 6 and len(high | {b}) > 6):
            counts.append(0)
            high = set()
        if b >= 6:
            high.add(b)
        counts[-1] += 1
    return counts


def launches(n: int, qubits, flags: int) -> int:
    """Tile passes plus the permutation, for qubit labels (qubit q = index bit n - 1 - q)."""
    swaps = not flags & NO_SWAPS and len(qubits) >= 2
    return len(greedy_counts(n, [n - 1 - q for q in qubits], flags)) + (1 if swaps else 0)


def random_ket(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    ket = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return ket / np.linalg.norm(ket)


def _reverse_legs(rows: np.ndarray, m: int) -> np.ndarray:
    """Row y of the result is row bit-reverse(y) of ``rows`` (2^m x anything)."""
    t = rows.reshape((2,) * m + (-1,))
    return np.ascontiguousarray(t.transpose(list(range(m))[::-1] + [m])).reshape(rows.shape)


def qft_statement(ket: np.ndarray, qubits, flags: int = 0) -> np.ndarray:
    """The transform of ``qsv_apply_qft`` on a ket of ``log2(len(ket))`` qubits, by ``numpy.fft``."""
    ket = np.asarray(ket, dtype=np.complex128)
    n, qubits = int(ket.size).bit_length() - 1, [int(q) for q in qubits]
    m = len(qubits)
    if m == 0:
        return ket.copy()
    if flags & CONJUGATE:
        return qft_statement(ket.conj(), qubits, flags & ~CONJUGATE).conj()
    rows = np.moveaxis(ket.reshape((2,) * n), qubits, range(m)).reshape(1 << m, -1)
    if flags & INVERSE:
        if flags & NO_SWAPS:
            rows = _reverse_legs(rows, m)
        rows = np.fft.fft(rows, axis=0, norm="ortho")
    else:
        rows = np.fft.ifft(rows, axis=0, norm="ortho")
        if flags & NO_SWAPS:
            rows = _reverse_legs(rows, m)
    out = np.moveaxis(rows.reshape((2,) * m + (2,) * (n - m)), range(m), qubits)
    return np.ascontiguousarray(out).reshape(-1)


def reverse_qubits(ket: np.ndarray, qubits) -> np.ndarray:
    """The reversal of the order of ``qubits`` as an axis permutation."""
    n, m = int(ket.size).bit_length() - 1, len(qubits)
    axes = list(range(n))
    for r in range(m):
        axes[qubits[r]] = qubits[m - 1 - r]
    return np.ascontiguousarray(ket.reshape((2,) * n).transpose(axes)).reshape(-1)


# ---- the driver's records -----------------------------------------------------------------------------------------------
def request(n: int, bits, flags: int, indices=()) -> str:
    return " ".join(str(v) for v in [n, flags, len(bits), *bits, len(indices), *indices])


def parse_plan(line: str, n_indices: int = 0) -> list[dict]:
    """The passes of one answer line of ``qft_plan_driver``."""
    tokens = iter(line.split())
    take = lambda: next(tokens)                                                       # noqa: E731
    passes = []
    for _ in range(int(take())):
        p = {"tile_bits": int(take()), "n_stages": int(take()), "twiddle_first": int(take()), "conj_twiddle": int(take()),
             "scale": float.fromhex(take())}
        p["pos"] = [int(take()) for _ in range(p["tile_bits"])]
        p["stages"] = []
        for _ in range(p["n_stages"]):
            s = {"rank": int(take()), "tile_index": int(take()), "L": int(take()), "run": int(take()), "reg": int(take())}
            s["later"] = [(int(take()), int(take()), int(take())) for _ in range(int(take()))]   # (in tile, index, shift)
            p["stages"].append(s)
        p["runs"] = []
        for _ in range(int(take())):
            first, count = int(take()), int(take())
            p["runs"].append({"first": first, "count": count, "q": [int(take()) for _ in range(min(4, p["tile_bits"]))]})
        p["turns"] = [[int(take()) for _ in range(p["n_stages"])] for _ in range(n_indices)]
        passes.append(p)
    assert next(tokens, None) is None
    return passes


def run_plan(ket: np.ndarray, passes: list[dict]) -> np.ndarray:
    """Apply printed pass records to a ket: what k_qft_tile does to every tile, on the whole register at once."""
    psi = np.array(ket, dtype=np.complex128)
    index = np.arange(psi.size, dtype=np.int64)
    for p in passes:
        for s in p["stages"]:
            bit = p["pos"][s["tile_index"]]
            turns = np.zeros(psi.size, dtype=np.int64)
            for in_tile, where, shift in s["later"]:
                turns |= ((index >> (p["pos"][where] if in_tile else where)) & 1) << shift
            t = np.exp((-2j if p["conj_twiddle"] else 2j) * np.pi * turns / float(1 << s["L"]))
            lo = index[(index >> bit) & 1 == 0]
            hi = lo | (1 << bit)
            a, b = psi[lo], psi[hi]
            if p["twiddle_first"]:
                b = b * t[lo]
                psi[lo], psi[hi] = a + b, a - b
            else:
                psi[lo], psi[hi] = a + b, (a - b) * t[lo]
        psi *= p["scale"]
    return psi


def run_plan_with_swaps(ket: np.ndarray, qubits, flags: int, passes: list[dict]) -> np.ndarray:
    psi = np.asarray(ket)
    swaps = not flags & NO_SWAPS and len(qubits) >= 2
    if swaps and flags & INVERSE:
        psi = reverse_qubits(psi, qubits)
    psi = run_plan(psi, passes)
    if swaps and not flags & INVERSE:
        psi = reverse_qubits(psi, qubits)
    return psi
