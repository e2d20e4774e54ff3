"""TEST INFRASTRUCTURE: the exact inverse CDF of basis-state sampling (tests/test_basis_sample_reference_host.py pins it on
the CPU; tests/test_gpu_sample_edges.py compares ``qsv_sample`` against it).

Everything is exact rational arithmetic: an amplitude's weight is ``Fraction(re)**2 + Fraction(im)**2``, the CDF is the
running sum of those Fractions over the support, and a draw's target is ``Fraction(u) * total``.  Dense and sparse
registers go the same way (no ``math.fsum``, no ``np.longdouble``): the weights of doubles are dyadic rationals, so the
whole CDF fits integers over one power-of-two denominator, and those integers are what the search compares.  A
correctly rounded float copy of the CDF only proposes where to look; the integers decide.

The SUPPORT is the set of indices whose weight is positive as the register holds it, ``re * re + im * im > 0`` in
float64.  An amplitude so small that its square underflows to exactly 0 is not in it: a sampler that works in float64
cannot tell it from a zero, and it must not return it.  What such amplitudes would add to the exact CDF is below
2^-1073 each.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np


def float_weights(amplitudes) -> np.ndarray:
    """``re * re + im * im`` in float64, per amplitude: what the test calls a possible outcome is ``> 0`` here."""
    a = np.asarray(amplitudes, dtype=np.complex128).reshape(-1)
    return a.real * a.real + a.imag * a.imag


class ExactCdf:
    """``support[k]``: the k-th index of positive weight.  ``edges[k]``: the exact sum of the weights of
    ``support[:k]``, so ``edges[0] = 0``, ``edges[m] = total``, and support[k] owns the targets in [edges[k], edges[k+1])."""

    def __init__(self, amplitudes):
        a = np.asarray(amplitudes, dtype=np.complex128).reshape(-1)
        self.size = a.shape[0]
        self.support = np.flatnonzero(float_weights(a) > 0.0)
        if self.support.size == 0:
            raise ValueError("a register of zero norm has no distribution")
        self.weights = [Fraction(float(a[i].real)) ** 2 + Fraction(float(a[i].imag)) ** 2 for i in self.support]
        self.edges = [Fraction(0)]
        for w in self.weights:
            self.edges.append(self.edges[-1] + w)
        self.total = self.edges[-1]
        # the same numbers as integers over one denominator (all denominators are powers of two: the largest is it)
        self._den = max(e.denominator for e in self.edges)
        self._int = [e.numerator * (self._den // e.denominator) for e in self.edges]
        self.edges_float = np.array([float(e / self.total) for e in self.edges])     # edge / total, correctly rounded

    def edge_of_index(self, index: int) -> int:
        """The number of the CDF edge at the START of amplitude ``index``: how many support points lie below it.  The
        upper edge of a chunk that ends before amplitude ``stop`` is ``edge_of_index(stop)``."""
        return int(np.searchsorted(self.support, index, side="left"))

    def bracket(self, edge: int) -> tuple[int, int]:
        """The support indices below and above edge number ``edge``; the register's two ends have one neighbour only."""
        m = len(self.support)
        return int(self.support[max(edge - 1, 0)]), int(self.support[min(edge, m - 1)])

    def draws_at_edge(self, edge: int) -> list[float]:
        """``fl(E / total)`` and its two float64 neighbours on either side, those of them that are draws: in [0, 1)."""
        mid = float(self.edges_float[edge])
        down1, up1 = np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf)
        five = [np.nextafter(down1, -np.inf), down1, mid, up1, np.nextafter(up1, np.inf)]
        return [float(x) for x in five if 0.0 <= x < 1.0]


def exact_inverse_cdf(amplitudes, u):
    """For every draw ``u[s]`` in [0, 1), with target ``Fraction(u[s]) * total``:

    ``answer[s]``    the smallest index whose CDF exceeds the target (always in the support);
    ``bracket[s]``   the two support indices on either side of the CDF edge nearest to the target;
    ``distance[s]``  |target - that edge| / total, rounded to float64 once at the end.

    ``amplitudes`` may be an ``ExactCdf`` already built from them."""
    cdf = amplitudes if isinstance(amplitudes, ExactCdf) else ExactCdf(amplitudes)
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    if not np.all((u >= 0.0) & (u < 1.0)):
        raise ValueError("uniform draws must lie in [0, 1)")
    m, ints, den, total = len(cdf.support), cdf._int, cdf._den, cdf._int[-1]
    guess = np.clip(np.searchsorted(cdf.edges_float, u, side="right"), 1, m)
    answer = np.empty(u.shape[0], dtype=np.int64)
    bracket = np.empty((u.shape[0], 2), dtype=np.int64)
    distance = np.empty(u.shape[0], dtype=np.float64)
    for s in range(u.shape[0]):
        num, uden = float(u[s]).as_integer_ratio()
        target = num * total                      # over the denominator uden * den; an edge e is ints[e] * uden over it
        j = int(guess[s])                         # want edges[j - 1] <= target < edges[j]
        while ints[j] * uden <= target:
            j += 1
        while ints[j - 1] * uden > target:
            j -= 1
        answer[s] = cdf.support[j - 1]
        below, above = target - ints[j - 1] * uden, ints[j] * uden - target
        edge, gap = (j - 1, below) if below <= above else (j, above)
        bracket[s] = cdf.bracket(edge)
        distance[s] = float(Fraction(gap, total * uden))
    return answer, bracket, distance
