"""CPU: the exact inverse CDF of basis-state sampling (tests/basis_sample_reference.py) against hand-made cases and against a
search written out in Fractions.  No device is used."""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

import basis_sample_reference as R

BELOW_ONE = float(np.nextafter(1.0, 0.0))


def test_dyadic_weights_by_hand():
    # weights 1/4, 1/4, 1/2 at indices 0, 1, 2: edges 0, 1/4, 1/2, 1
    amps = np.array([0.5, 0.5j, 0.5 + 0.5j])
    cdf = R.ExactCdf(amps)
    assert cdf.support.tolist() == [0, 1, 2]
    assert cdf.edges == [0, Fraction(1, 4), Fraction(1, 2), 1] and cdf.total == 1
    u = [0.0, 0.125, 0.25, float(np.nextafter(0.25, 0.0)), 0.375, 0.5, 0.75, BELOW_ONE]
    answer, bracket, distance = R.exact_inverse_cdf(amps, u)
    assert answer.tolist() == [0, 0, 1, 0, 1, 2, 2, 2]
    #                       edge 0   tie: lower  1/4     1/4     tie: 1/4  1/2     tie: 1/2  1
    assert bracket.tolist() == [[0, 0], [0, 0], [0, 1], [0, 1], [0, 1], [1, 2], [1, 2], [2, 2]]
    assert distance.tolist() == [0.0, 0.125, 0.0, 2.0 ** -55, 0.125, 0.0, 0.25, 2.0 ** -53]


def test_leading_inner_and_trailing_zeros():
    amps = np.zeros(12, dtype=complex)
    amps[[3, 4, 9]] = [1.0, 1.0j, -np.sqrt(2.0)]                  # leading 0..2, inner 5..8, trailing 10..11
    two = Fraction(float(np.sqrt(2.0))) ** 2                      # not 2: the double's own square
    cdf = R.ExactCdf(amps)
    assert cdf.support.tolist() == [3, 4, 9] and cdf.edges == [0, 1, 2, 2 + two]
    assert [cdf.edge_of_index(i) for i in (0, 3, 4, 5, 9, 10, 12)] == [0, 0, 1, 2, 2, 3, 3]
    assert [cdf.bracket(e) for e in range(4)] == [(3, 3), (3, 4), (4, 9), (9, 9)]
    quarter = float(Fraction(1) / (2 + two))                      # fl(edge 1 / total)
    answer, bracket, distance = R.exact_inverse_cdf(cdf, [0.0, quarter / 4, 0.4, 0.6, BELOW_ONE])
    assert answer.tolist() == [3, 3, 4, 9, 9], "never an index of weight zero"
    assert bracket.tolist() == [[3, 3], [3, 3], [4, 9], [4, 9], [9, 9]]
    assert distance[0] == 0.0 and distance[4] == 2.0 ** -53
    assert distance[2] == float(abs(Fraction(0.4) * cdf.total - 2) / cdf.total)


def test_draws_at_an_edge():
    amps = np.zeros(8, dtype=complex)
    amps[[1, 2, 6]] = [0.5, 0.5, np.sqrt(0.5)]
    cdf = R.ExactCdf(amps)
    mid = cdf.draws_at_edge(1)
    assert len(mid) == 5 and mid[2] == float(cdf.edges[1] / cdf.total) and np.all(np.diff(mid) > 0)
    assert mid[1] == np.nextafter(mid[2], 0.0) and mid[4] == np.nextafter(np.nextafter(mid[2], 1.0), 1.0)
    assert cdf.draws_at_edge(0) == [0.0, 5e-324, 1e-323], "nothing below zero"
    assert cdf.draws_at_edge(3) == [float(np.nextafter(BELOW_ONE, 0.0)), BELOW_ONE], "nothing from 1.0 on"
    answer, bracket, distance = R.exact_inverse_cdf(cdf, mid)
    assert set(answer.tolist()) == {1, 2} and bracket.tolist() == [[1, 2]] * 5 and np.all(distance < 2.0 ** -51)


def test_weights_that_underflow_are_outside_the_support():
    amps = np.array([1e-163, 1.0, 3e-163j, 0.0, 1e-160, 2.0])
    assert R.float_weights(amps).tolist()[:4] == [0.0, 1.0, 0.0, 0.0] and 0.0 < R.float_weights(amps)[4] < 1e-319
    cdf = R.ExactCdf(amps)
    assert cdf.support.tolist() == [1, 4, 5]                     # 1e-160 squares to a denormal, not to 0: it stays
    answer, _, _ = R.exact_inverse_cdf(cdf, [0.0, 0.1, 0.2, 0.5, BELOW_ONE])
    assert answer.tolist() == [1, 1, 5, 5, 5]
    with pytest.raises(ValueError):
        R.ExactCdf(np.array([1e-170, 0.0]))
    with pytest.raises(ValueError):
        R.exact_inverse_cdf(amps, [1.0])
    with pytest.raises(ValueError):
        R.exact_inverse_cdf(amps, [-1e-300])


@pytest.mark.parametrize("size, fill, scale", [(2, 1.0, 1.0), (3, 1.0, 1.0), (125, 0.3, 1.0), (700, 0.05, 1e-8), (300, 1.0, 1e8)])
def test_against_a_search_in_fractions(size, fill, scale):
    rng = np.random.default_rng(size)
    amps = (rng.normal(size=size) + 1j * rng.normal(size=size)) * scale * (rng.random(size) < fill)
    amps[int(rng.integers(size))] = scale                        # a support whatever the mask drew
    cdf = R.ExactCdf(amps)
    weights = [Fraction(float(z.real)) ** 2 + Fraction(float(z.imag)) ** 2 for z in amps]
    total = sum(weights)
    assert cdf.total == total and cdf.support.tolist() == [i for i, w in enumerate(weights) if w > 0]
    u = [0.0, BELOW_ONE] + [float(x) for x in rng.random(40)]
    for e in range(0, len(cdf.support) + 1, max(1, len(cdf.support) // 7)):
        u += cdf.draws_at_edge(e)
    answer, bracket, distance = R.exact_inverse_cdf(cdf, u)
    edges, owner, run = [Fraction(0)], [], Fraction(0)           # the CDF written out: owner[k] holds [edges[k], edges[k + 1])
    for i, w in enumerate(weights):
        run += w
        if w > 0:
            edges.append(run)
            owner.append(i)
    for s, draw in enumerate(u):
        target = Fraction(draw) * total
        want = next(owner[k] for k in range(len(owner)) if edges[k + 1] > target)
        assert answer[s] == want and weights[want] > 0
        gaps = [abs(target - e) for e in edges]
        least = min(gaps)
        assert distance[s] == float(least / total)
        nearest = [k for k, g in enumerate(gaps) if g == least]
        assert tuple(bracket[s]) in [cdf.bracket(k) for k in nearest]
