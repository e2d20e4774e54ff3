"""The NumPy reference of trajectory ensembles (ensemble_reference.py) against the serial reference (noise_reference.py): no GPU."""
from __future__ import annotations

import numpy as np

import ensemble_reference as E
import noise_reference as R

AD = [np.array([[1, 0], [0, np.sqrt(0.85)]], dtype=np.complex128), np.array([[0, np.sqrt(0.15)], [0, 0]], dtype=np.complex128)]
H = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2.0)
CX = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]], dtype=np.complex128)
CIRCUIT = [("gate", H, [0]), ("channel", AD, [0]), ("gate", CX, [0, 1]), ("channel", R.random_kraus(4, 3, 5), [1, 2]),
           ("gate", H, [2]), ("channel", AD, [2]), ("channel", R.random_kraus(2, 4, 6), [1])]
TERMS = [(1.0, "ZZ", [0, 1]), (0.5, "X", [2]), (-0.75, "ZY", [2, 0])]


def test_block_draw_equals_scalar_draws():
    for seed in (0, 7, 2024):
        for shots, channels in ((1, 1), (5, 3), (2000, 12), (3, 0)):
            block = E.block_draws(seed, shots, channels)
            rng = np.random.default_rng(seed)
            scalars = np.array([[float(rng.random()) for _ in range(channels)] for _ in range(shots)]).reshape(shots, channels)
            assert block.shape == (shots, channels)
            assert np.array_equal(block, scalars)


def test_batched_reference_run_equals_serial_runs_bit_for_bit():
    n, shots, seed = 3, 37, 11
    ket = R.random_ket(n, 4)
    rng = np.random.default_rng(seed)
    serial = [R.run_trajectory(CIRCUIT, ket, n, rng) for _ in range(shots)]
    serial_values = np.array([R.expect_terms_ket(TERMS, final, n) for final, _, _, _ in serial])
    assert len({tuple(b) for _, b, _, _ in serial}) > 4                    # the shots do differ
    for batch in (1, 8, 64):                                                # 37 = 4 x 8 + 5: a last chunk with surplus members
        finals, branches, values, closest = E.run_batched(CIRCUIT, ket, n, shots, seed, batch, TERMS)
        assert len(finals) == shots and len(branches) == shots
        for s in range(shots):
            assert branches[s] == serial[s][1], (batch, s)
            assert np.array_equal(finals[s], serial[s][0]), (batch, s)
        assert np.array_equal(values, serial_values)
        assert closest == min(near for _, _, _, near in serial)


def test_surplus_members_do_not_disturb_the_others():
    n = 3
    kets = [R.random_ket(n, 20 + m) for m in range(4)]
    u = np.array([0.1, 0.7, 0.4, 0.95])
    full, b_full, p_full = E.ensemble_step(AD, kets, [1], n, u)
    # the same first three members next to a different fourth, and alone
    other, b_other, p_other = E.ensemble_step(AD, kets[:3] + [np.zeros(1 << n, dtype=np.complex128)], [1], n, np.array([0.1, 0.7, 0.4, 0.0]))
    alone, b_alone, p_alone = E.ensemble_step(AD, kets[:3], [1], n, u[:3])
    for m in range(3):
        assert np.array_equal(full[m], other[m]) and np.array_equal(full[m], alone[m])
    assert np.array_equal(b_full[:3], b_other[:3]) and np.array_equal(b_full[:3], b_alone)
    assert np.array_equal(p_full[:3], p_other[:3]) and np.array_equal(p_full[:3], p_alone)
    assert np.all(other[3] == 0.0) and p_other[3] == 0.0 and np.all(np.isfinite(other[3]))
    # forced branches member by member, -1 = draw
    forced, b_forced, _ = E.ensemble_step(AD, kets, [1], n, u, forced=[1, -1, 0, -1])
    assert list(b_forced) == [1, b_full[1], 0, b_full[3]]
    assert np.array_equal(forced[1], full[1]) and np.array_equal(forced[3], full[3])
