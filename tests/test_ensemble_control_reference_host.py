"""tests/ensemble_control_reference.py pinned on the CPU: against kets the reference simulator's own ``M``, ``Insert`` and
``ClassicalControl`` produced (tests/golden/ensemble_control.npz, written by tests/golden/generate_ensemble_control_golden.py),
the draw stream of a batched run against the serial one, and the seeded inputs of tests/test_gpu_ensemble_control.py against
the branch boundary.

The reference removes a measured qubit.  The relation stated and checked here is
``keep = Insert(q, conj(e_s))(M(q, theta, phi, result=s)(psi))``; both sides are a handful of f64 products of unit-size numbers,
so they agree to ``1e-14 max|psi|``.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

import ensemble_control_reference as E
import noise_reference as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "ensemble_control.npz"
TOL = 1e-14


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as data:
        return {k: data[k] for k in data.files}


def close(a, b, scale):
    err = float(np.max(np.abs(np.asarray(a) - np.asarray(b))))
    assert err <= TOL * scale, (err, TOL * scale)


def insert(removed, q, vec, n):
    """A qubit in ``vec`` put at position ``q`` of an (n-1)-qubit ket: what the reference's ``Insert`` does."""
    t = np.asarray(removed).reshape((2,) * (n - 1))
    t = np.tensordot(t, np.asarray(vec), axes=0)              # the new leg last
    return np.ascontiguousarray(np.moveaxis(t, -1, q)).reshape(-1)


@pytest.mark.parametrize("name", ["general", "mx"])
def test_measure_keep_is_the_references_m_followed_by_insert(golden, name):
    psi, q = golden[f"{name}_in"], int(golden[f"{name}_qubit"])
    theta, phi = golden[f"{name}_angles"]
    e0, e1 = E.eigenvectors(theta, phi)
    close(np.stack([e0, e1]), golden[f"{name}_eigs"], 1.0)
    if name == "general":
        assert np.max(np.abs(e0.imag)) > 0.1                   # complex eigenvectors
    scale = float(np.max(np.abs(psi)))
    for s in (0, 1):
        kept, outcome, p = E.measure_keep(psi, q, e0, e1, 0.0, s)
        assert outcome == s
        close(kept, golden[f"{name}_{s}_kept"], scale / np.sqrt(p))
        # the relation itself, on the reference's arrays: kept = Insert(q, conj(e_s))(removed)
        close(golden[f"{name}_{s}_kept"], insert(golden[f"{name}_{s}_removed"], q, np.conj((e0, e1)[s]), 3), scale / np.sqrt(p))
        assert abs(float(np.linalg.norm(kept)) - 1.0) < 1e-14 * 8
        # reset: the same projection with the qubit left in |0>
        zeroed, _, p_reset = E.measure_keep(psi, q, e0, e1, 0.0, s, True)
        close(zeroed, insert(golden[f"{name}_{s}_removed"], q, np.array([1.0, 0.0]), 3), scale / np.sqrt(p))
        assert p_reset == pytest.approx(p, abs=1e-15)
    # drawn: the first s with w_0 + .. + w_s > u total
    w = E.measure_weights(psi, q, e0, e1)
    edge = float(w[0] / (w[0] + w[1]))
    assert E.measure_keep(psi, q, e0, e1, edge - 1e-6)[1] == 0 and E.measure_keep(psi, q, e0, e1, edge + 1e-6)[1] == 1
    assert E.measure_keep(psi, q, e0, e1, 0.0)[1] == 0 and E.measure_keep(psi, q, e0, e1, np.nextafter(1.0, 0.0))[1] == 1


def test_zero_weight_outcomes_and_norms():
    e0, e1 = E.Z_EIGS
    psi = np.array([0.0, 0.0, 0.6, 0.8j])                      # qubit 0 is certainly 1
    out, s, p = E.measure_keep(psi, 0, e0, e1, 0.0, 0)
    assert s == 0 and p == 0.0 and not np.any(out)             # forced, weight 0: zeroed, probability 0
    out, s, p = E.measure_keep(psi, 0, e0, e1, 0.0)
    assert s == 1 and p == 1.0                                  # rounding leaves none: the last positive one
    close(out, psi, 1.0)
    # a ket that is not normalised keeps its norm: sqrt(total / w_s)
    big = 3.0 * R.random_ket(3, 9)
    for s in (0, 1):
        assert float(np.linalg.norm(E.measure_keep(big, 1, *E.eigenvectors(0.4, 1.3), 0.0, s)[0])) == pytest.approx(3.0, abs=1e-13)


def test_conditional_takes_by_mask_and_leaves_the_rest_alone():
    kets = list(E.member_kets(3, 8, 1))
    words = [0, 1, 2, 3, 1 | 1 << 63, 1 << 63, 5, 7]
    out = E.conditional(kets, words, E.CX, [2, 0], *E.masks([0, 63], [1]))
    for m, (before, after) in enumerate(zip(kets, out)):
        if m == 4:
            close(after, R.apply_op(E.CX, before, [2, 0], 3), 2.0)
            assert np.max(np.abs(after - before)) > 1e-3
        else:
            assert after is before
    every = E.conditional(kets, words, E.H, [1], 0, 0)          # both masks 0: every member
    assert all(np.max(np.abs(a - b)) > 1e-3 for a, b in zip(every, kets))


def test_teleportation_for_all_four_forced_outcome_pairs(golden):
    start, message = golden["teleport_in"], golden["teleport_message"]
    for a in (0, 1):
        for b in (0, 1):
            final, results, branches, probs, _ = E.run_serial(E.teleport_circuit((a, b)), start, 0)
            assert results == [a, b] == list(golden[f"teleport_{a}{b}_results"]) and branches == results
            close(final, golden[f"teleport_{a}{b}_out"], 2.0)      # 1 / sqrt(p) = 2: each outcome pair has probability 1/4
            assert probs[0] == pytest.approx(0.5, abs=1e-15) and probs[1] == pytest.approx(0.5, abs=1e-15)
            # qubit 2 carries the message, qubits 0 and 1 are left in |a b>
            close(final.reshape(2, 2, 2)[a, b], message, 2.0)


def test_repetition_code_cycle_with_positive_and_negative_controls(golden):
    logical = golden["rep_in"]
    close(logical, E.encoded(*E.REPETITION_KET), 1.0)
    seen = set()
    for e in (0, 1, 2, 3):
        circuit = ([("gate", E.X, [e])] if e < 3 else []) + E.repetition_cycle(0.0, 3, reset=False)
        final, results, _, probs, _ = E.run_serial(circuit, logical, e)
        assert results == list(golden[f"rep_{e}_results"]) and probs == [1.0, 1.0]
        close(final, golden[f"rep_{e}_out"], 1.0)
        seen.add(tuple(results))
        # corrected: the data qubits hold the logical state again
        syndrome = results[0] * 2 + results[1]
        assert abs(final[syndrome]) == pytest.approx(0.6, abs=1e-15) and abs(final[0b11100 + syndrome]) == pytest.approx(0.8, abs=1e-15)
        # with reset the syndrome qubits end in |00>
        zeroed = E.run_serial(([("gate", E.X, [e])] if e < 3 else []) + E.repetition_cycle(0.0, 3), logical, e)[0]
        close(zeroed, logical, 1.0)
    assert seen == {(0, 0), (1, 0), (1, 1), (0, 1)}


def test_batched_draws_are_the_serial_stream_with_measurements_interleaved():
    circuit = E.repetition_cycle(E.REPETITION_P)                   # 3 channels, then 2 measurements
    mixed = circuit[:1] + [("measure", E.Z_EIGS, 4, None, False)] + circuit[1:]     # a measurement between the channels
    for circ in (circuit, mixed):
        shots, width = 13, E.n_draws(circ)
        block = E.block_draws(E.REPETITION_SEED, shots, circ)
        rng = np.random.default_rng(E.REPETITION_SEED)
        stream = np.array([[rng.random() for _ in range(width)] for _ in range(shots)])
        assert block.shape == (shots, width) and np.array_equal(block, stream)      # number for number
        ket = E.encoded(*E.REPETITION_KET)
        serial = E.run_shots(circ, ket, shots, E.REPETITION_SEED)
        for batch in (8, 64):
            batched = E.run_shots(circ, ket, shots, E.REPETITION_SEED, batch)
            assert len(batched) == shots
            for one, other in zip(serial, batched):
                assert one[1] == other[1] and one[2] == other[2] and np.array_equal(one[0], other[0])
    # a circuit without measurements: the stream of the channels alone, as before
    channels_only = [step for step in circuit if step[0] != "measure"]
    assert E.n_draws(channels_only) == 3


# ---- the seeded inputs of the GPU tests: no draw within 1e-9 of a branch boundary ---------------------------------------------------
def test_measure_inputs_keep_away_from_the_boundary():
    closest = 1.0
    for n, members, bit, basis in E.measure_cases():
        kets, u, (e0, e1) = E.measure_inputs(n, members, bit, basis)
        q = E.qubit_of(n, bit)
        for m in range(members):
            closest = min(closest, E.boundary_distance(kets[m], q, e0, e1, u[m]))
    print(f"measure inputs: smallest |u - w0/total| = {closest:.3e}")
    assert closest >= E.BOUNDARY


def test_forced_and_flush_inputs_keep_away_from_the_boundary():
    closest = 1.0
    for n in E.FORCED_QUBITS:
        for bit in E.target_bits(n):
            kets, u, forced = E.forced_inputs(n, bit)
            w3, w5 = E.measure_weights(kets[3], E.qubit_of(n, bit), *E.Z_EIGS), E.measure_weights(kets[5], E.qubit_of(n, bit), *E.Z_EIGS)
            assert w3[0] == 0.0 and w3[1] > 0.0 and w5[1] == 0.0 and w5[0] > 0.0 and forced[3] == 0 and forced[5] == 1     # weight exactly 0
            for m in range(E.FORCED_MEMBERS):                    # the test also runs these kets without forcing
                closest = min(closest, E.boundary_distance(kets[m], E.qubit_of(n, bit), *E.Z_EIGS, u[m]))
    kets, u = E.flush_inputs()
    eigs = E.eigenvectors(*E.MEASURE_BASES[1][1:])
    for m in range(E.FLUSH_MEMBERS):
        closest = min(closest, E.boundary_distance(E.flush_prepared(kets[m]), 4, *eigs, u[m]))
    assert closest >= E.BOUNDARY


def test_placement_inputs_keep_away_from_the_boundary():
    e0, e1 = E.eigenvectors(*E.MEASURE_BASES[1][1:])
    closest = 1.0
    for n in E.MEMBER_QUBITS:
        ket, _, u, others, _, us = E.placement_inputs(n)
        for bit in E.target_bits(n):
            q = E.qubit_of(n, bit)
            closest = min(closest, E.boundary_distance(ket, q, e0, e1, u))
            for m in range(64):
                closest = min(closest, E.boundary_distance(others[m], q, e0, e1, us[m]))
    assert closest >= E.BOUNDARY


def test_circuit_inputs_keep_away_from_the_boundary():
    _, kets, draws = E.teleport_inputs()
    closest = min(E.run_with(E.teleport_circuit(), kets[m], E.Fixed(draws[:, m]))[4] for m in range(E.TELEPORT_MEMBERS))
    pairs = {tuple(E.run_with(E.teleport_circuit(), kets[m], E.Fixed(draws[:, m]))[1]) for m in range(E.TELEPORT_MEMBERS)}
    assert pairs == {(0, 0), (0, 1), (1, 0), (1, 1)}            # all four outcome pairs occur
    ket = E.encoded(*E.REPETITION_KET)
    shots = E.run_shots(E.repetition_cycle(E.REPETITION_P), ket, E.REPETITION_SHOTS, E.REPETITION_SEED)
    closest = min([closest] + [shot[4] for shot in shots])
    assert len({tuple(shot[1]) for shot in shots}) == 4        # every syndrome occurs
    kets, draws = E.queue_inputs()
    circuit = E.queue_circuit()
    assert E.n_draws(circuit) == E.QUEUE_STEPS > 256
    closest = min([closest] + [E.run_with(circuit, kets[m], E.Fixed(draws[m]))[4] for m in range(E.QUEUE_MEMBERS)])
    print(f"circuit inputs: smallest distance from a branch boundary = {closest:.3e}")
    assert closest >= E.BOUNDARY
