"""Per-member measurement, classical bits and feed-forward of a trajectory ensemble on the device
(quantum_computations_amd/ensemble.py, csrc/qsv_ensemble.hip: k_ens_measure_select, k_ens_apply_conditional) against the NumPy
statement in tests/ensemble_control_reference.py, which tests/test_ensemble_control_reference_host.py pins against the reference
simulator's own gates.

Bounds (DESIGN.md sections 21 and 24): a measured member within ``TERM_TOL (2 + 1/p) max|psi_m|`` and its logged probability
within ``TERM_TOL`` -- a measurement is a channel of two operators; a conditional gate within ``TERM_TOL max|psi_m|`` -- at most
four complex products per amplitude; whole circuits within ``CIRCUIT_TOL``.  Every seeded draw is at least 1e-9 away from its
branch boundary (asserted on the CPU by the host test, over exactly the inputs used here), so device and reference take the same
outcome and no case is skipped.

Shapes: members of 1, 2, 3, 5 qubits (no lane form, many members per workgroup, a last unit only partly filled), 6 and 7 (lane
form, members share a workgroup), 8, 9, 10 (the three ways to 256 items per member), 13 with ``QSV_OPT_GRID_CAP = 2`` (units that
loop); each as 1, 2, 8 and 64 members.  What is bit-identical by construction is asserted bit for bit.
"""
from __future__ import annotations

import numpy as np
import pytest

import ensemble_control_reference as E
import noise_reference as R
from quantum_computations_amd import _lib, noise
from quantum_computations_amd.device import DeviceState
from quantum_computations_amd.dv_simulator import gates as G
from quantum_computations_amd.dv_simulator.simulator import ClassicalControl
from quantum_computations_amd.ensemble import TrajectoryEnsemble
from quantum_computations_amd.noise import Channel, KrausChannel, Measure

pytestmark = pytest.mark.gpu

TERM_TOL = 1e-13
CIRCUIT_TOL = 1e-12
SHAPES = E.shapes()
SHAPE_IDS = [f"n{n}x{members}" for n, members in SHAPES]


def maxabs(a):
    return float(np.max(np.abs(a))) if np.size(a) else 0.0


def report(what, err, bound):
    print(f"{what}: {err:.3e} (bound {bound:.3e})")
    assert err <= bound, what


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def make_ensemble(n, members, cap=None):
    ens = TrajectoryEnsemble(DeviceState.zeros(n + members.bit_length() - 1), n)
    assert ens.members == members and ens.member_qubits == n
    cap = E.grid_cap(n) if cap is None else cap
    if cap:
        ens.state.set_option(_lib.OPT_GRID_CAP, cap)
    return ens


def upload(ens, kets):
    ens.state.upload(np.ascontiguousarray(np.asarray(kets).reshape(-1)))


def download(ens):
    return ens.state.to_numpy().reshape(ens.members, -1)


def random_unitary(k, seed):
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.normal(size=(1 << k, 1 << k)) + 1j * rng.normal(size=(1 << k, 1 << k)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def unitary_gate(matrix, qubits):
    return G.Gate(list(qubits), np.asarray(matrix, dtype=np.complex128))


def kl_of(n, bits):
    return sum(1 for b in bits if b < 6) if n >= 6 else 0


def targets_of(n):
    return [(bit,) for bit in E.target_bits(n)] + E.target_pairs(n)


def word_patterns(members):
    """``(name, words, positive bits, negative bits)``"""
    one = np.zeros(members, dtype=np.uint64)
    one[members // 2] = np.uint64(1) << np.uint64(63)
    return [
        ("none", np.zeros(members, dtype=np.uint64), [0], []),
        ("all", np.full(members, (1 << 63) | 1, dtype=np.uint64), [0, 63], []),
        ("alternating", (np.arange(members, dtype=np.uint64) & np.uint64(1)), [0], []),
        ("single", one, [63], []),
        ("random", E.random_words(members, 5), [63], [0]),
        ("random2", E.random_words(members, 6), [0], [63]),
    ]


# ---- 1. conditional gates, bits written directly ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,members", SHAPES, ids=SHAPE_IDS)
def test_conditional_gate_takes_by_mask_and_leaves_the_rest_untouched(n, members):
    ens = make_ensemble(n, members)
    kets = E.member_kets(n, members, 100)
    assert same_bits(ens.bits(), np.zeros(members, dtype=np.uint64))      # zero at creation, made by the first read
    worst, takers_seen = 0.0, 0
    for t, bits in enumerate(targets_of(n)):
        k = len(bits)
        qubits = [E.qubit_of(n, b) for b in bits]
        matrix = random_unitary(k, 300 + t)
        gate = unitary_gate(matrix, qubits)
        upload(ens, kets)
        ens.set_bits(None)
        assert ens.apply_conditional(gate) is ens                         # both masks zero: every member
        assert ens.state.last_kernel() == f"k_ens_apply_conditional<{k}, {kl_of(n, bits)}, true>", ens.state.last_kernel()
        everyone = download(ens)
        want = [R.apply_op(matrix, kets[m], qubits, n) for m in range(members)]
        for m in range(members):
            bound = TERM_TOL * maxabs(kets[m])
            err = maxabs(everyone[m] - want[m])
            assert err <= bound, (n, members, bits, m, err, bound)
            worst = max(worst, err / bound)
        for name, words, positive, negative in word_patterns(members):
            upload(ens, kets)
            ens.set_bits(words)
            ens.apply_conditional(gate, positive, negative)
            got = download(ens)
            all_of, none_of = E.masks(positive, negative)
            for m in range(members):
                if E.takes(int(words[m]), all_of, none_of):
                    assert same_bits(got[m], everyone[m]), (name, bits, m)      # as when every member takes it
                    takers_seen += 1
                else:
                    assert same_bits(got[m], kets[m]), (name, bits, m)          # bit-identical to before
            assert same_bits(ens.bits(), words)                                 # the gate does not write the bits
    assert takers_seen > 0
    assert ens.channel_log()[0].shape[0] == 0                                   # nothing logged
    print(f"n={n} x{members}: worst error / bound of a conditional gate {worst:.3f}")
    ens.close()


def test_conditional_gate_where_a_workgroup_takes_chunks_of_units():
    """1024 members of 10 qubits: 4096 units for a target below bit 6, the smallest register in which a workgroup looks at
    more than one unit per load of the words (chunks of two), and 2048 units, one per workgroup, for a target above."""
    n, members = 10, 1024
    ens = make_ensemble(n, members)
    kets = E.member_kets(n, members, 101)
    index = np.arange(members, dtype=np.uint64)
    patterns = [("alternating", index & np.uint64(1)), ("pairs", (index >> np.uint64(1)) & np.uint64(1)), ("random", E.random_words(members, 8)),
                ("first", (index == 0).astype(np.uint64)), ("none", np.zeros(members, dtype=np.uint64))]
    for t, bits in enumerate([(0,), (9,), (5, 6), (1, 0)]):
        qubits = [E.qubit_of(n, b) for b in bits]
        matrix = random_unitary(len(bits), 400 + t)
        gate = unitary_gate(matrix, qubits)
        upload(ens, kets)
        ens.set_bits(None)
        ens.apply_conditional(gate)
        everyone = download(ens)
        flat = R.apply_op(matrix, kets.reshape(-1), [q + 10 for q in qubits], n + 10).reshape(members, -1)     # the plain gate on the register
        report(f"bits {bits}: every member against the reference", maxabs(everyone - flat) / maxabs(kets), TERM_TOL)
        for name, words in patterns:
            upload(ens, kets)
            ens.set_bits(words)
            ens.apply_conditional(gate, [0])
            got = download(ens)
            taking = (words & np.uint64(1)).astype(bool)
            assert same_bits(got[taking], everyone[taking]) and same_bits(got[~taking], kets[~taking]), (bits, name)
    ens.close()


# ---- 2. measurements, every member a different ket --------------------------------------------------------------------------------
def check_measure(ens, kets, q, eigs, u, forced, reset, bit, what, worst):
    n, members = ens.member_qubits, ens.members
    before_bits = ens.bits()
    upload(ens, kets)
    theta, phi = what
    assert ens.measure(q, theta, phi, u=u, result=forced, reset=reset, bit=bit) is ens
    got = download(ens)
    branches, probs = ens.channel_log()
    words = ens.bits()
    assert branches.shape == (1, members) and np.all(np.isfinite(got)) and np.all(np.isfinite(probs))
    for m in range(members):
        f = None if forced is None else int(forced[m])
        want, s, p = E.measure_keep(kets[m], q, *eigs, u[m], f, reset)
        assert branches[0, m] == s, (n, members, q, m, branches[0, m], s)
        if bit is not None:
            assert (int(words[m]) >> bit) & 1 == s and int(words[m]) & ~(1 << bit) == int(before_bits[m]) & ~(1 << bit)
        else:
            assert words[m] == before_bits[m]
        if p == 0.0:
            assert probs[0, m] == 0.0 and not np.any(got[m]), (n, members, q, m)     # a forced outcome of weight 0
            continue
        bound = TERM_TOL * (2.0 + 1.0 / p) * maxabs(kets[m])
        err = maxabs(got[m] - want)
        assert err <= bound, (n, members, q, m, err, bound)
        assert abs(probs[0, m] - p) <= TERM_TOL, (n, members, q, m, probs[0, m], p)
        worst[0] = max(worst[0], err / bound)
        worst[1] = max(worst[1], abs(probs[0, m] - p))
    return branches[0]


@pytest.mark.parametrize("n,members", SHAPES, ids=SHAPE_IDS)
def test_measure_every_member_a_different_ket(n, members):
    ens = make_ensemble(n, members)
    worst = [0.0, 0.0]
    outcomes = set()
    for bit in E.target_bits(n):
        for basis, (_, theta, phi) in enumerate(E.MEASURE_BASES):
            kets, u, eigs = E.measure_inputs(n, members, bit, basis)
            e_dev = Measure(0, theta, phi).eigenvectors()
            assert maxabs(np.stack(e_dev) - np.stack(eigs)) <= 1e-15
            for reset in (False, True):
                cbit = (7 * bit + 31 * basis + (63 if reset else 0)) % 64
                taken = check_measure(ens, kets, E.qubit_of(n, bit), eigs, u, None, reset, cbit, (theta, phi), worst)
                outcomes |= set(int(s) for s in taken)
                kl = 1 if (n >= 6 and bit < 6) else 0
                assert ens.state.last_kernel() == f"k_ens_channel_apply<1, {kl}, true> after k_ens_measure_select after k_ens_channel_rdm"
    assert members < 8 or outcomes == {0, 1}
    print(f"n={n} x{members}: worst error / bound of a measured member {worst[0]:.3f}, worst probability error {worst[1]:.3e} (bound {TERM_TOL:.0e})")
    ens.close()


@pytest.mark.parametrize("n", E.FORCED_QUBITS)
def test_forced_outcomes_one_of_weight_zero(n):
    members = E.FORCED_MEMBERS
    ens = make_ensemble(n, members)
    worst = [0.0, 0.0]
    for bit in E.target_bits(n):
        q = E.qubit_of(n, bit)
        kets, u, forced = E.forced_inputs(n, bit)          # members 3 and 5 are certain, and forced to the outcome of weight 0
        for reset in (False, True):
            ens.set_bits(np.full(members, 0xffff0000ffff0000, dtype=np.uint64))
            taken = check_measure(ens, kets, q, E.Z_EIGS, u, forced, reset, 5, (0.0, 0.0), worst)
            assert list(taken[1:7]) == [0, 1, 0, 1, 1, 0]
            assert [(int(w) >> 5) & 1 for w in ens.bits()][1:7] == [0, 1, 0, 1, 1, 0]      # the bit is the forced value, weight 0 or not
        # not forced, the same kets and draws: the certain outcome
        taken = check_measure(ens, kets, q, E.Z_EIGS, u, None, False, None, (0.0, 0.0), worst)
        assert taken[3] == 1 and taken[5] == 0
    ens.close()


# ---- 3. placement invariance ---------------------------------------------------------------------------------------------------------
def placed_run(n, position, members, ket, word, u, others, other_words, other_u, bit):
    """Measure (complex basis) then a gate conditioned on the outcome and on bit 0, with the member under test at ``position``."""
    ens = make_ensemble(n, members)
    kets, words, us = others[:members].copy(), other_words[:members].copy(), other_u[:members].copy()
    kets[position], words[position], us[position] = ket, word, u
    upload(ens, kets)
    ens.set_bits(words)
    _, theta, phi = E.MEASURE_BASES[1]
    q = E.qubit_of(n, bit)
    ens.measure(q, theta, phi, u=us, bit=40)
    measured = download(ens)
    ens.apply_conditional(unitary_gate(random_unitary(1, 7), [q]), [0, 40], [])
    pair = E.target_pairs(n)
    if pair:
        ens.apply_conditional(unitary_gate(random_unitary(2, 8), [E.qubit_of(n, b) for b in pair[-1]]), [0], [40])
    final = download(ens)
    branches, probs = ens.channel_log()
    out = (measured, final, ens.bits(), branches[0], probs[0])
    ens.close()
    return out


@pytest.mark.parametrize("n", E.MEMBER_QUBITS)
def test_a_member_gives_the_same_bits_wherever_it_sits(n):
    ket, word, u, others, other_words, other_u = E.placement_inputs(n)
    for bit in E.target_bits(n):
        runs = [(position, placed_run(n, position, members, ket, word, u, others, other_words, other_u, bit)) for position, members in E.PLACEMENTS]
        first_position, first = runs[0]
        for position, run in runs[1:]:
            for a, b in zip(first[:2], run[:2]):
                assert same_bits(a[first_position], b[position]), (n, bit, position)          # amplitudes, after each call
            assert first[2][first_position] == run[2][position]                              # bits
            assert first[3][first_position] == run[3][position]                              # outcome
            assert same_bits(first[4][first_position:first_position + 1], run[4][position:position + 1])     # logged probability
        # changing one member's ket and word leaves every other member bit-identical, for both calls
        position, members = E.PLACEMENTS[-1][0] // 2, 64
        changed = placed_run(n, position, members, ket, word, u, others, other_words, other_u, bit)
        plain = placed_run(n, position, members, others[position], other_words[position], other_u[position], others, other_words, other_u, bit)
        rest = [m for m in range(members) if m != position]
        for a, b in zip(changed, plain):
            assert same_bits(np.asarray(a)[rest], np.asarray(b)[rest]), (n, bit)


# ---- 4. queue and log ------------------------------------------------------------------------------------------------------------------
def test_queued_gates_are_applied_before_a_measurement_and_a_conditional_gate():
    n, members = E.FLUSH_QUBITS, E.FLUSH_MEMBERS
    kets, u = E.flush_inputs()
    _, theta, phi = E.MEASURE_BASES[1]
    eigs = E.eigenvectors(theta, phi)
    gate = random_unitary(2, 32)
    want = []
    for m in range(members):
        psi = kets[m]
        psi = E.flush_prepared(psi)
        psi, s, p = E.measure_keep(psi, 4, *eigs, u[m])
        psi = R.apply_op(E.H, psi, [2], n)
        if s:
            psi = R.apply_op(gate, psi, [9, 1], n)
        want.append((psi, s, p))
    results = []
    for defer in (2, 0):
        ens = make_ensemble(n, members)
        ens.state.set_option(_lib.OPT_DEFER, defer)
        upload(ens, kets)
        for q in (0, 4, 9):
            ens.apply(G.H(q))
        if defer:
            queued, launches = ens.state.defer_stats()
            assert queued >= 3 and launches == 0                           # nothing has run yet
        ens.measure(4, theta, phi, u=u, bit=0)
        if defer:
            launched = ens.state.defer_stats()[1]
            assert launched > 0                                            # the measurement flushed the queue
        ens.apply(G.H(2))
        ens.apply_conditional(unitary_gate(gate, [9, 1]), [0])
        if defer:
            assert ens.state.defer_stats()[1] > launched                  # ... and so did the conditional gate
        got = download(ens)
        branches, _ = ens.channel_log()
        assert list(branches[0]) == [w[1] for w in want]
        for m in range(members):
            assert maxabs(got[m] - want[m][0]) <= (TERM_TOL * (2.0 + 1.0 / want[m][2]) + CIRCUIT_TOL) * maxabs(want[m][0])
        results.append(got)
        ens.close()
    report("deferring against not deferring", maxabs(results[0] - results[1]), CIRCUIT_TOL)


def test_measurements_and_channels_interleaved_keep_call_order_in_the_log():
    kets, draws = E.queue_inputs()
    circuit = E.queue_circuit()
    n, members = E.QUEUE_QUBITS, E.QUEUE_MEMBERS
    want = [E.run_with(circuit, kets[m], E.Fixed(draws[m])) for m in range(members)]
    ens = make_ensemble(n, members)
    upload(ens, kets)
    _, theta, phi = E.MEASURE_BASES[1]
    damping = KrausChannel.amplitude_damping(0.3)
    c = 0
    for step in circuit:
        if step[0] == "measure":
            ens.measure(step[2], theta, phi, u=np.ascontiguousarray(draws[:, c]), reset=step[4], bit=c % 64)
            c += 1
        elif step[0] == "channel":
            ens.apply_channel(damping, step[2], u=np.ascontiguousarray(draws[:, c]))
            c += 1
        else:
            ens.apply(unitary_gate(step[1], step[2]))
    assert c == E.QUEUE_STEPS > 256
    branches, probs = ens.channel_log()
    assert branches.shape == (E.QUEUE_STEPS, members)
    assert np.array_equal(branches, np.array([w[2] for w in want], dtype=np.int32).T)        # call order, channels and measurements
    report("logged probabilities over 300 steps", maxabs(probs - np.array([w[3] for w in want]).T), CIRCUIT_TOL)
    got = download(ens)
    report("kets after 300 steps", max(maxabs(got[m] - want[m][0]) / maxabs(want[m][0]) for m in range(members)), CIRCUIT_TOL)
    assert ens.channel_log()[0].shape == (0, members)
    ens.close()


# ---- 5. circuits: teleportation -----------------------------------------------------------------------------------------------------------
def test_teleportation_of_64_different_messages():
    msg, kets, draws = E.teleport_inputs()
    members = E.TELEPORT_MEMBERS
    want = [E.run_with(E.teleport_circuit(), kets[m], E.Fixed(draws[:, m])) for m in range(members)]
    ens = make_ensemble(3, members)
    upload(ens, kets)
    circuit = [G.H(1), G.CX(1, 2), G.CX(0, 1), G.H(0), Measure(0), Measure(1), ClassicalControl(G.X(2), [1]), ClassicalControl(G.Z(2), [0])]
    us = iter(draws)
    for gate in circuit:
        ens.apply(gate, u=next(us)) if isinstance(gate, Measure) else ens.apply(gate)
    got = download(ens)
    outcomes = ens.outcomes(2)
    assert outcomes.dtype == np.int8 and outcomes.shape == (members, 2)
    assert [list(o) for o in outcomes] == [w[1] for w in want]                       # the reference's outcomes under the same draws
    assert {tuple(o) for o in outcomes} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    branches, _ = ens.channel_log()
    assert np.array_equal(branches.T, outcomes)
    worst = 0.0
    for m in range(members):
        a, b = outcomes[m]
        received = got[m].reshape(2, 2, 2)[a, b]
        worst = max(worst, abs(abs(np.vdot(msg[m], received)) ** 2 - 1.0), maxabs(got[m] - want[m][0]))
    report("teleportation: fidelity of qubit 2 with the message, and the kets", worst, CIRCUIT_TOL)
    # reset() clears the bits and the count of measurements
    ens.channel_log()
    ens.reset(kets[0])
    assert not np.any(ens.bits()) and ens._measured == []
    ens.close()


# ---- 6. the repetition code through run_trajectories -------------------------------------------------------------------------------------
def repetition_gates():
    flip = KrausChannel.bit_flip(E.REPETITION_P)
    return [Channel(flip, [q]) for q in range(3)] + [G.CX(0, 3), G.CX(1, 3), G.CX(1, 4), G.CX(2, 4), Measure(3, reset=True), Measure(4, reset=True),
                                                      ClassicalControl(G.X(0), [0], [1]), ClassicalControl(G.X(1), [0, 1], []), ClassicalControl(G.X(2), [1], [0])]


def test_repetition_code_cycles_take_the_reference_branches():
    ket = E.encoded(*E.REPETITION_KET)
    ref_circuit = E.repetition_cycle(E.REPETITION_P)
    shots = E.REPETITION_SHOTS
    ref = E.run_shots(ref_circuit, ket, shots, E.REPETITION_SEED, 64)
    ref_values = np.array([R.expect_terms_ket(E.REPETITION_TERMS, shot[0], 5) for shot in ref])
    runs = {}
    for batch in (64, 256):
        out = noise.run_trajectories(repetition_gates(), ket, shots, terms=E.REPETITION_TERMS, seed=E.REPETITION_SEED, batch=batch)
        assert len(out["results"]) == shots and all(r.dtype == np.int8 for r in out["results"])
        assert [list(r) for r in out["results"]] == [shot[1] for shot in ref]          # the reference's outcomes
        assert [list(b) for b in out["branches"]] == [shot[2][:3] for shot in ref]     # ... and the branches of its three channels
        report(f"batch={batch}: shot values against the reference", maxabs(out["values"] - ref_values), CIRCUIT_TOL)
        runs[batch] = out
    assert np.array_equal(runs[64]["values"], runs[256]["values"])                      # bit for bit
    assert all(np.array_equal(a, b) for a, b in zip(runs[64]["results"], runs[256]["results"]))
    assert len({tuple(r) for r in runs[64]["results"]}) == 4                             # every syndrome occurs
    serial = noise.run_trajectories(repetition_gates(), ket, shots, terms=E.REPETITION_TERMS, seed=E.REPETITION_SEED)
    assert [list(r) for r in serial["results"]] == [shot[1] for shot in ref]
    assert [list(b) for b in serial["branches"]] == [shot[2][:3] for shot in ref]
    report("serial against batched values", maxabs(serial["values"] - runs[64]["values"]), CIRCUIT_TOL)
    # a last chunk with surplus members: 13 = 8 + 5
    part = noise.run_trajectories(repetition_gates(), ket, 13, terms=E.REPETITION_TERMS, seed=E.REPETITION_SEED, batch=8)
    part_ref = E.run_shots(ref_circuit, ket, 13, E.REPETITION_SEED, 8)
    assert len(part["results"]) == 13 and [list(r) for r in part["results"]] == [shot[1] for shot in part_ref]
    report("13 shots in chunks of 8", maxabs(part["values"] - np.array([R.expect_terms_ket(E.REPETITION_TERMS, shot[0], 5) for shot in part_ref])), CIRCUIT_TOL)


def test_measure_as_a_gate_of_the_circuit_runner():
    """``Measure.apply`` on a register and on a NumPy ket returns ``(state, outcome)``; ``Simulator.run`` and ``ClassicalControl``
    work with it unchanged."""
    from quantum_computations_amd.dv_simulator.simulator import Simulator
    msg, kets, _ = E.teleport_inputs()
    for a in (0, 1):
        for b in (0, 1):
            circuit = [G.H(1), G.CX(1, 2), G.CX(0, 1), G.H(0), Measure(0, result=a), Measure(1, result=b),
                       ClassicalControl(G.X(2), [1]), ClassicalControl(G.Z(2), [0])]
            sim = Simulator(circuit)
            final = sim.run(kets[5])
            assert sim.results == [a, b]
            want = E.run_serial(E.teleport_circuit((a, b)), kets[5], 0)[0]
            report(f"Simulator.run with Measure, outcomes {a}{b}", maxabs(final - want), CIRCUIT_TOL)
    rng = np.random.default_rng(4)
    out, s = Measure(1, 1.1, 0.7, rng=rng).apply(kets[7])
    u = float(np.random.default_rng(4).random())
    want, s_ref, _ = E.measure_keep(kets[7], 1, *E.eigenvectors(1.1, 0.7), u)
    assert s == s_ref
    report("Measure.apply on a NumPy ket", maxabs(out - want), CIRCUIT_TOL)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_reach_python():
    n, members = 3, 4
    ens = make_ensemble(n, members)
    kets = E.member_kets(n, members, 3)
    upload(ens, kets)
    before = download(ens)
    with pytest.raises(ValueError):
        ens.apply(G.MZ(0))                                                   # the removing M stays refused
    with pytest.raises(ValueError):
        ens.apply(ClassicalControl(Channel(KrausChannel.bit_flip(0.1), [0]), [0]))      # a control around a channel
    with pytest.raises(ValueError):
        ens.apply(ClassicalControl(Measure(0), []))
    with pytest.raises(ValueError):
        ens.apply(ClassicalControl(G.X(0), [0]))                             # no measurement yet
    with pytest.raises(ValueError):
        ens.measure(n, u=np.zeros(members))
    with pytest.raises(ValueError):
        ens.measure(0, u=np.array([0.0, 0.5, 1.0, 0.1]))
    with pytest.raises(ValueError):
        ens.measure(0, u=np.zeros(members), result=[0, 2, -1, 0])
    with pytest.raises(ValueError):
        ens.measure(0, u=np.zeros(members), bit=64)
    with pytest.raises(ValueError):
        ens.apply_conditional(G.X(0), [3], [3])                              # a bit asked to be set and clear
    with pytest.raises(ValueError):
        ens.apply_conditional(G.X(n))
    with pytest.raises(ValueError):
        ens.set_bits(np.zeros(members + 1, dtype=np.uint64))
    assert same_bits(download(ens), before) and ens.channel_log()[0].shape == (0, members) and not np.any(ens.bits())
    # the 65th automatic bit
    for _ in range(64):
        ens.apply(Measure(0), u=np.full(members, 0.5))
    with pytest.raises(ValueError, match="reuse bits"):
        ens.apply(Measure(0), u=np.full(members, 0.5))
    ens.apply(Measure(0, bit=7), u=np.full(members, 0.5))                    # naming a bit is fine
    assert ens.channel_log()[0].shape == (65, members)
    ens.close()
    ket = E.encoded(*E.REPETITION_KET)
    for batch in (None, 4):
        with pytest.raises(ValueError, match="does not take measurements"):
            noise.run_trajectories([G.H(0), G.MZ(1)], ket, 4, terms=E.REPETITION_TERMS, batch=batch)
    with pytest.raises(ValueError):
        noise.run_density([G.H(0), Measure(1)], ket)
