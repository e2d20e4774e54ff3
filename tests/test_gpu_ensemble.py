"""Trajectory ensembles on the device (quantum_computations_amd/ensemble.py, csrc/qsv_ensemble.hip) against the NumPy reference.

Every member of an ensemble is compared with ``noise_reference`` on its own ket and its own draw, with the bounds of
test_gpu_noise.py: a member's new ket within ``TERM_TOL (2 + 1/p) max|psi|``, its logged probability within ``TERM_TOL``.
Draws sit at the midpoints of branch intervals and the reference asserts, before the device is touched, that none is within
1e-9 of a boundary, so device and reference must take the same branch.  Sizes are chosen so that every kernel form occurs:
members of 1 to 3 qubits (many members per workgroup, sums by butterfly), 7 to 9 (one or two waves, or a whole workgroup, per
member; lane bits), 13 and 14 with ``QSV_OPT_GRID_CAP = 2`` (parts that loop), each as 1, 2, 8 and 64 members -- fewer where
the register would pass 2^18 amplitudes, which no test here does.

What is bit-identical by construction is asserted bit for bit: a member's results wherever it sits and whoever its
neighbours are, and two runs of the same call.
"""
from __future__ import annotations

import numpy as np
import pytest

import ensemble_reference as E
import noise_reference as R
from quantum_computations_amd import _lib, noise
from quantum_computations_amd.device import DeviceState
from quantum_computations_amd.dv_simulator import gates as G
from quantum_computations_amd.ensemble import TrajectoryEnsemble
from quantum_computations_amd.noise import Channel, KrausChannel, NoiseModel

pytestmark = pytest.mark.gpu

TERM_TOL = 1e-13
CIRCUIT_TOL = 1e-12
MIN_WEIGHT = 1e-6
LAST_U = float(np.nextafter(1.0, 0.0))
MAX_AMPS = 1 << 18
SIZES = (1, 2, 3, 7, 8, 9, 13, 14)
MEMBERS = (1, 2, 8, 64)

ONE_QUBIT = {
    "amplitude_damping": KrausChannel.amplitude_damping(0.3),
    "random4": KrausChannel(R.random_kraus(2, 4, 41)),
}
TWO_QUBIT = {
    "random3": KrausChannel(R.random_kraus(4, 3, 42)),
}


def maxabs(a):
    return float(np.max(np.abs(a))) if np.size(a) else 0.0


def report(what, err, bound):
    print(f"{what}: {err:.3e} (bound {bound:.3e})")
    assert err <= bound, what


def members_for(n, members):
    return min(members, MAX_AMPS >> n)


def distinct_kets(n, members, seed):
    """Different random kets, not all of norm 1: a call keeps each member's norm."""
    return [(1.0 + 0.35 * (m % 3)) * R.random_ket(n, seed + 17 * m) for m in range(members)]


def make_ensemble(n, members, cap=0):
    assert (members << n) <= MAX_AMPS
    ens = TrajectoryEnsemble(DeviceState.zeros(n + members.bit_length() - 1), n)
    assert ens.members == members and ens.member_qubits == n
    if cap:
        ens.state.set_option(_lib.OPT_GRID_CAP, cap)
    return ens


def upload(ens, kets):
    ens.state.upload(np.concatenate(kets))


def download(ens):
    return ens.state.to_numpy().reshape(ens.members, -1)


def midpoint_draws(ch, kets, qubits, n, shift=0):
    """Member m draws the midpoint of the interval of its (m + shift)-th branch of weight >= MIN_WEIGHT.  Asserted on the
    reference: no draw within 1e-9 of a boundary."""
    u = np.zeros(len(kets))
    for m, psi in enumerate(kets):
        w = R.branch_weights(ch.kraus, psi, qubits, n)
        live = [j for j in range(len(w)) if w[j] / w.sum() >= MIN_WEIGHT]
        lo, hi = R.branch_intervals(w)[live[(m + shift) % len(live)]]
        u[m] = 0.5 * (lo + hi)
        assert R.boundary_distance(w, u[m]) >= 1e-9
    return u


def step_and_compare(ens, kets, ch, qubits, what, worst, *, u, forced=None):
    """Upload the kets, take one member-wise step, compare every member and its log entry with the reference's step."""
    n = ens.member_qubits
    want, want_j, want_p = E.ensemble_step(ch.kraus, kets, qubits, n, u, forced)
    upload(ens, kets)
    assert ens.apply_channel(ch, qubits, u=u, forced=forced) is ens
    assert ens.state.last_kernel().startswith(f"k_ens_channel_apply<{ch.num_qubits}, "), ens.state.last_kernel()
    got = download(ens)
    branches, probs = ens.channel_log()
    assert branches.shape == (1, ens.members) and probs.shape == (1, ens.members)
    assert list(branches[0]) == list(want_j), (what, branches[0], want_j)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(probs))
    for m in range(ens.members):
        p = want_p[m]
        assert p > 0.0, what                                             # zero-weight branches are checked on their own
        bound = TERM_TOL * (2.0 + 1.0 / p) * maxabs(want[m])
        err = maxabs(got[m] - want[m])
        assert err <= bound, (what, m, err, bound)
        assert abs(probs[0, m] - p) <= TERM_TOL, (what, m, probs[0, m], p)
        worst[0] = max(worst[0], err / bound)
        worst[1] = max(worst[1], abs(probs[0, m] - p))
    return branches[0]


# ---- one step, every member different --------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", MEMBERS)
@pytest.mark.parametrize("n", SIZES)
def test_one_step_every_member_different(n, members):
    members = members_for(n, members)
    cap = 2 if n >= 13 else 0
    ens = make_ensemble(n, members, cap)
    kets = distinct_kets(n, members, 1000 * n + members)
    worst = [0.0, 0.0]
    calls = 0
    for bit in sorted({b for b in (0, 5, 6, n - 1) if b < n}):
        for name, ch in ONE_QUBIT.items():
            qubits = [n - 1 - bit]
            u = midpoint_draws(ch, kets, qubits, n, shift=calls)
            taken = step_and_compare(ens, kets, ch, qubits, f"n={n} x{members} bit={bit} {name}", worst, u=u)
            assert members == 1 or len(set(taken)) >= 2                # different branches within one call
            calls += 1
    # both bits below 6, one below and one above, both above; in both orders
    pairs = {(a, b) for a, b in ((0, 1), (2, 5), (5, 6), (0, n - 1), (6, n - 1)) if a != b and 0 <= a < n and 0 <= b < n}
    for a, b in sorted(pairs):
        for bits in ((a, b), (b, a)):
            for name, ch in TWO_QUBIT.items():
                qubits = [n - 1 - bits[0], n - 1 - bits[1]]
                u = midpoint_draws(ch, kets, qubits, n, shift=calls)
                taken = step_and_compare(ens, kets, ch, qubits, f"n={n} x{members} bits={bits} {name}", worst, u=u)
                assert members == 1 or len(set(taken)) >= 2
                calls += 1
    print(f"n={n} x{members}: {calls} calls, worst error / bound {worst[0]:.3f}, worst probability error {worst[1]:.3e} (bound {TERM_TOL:.1e})")
    ens.close()


def test_members_cut_into_several_parts():
    """Members of 16 qubits: the read passes cut a member into eight parts (two at most up to 14 qubits), which the select
    kernel and the per-member sums add in index order."""
    n, members = 16, 4
    ens = make_ensemble(n, members)
    kets = distinct_kets(n, members, 160)
    worst = [0.0, 0.0]
    ch = ONE_QUBIT["random4"]
    for shift, bit in enumerate((0, 6, n - 1)):
        u = midpoint_draws(ch, kets, [n - 1 - bit], n, shift=shift)
        taken = step_and_compare(ens, kets, ch, [n - 1 - bit], f"n=16 bit={bit}", worst, u=u)
        assert len(set(taken)) >= 2
    for bits in ((5, n - 1), (n - 2, 0)):
        qubits = [n - 1 - bits[0], n - 1 - bits[1]]
        step_and_compare(ens, kets, TWO_QUBIT["random3"], qubits, f"n=16 bits={bits}", worst, u=midpoint_draws(TWO_QUBIT["random3"], kets, qubits, n))
    unit = [psi / np.linalg.norm(psi) for psi in kets]
    upload(ens, unit)
    terms = terms_for(n)
    values = ens.expect_pauli_sum(terms)
    norms = ens.norm2()
    for m, psi in enumerate(unit):
        assert abs(values[m] - R.expect_terms_ket(terms, psi, n)) <= TERM_TOL * sum(abs(c) for c, _, _ in terms)
        assert abs(norms[m] - 1.0) <= TERM_TOL
    print(f"n=16 x4: worst error / bound {worst[0]:.3f}, worst probability error {worst[1]:.3e}")
    ens.close()


# ---- forced branches and the edges of the draw ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 3, 7, 9, 13))
def test_forced_branches_and_edges_per_member(n):
    members = 8
    ens = make_ensemble(n, members, 2 if n >= 13 else 0)
    kets = distinct_kets(n, members, 50 + n)
    worst = [0.0, 0.0]
    ad = ONE_QUBIT["amplitude_damping"]
    for name, ch in ONE_QUBIT.items():
        last = len(ch.kraus) - 1
        for q in sorted({0, n - 1}):
            # u = 0 and u just below 1, side by side
            u = np.array([0.0, LAST_U] * (members // 2))
            taken = step_and_compare(ens, kets, ch, [q], f"{name} edges", worst, u=u)
            assert list(taken) == [0, last] * (members // 2)
            # forced per member, -1 = draw
            forced = np.array([(m % (last + 2)) - 1 for m in range(members)], dtype=np.int32)
            drawn = midpoint_draws(ch, kets, [q], n)
            taken = step_and_compare(ens, kets, ch, [q], f"{name} forced", worst, u=drawn, forced=forced)
            assert all(taken[m] == forced[m] for m in range(members) if forced[m] >= 0)
    # a member in |0...0> whose jump is forced: weight exactly 0 -> all zeros, probability 0; its neighbours are unaffected
    zero = np.zeros(1 << n, dtype=np.complex128)
    zero[0] = 1.0
    for q in sorted({0, n - 1}):
        mixed_kets = list(kets)
        mixed_kets[1] = zero
        mixed_kets[6] = zero
        forced = np.full(members, -1, dtype=np.int32)
        forced[1] = 1                                                    # member 6 draws: the jump is never drawn from |0>
        u = midpoint_draws(ad, mixed_kets, [q], n)
        u[6] = LAST_U
        want, want_j, want_p = E.ensemble_step(ad.kraus, mixed_kets, [q], n, u, forced)
        assert want_p[1] == 0.0 and want_j[6] == 0 and want_p[6] == 1.0
        upload(ens, mixed_kets)
        ens.apply_channel(ad, [q], u=u, forced=forced)
        got = download(ens)
        branches, probs = ens.channel_log()
        assert list(branches[0]) == list(want_j)
        assert np.all(got[1] == 0.0) and probs[0, 1] == 0.0
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(probs))
        assert probs[0, 6] == 1.0
        for m in range(members):
            if m != 1:
                assert maxabs(got[m] - want[m]) <= TERM_TOL * (2.0 + 1.0 / want_p[m]) * maxabs(want[m]), (n, q, m)
                assert abs(probs[0, m] - want_p[m]) <= TERM_TOL
    # channels whose branches can have weight exactly 0
    for name, ch in (("amplitude_damping(1)", KrausChannel.amplitude_damping(1.0)), ("reset(1)", KrausChannel.reset(1.0))):
        for q in sorted({0, n - 1}):
            u = midpoint_draws(ch, kets, [q], n, shift=1)
            step_and_compare(ens, kets, ch, [q], name, worst, u=u)
            mixed_kets = [zero] + list(kets[1:])                         # from |0...0> only the no-jump branches have weight
            u = np.array([0.0, 0.3, 0.5, 0.7, 0.9, LAST_U, 0.1, 0.6])
            for m, psi in enumerate(mixed_kets):
                assert R.boundary_distance(R.branch_weights(ch.kraus, psi, [q], n), u[m]) >= 1e-9 or m == 0
            step_and_compare(ens, mixed_kets, ch, [q], name + " with |0>", worst, u=u)
    ens.close()


# ---- placement independence, isolation, determinism ----------------------------------------------------------------------------
PAULI_TERMS = [(1.0, "ZZ", [0, 1]), (-0.5, "Z", [0]), (0.25, "XX", [0, 1]), (0.75, "YY", [0, 1]), (-0.75, "ZY", [1, 0]), (0.3, "", [])]


def terms_for(n):
    """A Z-only group, an XX / YY pair and an odd-Y term; on the last qubits too where there are some."""
    if n == 1:
        return [(1.0, "Z", [0]), (0.5, "X", [0]), (-0.75, "Y", [0]), (0.3, "", [])]
    extra = [(0.6, "ZZ", [0, n - 1]), (0.2, "XY", [n - 1, n - 2]), (-0.4, "YY", [n - 2, n - 1])] if n >= 4 else []
    return PAULI_TERMS + extra


def run_placed(n, members, place, ket, u, fill_seed, cap=0):
    """One general one-qubit step, one two-qubit step (where n allows) and the Pauli values, with (ket, u) at `place`."""
    ens = make_ensemble(n, members, cap)
    kets = distinct_kets(n, members, fill_seed)
    kets[place] = ket
    draws = np.random.default_rng(fill_seed).random((2, members))
    draws[:, place] = u
    upload(ens, kets)
    ens.apply_channel(ONE_QUBIT["random4"], [n - 1], u=draws[0])
    if n >= 2:
        ens.apply_channel(TWO_QUBIT["random3"], [0, n - 1], u=draws[1])
    amps = download(ens)
    values, per_term = ens.expect_pauli_sum(terms_for(n), return_terms=True)
    norms = ens.norm2()
    branches, probs = ens.channel_log()
    ens.close()
    return amps, branches, probs, values, per_term, norms


@pytest.mark.parametrize("n", (1, 3, 7, 8, 9, 12, 16))
def test_a_member_gives_the_same_bits_wherever_it_sits(n):
    ket = 1.3 * R.random_ket(n, 4000 + n)
    u = 0.4375
    alone = run_placed(n, 1, 0, ket, u, 1)
    for members, place in ((8, 5), (64, 63)):
        members = members_for(n, members)                                # n = 16: member 3 of 4, eight parts per member
        place = min(place, members - 1)
        other = run_placed(n, members, place, ket, u, 2 + members)
        assert np.array_equal(alone[0][0], other[0][place])
        for a, b in zip(alone[1:3], other[1:3]):                         # branches and probabilities, [steps, members]
            assert np.array_equal(a[:, 0], b[:, place])
        for a, b in zip(alone[3:], other[3:]):                           # values, per-term values, norms
            assert np.array_equal(a[0], b[place])


@pytest.mark.parametrize("n", (2, 8, 13))
def test_changing_one_member_leaves_the_others_bit_identical(n):
    cap = 2 if n >= 13 else 0
    base = run_placed(n, 8, 3, R.random_ket(n, 1), 0.2, 99, cap)
    changed = run_placed(n, 8, 3, 2.0 * R.random_ket(n, 2), 0.9, 99, cap)
    again = run_placed(n, 8, 3, R.random_ket(n, 1), 0.2, 99, cap)
    keep = [m for m in range(8) if m != 3]
    assert np.array_equal(base[0][keep], changed[0][keep]) and not np.array_equal(base[0][3], changed[0][3])
    for a, b in zip(base[1:3], changed[1:3]):
        assert np.array_equal(a[:, keep], b[:, keep])
    for a, b in zip(base[3:], changed[3:]):
        assert np.array_equal(a[keep], b[keep])
    for a, b in zip(base, again):                                        # two runs of the same calls: bit-equal
        assert np.array_equal(a, b)


# ---- mixed-unitary channels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (2, 8))
def test_mixed_unitary_channels_pick_per_member_without_a_read_pass(n):
    members = 8
    ens = make_ensemble(n, members)
    kets = distinct_kets(n, members, 7)
    worst = [0.0, 0.0]
    pauli = KrausChannel.pauli_channel(0.3, 0.2, 0.1)                    # I 0.4 | X 0.3 | Y 0.2 | Z 0.1
    assert pauli.is_mixed_unitary
    u = np.array([0.2, 0.55, 0.8, 0.95, 0.0, LAST_U, 0.45, 0.75])
    upload(ens, kets)
    taken = step_and_compare(ens, kets, pauli, [n - 1], "pauli channel", worst, u=u)
    assert list(taken) == [0, 1, 2, 3, 0, 3, 1, 2]                       # different Paulis on different members in one call
    assert "k_ens_channel_rdm" not in ens.state.last_kernel() and "k_ens_channel_select" in ens.state.last_kernel()
    upload(ens, kets)
    ens.apply_channel(pauli, [0], u=u)
    _, probs = ens.channel_log()
    report("logged probabilities against p_j", maxabs(probs[0] - np.array([0.4, 0.3, 0.2, 0.1, 0.4, 0.1, 0.3, 0.2])), TERM_TOL)
    dep = KrausChannel.depolarizing(0.3, 2)
    assert dep.is_mixed_unitary
    u = (np.arange(members) + 0.5) / members
    taken = step_and_compare(ens, kets, dep, [0, n - 1], "two-qubit depolarizing", worst, u=u)
    assert len(set(taken)) >= 3
    assert "k_ens_channel_rdm" not in ens.state.last_kernel()
    # a general channel does have one
    step_and_compare(ens, kets, ONE_QUBIT["random4"], [0], "general", worst, u=midpoint_draws(ONE_QUBIT["random4"], kets, [0], n))
    assert "k_ens_channel_rdm" in ens.state.last_kernel()
    ens.close()


# ---- read-outs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", MEMBERS)
@pytest.mark.parametrize("n", SIZES)
def test_norms_and_pauli_sums_per_member(n, members):
    members = members_for(n, members)
    ens = make_ensemble(n, members, 2 if n >= 13 else 0)
    kets = [R.random_ket(n, 300 * n + 7 * m) for m in range(members)]
    upload(ens, kets)
    terms = terms_for(n)
    weight = sum(abs(c) for c, _, _ in terms)
    values, per_term = ens.expect_pauli_sum(terms, return_terms=True)
    assert values.shape == (members,) and per_term.shape == (members, len(terms))
    assert np.array_equal(values, ens.expect_pauli_sum(terms))
    norms = ens.norm2()
    assert norms.shape == (members,)
    worst = 0.0
    for m, psi in enumerate(kets):
        worst = max(worst, abs(values[m] - R.expect_terms_ket(terms, psi, n)))
        for t, (c, letters, qubits) in enumerate(terms):
            assert abs(per_term[m, t] - R.expect_terms_ket([(1.0, letters, qubits)], psi, n)) <= TERM_TOL
        assert abs(norms[m] - np.vdot(psi, psi).real) <= TERM_TOL
    report(f"n={n} x{members} Pauli sums", worst, TERM_TOL * weight)
    scaled = [(1.0 + m % 4) * psi for m, psi in enumerate(kets)]        # norms that differ from member to member
    upload(ens, scaled)
    norms = ens.norm2()
    for m, psi in enumerate(scaled):
        assert abs(norms[m] - np.vdot(psi, psi).real) <= TERM_TOL * np.vdot(psi, psi).real
    ens.close()


# ---- the log -------------------------------------------------------------------------------------------------------------------
def test_log_longer_than_the_device_slots_keeps_call_order():
    n, members, steps = 3, 8, 300
    ens = make_ensemble(n, members)
    upload(ens, distinct_kets(n, members, 5))
    ch = ONE_QUBIT["random4"]
    pattern = np.array([[(3 * i + m) % 4 for m in range(members)] for i in range(steps)], dtype=np.int32)
    for i in range(steps):
        ens.apply_channel(ch, [i % n], u=np.zeros(members), forced=pattern[i])
    branches, probs = ens.channel_log()
    assert branches.shape == (steps, members) and probs.shape == (steps, members)
    assert np.array_equal(branches, pattern)
    assert np.all((probs > 0.0) & (probs < 1.0))
    again, _ = ens.channel_log()
    assert again.shape == (0, members)                                   # read and cleared
    ens.close()


# ---- the deferred queue --------------------------------------------------------------------------------------------------------
def test_queued_gates_are_applied_before_an_ensemble_channel():
    n, members = 10, 8                                                   # a 13-qubit register: deferral can be forced on
    kets = distinct_kets(n, members, 31)
    ch = ONE_QUBIT["random4"]
    h = np.array([[1, 1], [1, -1]]) / np.sqrt(2)
    after_gates = []
    for psi in kets:
        for q in (0, 4, 9):
            psi = R.apply_op(h, psi, [q], n)
        after_gates.append(psi)
    u = midpoint_draws(ch, after_gates, [4], n)
    want, want_j, want_p = E.ensemble_step(ch.kraus, after_gates, [4], n, u)
    results = []
    for defer in (2, 0):
        ens = make_ensemble(n, members)
        ens.state.set_option(_lib.OPT_DEFER, defer)
        upload(ens, kets)
        for q in (0, 4, 9):
            ens.apply(G.H(q))
        queued, launches = ens.state.defer_stats()
        if defer:
            assert queued >= 3 and launches == 0                         # nothing has run yet
        ens.apply_channel(ch, [4], u=u)
        if defer:
            assert ens.state.defer_stats()[1] > 0                        # the call flushed the queue
        got = download(ens)
        branches, probs = ens.channel_log()
        assert list(branches[0]) == list(want_j)
        for m in range(members):
            assert maxabs(got[m] - want[m]) <= (TERM_TOL * (2.0 + 1.0 / want_p[m]) + CIRCUIT_TOL) * maxabs(want[m])
        results.append(got)
        ens.close()
    report("deferring against not deferring", maxabs(results[0] - results[1]), CIRCUIT_TOL)


# ---- whole runs ----------------------------------------------------------------------------------------------------------------
def noisy_circuit(rng=None):
    """4 qubits, 12 gates; amplitude damping after every one-qubit gate, two-qubit depolarising after every CX."""
    circuit = [G.H(0), G.CX(0, 1), G.RZ(1, 0.7), G.H(2), G.CX(2, 3), G.X(3), G.CX(1, 2), G.RZ(2, -1.1), G.H(3), G.CX(3, 0), G.Y(0), G.H(1)]
    model = NoiseModel().add(KrausChannel.amplitude_damping(0.15), after=1).add(KrausChannel.depolarizing(0.1, 2), after=(G.CX,))
    return model.insert(circuit, rng)


def as_reference_circuit(circuit):
    return [("channel", list(g.channel.kraus), list(g.indices)) if isinstance(g, Channel) else ("gate", g.matrix, list(g.indices))
            for g in circuit]


TERMS = [(1.0, "ZZ", [0, 1]), (0.5, "X", [2]), (-0.75, "ZY", [3, 0])]
TRAJECTORY_SEED = 2024
SHOTS = 2000


def test_batched_runs_take_the_reference_branches():
    """The acceptance test: ``run_trajectories(batch=64)`` and ``batch=256`` take exactly the reference's branches, agree with
    its values to ``CIRCUIT_TOL`` and with each other bit for bit, and the serial path agrees with both."""
    n = 4
    ket = R.random_ket(n, 78)
    circuit = noisy_circuit()
    ref_circuit = as_reference_circuit(circuit)
    exact_rho = R.run_exact(ref_circuit, np.outer(ket, ket.conj()), n)
    exact = sum(c * np.trace(R.pauli_matrix(letters, qubits, n) @ exact_rho).real for c, letters, qubits in TERMS)
    _, ref_branches, ref_values, closest = E.run_batched(ref_circuit, ket, n, SHOTS, TRAJECTORY_SEED, 64, TERMS)
    ref_stderr = ref_values.std(ddof=1) / np.sqrt(SHOTS)
    print(f"reference: mean {ref_values.mean():.6f} exact {exact:.6f} stderr {ref_stderr:.2e}, closest draw to a boundary {closest:.2e}")
    assert closest >= 1e-9                                               # the seed's draws stay clear of every boundary
    assert abs(ref_values.mean() - exact) <= 5 * ref_stderr              # the seed passes on the CPU
    runs = {}
    for batch in (64, 256):
        out = noise.run_trajectories(circuit, ket, SHOTS, terms=TERMS, seed=TRAJECTORY_SEED, batch=batch)
        assert len(out["branches"]) == SHOTS and out["values"].shape == (SHOTS,)
        assert [list(b) for b in out["branches"]] == ref_branches        # exactly the reference's branches
        report(f"batch={batch}: shot values against the reference", maxabs(out["values"] - ref_values), CIRCUIT_TOL)
        print(f"batch={batch}: mean {out['mean']:.6f} exact {exact:.6f} stderr {out['stderr']:.2e}")
        assert abs(out["mean"] - exact) <= 5 * out["stderr"]
        runs[batch] = out
    assert np.array_equal(runs[64]["values"], runs[256]["values"])      # placement independence
    serial = noise.run_trajectories(circuit, ket, SHOTS, terms=TERMS, seed=TRAJECTORY_SEED)
    assert [list(b) for b in serial["branches"]] == ref_branches
    report("serial against batched values", maxabs(serial["values"] - runs[64]["values"]), CIRCUIT_TOL)


WIDE_SEED = 11


def wide_circuit():
    """9 qubits: a member spans more than one workgroup.  Lane bits and bits above them, general and mixed-unitary channels."""
    n = 9
    circuit = [G.H(q) for q in range(n)] + [G.CX(q, q + 1) for q in range(0, n - 1, 2)] + [G.RZ(q, 0.3 + 0.1 * q) for q in range(n)] + \
              [G.CX(q, q + 1) for q in range(1, n - 1, 2)] + [G.H(0), G.H(8)]
    model = NoiseModel().add(KrausChannel.generalized_amplitude_damping(0.2, 0.3), after=1).add(KrausChannel.depolarizing(0.15, 2), after=(G.CX,))
    out = model.insert(circuit)
    out.append(Channel(TWO_QUBIT["random3"], [0, 8]))
    out.append(Channel(TWO_QUBIT["random3"], [7, 1]))
    return out


def test_a_wider_batched_run():
    n, shots, batch = 9, 32, 8
    ket = R.random_ket(n, 90)
    circuit = wide_circuit()
    ref_circuit = as_reference_circuit(circuit)
    terms = [(1.0, "ZZ", [0, 8]), (0.5, "X", [4]), (-0.75, "ZY", [7, 2]), (0.4, "XX", [1, 2]), (0.4, "YY", [1, 2])]
    _, ref_branches, ref_values, closest = E.run_batched(ref_circuit, ket, n, shots, WIDE_SEED, batch, terms)
    print(f"closest draw to a boundary {closest:.2e}")
    assert closest >= 1e-9
    assert len({tuple(b) for b in ref_branches}) > shots // 2
    out = noise.run_trajectories(circuit, ket, shots, terms=terms, seed=WIDE_SEED, batch=batch)
    assert [list(b) for b in out["branches"]] == ref_branches
    report("9 qubits, batch=8: shot values against the reference", maxabs(out["values"] - ref_values), CIRCUIT_TOL)
    # a last chunk with surplus members: 13 = 8 + 5
    part = noise.run_trajectories(circuit, ket, 13, terms=terms, seed=WIDE_SEED, batch=batch)
    _, part_branches, part_values, near = E.run_batched(ref_circuit, ket, n, 13, WIDE_SEED, batch, terms)
    assert near >= 1e-9
    assert [list(b) for b in part["branches"]] == part_branches and len(part["branches"]) == 13
    report("13 shots in chunks of 8", maxabs(part["values"] - part_values), CIRCUIT_TOL)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_reach_python():
    n, members = 3, 4
    ens = make_ensemble(n, members)
    upload(ens, distinct_kets(n, members, 3))
    before = download(ens)
    ad = ONE_QUBIT["amplitude_damping"]
    with pytest.raises(ValueError):
        ens.apply(G.H(n))                                                # a member bit of the register
    with pytest.raises(ValueError):
        ens.apply(G.CX(0, n + 1))
    with pytest.raises(ValueError):
        ens.apply_channel(ad, [n], u=np.zeros(members))
    with pytest.raises(ValueError):
        ens.apply_channel(ad, [0], u=np.array([0.0, 0.5, 1.0, 0.1]))     # a draw outside [0, 1)
    with pytest.raises(ValueError):
        ens.apply_channel(ad, [0], u=np.zeros(members), forced=[0, 2, -1, 0])
    with pytest.raises(ValueError):
        ens.apply_channel(ad, [0], u=np.zeros(members - 1))
    with pytest.raises(ValueError):
        ens.apply_channel(TWO_QUBIT["random3"], [1, 1], u=np.zeros(members))
    with pytest.raises(ValueError):
        ens.expect_pauli_sum([(1.0, "Z", [n])])
    with pytest.raises(ValueError):
        ens.expect_pauli_sum([(1.0j, "Z", [0])])
    assert np.array_equal(download(ens), before) and ens.channel_log()[0].shape == (0, members)
    ens.close()
    with pytest.raises(ValueError):
        TrajectoryEnsemble.from_ket(R.random_ket(3, 1), 6)               # not a power of two
    with pytest.raises(ValueError):
        noise.run_trajectories(noisy_circuit(), R.random_ket(4, 1), 4, observable=lambda st: 0.0, batch=4)
    with pytest.raises(ValueError):
        noise.run_trajectories(noisy_circuit(), R.random_ket(4, 1), 4, terms=TERMS, batch=3)
    from_ket = TrajectoryEnsemble.from_ket(R.random_ket(3, 1), 4)
    for m in range(4):
        assert np.array_equal(from_ket.member(m), R.random_ket(3, 1))   # the broadcast copies bits
    from_ket.close()
