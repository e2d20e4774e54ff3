"""Kraus channels on the device (qsv_apply_channel, qsv_channel_log_read, qsv_density_expect_paulis and
``quantum_computations_amd.noise``) against tests/noise_reference.py, which tests/test_noise_reference_host.py pins on the CPU.

Tolerances (TERM_TOL = 1e-13 and CIRCUIT_TOL = 1e-12, the project's conventions):

* a trajectory step that takes branch j: max-abs ``TERM_TOL (2 + total / w_j) max|want|``.  The device forms
  ``w_j = Re tr(E_j rho_q)`` from a reduced density matrix whose entries carry an absolute error of a few eps ``total``; the
  scale ``sqrt(total / w_j)`` turns an absolute error of ``TERM_TOL total`` in ``w_j`` into a relative ``TERM_TOL total / (2 w_j)``
  of every amplitude, and the 2 covers the matrix product itself.  Only branches with ``w_j / total >= 1e-6`` are compared
  this way;
* the logged probability ``w_j / total``: absolute ``TERM_TOL``;
* density registers against ``sum K rho K^dagger`` and whole circuits: ``CIRCUIT_TOL``;
* ``trace`` and ``expect_terms``: ``TERM_TOL sum|c_t|`` (rho has unit trace).

Draws are never left to chance near a boundary: a branch is forced, or ``u`` is the midpoint of its interval, or -- in the
seeded runs -- the test asserts that every draw stays 1e-9 away from the reference's boundaries.

Register sizes: SIZES, at most 2^14 amplitudes, except n = 19 once (the smallest register on which the capped reduction
grid of 1024 x 256 threads loops), QSV_OPT_GRID_CAP = 2 at n = 13 and 14 (same reason), and n = 22 (the smallest register
that defers).  Worst observed errors are printed with their bounds (run with -s).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import noise_reference as R
from quantum_computations_amd import _lib, noise
from quantum_computations_amd.device import DensityState, DeviceState, QuditState
from quantum_computations_amd.dv_simulator import gates as G
from quantum_computations_amd.dv_simulator.simulator import Simulator
from quantum_computations_amd.noise import Channel, KrausChannel, NoiseModel

pytestmark = pytest.mark.gpu

TERM_TOL = 1e-13
CIRCUIT_TOL = 1e-12
SIZES = (1, 2, 3, 6, 7, 13, 14)
MIN_WEIGHT = 1e-6
LAST_U = float(np.nextafter(1.0, 0.0))


def maxabs(a):
    return float(np.max(np.abs(a))) if np.size(a) else 0.0


def report(what, err, bound):
    print(f"{what}: {err:.3e} (bound {bound:.3e})")
    assert err <= bound, what


ONE_QUBIT = {
    "amplitude_damping": KrausChannel.amplitude_damping(0.3),
    "generalized_amplitude_damping": KrausChannel.generalized_amplitude_damping(0.3, 0.2),
    "random4": KrausChannel(R.random_kraus(2, 4, 41)),
}
TWO_QUBIT = {
    "random3": KrausChannel(R.random_kraus(4, 3, 42)),
    "depolarizing_then_damping": KrausChannel(R.compose_minimal(KrausChannel.depolarizing(0.1, 2).kraus,
                                                                 [np.kron(K, np.eye(2)) for K in KrausChannel.amplitude_damping(0.3).kraus])),
}
NAMED = [KrausChannel.bit_flip(0.1), KrausChannel.phase_flip(0.2), KrausChannel.bit_phase_flip(0.3),
         KrausChannel.pauli_channel(0.1, 0.05, 0.2), KrausChannel.depolarizing(0.2), KrausChannel.depolarizing(0.1, 2),
         KrausChannel.amplitude_damping(0.3), KrausChannel.generalized_amplitude_damping(0.3, 0.2),
         KrausChannel.phase_damping(0.25), KrausChannel.reset(0.4)]


def test_fixture_channels_take_the_kernel_path():
    for ch in list(ONE_QUBIT.values()) + list(TWO_QUBIT.values()):
        assert not ch.is_mixed_unitary and len(ch.kraus) <= 16
    assert len(TWO_QUBIT["depolarizing_then_damping"].kraus) > 4


def step_and_compare(dev, ket, ch, qubits, n, what, worst, *, u=0.0, forced=None, want_branch=None):
    """Upload ``ket``, take one step on the device, compare register and log with the reference's step."""
    want, j, p = R.trajectory_step(ch.kraus, ket, qubits, n, u, forced)
    if want_branch is not None:
        assert j == want_branch, what
    dev.upload(ket)
    out = dev.apply_channel(ch, qubits, u=u, forced=forced)
    assert out is dev
    assert dev.last_kernel().startswith(f"k_channel_apply<{ch.num_qubits}, "), dev.last_kernel()
    got = dev.to_numpy()
    branches, probs = dev.channel_log()
    assert list(branches) == [j], (what, branches, j)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(probs))
    assert p > 0.0, what                                            # zero-weight branches are checked on their own
    bound = TERM_TOL * (2.0 + 1.0 / p) * maxabs(want)
    err = maxabs(got - want)
    assert err <= bound, (what, err, bound)
    assert abs(probs[0] - p) <= TERM_TOL, (what, probs[0], p)
    worst[0] = max(worst[0], err / bound if bound else 0.0)
    worst[1] = max(worst[1], abs(probs[0] - p))
    if p > 0.0:
        norm_in, norm_out = np.linalg.norm(ket), np.linalg.norm(got)
        assert abs(norm_out / norm_in - 1.0) <= TERM_TOL * (2.0 + 1.0 / p) * np.sqrt(ket.size), (what, norm_in, norm_out)
    return j, p


def walk_branches(dev, ket, ch, qubits, n, what, worst):
    """Every branch of weight >= MIN_WEIGHT: forced, and drawn with u at the midpoint of its interval."""
    w = R.branch_weights(ch.kraus, ket, qubits, n)
    intervals = R.branch_intervals(w)
    taken = 0
    for j, (lo, hi) in enumerate(intervals):
        if w[j] / w.sum() < MIN_WEIGHT:
            continue
        step_and_compare(dev, ket, ch, qubits, n, f"{what} forced {j}", worst, forced=j, want_branch=j)
        step_and_compare(dev, ket, ch, qubits, n, f"{what} drawn {j}", worst, u=0.5 * (lo + hi), want_branch=j)
        taken += 1
    assert taken >= 2, what
    return taken


# ---- forced branches, exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_one_qubit_channels_every_branch_every_bit(n):
    dev = DeviceState.zeros(n)
    worst = [0.0, 0.0]
    steps = 0
    for scale in (1.0, 1.7):                                     # the second register is not normalised: its norm is kept
        ket = scale * R.random_ket(n, 100 * n + 3)
        for bit in sorted({b for b in (0, 1, 5, 6, 7, n - 1) if b < n}):
            for name, ch in ONE_QUBIT.items():
                steps += walk_branches(dev, ket, ch, [n - 1 - bit], n, f"n={n} bit={bit} {name} norm={scale}", worst)
    assert dev.num_qubits == n
    print(f"n={n}: {steps} branches, worst error / bound {worst[0]:.3f}, worst probability error {worst[1]:.3e} (bound {TERM_TOL:.1e})")
    dev.close()


@pytest.mark.parametrize("n", [n for n in SIZES if n >= 2])
def test_two_qubit_channels_every_branch_every_placement(n):
    dev = DeviceState.zeros(n)
    worst = [0.0, 0.0]
    pairs = {(a, b) for a, b in ((0, 1), (1, 5), (5, 6), (0, n - 1), (6, 7), (n - 2, n - 1)) if a != b and max(a, b) < n and min(a, b) >= 0}
    steps = 0
    ket = 1.7 * R.random_ket(n, 100 * n + 5)
    for a, b in sorted(pairs):
        for bits in ((a, b), (b, a)):                             # both leg orders
            for name, ch in TWO_QUBIT.items():
                steps += walk_branches(dev, ket, ch, [n - 1 - bits[0], n - 1 - bits[1]], n, f"n={n} bits={bits} {name}", worst)
    print(f"n={n}: {steps} branches, worst error / bound {worst[0]:.3f}, worst probability error {worst[1]:.3e} (bound {TERM_TOL:.1e})")
    dev.close()


# ---- edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 7, 14))
def test_edges_of_the_draw_and_zero_weights(n):
    dev = DeviceState.zeros(n)
    worst = [0.0, 0.0]
    ket = R.random_ket(n, 9)
    ad = ONE_QUBIT["amplitude_damping"]
    for name, ch in ONE_QUBIT.items():
        last = len(ch.kraus) - 1
        for q in {0, n - 1}:
            step_and_compare(dev, ket, ch, [q], n, f"{name} u=0", worst, u=0.0, want_branch=0)
            step_and_compare(dev, ket, ch, [q], n, f"{name} u=1-", worst, u=LAST_U, want_branch=last)
    # |0...0> and amplitude damping: the jump has weight exactly 0 and is never drawn
    zero = np.zeros(1 << n, dtype=np.complex128)
    zero[0] = 1.0
    for q in {0, n - 1}:
        for u in (0.0, 0.5, LAST_U):
            _, p = step_and_compare(dev, zero, ad, [q], n, "no jump from |0>", worst, u=u, want_branch=0)
            assert p == 1.0
        # forcing it: an all-zero register, probability 0, no nan
        dev.upload(zero)
        dev.apply_channel(ad, [q], forced=1)
        got = dev.to_numpy()
        branches, probs = dev.channel_log()
        assert not np.any(got) and list(branches) == [1] and list(probs) == [0.0]
    # a zero register stays zero
    dev.upload(np.zeros(1 << n, dtype=np.complex128))
    dev.apply_channel(ad, [0], u=0.3)
    branches, probs = dev.channel_log()
    assert not np.any(dev.to_numpy()) and list(probs) == [0.0] and 0 <= branches[0] < 2
    dev.close()


def test_refusals_reach_python_as_the_reference_exceptions():
    dev = DeviceState.zeros(3)
    ad, two = ONE_QUBIT["amplitude_damping"], TWO_QUBIT["random3"]
    before = dev.to_numpy()
    for bad in (dict(u=1.0), dict(u=-0.1), dict(u=float("nan")), dict(forced=2), dict(forced=-2)):
        with pytest.raises(ValueError):
            dev.apply_channel(ad, [0], **bad)
    for qubits in ([3], [-1]):
        with pytest.raises(ValueError):
            dev.apply_channel(ad, qubits, u=0.1)
    with pytest.raises(ValueError):
        dev.apply_channel(two, [1, 1], u=0.1)
    with pytest.raises(ValueError):
        dev.apply_channel(two, [1], u=0.1)
    modes = QuditState.zeros(2, 3)
    with pytest.raises(TypeError):
        _lib.call("qsv_apply_channel", modes._h, ad.handle(0), (C.c_int * 1)(0), 0.1, -1)
    assert np.array_equal(dev.to_numpy(), before)
    assert [len(x) for x in dev.channel_log()] == [0, 0]
    dev.close()


def test_log_longer_than_the_device_slots_keeps_call_order():
    n = 3
    dev = DeviceState.from_numpy(R.random_ket(n, 4))
    ket = dev.to_numpy()
    ad, flip = ONE_QUBIT["random4"], KrausChannel.bit_flip(0.5)
    rng = np.random.default_rng(12)
    want = []
    for step in range(300):                                         # more than the 256 device slots
        u = float(rng.random())
        ch, q = (flip, step % n) if step % 3 == 2 else (ad, (step + 1) % n)
        assert R.boundary_distance(R.branch_weights(ch.kraus, ket, [q], n), u) > 1e-9
        ket, j, p = R.trajectory_step(ch.kraus, ket, [q], n, u)
        dev.apply_channel(ch, [q], u=u)
        want.append((j, p))
    branches, probs = dev.channel_log()
    assert list(branches) == [j for j, _ in want]
    report("300 logged probabilities", maxabs(probs - np.array([p for _, p in want])), 300 * TERM_TOL)
    report("state after 300 steps", maxabs(dev.to_numpy() - ket), 300 * CIRCUIT_TOL)
    assert [len(x) for x in dev.channel_log()] == [0, 0]          # read and cleared
    dev.close()


# ---- the loop of the capped reduction grid -------------------------------------------------------------------------------
def test_n19_the_reduction_grid_loops():
    n = 19
    dev = DeviceState.zeros(n)
    worst = [0.0, 0.0]
    ket = R.random_ket(n, 19)
    for bit in (0, 5, 6, 18):
        step_and_compare(dev, ket, ONE_QUBIT["random4"], [n - 1 - bit], n, f"n=19 bit={bit}", worst, forced=2)
    for bits in ((0, 1), (5, 13), (18, 3), (17, 18)):
        w = R.branch_weights(TWO_QUBIT["random3"].kraus, ket, [n - 1 - bits[0], n - 1 - bits[1]], n)
        mid = R.branch_intervals(w)[1]
        step_and_compare(dev, ket, TWO_QUBIT["random3"], [n - 1 - bits[0], n - 1 - bits[1]], n, f"n=19 bits={bits}", worst,
                         u=0.5 * (mid[0] + mid[1]), want_branch=1)
    print(f"n=19: worst error / bound {worst[0]:.3f}, worst probability error {worst[1]:.3e}")
    dev.close()


@pytest.mark.parametrize("n", (13, 14))
def test_grid_cap_two_makes_every_kernel_loop(n):
    dev = DeviceState.zeros(n)
    dev.set_option(_lib.OPT_GRID_CAP, 2)
    worst = [0.0, 0.0]
    ket = 1.7 * R.random_ket(n, 13)
    for bit in (0, 6, n - 1):
        walk_branches(dev, ket, ONE_QUBIT["generalized_amplitude_damping"], [n - 1 - bit], n, f"cap n={n} bit={bit}", worst)
    for bits in ((0, 1), (5, 6), (n - 1, 2), (n - 2, n - 1)):
        walk_branches(dev, ket, TWO_QUBIT["random3"], [n - 1 - bits[0], n - 1 - bits[1]], n, f"cap n={n} bits={bits}", worst)
    dev.close()


# ---- mixed-unitary channels join the deferred queue ------------------------------------------------------------------------
def test_mixed_unitary_channel_is_queued_and_general_channel_flushes():
    n = 22
    ket = R.random_ket(n, 22)
    dev = DeviceState.from_numpy(ket)
    h = np.array([[1, 1], [1, -1]]) / np.sqrt(2)
    dep = KrausChannel.depolarizing(0.2)
    assert dep.is_mixed_unitary
    want = ket
    for q in (0, 9, 21):
        dev.apply_matrix(h, [q])
        want = R.apply_op(h, want, [q], n)
    queued, launches = dev.defer_stats()
    assert queued >= 3 and launches == 0                             # this register defers: nothing has run yet
    logged = []
    for u, q in ((0.85, 3), (0.90, 21), (0.97, 10), (0.5, 4)):      # X, Y, Z and the identity branch
        want, j, p = R.trajectory_step(dep.kraus, want, [q], n, u)
        dev.apply_channel(dep, [q], u=u)
        logged.append((j, p))
    assert [j for j, _ in logged] == [1, 2, 3, 0]
    queued_after, launches_after = dev.defer_stats()
    assert queued_after >= queued + 3                                # the three Paulis went through the queue ...
    assert launches_after == 0                                       # ... and nothing was flushed
    got = dev.to_numpy()                                             # the next read applies them
    assert dev.defer_stats()[1] > 0
    report("n=22 depolarizing through the queue", maxabs(got - want), CIRCUIT_TOL * maxabs(want))
    # a general channel with gates pending flushes them first
    for q in (1, 20):
        dev.apply_matrix(h, [q])
        want = R.apply_op(h, want, [q], n)
    launches_before = dev.defer_stats()[1]
    ch = ONE_QUBIT["generalized_amplitude_damping"]
    w = R.branch_weights(ch.kraus, want, [20], n)
    lo, hi = R.branch_intervals(w)[2]
    want, j, p = R.trajectory_step(ch.kraus, want, [20], n, 0.5 * (lo + hi))
    dev.apply_channel(ch, [20], u=0.5 * (lo + hi))
    assert dev.defer_stats()[1] > launches_before and dev.last_kernel().startswith("k_channel_apply<1, ")
    logged.append((j, p))
    branches, probs = dev.channel_log()                              # host-picked and device-picked entries, in call order
    assert list(branches) == [j for j, _ in logged]
    report("n=22 logged probabilities", maxabs(probs - np.array([p for _, p in logged])), TERM_TOL)
    report("n=22 general channel after a flush", maxabs(dev.to_numpy() - want), TERM_TOL * (2 + 1 / p) * maxabs(want) + CIRCUIT_TOL * maxabs(want))
    dev.close()


# ---- density registers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 6, 7))
def test_density_registers_apply_channels_exactly(n):
    rho0 = R.random_density(n, 30 + n)
    worst = 0.0
    for ch in NAMED:
        k = ch.num_qubits
        if k > n:
            continue
        places = [[q] for q in range(n)] if k == 1 else [[a, b] for a in range(n) for b in range(n) if a != b]
        rho = DensityState.from_numpy(rho0)
        for qubits in places:
            rho.upload(rho0.reshape(-1))
            assert rho.apply_channel(ch, qubits) is rho
            err = maxabs(rho.to_numpy() - R.channel_on_density(ch.kraus, rho0, qubits, n))
            assert err <= CIRCUIT_TOL, (n, qubits, err)
            worst = max(worst, err)
        rho.close()
    print(f"n={n}: worst error {worst:.3e} (bound {CIRCUIT_TOL:.1e})")


@pytest.mark.parametrize("n", (3, 6, 7))
def test_trap_superoperators_on_the_per_gate_and_the_deferred_path(n):
    """reset(1) and amplitude_damping(1): superoperators with rows of zeros and only 0 / 1 entries -- not unitary, not a
    permutation -- must pass the exact-match specialisations and the deferred planner unchanged."""
    rho0 = R.random_density(n, 60 + n)
    for ch in (KrausChannel.reset(1.0), KrausChannel.amplitude_damping(1.0)):
        S = ch.superoperator()
        assert set(np.unique(S.real)) <= {0.0, 1.0} and not np.any(S.imag) and np.any(~np.any(S, axis=1))
        for defer in (0, 2):                                       # 2 queues on registers of at least 12 qubits (n >= 6)
            rho = DensityState.from_numpy(rho0)
            rho.set_option(_lib.OPT_DEFER, defer)
            want = rho0
            hq = np.array([[1, 1], [1, -1]]) / np.sqrt(2)
            for q in range(n):
                rho.apply_matrix(hq, [q])                          # something for the channel to share a pass with
                full = R.embed(hq, [q], n)
                want = full @ want @ full.conj().T
                rho.apply_channel(ch, [q])
                want = R.channel_on_density(ch.kraus, want, [q], n)
            if defer == 2 and n >= 6:
                assert rho.defer_stats()[0] >= 2 * n               # gates and superoperators went through the queue
            report(f"n={n} defer={defer} trap", maxabs(rho.to_numpy() - want), CIRCUIT_TOL)
            report(f"n={n} defer={defer} trace", abs(rho.trace() - 1.0), CIRCUIT_TOL)
            rho.close()


@pytest.mark.parametrize("n", (1, 2, 3, 6, 7))
def test_trace_and_expect_terms_against_numpy(n):
    rho0 = R.random_density(n, 80 + n)
    rho = DensityState.from_numpy(rho0)
    rng = np.random.default_rng(n)
    terms = [(0.75, "", []), (1.0, "Z", [0]), (-0.5, "X", [n - 1]), (0.25, "Y", [0]), (2.0, "y", [n - 1])]
    for _ in range(12):
        k = int(rng.integers(1, min(n, 5) + 1))
        qubits = [int(q) for q in rng.choice(n, size=k, replace=False)]
        terms.append((float(rng.normal()), "".join(rng.choice(list("IXYZ"), size=k)), qubits))
    if n >= 2:
        terms += [(1.5, "YY", [0, n - 1]), (-1.0, "XY", [n - 1, 0]), (0.5, "ZI", [0, 1])]
    want_each = np.array([np.trace(R.pauli_matrix(letters, qubits, n) @ rho0) for _, letters, qubits in terms])
    want = sum(c * v for (c, _, _), v in zip(terms, want_each))
    bound = TERM_TOL * sum(abs(c) for c, _, _ in terms)
    value, each = rho.expect_terms(terms, return_terms=True)
    assert rho.last_kernel() == "k_density_expect_paulis"
    report(f"n={n} expect_terms", abs(value - want), bound)
    report(f"n={n} per term", maxabs(each - want_each), TERM_TOL)
    report(f"n={n} trace", abs(rho.trace() - np.trace(rho0).real), TERM_TOL)
    assert rho.expect_terms([]) == 0.0
    with pytest.raises(ValueError):
        rho.expect_terms([(1.0, "Z", [n])])
    with pytest.raises(ValueError):
        rho.expect_terms([(1.0, "Q", [0])])
    odd = DeviceState.zeros(3)
    with pytest.raises(ValueError):
        _lib.call("qsv_density_expect_paulis", odd._h, 0, None, None, None, None)
    odd.close()
    rho.close()


# ---- whole circuits --------------------------------------------------------------------------------------------------------
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


def test_simulator_runs_a_noisy_circuit_the_same_with_and_without_fusion():
    n = 4
    ket = R.random_ket(n, 77)
    seed = 5
    want, want_branches, _, closest = R.run_trajectory(as_reference_circuit(noisy_circuit()), ket, n, np.random.default_rng(seed))
    assert closest > 1e-9
    assert sum(isinstance(g, Channel) for g in noisy_circuit()) == 8 + 4
    runs = []
    for fuse in (0, 4):
        circuit = noisy_circuit(np.random.default_rng(seed))
        sim = Simulator(circuit, fuse=fuse)
        dev = sim.run(DeviceState.from_numpy(ket))
        assert not sim.single_launch_used
        if fuse:
            assert [g for g in sim.launch_list if isinstance(g, Channel)] == [g for g in circuit if isinstance(g, Channel)]
        runs.append((dev.to_numpy(), list(dev.channel_log()[0])))
        dev.close()
    assert runs[0][1] == runs[1][1] == want_branches
    report("fuse=0 against fuse=4", maxabs(runs[0][0] - runs[1][0]), CIRCUIT_TOL)
    report("fuse=0 against the reference", maxabs(runs[0][0] - want), CIRCUIT_TOL)
    # a host ket: the single-launch executor refuses the gate and the simulator goes gate by gate
    sim = Simulator(noisy_circuit(np.random.default_rng(seed)))
    final = sim.run(ket)
    assert not sim.single_launch_used and sim.results == []
    report("host ket against the reference", maxabs(final - want), CIRCUIT_TOL)


def test_channel_gate_on_host_arrays_and_sharded_registers():
    n = 3
    ket, rho0 = R.random_ket(n, 91), R.random_density(n, 92)
    for ch, qubits in ((ONE_QUBIT["generalized_amplitude_damping"], [1]), (TWO_QUBIT["random3"], [2, 0])):
        gate = Channel(ch, qubits)
        assert gate.matrix is None and gate.indices == qubits
        out = gate.apply(rho0)                                      # a 2-D array: exact, on a borrowed register
        assert isinstance(out, np.ndarray) and out.shape == rho0.shape
        report("host density matrix", maxabs(out - R.channel_on_density(ch.kraus, rho0, qubits, n)), CIRCUIT_TOL)
        np.random.seed(17)
        u = float(np.random.random())                               # the draw the gate will make from the global generator
        assert R.boundary_distance(R.branch_weights(ch.kraus, ket, qubits, n), u) > 1e-9
        want, _, p = R.trajectory_step(ch.kraus, ket, qubits, n, u)
        np.random.seed(17)
        out = gate.apply(ket)                                       # a 1-D array: one trajectory step, the state alone
        assert isinstance(out, np.ndarray) and out.shape == ket.shape
        report("host ket", maxabs(out - want), TERM_TOL * (2 + 1 / p) * maxabs(want))
        seeded = Channel(ch, qubits, rng=np.random.default_rng(5)).apply(ket)
        want = R.trajectory_step(ch.kraus, ket, qubits, n, float(np.random.default_rng(5).random()))[0]
        report("host ket, own generator", maxabs(seeded - want), CIRCUIT_TOL)

    class Sharded:                                                  # what is_device_register takes for a sharded register
        def apply_matrix(self, matrix, indices):
            raise AssertionError("a channel must not reach apply_matrix")

    with pytest.raises(NotImplementedError):
        Channel(ONE_QUBIT["amplitude_damping"], [0]).apply(Sharded())
    rho = DensityState.from_numpy(rho0)
    with pytest.raises(ValueError):
        rho.channel_log()
    with pytest.raises(ValueError):
        rho.apply_channel(ONE_QUBIT["amplitude_damping"], [n])
    rho.close()


def test_trajectories_average_to_the_density_run():
    """``|mean - exact| <= 5 stderr`` over 2000 shots with a fixed seed: a condition on the seed, checked on the CPU with the
    NumPy reference fed the same draws, and then on the device, which must take exactly the reference's branches."""
    n = 4
    ket = R.random_ket(n, 78)
    circuit = noisy_circuit()
    ref_circuit = as_reference_circuit(circuit)
    exact_rho = R.run_exact(ref_circuit, np.outer(ket, ket.conj()), n)
    exact = sum(c * np.trace(R.pauli_matrix(letters, qubits, n) @ exact_rho).real for c, letters, qubits in TERMS)
    rng = np.random.default_rng(TRAJECTORY_SEED)
    ref_values, ref_branches, closest = np.zeros(SHOTS), [], 1.0
    full = R.full_matrices(ref_circuit, n)
    for s in range(SHOTS):
        final, branches, _, near = R.run_trajectory(ref_circuit, ket, n, rng, full)
        ref_values[s] = R.expect_terms_ket(TERMS, final, n)
        ref_branches.append(branches)
        closest = min(closest, near)
    ref_mean, ref_stderr = ref_values.mean(), ref_values.std(ddof=1) / np.sqrt(SHOTS)
    print(f"reference: mean {ref_mean:.6f} exact {exact:.6f} stderr {ref_stderr:.2e}, closest draw to a boundary {closest:.2e}")
    assert closest >= 1e-9                                           # the seed's draws stay clear of every boundary
    assert abs(ref_mean - exact) <= 5 * ref_stderr                   # the seed passes on the CPU
    # the exact answer on the device
    rho = noise.run_density(circuit, ket)
    report("run_density against the reference", maxabs(rho.to_numpy() - exact_rho), CIRCUIT_TOL)
    exact_dev = rho.expect_terms(TERMS).real
    report("tr(H rho) on the device", abs(exact_dev - exact), TERM_TOL * sum(abs(c) for c, _, _ in TERMS) + CIRCUIT_TOL)
    rho.close()
    out = noise.run_trajectories(circuit, ket, SHOTS, terms=TERMS, seed=TRAJECTORY_SEED)
    assert [list(b) for b in out["branches"]] == ref_branches        # exactly the reference's branches
    report("shot values against the reference", maxabs(out["values"] - ref_values), CIRCUIT_TOL)
    print(f"device: mean {out['mean']:.6f} exact {exact_dev:.6f} stderr {out['stderr']:.2e}")
    assert abs(out["mean"] - exact_dev) <= 5 * out["stderr"]
    assert out["values"].shape == (SHOTS,)
