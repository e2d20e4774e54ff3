"""CPU: the NumPy reference of the noise entry points (tests/noise_reference.py) and the host side of
``quantum_computations_amd.noise`` agree with each other and with the textbook definitions.  No device is used."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

import noise_reference as R
from quantum_computations_amd.noise import Channel, KrausChannel, NoiseModel
from quantum_computations_amd.dv_simulator import gates as G

NAMED = {
    "bit_flip": (lambda: KrausChannel.bit_flip(0.1), True),
    "phase_flip": (lambda: KrausChannel.phase_flip(0.2), True),
    "bit_phase_flip": (lambda: KrausChannel.bit_phase_flip(0.3), True),
    "pauli_channel": (lambda: KrausChannel.pauli_channel(0.1, 0.05, 0.2), True),
    "depolarizing_1": (lambda: KrausChannel.depolarizing(0.2), True),
    "depolarizing_2": (lambda: KrausChannel.depolarizing(0.1, 2), True),
    "amplitude_damping": (lambda: KrausChannel.amplitude_damping(0.3), False),
    "generalized_amplitude_damping": (lambda: KrausChannel.generalized_amplitude_damping(0.3, 0.2), False),
    "phase_damping": (lambda: KrausChannel.phase_damping(0.25), False),
    "reset": (lambda: KrausChannel.reset(0.4), False),
}


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_channels_are_trace_preserving_and_classified(name):
    make, mixed = NAMED[name]
    ch = make()
    dim = 1 << ch.num_qubits
    total = sum(K.conj().T @ K for K in ch.kraus)
    assert np.max(np.abs(total - np.eye(dim))) <= 1e-14
    assert ch.is_mixed_unitary is mixed
    assert ch.kraus.shape == (len(ch.kraus), dim, dim) and not ch.kraus.flags.writeable


def test_extreme_parameters_stay_trace_preserving():
    for ch in (KrausChannel.reset(1.0), KrausChannel.amplitude_damping(1.0), KrausChannel.amplitude_damping(0.0),
               KrausChannel.depolarizing(1.0), KrausChannel.bit_flip(0.0)):
        total = sum(K.conj().T @ K for K in ch.kraus)
        assert np.max(np.abs(total - np.eye(total.shape[0]))) <= 1e-14
    assert KrausChannel.bit_flip(0.0).is_mixed_unitary and not KrausChannel.reset(1.0).is_mixed_unitary


def test_constructor_refusals():
    with pytest.raises(ValueError):
        KrausChannel([np.eye(2) * 0.5])                             # not trace preserving
    KrausChannel([np.eye(2) * 0.5], check=False)
    with pytest.raises(ValueError):
        KrausChannel([np.eye(3)], check=False)
    with pytest.raises(ValueError):
        KrausChannel([np.eye(2), np.eye(4)], check=False)
    with pytest.raises(ValueError):
        KrausChannel([np.eye(2)] * 17, check=False)
    with pytest.raises(ValueError):
        KrausChannel(([-1.0], [np.eye(2)]), check=False)
    with pytest.raises(ValueError):
        KrausChannel.bit_flip(1.5)
    with pytest.raises(ValueError):
        Channel(KrausChannel.bit_flip(0.1), [0, 1])


@pytest.mark.parametrize("name", sorted(NAMED))
def test_superoperator_reproduces_the_kraus_sum_at_every_position(name):
    ch = NAMED[name][0]()
    n, k = 4, ch.num_qubits
    rho = R.random_density(n, 11)
    S = ch.superoperator()
    for qubits in itertools.permutations(range(n), k):
        want = R.channel_on_density(ch.kraus, rho, list(qubits), n)
        # rho flattened row-major is a 2n-qubit ket: rows are qubits 0..n-1, columns n..2n-1
        legs = list(qubits) + [n + q for q in qubits]
        got = R.apply_op(S, rho.reshape(-1), legs, 2 * n).reshape(rho.shape)
        assert np.max(np.abs(got - want)) <= 1e-14


@pytest.mark.parametrize("name", ["amplitude_damping", "generalized_amplitude_damping", "depolarizing_2", "reset"])
def test_average_over_all_branches_of_one_step_is_the_channel(name):
    ch = NAMED[name][0]()
    n, k = 4, ch.num_qubits
    psi = R.random_ket(n, 5)
    for qubits in ([1], [3]) if k == 1 else ([0, 2], [3, 1]):
        w = R.branch_weights(ch.kraus, psi, qubits, n)
        assert abs(w.sum() - 1.0) <= 1e-14
        mixed = np.zeros((1 << n, 1 << n), dtype=np.complex128)
        for j in range(len(ch.kraus)):
            out, jj, p = R.trajectory_step(ch.kraus, psi, qubits, n, forced=j)
            assert jj == j and abs(p - w[j]) <= 1e-15
            mixed += p * np.outer(out, out.conj())
        want = R.channel_on_density(ch.kraus, np.outer(psi, psi.conj()), qubits, n)
        assert np.max(np.abs(mixed - want)) <= 1e-14


def test_selection_rule():
    w = [0.25, 0.0, 0.5, 0.25]
    assert R.pick_branch(w, 0.0) == 0 and R.pick_branch(w, 0.2499) == 0
    assert R.pick_branch(w, 0.25) == 2                    # the zero-weight branch is never drawn
    assert R.pick_branch(w, 0.74) == 2 and R.pick_branch(w, 0.75) == 3
    assert R.pick_branch(w, np.nextafter(1.0, 0.0)) == 3
    assert R.pick_branch([0.0, 1.0, 0.0], np.nextafter(1.0, 0.0)) == 1
    assert R.pick_branch([0.0, 0.0], 0.5) == 0            # a zero register
    # every midpoint of branch_intervals picks its own branch
    for j, (lo, hi) in enumerate(R.branch_intervals(w)):
        if hi > lo:
            assert R.pick_branch(w, 0.5 * (lo + hi)) == j
    assert R.boundary_distance(w, 0.3) == pytest.approx(0.05)
    # weights relative to the total: scaling them changes nothing
    assert [R.pick_branch([3 * x for x in w], u) for u in (0.1, 0.3, 0.8)] == [R.pick_branch(w, u) for u in (0.1, 0.3, 0.8)]


def test_zero_weight_branch_gives_zeros_not_nan():
    ch = KrausChannel.amplitude_damping(0.3)
    psi = np.zeros(8, dtype=np.complex128)
    psi[0] = 1.0
    out, j, p = R.trajectory_step(ch.kraus, psi, [1], 3, forced=1)
    assert j == 1 and p == 0.0 and not np.any(out) and np.all(np.isfinite(out))
    for u in (0.0, 0.5, np.nextafter(1.0, 0.0)):
        assert R.trajectory_step(ch.kraus, psi, [1], 3, u)[1] == 0


def test_weights_and_ks_form_agrees_with_the_plain_list():
    base = R.random_kraus(2, 3, 3)
    weights = [0.5, 2.0, 0.25]
    scaled = [K / np.sqrt(d) for d, K in zip(weights, base)]
    a = KrausChannel(base)
    b = KrausChannel((np.array(weights), scaled))
    assert np.max(np.abs(a.kraus - b.kraus)) <= 1e-15
    rho = R.random_density(1, 2)
    want = sum(d * K @ rho @ K.conj().T for d, K in zip(weights, scaled))          # the reference's quantum_channel
    assert np.max(np.abs(R.channel_on_density(b.kraus, rho, [0], 1) - want)) <= 1e-15


def test_whole_trajectory_run_averages_to_the_exact_run():
    n = 2
    h = np.array([[1, 1], [1, -1]]) / np.sqrt(2)
    ad = KrausChannel.amplitude_damping(0.4).kraus
    circuit = [("gate", h, [0]), ("channel", ad, [0]), ("gate", h, [1]), ("channel", ad, [1])]
    psi = np.zeros(4, dtype=np.complex128)
    psi[0] = 1.0
    exact = R.run_exact(circuit, np.outer(psi, psi.conj()), n)
    # all four branch paths, weighted: the exact density matrix
    mixed = np.zeros_like(exact)
    for path in itertools.product(range(2), repeat=2):
        v, weight, step = psi.copy(), 1.0, 0
        for kind, op, qubits in circuit:
            if kind == "gate":
                v = R.apply_op(op, v, qubits, n)
            else:
                v, _, p = R.trajectory_step(op, v, qubits, n, forced=path[step])
                weight *= p
                step += 1
        mixed += weight * np.outer(v, v.conj())
    assert np.max(np.abs(mixed - exact)) <= 1e-14
    final, branches, draws, closest = R.run_trajectory(circuit, psi, n, np.random.default_rng(1))
    assert len(branches) == 2 and len(draws) == 2 and 0.0 <= closest <= 1.0
    assert abs(np.linalg.norm(final) - 1.0) <= 1e-14


def test_noise_model_inserts_after_matching_gates_and_fusion_keeps_channels_apart():
    from quantum_computations_amd.fusion import fuse_circuit

    ad, dep = KrausChannel.amplitude_damping(0.1), KrausChannel.depolarizing(0.05, 2)
    model = NoiseModel().add(ad, after=1).add(dep, after=(G.CX,)).add(lambda gate: KrausChannel.phase_flip(0.01), after=(G.CX,))
    circuit = [G.H(0), G.CX(0, 1), G.X(2)]
    noisy = model.insert(circuit)
    kinds = [(type(g).__name__, list(g.indices)) for g in noisy]
    assert kinds == [("H", [0]), ("Channel", [0]), ("CX", [0, 1]), ("Channel", [0, 1]), ("Channel", [0]), ("Channel", [1]),
                     ("X", [2]), ("Channel", [2])]
    assert noisy[1].channel is ad and noisy[3].channel is dep
    assert len(circuit) == 3                                     # a new list
    fused = fuse_circuit(noisy, 4)
    assert [g for g in fused if isinstance(g, Channel)] == [g for g in noisy if isinstance(g, Channel)]
    # a barrier: no block holds gates from both sides of a channel
    position = {id(g): i for i, g in enumerate(noisy)}
    marks = [position[id(g)] for g in noisy if isinstance(g, Channel)]
    for block in fused:
        members = [position[id(s)] for s in getattr(block, "sources", [block])]
        assert not any(min(members) < m < max(members) for m in marks)
    # the single-launch executor refuses the gate, so Simulator falls back to gate by gate
    from quantum_computations_amd.dv_simulator import program as P
    with pytest.raises(P.Unsupported):
        P.compile_circuit(noisy, 3)
