"""Per-member adjoint walks on the device: every member of an ``Ensemble`` runs the backward walk over a
Pauli-rotation list and over a cost phase with its own angles and reads back its own ``<lambda_m|P_t|psi_m>``,
``<lambda_m|D|psi_m>`` and ``<a_m|b_m>`` -- against tests/ensemble_adjoint_reference.py, and the rewound registers BIT FOR BIT
against single ``DeviceState`` registers of the member's size.

Sizes follow tests/test_gpu_sweep.py: members of 1, 2, 3, 7, 8, 9, 13 and 14 qubits, and 15, the smallest size at which a
FLIPPING pass of the walk is cut into two parts per member (tests/test_ensemble_adjoint_layout_host.py: the walk takes the
cut of a read pass, so a diagonal pass has two parts from 14 qubits on and a flipping one from 15); each as 1, 2, 8 and 64
members, fewer where the register would pass 2^18 amplitudes.  13 and above also run with ``QSV_OPT_GRID_CAP = 2``, so that
workgroups loop over units.  Kets differ from member to member, are not all of norm 1, and ``lambda`` is unrelated to ``psi``.

Tolerances are the project's (tests/test_gpu_pauli_operator.py, tests/test_gpu_qaoa.py, tests/test_gpu_sweep.py):
  * values within ``ADJOINT_TOL ||lambda_m|| ||psi_m||``, ADJOINT_TOL = 1e-12;
  * rewound registers within ``CIRCUIT_TOL`` = 1e-12 times the member's norm (a list of rotations), after the cost phase within
    ``TERM_TOL (1 + |gamma| max|d|) max|psi|``, TERM_TOL = 1e-13;
  * energies and gradients within ``ADJOINT_TOL sum|c_t| ||psi_m||^2``;
  * the inner product within ``TERM_TOL ||a_m|| ||b_m||``.  ``<a_m|a_m>`` has an imaginary part of EXACTLY 0: the kernel rounds
    the two products of the imaginary part one by one, and they are the same two numbers.

Worst observed errors are printed with their bounds (run with -s).
"""
from __future__ import annotations

import numpy as np
import pytest

import diagonal_reference as D
import ensemble_adjoint_reference as A
import noise_reference as R
import sweep_reference as S
from quantum_computations_amd import DiagonalOperator, _lib, qaoa, sweep
from quantum_computations_amd import workloads as W
from quantum_computations_amd.device import DeviceState
from quantum_computations_amd.dv_simulator import gates as G
from quantum_computations_amd.ensemble import Ensemble, TrajectoryEnsemble
from test_gpu_ensemble import ONE_QUBIT
from test_gpu_sweep import (ADJOINT_TOL, CIRCUIT_TOL, MEMBERS, TERM_TOL, angle_rows, distinct_kets, download, low_and_high_lists,
                            make_ensemble, maxabs, members_for, qubit_of, random_diagonal, report, shared_pass_list, upload)

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 7, 8, 9, 13, 14, 15)        # 15: two parts per member in a flipping pass


def caps_for(n):
    return (0, 2) if n >= 13 else (0,)


def walk_list(n):
    """The diagonal, one flipping group of eight and a ninth term behind it, pivots on bit 0 and on the top bit, Y letters, the
    identity string, and strings of full weight (flipping and diagonal)."""
    low, high = low_and_high_lists(n)
    full = [(0.0, "".join("XYZ"[q % 3] for q in range(n)), list(range(n))), (0.0, "Z" * n, list(range(n))), (0.0, "Y" * n, list(range(n)))]
    return shared_pass_list(n)[1] + low + full + high + [(0.0, "I", [qubit_of(n, 0)])]


def lambda_kets(n, members, seed):
    """Unrelated to psi, not of norm 1."""
    return [(0.6 + 0.5 * (m % 4)) * R.random_ket(n, seed + 31 * m + 5) for m in range(members)]


def make_pair(n, members, cap, psis, lams):
    psi, lam = make_ensemble(n, members, cap), make_ensemble(n, members, cap)
    upload(psi, psis)
    upload(lam, lams)
    return psi, lam


def norms(kets):
    return np.array([np.linalg.norm(k) for k in kets])


# ---- 1. both walks against the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", MEMBERS)
@pytest.mark.parametrize("n", SIZES)
def test_both_walks_against_the_reference(n, members):
    members = members_for(n, members)
    rotations = walk_list(n)
    thetas = angle_rows(members, len(rotations), 11 * n + members)
    psis, lams = distinct_kets(n, members, 100 + n), lambda_kets(n, members, 500 + n)
    want_values, want_psi, want_lam = A.rotations_adjoint_members(rotations, thetas, psis, lams)
    d = random_diagonal(n, 3 * n)
    gammas = angle_rows(members, 1, 7 * n + members)[:, 0]
    want_d, want_dpsi, want_dlam = A.diag_phase_adjoint_members(d, gammas, psis, lams)
    op = DiagonalOperator.from_numpy(d)
    np_, nl = norms(psis), norms(lams)
    for cap in caps_for(n):
        psi, lam = make_pair(n, members, cap, psis, lams)
        values = psi.pauli_rotations_adjoint(rotations, lam, thetas)
        assert values.shape == (members, len(rotations))
        assert psi.state.last_kernel().startswith("k_ens_pauli_adjoint_group<"), psi.state.last_kernel()
        assert psi.last_passes >= 1
        got_psi, got_lam = download(psi), download(lam)
        err = max(maxabs(values[m] - want_values[m]) / (nl[m] * np_[m]) for m in range(members))
        report(f"n={n} members={members} cap={cap}: rotation walk values / (|lam| |psi|)", err, ADJOINT_TOL)
        err = max(max(maxabs(got_psi[m] - want_psi[m]) / np_[m], maxabs(got_lam[m] - want_lam[m]) / nl[m]) for m in range(members))
        report(f"n={n} members={members} cap={cap}: rewound registers / norm", err, CIRCUIT_TOL)
        upload(psi, psis)
        upload(lam, lams)
        values = psi.diagonal_phase_adjoint(op, lam, gammas)
        assert psi.state.last_kernel().startswith("k_ens_diag_phase_adjoint<"), psi.state.last_kernel()
        got_psi, got_lam = download(psi), download(lam)
        err = max(abs(values[m] - want_d[m]) / (nl[m] * np_[m] * maxabs(d)) for m in range(members))
        report(f"n={n} members={members} cap={cap}: cost-phase value / (|lam| |psi| max|d|)", err, ADJOINT_TOL)
        for m in range(members):
            bound = TERM_TOL * (1 + abs(gammas[m]) * maxabs(d))
            assert maxabs(got_psi[m] - want_dpsi[m]) <= bound * maxabs(psis[m]), (n, m, cap)
            assert maxabs(got_lam[m] - want_dlam[m]) <= bound * maxabs(lams[m]), (n, m, cap)
        psi.close()
        lam.close()
    op.close()


def test_the_pass_count_is_the_forward_lists_and_the_list_angles_serve_every_member():
    n, members = 8, 8
    rotations = S.with_angles(walk_list(n), angle_rows(1, len(walk_list(n)), 3)[0])
    psis, lams = distinct_kets(n, members, 1), lambda_kets(n, members, 2)
    psi, lam = make_pair(n, members, 0, psis, lams)
    psi.apply_pauli_rotations(rotations)
    forward = psi.last_passes
    upload(psi, psis)
    values = psi.pauli_rotations_adjoint(rotations, lam)              # thetas=None: the list's own angles for every member
    assert psi.last_passes == forward and forward >= 3
    want, _, _ = A.rotations_adjoint_members(rotations, np.tile([t for t, _, _ in rotations], (members, 1)), psis, lams)
    report("list angles for every member", maxabs(values - want) / (maxabs(norms(psis)) * maxabs(norms(lams))), ADJOINT_TOL)
    assert psi.pauli_rotations_adjoint([], lam).shape == (members, 0)  # n_terms = 0 launches nothing
    assert psi.last_passes == 0
    psi.close()
    lam.close()


# ---- 2. the rewound registers, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_rewound_registers_are_bit_identical_to_registers_of_the_members_own(n):
    members = members_for(n, 8)
    rotations = walk_list(n)
    thetas = angle_rows(members, len(rotations), 5 * n)
    psis, lams = distinct_kets(n, members, 200 + n), lambda_kets(n, members, 600 + n)
    d = random_diagonal(n, n)
    op = DiagonalOperator.from_numpy(d)
    gammas = angle_rows(members, 1, 9 * n)[:, 0]
    single_walk, single_phase, single_values, single_d = [], [], [], []
    for m in range(members):
        a, b = DeviceState.from_numpy(psis[m]), DeviceState.from_numpy(lams[m])
        single_values.append(a.pauli_rotations_adjoint(S.with_angles(rotations, thetas[m]), b))
        single_walk.append((a.to_numpy(), b.to_numpy()))
        a.upload(psis[m])
        b.upload(lams[m])
        single_d.append(a.diagonal_phase_adjoint(op, b, gammas[m]))
        single_phase.append((a.to_numpy(), b.to_numpy()))
        a.close()
        b.close()
    for cap in caps_for(n):
        psi, lam = make_pair(n, members, cap, psis, lams)
        values = psi.pauli_rotations_adjoint(rotations, lam, thetas)
        got_psi, got_lam = download(psi), download(lam)
        for m in range(members):
            assert np.array_equal(got_psi[m], single_walk[m][0]) and np.array_equal(got_lam[m], single_walk[m][1]), (n, cap, m)
            # the values agree within tolerance, not bit for bit: the order of the sums differs
            assert maxabs(values[m] - single_values[m]) <= ADJOINT_TOL * np.linalg.norm(psis[m]) * np.linalg.norm(lams[m]), (n, cap, m)
        upload(psi, psis)
        upload(lam, lams)
        values = psi.diagonal_phase_adjoint(op, lam, gammas)
        got_psi, got_lam = download(psi), download(lam)
        for m in range(members):
            assert np.array_equal(got_psi[m], single_phase[m][0]) and np.array_equal(got_lam[m], single_phase[m][1]), (n, cap, m)
            assert abs(values[m] - single_d[m]) <= ADJOINT_TOL * np.linalg.norm(psis[m]) * np.linalg.norm(lams[m]) * maxabs(d), (n, cap, m)
        psi.close()
        lam.close()
    op.close()


# ---- 3. a member's values wherever it sits ------------------------------------------------------------------------------------
def placed_values(n, members, place, cap, ket, lket, row, gamma, rotations, op, seed):
    psis, lams = distinct_kets(n, members, seed), lambda_kets(n, members, seed + 1)
    psis[place], lams[place] = ket, lket
    rows = angle_rows(members, len(rotations), seed)
    rows[place] = row
    gammas = np.linspace(-1.0, 1.0, members) + 0.01 * seed
    gammas[place] = gamma
    psi, lam = make_pair(n, members, cap, psis, lams)
    inner = psi.inner(lam)[place]
    walk = psi.pauli_rotations_adjoint(rotations, lam, rows)[place]
    upload(psi, psis)
    upload(lam, lams)
    phase = psi.diagonal_phase_adjoint(op, lam, gammas)[place]
    psi.close()
    lam.close()
    return inner, walk, phase


@pytest.mark.parametrize("n", SIZES)
def test_a_members_values_are_bit_identical_wherever_it_sits(n):
    ket, lket = 1.3 * R.random_ket(n, 77), 0.8 * R.random_ket(n, 78)
    rotations = walk_list(n)
    row = angle_rows(1, len(rotations), n)[0]
    op = DiagonalOperator.from_numpy(random_diagonal(n, 40 + n))
    most = members_for(n, 64)
    for cap in caps_for(n):
        first = placed_values(n, min(2, most), 0, cap, ket, lket, row, 0.37, rotations, op, 1)
        last = placed_values(n, most, most - 1, cap, ket, lket, row, 0.37, rotations, op, 2)
        alone = placed_values(n, 1, 0, cap, ket, lket, row, 0.37, rotations, op, 3)
        for other in (last, alone):
            assert first[0] == other[0] and np.array_equal(first[1], other[1]) and first[2] == other[2], (n, cap)
    op.close()


# ---- 4. H psi per member ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 3, 8, 9, 13))
def test_apply_pauli_sum_is_bit_identical_to_a_register_of_the_members_own(n):
    members = members_for(n, 8)
    terms = [(0.3 - 0.1 * k, letters, qubits) for k, (_, letters, qubits) in enumerate(walk_list(n))]
    kets = distinct_kets(n, members, 300 + n)
    ens = make_ensemble(n, members)
    upload(ens, kets)
    out = ens.apply_pauli_sum(terms)
    assert isinstance(out, TrajectoryEnsemble) and out.members == members and out.member_qubits == n
    again = ens.apply_pauli_sum(terms, out=out, accumulate=True)
    assert again is out
    got = download(out)
    assert np.array_equal(download(ens), np.array(kets))                  # the source is not changed
    for m in range(members):
        single = DeviceState.from_numpy(kets[m])
        h = single.apply_pauli_sum(terms)
        single.apply_pauli_sum(terms, out=h, accumulate=True)
        assert np.array_equal(got[m], h.to_numpy()), (n, m)
        h.close()
        single.close()
    with pytest.raises(ValueError):
        ens.apply_pauli_sum(terms, out=make_ensemble(n, 1) if members > 1 else make_ensemble(n + 1, 1))
    with pytest.raises(ValueError):
        ens.apply_pauli_sum([(1.0, "X", [n])])
    out.close()
    ens.close()


# ---- 5. inner products ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", MEMBERS)
@pytest.mark.parametrize("n", SIZES)
def test_inner_products(n, members):
    members = members_for(n, members)
    psis, lams = distinct_kets(n, members, 700 + n), lambda_kets(n, members, 800 + n)
    want = A.inner_members(psis, lams)
    for cap in caps_for(n):
        a, b = make_pair(n, members, cap, psis, lams)
        got = a.inner(b)
        assert a.state.last_kernel() == "k_ens_inner"
        err = max(abs(got[m] - want[m]) / (np.linalg.norm(psis[m]) * np.linalg.norm(lams[m])) for m in range(members))
        report(f"n={n} members={members} cap={cap}: <a_m|b_m> / (|a| |b|)", err, TERM_TOL)
        own = a.inner(a)
        assert np.all(own.imag == 0.0)                                   # exactly
        err = maxabs((own.real - a.norm2()) / norms(psis) ** 2)
        report(f"n={n} members={members} cap={cap}: <a_m|a_m> against norm2 / |a|^2", err, TERM_TOL)
        assert np.array_equal(download(a), np.array(psis)) and np.array_equal(download(b), np.array(lams))      # read-only
        a.close()
        b.close()


# ---- 6. sweep.energies_and_gradients -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (4, 9))
def test_energies_and_gradients_of_a_trotter_step(n):
    terms = W.heisenberg_chain_terms(n)
    weight = sum(abs(c) for c, _, _ in terms)
    rotations = A.trotter_step(terms, 0.4)
    ket = 1.2 * R.random_ket(n, 8 + n)
    norm2 = float(np.linalg.norm(ket) ** 2)
    all_rows = angle_rows(70, len(rotations), 4 + n)
    bound = ADJOINT_TOL * weight * norm2
    worst = {"shift E": 0.0, "shift G": 0.0, "single E": 0.0, "single G": 0.0}
    for points in (1, 5, 70):                                             # batch = 64: 70 = 64 + a short last chunk of 6 in 8
        rows = all_rows[:points]
        energy, gradient = sweep.energies_and_gradients(rotations, rows, terms, ket=ket, batch=64)
        assert energy.shape == (points,) and gradient.shape == rows.shape
        for m in range(points):
            e, g = sweep.parameter_shift(rotations, rows[m], terms, ket=ket, batch=64)
            worst["shift E"] = max(worst["shift E"], abs(energy[m] - e))
            worst["shift G"] = max(worst["shift G"], maxabs(gradient[m] - g))
        for m in range(points):
            state = DeviceState.from_numpy(ket)
            e, g = state.energy_and_gradient(S.with_angles(rotations, rows[m]), terms)
            state.close()
            worst["single E"] = max(worst["single E"], abs(energy[m] - e))
            worst["single G"] = max(worst["single G"], maxabs(gradient[m] - g))
        assert maxabs(gradient) > 1e-3                                    # not a comparison of zeros
    for what, err in worst.items():
        report(f"n={n} energies_and_gradients against {what}", err, bound)
    ref_e, ref_g = A.energies_and_gradients(rotations, all_rows[:3], terms, ket)
    energy, gradient = sweep.energies_and_gradients(rotations, all_rows[:3], terms, ket=ket, batch=2)
    report(f"n={n} energies against the reference", maxabs(energy - ref_e), bound)
    report(f"n={n} gradients against the reference", maxabs(gradient - ref_g), bound)
    with pytest.raises(ValueError):
        sweep.energies_and_gradients(rotations, all_rows[:3, :-1], terms, ket=ket)
    with pytest.raises(ValueError):
        sweep.energies_and_gradients(rotations, all_rows[:3], [(1j, "Z", [0])], ket=ket)
    assert sweep.energies_and_gradients(rotations, np.zeros((0, len(rotations))), terms, ket=ket)[1].shape == (0, len(rotations))


# ---- 7. qaoa.energies_and_gradients ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (6, 10))
def test_qaoa_energies_and_gradients_on_a_three_regular_maxcut(n):
    p, points = 2, 7
    terms = W.maxcut_terms(n, W.ring_chord_edges(n))
    weight = sum(abs(c) for c, _, _ in terms)
    op = DiagonalOperator.from_terms(n, terms)
    rng = np.random.default_rng(12 + n)
    gammas, betas = rng.uniform(-0.6, 0.6, (points, p)), rng.uniform(-0.6, 0.6, (points, p))
    gammas[1], betas[2] = 0.0, 0.0
    energy, d_gamma, d_beta = qaoa.energies_and_gradients(op, gammas, betas, batch=4)       # 4 + 3 of 4
    assert energy.shape == (points,) and d_gamma.shape == (points, p) and d_beta.shape == (points, p)
    worst = np.zeros(3)
    for m in range(points):
        e, dg, db = qaoa.energy_and_gradient(op, gammas[m], betas[m])
        worst = np.maximum(worst, [abs(energy[m] - e), maxabs(d_gamma[m] - dg), maxabs(d_beta[m] - db)])
    for what, err in zip(("E", "dE/dgamma", "dE/dbeta"), worst):
        report(f"n={n} qaoa.energies_and_gradients: {what} against qaoa.energy_and_gradient", err, ADJOINT_TOL * weight)
    ref = A.qaoa_energies_and_gradients(D.diagonal_from_terms(n, terms), gammas, betas)
    for what, got, want in zip(("E", "dE/dgamma", "dE/dbeta"), (energy, d_gamma, d_beta), ref):
        report(f"n={n} qaoa.energies_and_gradients: {what} against the reference", maxabs(got - want), ADJOINT_TOL * weight)
    assert maxabs(d_gamma) > 1e-3 and maxabs(d_beta) > 1e-3
    with pytest.raises(ValueError):
        qaoa.energies_and_gradients(op, gammas, betas[:, :1])
    op.close()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_raise_and_leave_both_registers_as_they_were():
    n, members = 10, 8                                                   # 13-qubit registers: deferral can be forced on
    psis, lams = distinct_kets(n, members, 3), lambda_kets(n, members, 4)
    psi, lam = make_pair(n, members, 0, psis, lams)
    for ens in (psi, lam):
        ens.state.set_option(_lib.OPT_DEFER, 2)
        ens.apply(G.H(1))                                                # stays in the queue through every refusal
    queued = (psi.state.defer_stats(), lam.state.defer_stats())
    assert queued == ((1, 0), (1, 0))
    op, wide = DiagonalOperator.from_numpy(random_diagonal(n, 1)), DiagonalOperator.from_numpy(random_diagonal(n + 3, 1))
    rotation = [(0.1, "X", [0]), (0.2, "ZZ", [1, 2])]
    nan_rows = np.zeros((members, 2))
    nan_rows[2, 1] = np.nan
    small = make_ensemble(n, members // 2)
    other_cut = Ensemble(DeviceState.zeros(n + 3), n + 1)                 # the same register size, another member size
    for call in (lambda: psi.pauli_rotations_adjoint(rotation, lam, np.zeros((members, 3))),
                 lambda: psi.pauli_rotations_adjoint(rotation, lam, np.zeros((members - 1, 2))),
                 lambda: psi.pauli_rotations_adjoint(rotation, lam, nan_rows),
                 lambda: psi.pauli_rotations_adjoint([(0.1, "X", [n])], lam),
                 lambda: psi.pauli_rotations_adjoint([(0.1, "XX", [1, 1])], lam),
                 lambda: psi.pauli_rotations_adjoint([(0.1, "XQ", [0, 1])], lam),
                 lambda: psi.pauli_rotations_adjoint(rotation, psi),
                 lambda: psi.pauli_rotations_adjoint(rotation, small),
                 lambda: psi.pauli_rotations_adjoint(rotation, other_cut),
                 lambda: psi.pauli_rotations_adjoint(rotation, lam.state),
                 lambda: psi.diagonal_phase_adjoint(op, lam, np.zeros(members + 1)),
                 lambda: psi.diagonal_phase_adjoint(op, lam, [0.0, np.inf] + [0.0] * (members - 2)),
                 lambda: psi.diagonal_phase_adjoint(wide, lam, np.zeros(members)),
                 lambda: psi.diagonal_phase_adjoint(op, psi, np.zeros(members)),
                 lambda: psi.diagonal_phase_adjoint(op, small, np.zeros(members)),
                 lambda: psi.inner(small),
                 lambda: psi.inner(other_cut),
                 lambda: psi.apply_diagonal_operator(wide, out=lam),
                 lambda: psi.apply_diagonal_operator(op, out=small)):
        with pytest.raises(ValueError):
            call()
        assert (psi.state.defer_stats(), lam.state.defer_stats()) == queued      # both queues as they were
    with pytest.raises(TypeError):
        psi.diagonal_phase_adjoint(np.zeros(1 << n), lam, np.zeros(members))
    h = np.array([[1, 1], [1, -1]]) / np.sqrt(2)
    for ens, kets in ((psi, psis), (lam, lams)):
        want = np.array([R.apply_op(h, k, [1], n) for k in kets])
        assert maxabs(download(ens) - want) <= CIRCUIT_TOL * 2            # the register as it was, up to the queued gate
    small.close()
    other_cut.close()
    # without a queue: bit-identical after every refusal
    upload(psi, psis)
    upload(lam, lams)
    for call in (lambda: psi.pauli_rotations_adjoint(rotation, lam, nan_rows), lambda: psi.pauli_rotations_adjoint(rotation, psi),
                 lambda: psi.diagonal_phase_adjoint(wide, lam, np.zeros(members)), lambda: psi.diagonal_phase_adjoint(op, psi, np.zeros(members))):
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(download(psi), np.array(psis)) and np.array_equal(download(lam), np.array(lams))
    # a view: a window on another register's memory
    base = DeviceState.zeros(n + 3)
    view = TrajectoryEnsemble(DeviceState.view(n + 3, base.device_ptr, 1 << (n + 3), keepalive=base), n)
    for call in (lambda: view.pauli_rotations_adjoint(rotation, lam), lambda: psi.pauli_rotations_adjoint(rotation, view),
                 lambda: view.diagonal_phase_adjoint(op, lam, np.zeros(members)), lambda: psi.inner(view), lambda: view.inner(view)):
        with pytest.raises(ValueError):
            call()
    untouched = np.zeros(1 << (n + 3), dtype=complex)
    untouched[0] = 1.0
    assert np.array_equal(base.to_numpy(), untouched)
    assert np.array_equal(download(psi), np.array(psis)) and np.array_equal(download(lam), np.array(lams))
    view.close()
    base.close()
    for thing in (psi, lam, op, wide):
        thing.close()


# ---- 9. next to the channel calls ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drained", (True, False))
def test_a_walk_after_channel_and_measure_calls(drained):
    n, members = 7, 8
    ad = ONE_QUBIT["amplitude_damping"]
    psis, lams = distinct_kets(n, members, 900), lambda_kets(n, members, 901)
    psi, lam = make_pair(n, members, 0, psis, lams)
    rng = np.random.default_rng(5)
    psi.apply_channel(ad, [3], u=rng.random(members)).measure(2, u=rng.random(members), bit=0)
    if drained:
        assert psi.channel_log()[0].shape == (2, members)
    now = list(download(psi))
    rotations = walk_list(n)
    thetas = angle_rows(members, len(rotations), 6)
    want, want_psi, _ = A.rotations_adjoint_members(rotations, thetas, now, lams)
    values = psi.pauli_rotations_adjoint(rotations, lam, thetas)         # member_qubits unchanged: the log may hold steps
    bound = ADJOINT_TOL * maxabs(norms(now)) * maxabs(norms(lams))
    report(f"walk after a channel and a measurement (log drained: {drained})", maxabs(values - want), bound)
    assert maxabs(download(psi) - np.array(want_psi)) <= CIRCUIT_TOL * maxabs(norms(now))
    d = random_diagonal(n, 9)
    op = DiagonalOperator.from_numpy(d)
    now_psi, now_lam = list(download(psi)), list(download(lam))
    gammas = np.linspace(-1.0, 1.0, members)
    want_d, _, _ = A.diag_phase_adjoint_members(d, gammas, now_psi, now_lam)
    got_d = psi.diagonal_phase_adjoint(op, lam, gammas)
    report("cost-phase walk after them", maxabs(got_d - want_d), bound * maxabs(d))
    report("inner product after them", maxabs(psi.inner(lam) - A.inner_members(list(download(psi)), list(download(lam)))), TERM_TOL * bound / ADJOINT_TOL)
    if not drained:
        assert psi.channel_log()[0].shape == (2, members)                # the steps are still there, in order
        psi.apply_channel(ad, [1], u=rng.random(members))                # one step pending: the member size may not change now
        recut, lam_recut = TrajectoryEnsemble(psi.state, n - 1), TrajectoryEnsemble(lam.state, n - 1)
        with pytest.raises(TypeError):
            recut.pauli_rotations_adjoint([(0.1, "X", [0])], lam_recut)
        with pytest.raises(TypeError):
            recut.inner(lam_recut)
        assert psi.channel_log()[0].shape == (1, members)
        assert recut.inner(lam_recut).shape == (2 * members,)            # drained: now it may
    op.close()
    psi.close()
    lam.close()
