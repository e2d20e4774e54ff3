"""``DiagonalOperator`` (qsv_diag_*) and the register x diagonal passes (qsv_apply_diag_phase / _mul, qsv_expect_diag,
qsv_diag_transition, qsv_diag_phase_adjoint) against tests/diagonal_reference.py, which tests/test_diagonal_reference_host.py
pins against dense matrices.

Construction is compared for EQUALITY: the build kernel and the NumPy loop make the same correctly rounded additions
``acc += c_t * (+-1)`` in the same order, so there is nothing to tolerate.  ``extrema`` equals numpy's min / argmin / max /
argmax exactly.

Tolerances of the passes (TERM_TOL = 1e-13, the project's convention; every bound is a few hundred eps of its scale):

* phase: max-abs ``TERM_TOL (1 + |gamma| max|d|) max|psi|`` -- the rounded product gamma d carries eps |gamma d| into the
  angle, sincos and the complex product add a few eps;
* mul: ``TERM_TOL (|c| max|d| max|src| + max|old dst|)``;
* norm2: relative 1e-13; mean: ``TERM_TOL max|d| norm2``; second_moment: ``TERM_TOL max|d|^2 norm2``;
  probability_below: ``TERM_TOL norm2``, with thresholds taken from the downloaded vector so that ``d_i <= threshold``
  is the same comparison on both sides;
* transition and the value of phase_adjoint: ``TERM_TOL max|d| ||bra|| ||ket||``; the registers after phase_adjoint meet
  the phase bound;
* against the existing calls: ``expect_diagonal(...).mean`` against ``expect_pauli_sum`` within ``2 TERM_TOL sum|c_t|``,
  ``apply_diagonal_phase`` against ``apply_pauli_rotations`` within CIRCUIT_TOL = 1e-12.

Register sizes: SIZES, at most 2^14 amplitudes, except: n = 19 once for every reducing kernel (the smallest register on
which the capped grid of 1024 x 256 threads loops more than once), QSV_OPT_GRID_CAP = 2 at n = 13 for the streaming
kernels (same reason), and n = 22 with gates pending in the deferred queue (the smallest register that defers).

Worst observed errors are printed with their bounds (run with -s).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import diagonal_reference as R
from quantum_computations_amd import DiagonalOperator, _lib
from quantum_computations_amd import workloads as W
from quantum_computations_amd.device import DensityState, DeviceState, QuditState
from quantum_computations_amd.diagonal import flat_diagonal_terms
from quantum_computations_amd.dv_simulator import numpy_quantum as npq

pytestmark = pytest.mark.gpu

TERM_TOL = 1e-13
CIRCUIT_TOL = 1e-12
SIZES = (1, 2, 3, 6, 7, 13, 14)
TERM_COUNTS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 200)      # 3, 4, 5: the build kernel requests four table rows at a time


def maxabs(a):
    return float(np.max(np.abs(a))) if np.size(a) else 0.0


def report(what, err, bound):
    print(f"{what}: {err:.3e} (bound {bound:.3e})")
    assert err <= bound, what


def case(n, seed=0, count=12):
    """(terms, host diagonal, DiagonalOperator, ket, second ket) for an n-qubit register."""
    terms = R.random_z_terms(n, count, seed=100 * n + seed)
    d = R.diagonal_from_terms(n, terms)
    return terms, d, DiagonalOperator.from_terms(n, terms), R.random_ket(n, 10 * n + seed), 1.7 * R.random_ket(n, 10 * n + seed + 1)


# ---- construction -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0,) + SIZES)
def test_from_terms_is_bit_equal_to_the_numpy_loop(n):
    for count in TERM_COUNTS:
        terms = R.random_z_terms(n, count, seed=7 * n + count)
        if n and count >= 2:
            assert 0 in terms[0][2] and n - 1 in terms[1][2]               # masks that touch qubit 0 and qubit n - 1
        want = R.diagonal_from_terms(n, terms)
        op = DiagonalOperator.from_terms(n, terms)
        assert op.num_qubits == n and len(op) == 1 << n
        assert op.last_kernel() == "k_diag_build<false>"
        got = op.to_numpy()
        assert np.array_equal(got, want), (n, count, maxabs(got - want))
        assert np.array_equal(npq.diagonal_of(terms, n), want)
        # accumulate: the second half on top of the first
        half = DiagonalOperator.from_terms(n, terms[:count // 2])
        assert half.add_terms(terms[count // 2:]) is half
        assert np.array_equal(half.to_numpy(), want), (n, count)
        if count > count // 2:
            assert half.last_kernel() == "k_diag_build<true>"
        assert op.extrema() == R.extrema(want)
        assert op.last_kernel() == "k_diag_extrema"


def test_empty_lists_identity_terms_and_the_letter_limit():
    n = 6
    op = DiagonalOperator.from_numpy(np.arange(64.0))
    assert op.add_terms([]) is op and np.array_equal(op.to_numpy(), np.arange(64.0))      # nothing to add: left alone
    op._set_terms(flat_diagonal_terms([]), accumulate=False)
    assert not op.to_numpy().any()                                                         # n_terms = 0 zeroes the vector
    op.add_terms([(2.5, "", []), (-1.0, "II", [3, 0])])
    assert np.array_equal(op.to_numpy(), np.full(64, 1.5))                                 # identities add constants
    assert np.array_equal(DiagonalOperator.zeros(n).to_numpy(), np.zeros(64))
    with pytest.raises(ValueError):
        DiagonalOperator.from_terms(n, [(1.0, "I" * 65, list(range(65)))])                 # 65 letters: past the limit of 64
    lib, h = _lib.load(), op._h                                                            # and the C entry point itself
    assert lib.qsv_diag_set_pauli_sum(h, 1, (C.c_int * 2)(0, 65), (C.c_int * 65)(*([0] * 65)), b"I" * 65, None, 1, None) == _lib.QSV_EINVAL
    assert np.array_equal(op.to_numpy(), np.full(64, 1.5))


def test_windows_of_upload_and_download():
    n = 7
    values = np.random.default_rng(1).standard_normal(128)
    op = DiagonalOperator.from_numpy(values)
    assert np.array_equal(op.to_numpy(), values)
    assert np.array_equal(op.download(0, 5), values[:5]) and np.array_equal(op.download(120, 8), values[120:])
    assert np.array_equal(op.download(127, 1), values[127:]) and op.download(128, 0).size == 0
    op.upload([9.0, 8.0], offset=126)
    op.upload([7.0], offset=0)
    values[126:], values[0] = [9.0, 8.0], 7.0
    assert np.array_equal(op.to_numpy(), values)
    for offset, count in ((0, 129), (128, 1), (129, 0), (1, 128)):
        with pytest.raises(ValueError):
            op.download(offset, count)
    with pytest.raises(ValueError):
        op.upload(np.zeros(3), offset=126)
    assert np.array_equal(op.to_numpy(), values)
    assert DiagonalOperator.from_numpy([4.0]).num_qubits == 0


def test_extrema_with_repeated_values():
    values = np.array([3.0, -1.0, 7.0, -1.0, 7.0, 0.0, 2.0, -1.0] * 1024)             # 2^13: minima and maxima in every workgroup
    op = DiagonalOperator.from_numpy(values)
    assert op.extrema() == (-1.0, 1, 7.0, 2)
    values[1], values[2] = 0.0, 0.0
    op.upload(values)
    assert op.extrema() == (-1.0, 3, 7.0, 4)
    flat = DiagonalOperator.from_numpy(np.full(1 << 13, 2.5))
    assert flat.extrema() == (2.5, 0, 2.5, 0)
    late = np.zeros(1 << 13)
    late[-1], late[-2] = -4.0, 5.0
    assert DiagonalOperator.from_numpy(late).extrema() == (-4.0, (1 << 13) - 1, 5.0, (1 << 13) - 2)


# ---- the passes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_phase_and_mul_against_numpy(n):
    terms, d, op, psi, phi = case(n)
    scale = maxabs(d)
    for gamma in (0.0, 0.37, -2.9, 41.0):
        st = DeviceState.from_numpy(psi)
        assert st.apply_diagonal_phase(op, gamma) is st and st.last_kernel() == "k_diag_phase<true>"
        report(f"n={n} phase gamma={gamma}", maxabs(st.to_numpy() - R.phase(psi, d, gamma)), TERM_TOL * (1 + abs(gamma) * scale) * maxabs(psi))
    src = DeviceState.from_numpy(psi)
    for coeff in (1.0, -0.6 + 1.3j):
        out = src.apply_diagonal_operator(op, coeff=coeff)
        assert out.last_kernel() == "k_diag_mul<false, true>" and out.num_qubits == n
        report(f"n={n} mul c={coeff}", maxabs(out.to_numpy() - R.mul(psi, d, coeff)), TERM_TOL * abs(coeff) * scale * maxabs(psi))
        dst = DeviceState.from_numpy(phi)
        assert src.apply_diagonal_operator(op, out=dst, coeff=coeff, accumulate=True) is dst
        assert dst.last_kernel() == "k_diag_mul<true, true>"
        report(f"n={n} mul accumulate c={coeff}", maxabs(dst.to_numpy() - R.mul(psi, d, coeff, dst=phi)),
               TERM_TOL * (abs(coeff) * scale * maxabs(psi) + maxabs(phi)))
    assert np.array_equal(src.to_numpy(), psi)                                   # the source is only read
    # a destination full of NaN comes out clean when not accumulating, and takes the source's size
    dirty = DeviceState.from_numpy(np.full(1 << (n + 1), np.nan + 1j * np.nan))
    src.apply_diagonal_operator(op, out=dirty, coeff=2.0)
    assert dirty.num_qubits == n
    report(f"n={n} mul into NaN", maxabs(dirty.to_numpy() - R.mul(psi, d, 2.0)), TERM_TOL * 2.0 * scale * maxabs(psi))
    # D psi in place
    assert src.apply_diagonal_operator(op, out=src, coeff=1j) is src
    report(f"n={n} mul in place", maxabs(src.to_numpy() - R.mul(psi, d, 1j)), TERM_TOL * scale * maxabs(psi))
    with pytest.raises(ValueError):
        src.apply_diagonal_operator(op, out=src, accumulate=True)
    src.set_option(_lib.OPT_NONTEMPORAL, 0)
    src.upload(psi)
    src.apply_diagonal_phase(op, 0.37)
    assert src.last_kernel() == "k_diag_phase<false>"
    report(f"n={n} phase, plain loads", maxabs(src.to_numpy() - R.phase(psi, d, 0.37)), TERM_TOL * (1 + 0.37 * scale) * maxabs(psi))
    src.apply_diagonal_operator(op, out=src)
    assert src.last_kernel() == "k_diag_mul<false, false>"


def check_moments(what, st, op, psi, d):
    scale = maxabs(d)
    norm2 = float(np.sum(np.abs(psi) ** 2))
    for threshold in (None, float(d.min()), float(np.sort(d)[d.size // 2]), float(d.max())):
        got = st.expect_diagonal(op, threshold)
        assert st.last_kernel() == ("k_diag_expect<false>" if threshold is None else "k_diag_expect<true>")
        want = R.moments(psi, d, threshold)
        report(f"{what} norm2", abs(got.norm2 - want[0]), 1e-13 * norm2)
        report(f"{what} mean", abs(got.mean - want[1]), TERM_TOL * scale * norm2)
        report(f"{what} second moment", abs(got.second_moment - want[2]), TERM_TOL * scale ** 2 * norm2)
        report(f"{what} probability below {threshold}", abs(got.probability_below - want[3]), TERM_TOL * norm2)
        if threshold is None:
            assert got.probability_below == 0.0
        elif threshold == d.max():
            assert got.probability_below == got.norm2                            # every amplitude counted, the same sum
        assert st.expect_diagonal(op, threshold) == got                          # deterministic
    return scale, norm2


@pytest.mark.parametrize("n", SIZES)
def test_reductions_against_numpy(n):
    terms, d, op, psi, phi = case(n, seed=1)
    st, other = DeviceState.from_numpy(phi), DeviceState.from_numpy(psi)
    scale, norm2 = check_moments(f"n={n}", st, op, phi, d)
    want = R.moments(phi, d)
    # second - mean^2: the bound of the second moment plus 2 |mean| times the bound of the mean, |mean| <= max|d| norm2
    report(f"n={n} variance", abs(st.variance_diagonal(op) - (want[2] - want[1] ** 2)), TERM_TOL * scale ** 2 * norm2 * (1 + 2 * norm2))
    bound = TERM_TOL * scale * np.linalg.norm(phi) * np.linalg.norm(psi)
    value = st.transition_diagonal(op, other)
    assert st.last_kernel() == "k_diag_transition"
    report(f"n={n} transition", abs(value - R.transition(phi, psi, d)), bound)
    report(f"n={n} transition, one register twice", abs(st.transition_diagonal(op, st) - want[1]), TERM_TOL * scale * norm2)
    assert st.transition_diagonal(op, other) == value
    assert np.array_equal(st.to_numpy(), phi) and np.array_equal(other.to_numpy(), psi)      # read-only
    # the fused step: <lambda|D|psi>, then the phase on both
    gamma = -0.83
    got = other.diagonal_phase_adjoint(op, st, gamma)                                        # psi = other, lambda = st
    assert other.last_kernel() == "k_diag_phase_adjoint<true>"
    value, psi2, lam2 = R.phase_adjoint(psi, phi, d, gamma)
    report(f"n={n} phase_adjoint value", abs(got - value), bound)
    report(f"n={n} phase_adjoint psi", maxabs(other.to_numpy() - psi2), TERM_TOL * (1 + abs(gamma) * scale) * maxabs(psi))
    report(f"n={n} phase_adjoint lambda", maxabs(st.to_numpy() - lam2), TERM_TOL * (1 + abs(gamma) * scale) * maxabs(phi))
    report(f"n={n} the value after the phase", abs(st.transition_diagonal(op, other) - value), 3 * bound)


def test_reducing_kernels_beyond_the_capped_grid():
    n = 19
    terms, d, op, psi, phi = case(n, seed=2, count=5)
    assert op.extrema() == R.extrema(d)
    st, other = DeviceState.from_numpy(phi), DeviceState.from_numpy(psi)
    scale, norm2 = check_moments(f"n={n}", st, op, phi, d)
    bound = TERM_TOL * scale * np.linalg.norm(phi) * np.linalg.norm(psi)
    report(f"n={n} transition", abs(st.transition_diagonal(op, other) - R.transition(phi, psi, d)), bound)
    value, psi2, lam2 = R.phase_adjoint(psi, phi, d, 0.41)
    report(f"n={n} phase_adjoint value", abs(other.diagonal_phase_adjoint(op, st, 0.41) - value), bound)
    report(f"n={n} phase_adjoint psi", maxabs(other.to_numpy() - psi2), TERM_TOL * (1 + 0.41 * scale) * maxabs(psi))
    report(f"n={n} phase_adjoint lambda", maxabs(st.to_numpy() - lam2), TERM_TOL * (1 + 0.41 * scale) * maxabs(phi))


def test_streaming_kernels_under_a_small_grid_cap():
    n = 13
    terms = R.random_z_terms(n, 65, seed=3)
    d = R.diagonal_from_terms(n, terms)
    op = DiagonalOperator.zeros(n)
    op.set_option(_lib.OPT_GRID_CAP, 2)                    # 512 threads walk 8192 entries: sixteen trips each
    op.add_terms(terms[:30])
    op.add_terms(terms[30:])
    assert np.array_equal(op.to_numpy(), d)
    assert op.extrema() == R.extrema(d)
    for bad in (_lib.OPT_NONTEMPORAL, _lib.OPT_UNROLL, 99):
        with pytest.raises(ValueError):
            op.set_option(bad, 1)
    psi, phi = R.random_ket(n, 4), R.random_ket(n, 5)
    scale = maxabs(d)
    st, dst = DeviceState.from_numpy(psi), DeviceState.from_numpy(phi)
    for register in (st, dst):
        register.set_option(_lib.OPT_GRID_CAP, 2)
    st.apply_diagonal_phase(op, 0.7)
    report("capped phase", maxabs(st.to_numpy() - R.phase(psi, d, 0.7)), TERM_TOL * (1 + 0.7 * scale) * maxabs(psi))
    st.upload(psi)
    st.apply_diagonal_operator(op, out=dst, coeff=0.5j, accumulate=True)
    report("capped mul", maxabs(dst.to_numpy() - R.mul(psi, d, 0.5j, dst=phi)), TERM_TOL * (0.5 * scale * maxabs(psi) + maxabs(phi)))
    st.apply_diagonal_operator(op, out=dst)
    report("capped mul, overwriting", maxabs(dst.to_numpy() - R.mul(psi, d)), TERM_TOL * scale * maxabs(psi))
    check_moments("capped", st, op, psi, d)


def test_pending_deferred_queues_are_flushed_first():
    import test_gpu_deferred as D
    n = 22
    op = DiagonalOperator.from_terms(n, R.random_z_terms(n, 9, seed=8))
    a, b = D.pending_pair(n)                              # a has gates queued, b is its un-deferred twin
    queued = a.defer_stats()[0]
    assert a.expect_diagonal(op, 0.0) == b.expect_diagonal(op, 0.0)
    a, b = D.pending_pair(n)
    a.apply_diagonal_phase(op, 0.3)
    b.apply_diagonal_phase(op, 0.3)
    assert a.defer_stats()[0] == queued                   # the call was never queued itself
    assert np.array_equal(a.to_numpy(), b.to_numpy())     # the QSV_DEFER=0 order of operations, bit for bit


# ---- against the existing calls -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,name", [(6, "random"), (13, "random"), (12, "maxcut"), (8, "sk")])
def test_against_the_pauli_sum_calls(n, name):
    terms = {"random": lambda: R.random_z_terms(n, 20, seed=n), "maxcut": lambda: W.maxcut_terms(n, W.ring_chord_edges(n)),
             "sk": lambda: W.sk_terms(n, 2)}[name]()
    weight = sum(abs(c) for c, _, _ in terms)
    op = DiagonalOperator.from_terms(n, terms)
    psi = R.random_ket(n, 6)
    a, b = DeviceState.from_numpy(psi), DeviceState.from_numpy(psi)
    report(f"{name} n={n} mean against expect_pauli_sum", abs(a.expect_diagonal(op).mean - a.expect_pauli_sum(terms).real), 2 * TERM_TOL * weight)
    gamma = 0.45
    a.apply_diagonal_phase(op, gamma)
    b.apply_pauli_rotations([(2 * gamma * c, letters, qubits) for c, letters, qubits in terms if "Z" in letters.upper()])
    constant = sum(c for c, letters, _ in terms if "Z" not in letters.upper())      # the identity terms: a global phase
    report(f"{name} n={n} phase against apply_pauli_rotations", maxabs(a.to_numpy() - np.exp(-1j * gamma * constant) * b.to_numpy()), CIRCUIT_TOL)
    # npq: host arrays are lifted, registers are used as they are
    report(f"{name} n={n} npq phase of a host ket", maxabs(npq.apply_diagonal_phase(op, psi, gamma) - a.to_numpy()), 0.0)
    assert npq.apply_diagonal_phase(npq.diagonal_of(terms, n), b.copy(), 0.0).num_qubits == n
    assert npq.expect_diagonal(npq.diagonal_of(terms, n), psi, 0.0) == DeviceState.from_numpy(psi).expect_diagonal(op, 0.0)
    with pytest.raises(TypeError):
        npq.expect_diagonal(op, R.random_ket(n - 1, 1))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_from_python():
    n = 6
    terms, d, op, psi, phi = case(n, seed=3)
    st, other = DeviceState.from_numpy(psi), DeviceState.from_numpy(phi)
    for bad in ([(1.0, "X", [0])], [(1.0, "ZY", [0, 1])], [(0.5j, "Z", [0])], [(1.0 + 1e-30j, "ZZ", [0, 1])], [(1.0, "Z", [n])],
                [(1.0, "Z", [-1])], [(1.0, "ZZ", [2, 2])], [(1.0, "ZZ", [2])]):
        with pytest.raises(ValueError):
            DiagonalOperator.from_terms(n, bad)
        with pytest.raises(ValueError):
            op.add_terms(terms[:2] + bad)
    assert np.array_equal(op.to_numpy(), d)                                     # a refused list changes nothing
    for bad in (np.zeros(3), np.zeros((2, 2)), np.zeros(4, dtype=complex), np.zeros(0)):
        with pytest.raises(ValueError):
            DiagonalOperator.from_numpy(bad)
    with pytest.raises(ValueError):
        DiagonalOperator.zeros(41)
    # sizes
    small_op, small = DiagonalOperator.zeros(n - 1), DeviceState.from_numpy(R.random_ket(n - 1, 1))
    for call in (lambda: st.apply_diagonal_phase(small_op, 0.1), lambda: small.apply_diagonal_phase(op, 0.1),
                 lambda: st.expect_diagonal(small_op), lambda: st.apply_diagonal_operator(small_op, out=other),
                 lambda: st.transition_diagonal(op, small), lambda: small.transition_diagonal(op, st),
                 lambda: st.diagonal_phase_adjoint(op, small, 0.1), lambda: st.diagonal_phase_adjoint(op, st, 0.1),
                 lambda: small.apply_diagonal_operator(small_op, out=other, accumulate=True)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(MemoryError):
        st.apply_diagonal_operator(op, out=small)
    # devices
    if _lib.device_count() > 1:
        far = DiagonalOperator.from_terms(n, terms, device=1)
        with pytest.raises(ValueError):
            st.apply_diagonal_phase(far, 0.1)
        with pytest.raises(ValueError):
            st.expect_diagonal(far)
    with pytest.raises(ValueError):
        DiagonalOperator.zeros(n, device=_lib.device_count())
    # mode registers
    modes, lib = QuditState.zeros(3, 3), _lib.load()
    out, re, im = np.zeros(4), C.c_double(), C.c_double()
    S = _lib.QSV_ESTATE
    assert lib.qsv_apply_diag_phase(modes._h, op._h, 0.1) == S
    assert lib.qsv_apply_diag_mul(modes._h, st._h, op._h, 1.0, 0.0, 0) == S and lib.qsv_apply_diag_mul(st._h, modes._h, op._h, 1.0, 0.0, 0) == S
    assert lib.qsv_expect_diag(modes._h, op._h, None, out.ctypes.data_as(C.POINTER(C.c_double))) == S
    assert lib.qsv_diag_transition(modes._h, st._h, op._h, C.byref(re), C.byref(im)) == S
    assert lib.qsv_diag_transition(st._h, modes._h, op._h, C.byref(re), C.byref(im)) == S
    assert lib.qsv_diag_phase_adjoint(modes._h, st._h, op._h, 0.1, C.byref(re), C.byref(im)) == S
    assert lib.qsv_diag_phase_adjoint(st._h, modes._h, op._h, 0.1, C.byref(re), C.byref(im)) == S
    # something that is not a DiagonalOperator
    with pytest.raises(TypeError):
        st.apply_diagonal_phase(d, 0.1)
    with pytest.raises(TypeError):
        st.expect_diagonal(other)
    # density registers
    rho = DensityState.from_numpy(np.eye(1 << (n // 2)) / (1 << (n // 2)))          # a 2 (n/2) = n-qubit register underneath
    for call in (lambda: rho.apply_diagonal_phase(op, 0.1), lambda: rho.apply_diagonal_operator(op), lambda: rho.expect_diagonal(op),
                 lambda: rho.variance_diagonal(op), lambda: rho.transition_diagonal(op, st), lambda: st.transition_diagonal(op, rho),
                 lambda: st.apply_diagonal_operator(op, out=rho), lambda: st.diagonal_phase_adjoint(op, rho, 0.1),
                 lambda: rho.diagonal_phase_adjoint(op, st, 0.1)):
        with pytest.raises(ValueError):
            call()
    # a closed handle
    closed = DiagonalOperator.from_terms(n, terms)
    closed.close()
    closed.close()
    for call in (lambda: st.apply_diagonal_phase(closed, 0.1), lambda: st.expect_diagonal(closed), closed.to_numpy, closed.extrema,
                 lambda: closed.add_terms(terms), lambda: st.transition_diagonal(closed, other)):
        with pytest.raises(ValueError):
            call()
    # nothing was touched by any of it
    assert np.array_equal(st.to_numpy(), psi) and np.array_equal(other.to_numpy(), phi) and np.array_equal(op.to_numpy(), d)
