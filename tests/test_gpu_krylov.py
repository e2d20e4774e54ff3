"""qsv_lincomb / qsv_inner_many, ``DeviceState.lincomb`` / ``inner_many`` and quantum_computations_amd/krylov.py
(``lanczos``, ``ground_state``, ``evolve_krylov`` and the ``npq`` wrappers) against NumPy: the BLAS-1 passes against
``numpy`` sums and ``numpy.vdot``, the Krylov methods against tests/krylov_reference.py (pinned against dense matrices in
tests/test_krylov_reference_host.py) and against ``eigvalsh`` / ``expm`` of the dense matrix.

Tolerances.

* lincomb: max-abs ``1e-13 (|beta| max|dst| + sum_k |c_k| max|src_k|)``, the project's TERM_TOL convention: an element is
  a sum of at most 18 complex products, rounding error at most about 20 eps of that scale.  ``norm2``: 1e-13 relative to
  the squared norm of the values the call stored (downloaded): at most 2^19 non-negative summands added in a tree of
  per-thread, per-wave, per-workgroup and host sums, error a few eps relative.
* inner_many: ``1e-13 ||x_k|| ||y||``.
* Lanczos (10 qubits, m = 20): orthogonality 1e-12, the Lanczos relation and alphas / betas ``1e-12 sum|c_t|``, Ritz
  values ``1e-11 sum|c_t|`` -- the host restatement reaches 7e-16, 7e-17 and 1.4e-16 of those scales.
* ground_state: ``|E - E0| <= 1e-12 sum|c_t|`` against eigvalsh, true residual ``<= 10 tol sum|c_t|``.
* evolve_krylov: error against expm at most ``tol`` (relative to the state's norm), norm preserved to 1e-12.

Register sizes: at most 2^14 amplitudes, except in two kinds of test.  The reducing kernels (k_inner_many, and k_lincomb
when it forms the norm) run on a grid of at most 1024 workgroups x 256 threads, one amplitude per thread and trip: 2^19
amplitudes (8 MiB) is the smallest register on which their loop runs more than once (test_beyond_the_capped_grid).  A
k_lincomb pass without the norm has no cap but the dispatch limit, its loop runs more than once only beyond 2^32
amplitudes; QSV_OPT_GRID_CAP, which both kernels honour, makes it loop on a small register instead
(test_small_grid_cap).  The deferred-queue test uses 2^22 amplitudes, as tests/test_gpu_deferred.py needs for a queue to
be pending.

Worst observed errors are printed with their bounds (run with -s).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import scipy.linalg

import krylov_reference as K
from quantum_computations_amd import _lib, krylov
from quantum_computations_amd import workloads as W
from quantum_computations_amd.device import DensityState, DeviceState, QuditState
from quantum_computations_amd.dv_simulator import numpy_quantum as npq

pytestmark = pytest.mark.gpu

TERM_TOL = 1e-13
SIZES = (1, 2, 3, 6, 7, 13, 14)
BETAS = (0.0, 1.0, 0.4 - 0.9j)


def random_ket(n, seed=0, norm=1.0):
    rng = np.random.default_rng(1000 * n + seed)
    ket = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    return ket * (norm / np.linalg.norm(ket))


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))))


def handles(registers):
    return (C.c_void_p * max(len(registers), 1))(*[r._h for r in registers])


def dbl(array):
    return array.ctypes.data_as(C.POINTER(C.c_double))


def raw_lincomb(dst, coeffs, sources, beta=0.0, want_norm=False):
    """The C entry point itself: (status, norm2 or None, passes)."""
    cbuf = np.ascontiguousarray(coeffs, dtype=np.complex128).reshape(-1)
    norm2, passes = C.c_double(np.nan), C.c_uint64(12345)
    status = _lib.load().qsv_lincomb(dst._h, complex(beta).real, complex(beta).imag, len(sources), handles(sources), dbl(cbuf.view(np.float64)),
                                     C.byref(norm2) if want_norm else None, C.byref(passes))
    return status, (norm2.value if want_norm else None), passes.value


def raw_inner_many(y, xs):
    values = np.full(max(len(xs), 1), np.nan, dtype=np.complex128)
    passes = C.c_uint64(12345)
    status = _lib.load().qsv_inner_many(y._h, len(xs), handles(xs), dbl(values.view(np.float64)), C.byref(passes))
    return status, values[:len(xs)], passes.value


def lincomb_model(beta, old, coeffs, kets):
    want = beta * old if beta != 0 else np.zeros_like(old)
    for c, ket in zip(coeffs, kets):
        want = want + c * ket
    bound = TERM_TOL * (abs(beta) * (np.max(np.abs(old)) if beta != 0 else 0.0) + sum(abs(c) * np.max(np.abs(k)) for c, k in zip(coeffs, kets)))
    return want, bound


def check_lincomb(dst, old, beta, coeffs, registers, kets, label):
    """One qsv_lincomb with the norm and one without, on a destination holding ``old`` (NaN where beta == 0)."""
    worst = 0.0
    for want_norm in (True, False):
        dst.upload(np.full_like(old, np.nan) if beta == 0 else old)
        status, norm2, passes = raw_lincomb(dst, coeffs, registers, beta, want_norm)
        assert status == _lib.QSV_OK, label
        got = dst.to_numpy()
        want, bound = lincomb_model(beta, old, coeffs, kets)
        bound = max(bound, 0.0)
        assert np.all(np.isfinite(got.view(np.float64))), label
        error = maxdiff(got, want)
        assert error <= bound, (label, error, bound)
        worst = max(worst, error / bound if bound else 0.0)
        count = len(registers)
        assert passes == max(1, -(-count // 8)), label
        last = count - 8 * (passes - 1)
        nt = "true"
        assert dst.last_kernel() == f"k_lincomb<{last}, {'true' if (beta != 0 or passes > 1) else 'false'}, {'true' if want_norm else 'false'}, {nt}>", label
        if want_norm:
            stored = float(np.vdot(got, got).real)
            assert abs(norm2 - stored) <= 1e-13 * stored, (label, norm2, stored)
    return worst


# ---- lincomb ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_lincomb_against_numpy(n):
    rng = np.random.default_rng(n)
    kets = [random_ket(n, 10 + k, norm=0.5 + 0.25 * k) for k in range(17)]
    registers = [DeviceState.from_numpy(ket) for ket in kets]
    old = random_ket(n, 99, norm=1.3)
    dst = DeviceState.from_numpy(old)
    worst = 0.0
    for count in (0, 1, 2, 3, 5, 8, 9, 17):
        coeffs = rng.standard_normal(count) + 1j * rng.standard_normal(count)
        for beta in BETAS:
            worst = max(worst, check_lincomb(dst, old, beta, coeffs, registers[:count], kets[:count], (n, count, beta)))
    # sources repeat
    pick = [0, 3, 0, 0, 5, 3]
    coeffs = rng.standard_normal(len(pick)) + 1j * rng.standard_normal(len(pick))
    worst = max(worst, check_lincomb(dst, old, 0.0, coeffs, [registers[k] for k in pick], [kets[k] for k in pick], (n, "repeated")))
    # the sources are exactly what was uploaded
    for register, ket in zip(registers, kets):
        assert np.array_equal(register.to_numpy(), ket)
    print(f"lincomb n={n}: worst error / bound = {worst:.3f} (bound: 1e-13 (|beta| max|dst| + sum |c_k| max|src_k|))")


def test_lincomb_methods_and_a_view_as_destination():
    n = 9
    kets = [random_ket(n, k) for k in range(3)]
    registers = [DeviceState.from_numpy(ket) for ket in kets]
    coeffs = [0.5 - 1j, 2.0, -0.25j]
    owner = DeviceState.from_numpy(np.full(2 << n, np.nan + 0j))               # the view is a window into its second half
    view = DeviceState.view(n, owner.device_ptr + 16 * (1 << n), 1 << n, keepalive=owner)
    assert view.lincomb(coeffs, registers) is view
    view.sync()
    want, bound = lincomb_model(0.0, kets[0], coeffs, kets)
    assert maxdiff(owner.download(1 << n, 1 << n), want) <= bound and np.all(np.isnan(owner.download(0, 1 << n).real))
    out, norm2 = view.lincomb(coeffs[:2], registers[:2], beta=-0.5j, return_norm2=True)
    want2, bound2 = lincomb_model(-0.5j, want, coeffs[:2], kets[:2])
    assert out is view and maxdiff(view.to_numpy(), want2) <= bound2 + 0.5 * bound
    assert abs(norm2 - np.vdot(want2, want2).real) <= 1e-12 * norm2
    # a smaller destination takes the sources' size when beta == 0
    big = DeviceState.zeros(n)
    big.lincomb([1.0], [DeviceState.from_numpy(random_ket(n - 2, 7))])
    assert big.num_qubits == n - 2 and np.array_equal(big.to_numpy(), random_ket(n - 2, 7))
    with pytest.raises(ValueError):
        view.lincomb([1.0, 2.0], registers[:1])                               # one coefficient per source
    # a density register inherits both
    rho = DensityState.from_numpy(np.outer(kets[0][:8], kets[1][:8].conj()))
    sigma = DensityState.from_numpy(np.outer(kets[2][:8], kets[2][:8].conj()))
    values = rho.inner_many([sigma, rho])
    assert abs(values[0] - np.vdot(sigma.to_numpy(), rho.to_numpy())) <= 1e-13
    rho.lincomb([2.0], [sigma], beta=1.0)


# ---- inner_many -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_inner_many_against_vdot(n):
    kets = [random_ket(n, 20 + k, norm=0.5 + 0.25 * k) for k in range(17)]
    registers = [DeviceState.from_numpy(ket) for ket in kets]
    y_ket = random_ket(n, 77, norm=1.9)
    y = DeviceState.from_numpy(y_ket)
    worst = 0.0
    for count in (1, 2, 3, 8, 9, 17):
        xs, x_kets = list(registers[:count]), list(kets[:count])
        xs[count // 2], x_kets[count // 2] = y, y_ket                        # one x_k is y itself
        status, values, passes = raw_inner_many(y, xs)
        assert status == _lib.QSV_OK and passes == -(-count // 8)
        assert y.last_kernel() == f"k_inner_many<{count - 8 * (passes - 1)}>"
        for k in range(count):
            bound = 1e-13 * np.linalg.norm(x_kets[k]) * np.linalg.norm(y_ket)
            error = abs(values[k] - np.vdot(x_kets[k], y_ket))
            assert error <= bound, (n, count, k, error, bound)
            worst = max(worst, error / bound)
        again = raw_inner_many(y, xs)[1]
        assert np.array_equal(values.view(np.float64), again.view(np.float64)), "bit-identical from run to run"
        assert np.array_equal(y.inner_many(xs).view(np.float64), values.view(np.float64))
    assert np.array_equal(y.to_numpy(), y_ket) and all(np.array_equal(r.to_numpy(), k) for r, k in zip(registers, kets))
    assert y.inner_many([]).size == 0
    print(f"inner_many n={n}: worst error / bound = {worst:.3f} (bound: 1e-13 ||x_k|| ||y||)")


# ---- grid-stride loops ------------------------------------------------------------------------------------------------------------
def test_beyond_the_capped_grid():
    """2^19 amplitudes on 1024 x 256 threads: two trips per thread in k_inner_many and in k_lincomb with the norm."""
    n = 19
    kets = [random_ket(n, k) for k in range(3)]
    registers = [DeviceState.from_numpy(ket) for ket in kets]
    y = registers[2]
    status, values, passes = raw_inner_many(y, registers)
    assert status == _lib.QSV_OK and passes == 1
    for k in range(3):
        assert abs(values[k] - np.vdot(kets[k], kets[2])) <= 1e-13
    dst = DeviceState.zeros(n)
    for beta in (0.0, 0.3 + 0.2j):
        old = random_ket(n, 9)
        worst = check_lincomb(dst, old, beta, [0.5 - 1j, 2.0], registers[:2], kets[:2], ("beyond the grid", beta))
        pick = [0, 1, 2, 1, 0]               # five sources, some repeated
        worst = max(worst, check_lincomb(dst, old, beta, np.arange(1, 6) * (0.2 + 0.1j), [registers[k] for k in pick], [kets[k] for k in pick],
                                         ("beyond the grid, 5 sources", beta)))
        print(f"n=19, beta={beta}: lincomb worst error / bound = {worst:.3f}")


def test_small_grid_cap():
    """QSV_OPT_GRID_CAP = 3: every thread of every kernel loops, 11 trips on 2^13 amplitudes."""
    n = 13
    kets = [random_ket(n, k) for k in range(9)]
    registers = [DeviceState.from_numpy(ket) for ket in kets]
    old = random_ket(n, 9)
    dst = DeviceState.from_numpy(old)
    dst.set_option(_lib.OPT_GRID_CAP, 3)
    coeffs = np.arange(1, 10) * (0.3 - 0.1j)
    for count in (9, 5, 2):                  # the last pass, which forms the norm, has 1, 5 and 2 sources
        for beta in (0.0, 1.0):
            check_lincomb(dst, old, beta, coeffs[:count], registers[:count], kets[:count], ("grid cap", count, beta))
    y = registers[0]
    y.set_option(_lib.OPT_GRID_CAP, 3)
    values = y.inner_many(registers)
    for k in range(9):
        assert abs(values[k] - np.vdot(kets[k], kets[0])) <= 1e-13


# ---- Lanczos ----------------------------------------------------------------------------------------------------------------------
N = 10


@pytest.fixture(scope="module", params=["heisenberg", "ising"])
def model(request):
    """(terms, dense H, eigenvalues, sum|c_t|, start ket), computed once."""
    terms = W.heisenberg_chain_terms(N) if request.param == "heisenberg" else W.ising_terms(N, 1.0)
    H = K.dense(terms, N)
    return terms, H, np.linalg.eigvalsh(H), K.scale_of(terms), random_ket(N, 3)


def test_lanczos_with_reorthogonalisation(model):
    terms, H, _, scale, ket = model
    start = DeviceState.from_numpy(1.7 * ket)
    alphas, betas, basis, breakdown = krylov.lanczos(terms, start, 20)
    assert not breakdown and len(alphas) == len(betas) == len(basis) == 20
    assert np.array_equal(start.to_numpy(), 1.7 * ket)
    V = np.array([v.to_numpy() for v in basis])
    orth = np.abs(V.conj() @ V.T - np.eye(20)).max()
    residual = H @ V.T - V.T @ K.tridiagonal(alphas, betas)
    relation = max(np.abs(residual[:, :-1]).max(), abs(np.linalg.norm(residual[:, -1]) - betas[-1])) / scale
    ref_alphas, ref_betas, *_ = K.lanczos(terms, 1.7 * ket, 20)
    ritz = np.abs(np.linalg.eigvalsh(K.tridiagonal(alphas, betas)) - np.linalg.eigvalsh(K.tridiagonal(ref_alphas, ref_betas))).max() / scale
    print(f"lanczos: orthogonality {orth:.2e} (1e-12), relation {relation:.2e} (1e-12), Ritz values {ritz:.2e} (1e-11)")
    assert orth <= 1e-12 and relation <= 1e-12 and ritz <= 1e-11
    for v in basis:
        v.close()


def test_lanczos_without_reorthogonalisation(model):
    terms, _, _, scale, ket = model
    alphas, betas, basis, breakdown = krylov.lanczos(terms, DeviceState.from_numpy(ket), 10, reorthogonalise=False)
    ref_alphas, ref_betas, *_ = K.lanczos(terms, ket, 10, False)
    worst = max(np.abs(alphas - ref_alphas).max(), np.abs(betas - ref_betas).max()) / scale
    print(f"three-term recurrence: alphas / betas off by {worst:.2e} sum|c_t| (bound 1e-12)")
    assert not breakdown and len(basis) == 10 and worst <= 1e-12


def test_breakdown_on_an_invariant_subspace():
    terms = W.heisenberg_chain_terms(3)
    ket = random_ket(3, 1)
    for reorthogonalise in (True, False):
        alphas, betas, basis, breakdown = krylov.lanczos(terms, DeviceState.from_numpy(ket), 20, reorthogonalise=reorthogonalise)
        assert breakdown and len(alphas) == len(betas) == len(basis) == 3
        assert np.all(np.isfinite(alphas)) and np.all(np.isfinite(betas)) and betas[-1] <= 1e-12 * K.scale_of(terms)
        assert all(np.all(np.isfinite(v.to_numpy().view(np.float64))) for v in basis)
    state = DeviceState.from_numpy(ket)
    info = state.evolve_krylov(terms, 1.0, m=20)
    error = np.linalg.norm(state.to_numpy() - scipy.linalg.expm(-1j * K.dense(terms, 3)) @ ket)
    print(f"3-qubit chain: one substep, error {error:.2e} (bound 1e-14)")
    assert info["substeps"] == 1 and error <= 1e-14
    energy, ground, ginfo = DeviceState.from_numpy(ket).ground_state_of(terms, m=20)
    assert ginfo["breakdown"] and ginfo["restarts"] == 0
    assert abs(energy - np.linalg.eigvalsh(K.dense(terms, 3))[0]) <= 1e-12 * K.scale_of(terms)


# ---- ground_state -----------------------------------------------------------------------------------------------------------------
def test_ground_state(model):
    terms, H, eigenvalues, scale, ket = model
    tol = 1e-10
    start = DeviceState.from_numpy(ket)
    energy, ground, info = krylov.ground_state(terms, start, m=20, tol=tol)
    v = ground.to_numpy()
    error, residual = abs(energy - eigenvalues[0]), np.linalg.norm(H @ v - energy * v)
    print(f"ground_state: |E - E0| = {error:.2e} (bound {1e-12 * scale:.2e}), residual {residual:.2e} (bound {10 * tol * scale:.2e}), "
          f"estimate {info['residual']:.2e}, restarts {info['restarts']}, applications {info['applications']}, passes {info['passes']}")
    assert np.array_equal(start.to_numpy(), ket)
    assert error <= 1e-12 * scale and residual <= 10 * tol * scale and abs(np.linalg.norm(v) - 1.0) <= 1e-12
    cycles = info["restarts"] + 1
    assert info["applications"] == 20 * cycles and not info["breakdown"] and info["residual"] <= tol * scale
    # per cycle: copy + scale, 20 x (H passes + 2 inner_many + 2 lincomb), 19 scalings, ceil(20 / 8) passes for the Ritz vector
    h_passes = krylov._Counter()
    krylov._apply(krylov._flat_terms(krylov._real_terms(terms, "test")), start, ground, h_passes)
    vector = sum(2 * -(-(j + 1) // 8) * 2 for j in range(20))
    assert info["passes"] == cycles * (2 + 20 * h_passes.passes + vector + 19 + 3)
    assert len(info["ritz_values"]) == 20 and info["ritz_values"][0] == energy
    # a random start by number of qubits, through npq
    energy2, ground2, info2 = npq.ground_state(npq.PauliSum(N, terms), m=20, seed=4)
    assert abs(energy2 - eigenvalues[0]) <= 1e-12 * scale and isinstance(ground2, DeviceState)
    energy3, ground3, _ = npq.ground_state(npq.PauliSum(N, terms), ket, m=20)
    assert isinstance(ground3, np.ndarray) and energy3 == energy
    with pytest.raises(RuntimeError):
        krylov.ground_state(terms, start, m=4, max_restarts=1)


# ---- evolve_krylov ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1.0, -2.0])
def test_evolve_krylov_against_expm(model, t):
    terms, H, _, _, ket = model
    tol = 1e-10
    psi = 1.7 * ket
    want = scipy.linalg.expm(-1j * t * H) @ psi
    state = DeviceState.from_numpy(psi)
    info = state.evolve_krylov(terms, t, m=20, tol=tol)
    got = state.to_numpy()
    error = np.linalg.norm(got - want) / 1.7
    print(f"evolve_krylov t={t}: error {error:.2e} (bound {tol:.0e}), estimate {info['error_estimate']:.2e}, substeps {info['substeps']}, "
          f"applications {info['applications']}, passes {info['passes']}")
    assert error <= tol and abs(np.linalg.norm(got) - 1.7) <= 1e-12
    assert info["applications"] == 20 * info["substeps"]
    host = npq.evolve_exact(npq.PauliSum(N, terms), psi, t, m=20, tol=tol)
    assert isinstance(host, np.ndarray) and np.array_equal(host, got) and np.array_equal(psi, 1.7 * ket)


def test_trotter_lies_within_its_own_error_of_the_krylov_result():
    n, t, steps, tol = 8, 1.0, 200, 1e-10
    terms = W.heisenberg_chain_terms(n)
    hamiltonian = npq.PauliSum(n, terms)
    ket = random_ket(n, 2)
    # the dense reference: one second-order step as a product of exp(-i theta/2 P) = cos - i sin P, to the 200th power
    step = np.eye(1 << n, dtype=complex)
    for theta, letters, qubits in npq.trotter_rotations(hamiltonian, t, steps, 2)[:2 * len(terms)]:
        P = npq.PauliSum(n, [(1.0, letters, qubits)]).matrix()
        step = (np.cos(theta / 2) * np.eye(1 << n) - 1j * np.sin(theta / 2) * P) @ step
    exact = scipy.linalg.expm(-1j * t * hamiltonian.matrix()) @ ket
    trotter_error = np.linalg.norm(np.linalg.matrix_power(step, steps) @ ket - exact)
    a, b = DeviceState.from_numpy(ket), DeviceState.from_numpy(ket)
    a.evolve(terms, t, steps=steps, order=2)
    b.evolve_krylov(terms, t, m=20, tol=tol)
    distance = np.linalg.norm(a.to_numpy() - b.to_numpy())
    # triangle inequality: the Trotter error of the dense reference, the Krylov tolerance, and the rounding of 8400
    # rotations (about 4 eps each in the 2-norm: 4e-12, taken as 1e-11)
    bound = trotter_error + tol + 1e-11
    print(f"Trotter (order 2, {steps} steps) against Krylov: distance {distance:.3e}, reference Trotter error {trotter_error:.3e}")
    assert trotter_error - tol - 1e-11 <= distance <= bound and trotter_error > 1e-8


# ---- deferred queues and refusals ---------------------------------------------------------------------------------------------------
def test_pending_deferred_queues_are_flushed_first():
    import test_gpu_deferred as D
    n = 22
    # destination and sources have gates queued (a, c); b and d are their un-deferred twins
    a, b = D.pending_pair(n)
    c, d = D.pending_pair(n, seed=6)
    queued = a.defer_stats()[0], c.defer_stats()[0]
    _, norm_a = a.lincomb([0.5 - 0.25j], [c], beta=1.5j, return_norm2=True)
    _, norm_b = b.lincomb([0.5 - 0.25j], [d], beta=1.5j, return_norm2=True)
    assert (a.defer_stats()[0], c.defer_stats()[0]) == queued                  # the call was never queued itself
    assert norm_a == norm_b and np.array_equal(a.to_numpy(), b.to_numpy())     # bit for bit
    a, b = D.pending_pair(n)
    c, d = D.pending_pair(n, seed=6)
    assert np.array_equal(a.inner_many([c, a]).view(np.float64), b.inner_many([d, b]).view(np.float64))


def test_refusals_leave_every_register_untouched():
    n = 6
    kets = [random_ket(n, k) for k in range(3)]
    dst, a, b = (DeviceState.from_numpy(ket) for ket in kets)
    small, modes = DeviceState.from_numpy(random_ket(n - 1, 5)), QuditState.zeros(3, 3)
    lib, c = _lib.load(), np.array([1.0, 0.0, 0.5, -0.5])
    values, norm2, passes = np.zeros(4), C.c_double(), C.c_uint64()
    two, with_null, with_dst = handles([a, b]), (C.c_void_p * 2)(a._h, None), handles([a, dst])
    E, S = _lib.QSV_EINVAL, _lib.QSV_ESTATE
    assert lib.qsv_lincomb(None, 0.0, 0.0, 2, two, dbl(c), None, None) == E
    assert lib.qsv_lincomb(dst._h, 0.0, 0.0, 2, None, dbl(c), None, None) == E
    assert lib.qsv_lincomb(dst._h, 0.0, 0.0, 2, two, None, None, None) == E
    assert lib.qsv_lincomb(dst._h, 0.0, 0.0, 2, with_null, dbl(c), C.byref(norm2), C.byref(passes)) == E
    assert lib.qsv_lincomb(dst._h, 0.0, 0.0, -1, two, dbl(c), None, None) == E
    assert lib.qsv_lincomb(dst._h, 0.0, 0.0, 2, with_dst, dbl(c), None, None) == E           # dst among the sources
    assert lib.qsv_lincomb(dst._h, 1.0, 0.0, 2, handles([a, small]), dbl(c), None, None) == E  # sizes
    assert lib.qsv_lincomb(dst._h, 1.0, 0.0, 1, handles([small]), dbl(c), None, None) == E     # beta != 0 needs dst's size
    assert lib.qsv_lincomb(small._h, 0.0, 0.0, 2, two, dbl(c), None, None) == _lib.QSV_ENOMEM
    assert lib.qsv_lincomb(modes._h, 0.0, 0.0, 2, two, dbl(c), None, None) == S
    assert lib.qsv_lincomb(dst._h, 0.0, 0.0, 2, (C.c_void_p * 2)(a._h, modes._h), dbl(c), None, None) == S
    assert lib.qsv_inner_many(None, 2, two, dbl(values), None) == E
    assert lib.qsv_inner_many(dst._h, 2, None, dbl(values), None) == E
    assert lib.qsv_inner_many(dst._h, 2, two, None, None) == E
    assert lib.qsv_inner_many(dst._h, 2, with_null, dbl(values), None) == E
    assert lib.qsv_inner_many(dst._h, -1, two, dbl(values), None) == E
    assert lib.qsv_inner_many(dst._h, 2, handles([a, small]), dbl(values), None) == E
    assert lib.qsv_inner_many(modes._h, 2, two, dbl(values), None) == S
    assert lib.qsv_inner_many(dst._h, 2, (C.c_void_p * 2)(a._h, modes._h), dbl(values), None) == S
    # views of one buffer: a destination that meets a source is refused
    owner = DeviceState.zeros(n + 1).apply_scale(0.0)
    low = DeviceState.view(n, owner.device_ptr, 64, keepalive=owner)
    mid = DeviceState.view(n, owner.device_ptr + 16 * 32, 64, keepalive=owner)
    assert lib.qsv_lincomb(low._h, 0.0, 0.0, 2, handles([a, mid]), dbl(c), None, None) == E
    assert not values.any()
    for register, ket in zip((dst, a, b), kets):
        assert np.array_equal(register.to_numpy(), ket)
    assert np.array_equal(small.to_numpy(), random_ket(n - 1, 5)) and not owner.to_numpy().any()
    # the Python layer: complex coefficients and bad terms are refused before anything is touched
    for bad in ([(0.5j, "X", [0])], [(0.3, "XQ", [0, 1])], [(0.3, "X", [n])], [(0.3, "XX", [0, 0])]):
        with pytest.raises(ValueError):
            krylov.lanczos(bad, dst, 4)
        with pytest.raises(ValueError):
            dst.ground_state_of(bad)
        with pytest.raises(ValueError):
            dst.evolve_krylov(bad, 1.0)
    with pytest.raises(ValueError):
        krylov.lanczos([(1.0, "X", [0])], DeviceState.zeros(n).apply_scale(0.0), 4)       # no norm
    assert np.array_equal(dst.to_numpy(), kets[0])


def test_density_registers_refuse_the_krylov_methods():
    rho = DensityState.from_numpy(np.eye(4) / 4)
    terms = [(1.0, "ZZ", [0, 1])]
    with pytest.raises(ValueError):
        rho.ground_state_of(terms)
    with pytest.raises(ValueError):
        rho.evolve_krylov(terms, 1.0)
    with pytest.raises(ValueError):
        krylov.lanczos(terms, rho, 4)
    with pytest.raises(ValueError):
        krylov.evolve_krylov(rho, terms, 1.0)
    with pytest.raises(ValueError):
        krylov.ground_state(terms, rho)
