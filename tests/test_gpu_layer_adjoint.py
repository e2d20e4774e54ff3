"""The adjoint walk through a product layer on the device: ``DeviceState.layer_adjoint``,
``layer_transition`` and ``one_qubit_densities`` against tests/layer_adjoint_reference.py, the registers BIT FOR BIT against
``apply_layer`` with the same matrices, and the gradients built on them (``ansatz.Ansatz.energy_and_gradient``,
``qaoa.energy_and_gradient(walk="fused")``) against the routes through Pauli rotations and Pauli sums.

Sizes: 3 qubits (the small form below a wave), 11 (the small form, one full chunk), 12 (one tile of all bits), 13 (two passes
with all qubits: seven bits >= 6) and 19 (three passes).  Stage sets: all qubits; index bits 0..5; the top bit; bits 5 and 6, one
on each side of the lane boundary (from 7 qubits on); one random subset in random order.

Tolerances.  Values: ``4 * 2^n * eps * ||psi|| ||lambda||``, the any-order bound on a sum of 2^n rounded products with a factor 4
for the complex arithmetic and the reference's own rounding; ``layer_transition`` against ``layer_adjoint`` (unitaries) takes the
same bound.  Runs per case: ``lambda`` independent and ``H psi`` with unitaries; ``H psi`` with contractions (singular values in
[0.6, 1]: no register outgrows the norms it entered with, so the bound needs no further factor); an independent ``lambda`` with
norm-growing matrices ``1.2 U + 0.05``, where each register may grow by ``prod_q max(1, ||W_q||_2)`` during the walk and the
bound on the walk's values takes that product squared (the read-only call keeps the plain bound).  Gradients:
``2 * (4 * 2^n + 16 * G) * eps * sum |c_t|`` with G the gates of the circuit -- the bound on the values, the per-stage bound on
the states (``layer_reference.bound``) and ``||lambda|| <= sum |c_t|``, for both sides of the comparison.  The rewound register:
``16 * G * eps``.  Observed figures are printed next to their bounds (run with -s).
"""
from __future__ import annotations

import numpy as np
import pytest

import diagonal_reference as R
import layer_adjoint_reference as A
import layer_reference as L
from quantum_computations_amd import _lib, ansatz, layers, qaoa
from quantum_computations_amd.device import DensityState, DeviceState, QuditState
from quantum_computations_amd.diagonal import DiagonalOperator
from quantum_computations_amd.dv_simulator import numpy_quantum as npq
from test_gpu_sweep import report

pytestmark = pytest.mark.gpu

SIZES = (3, 11, 12, 13, 19)
CAPPED = (13, 19)
SETS = ("all", "low", "top", "boundary", "random")
EPS = L.EPS


def stage_set(n, name):
    if name == "all":
        return list(range(n))
    if name == "low":
        return [n - 1 - b for b in range(min(n, 6))]
    if name == "top":
        return [0]
    if name == "boundary":
        return [n - 1 - 5, n - 1 - 6]
    rng = np.random.default_rng(900 + n)
    return [int(q) for q in rng.permutation(n)[:max(1, n // 2)]]


def contractions(k, seed):
    """Random non-unitary matrices ``U diag(s) V`` with singular values in [0.6, 1]."""
    u, v = L.random_unitaries((k,), seed), L.random_unitaries((k,), seed + 1)
    s = np.random.default_rng(seed + 2).uniform(0.6, 1.0, (k, 2))
    return u * s[:, None, :] @ v


def growing(k, seed):
    """General matrices that make a register grow: ``1.2 U + 0.05``, spectral norms between about 1.1 and 1.3."""
    return 1.2 * L.random_unitaries((k,), seed) + 0.05


def dagger(mats):
    return np.conjugate(np.swapaxes(mats, -1, -2))


def expected_kernel(n, apply):
    return f"{'k_layer_adjoint_tile' if n >= 12 else 'k_layer_adjoint_small'}<true, {'true' if apply else 'false'}>"


def walk(psi, lam, W, qubits, cap=0, nontemporal=1):
    """``layer_adjoint`` with the matrices ``W`` applied (the forward factors handed over are their conjugate transposes, an
    exact operation): (T, psi after, lambda after, passes, kernel)."""
    a, b = DeviceState.from_numpy(psi), DeviceState.from_numpy(lam)
    for st in (a, b):
        if cap:
            st.set_option(_lib.OPT_GRID_CAP, cap)
        if not nontemporal:
            st.set_option(_lib.OPT_NONTEMPORAL, 0)
    T, passes = a._layer_adjoint(dagger(L.table(W, len(qubits))), b, qubits)
    out = T, a.to_numpy(), b.to_numpy(), passes, a.last_kernel()
    a.close()
    b.close()
    return out


def through_apply_layer(ket, W, qubits, cap=0, nontemporal=1):
    st = DeviceState.from_numpy(ket)
    if cap:
        st.set_option(_lib.OPT_GRID_CAP, cap)
    if not nontemporal:
        st.set_option(_lib.OPT_NONTEMPORAL, 0)
    st.apply_layer(W, qubits)
    out = st.to_numpy()
    st.close()
    return out


def h_psi(psi, n):
    st = DeviceState.from_numpy(psi)
    out = st.apply_pauli_sum(A.heisenberg_chain(n))
    lam = out.to_numpy()
    st.close()
    out.close()
    return lam


@pytest.fixture(scope="module")
def kets():
    """Per size: psi, an independent lambda, and H psi for the Heisenberg chain -- made once and never changed."""
    out = {}
    for n in SIZES:
        psi = L.random_ket(n, 70 + n)
        out[n] = {"psi": psi, "independent": 0.9 * L.random_ket(n, 80 + n), "H psi": h_psi(psi, n)}
        for ket in out[n].values():
            ket.setflags(write=False)
    return out


# ---- the walk: registers bit for bit, values within the bound, the same bits twice -----------------------------------------
@pytest.mark.parametrize("n, set_name", [(n, name) for n in SIZES for name in SETS if n > 6 or name != "boundary"])
def test_registers_bit_for_bit_and_values_within_the_bound(kets, n, set_name):
    qubits = stage_set(n, set_name)
    k, psi = len(qubits), kets[n]["psi"]
    runs = (("independent", "unitaries", L.random_unitaries((k,), 10 * n + k)), ("H psi", "unitaries", L.random_unitaries((k,), 30 * n + k)),
            ("H psi", "non-unitary", contractions(k, 20 * n + k)), ("independent", "norm-growing", growing(k, 40 * n + k)))
    for lam_name, kind, W in runs:
        lam = kets[n][lam_name]
        what = f"n={n} {set_name} lambda={lam_name} {kind}"
        bound = A.value_bound(n, np.linalg.norm(psi), np.linalg.norm(lam))
        entry_bound = bound                                  # for the values of the registers as they entered
        if kind == "norm-growing":                           # each register may grow by prod_q max(1, ||W_q||_2) during the walk
            bound *= L.spectral_norm_product(W, k) ** 2
        T, psi_out, lam_out, passes, kernel = walk(psi, lam, W, qubits)
        assert passes == L.pass_count(n, qubits) and kernel == expected_kernel(n, True), (what, passes, kernel)
        assert np.array_equal(psi_out, through_apply_layer(psi, W, qubits)), what
        assert np.array_equal(lam_out, through_apply_layer(lam, W, qubits)), what
        T_ref, _, _ = A.layer_adjoint(psi, lam, W, qubits)
        report(f"{what}: values against the reference", np.max(np.abs(T - T_ref)), bound)
        again = walk(psi, lam, W, qubits)
        assert np.array_equal(again[0], T) and np.array_equal(again[1], psi_out) and np.array_equal(again[2], lam_out), what
        if n in CAPPED:                                      # a workgroup walks several tiles: the registers take no other bit
            T_cap, psi_cap, lam_cap, passes_cap, _ = walk(psi, lam, W, qubits, cap=2)
            assert passes_cap == passes and np.array_equal(psi_cap, psi_out) and np.array_equal(lam_cap, lam_out), what
            report(f"{what}: values with the grid capped at 2", np.max(np.abs(T_cap - T_ref)), bound)
            assert np.array_equal(walk(psi, lam, W, qubits, cap=2)[0], T_cap), what
        if set_name == "all":                                # cached loads and stores instead of non-temporal ones
            T_c, psi_c, lam_c, _, kernel_c = walk(psi, lam, W, qubits, nontemporal=0)
            assert kernel_c == expected_kernel(n, True).replace("<true", "<false"), kernel_c
            assert np.array_equal(psi_c, through_apply_layer(psi, W, qubits, nontemporal=0)) and np.array_equal(psi_c, psi_out), what
            assert np.array_equal(lam_c, lam_out) and np.array_equal(T_c, T), what
        # the read-only call: the entry values, both registers untouched
        bra, ket = DeviceState.from_numpy(lam), DeviceState.from_numpy(psi)
        T_tr, passes_tr = bra._layer_transition(ket, qubits)
        assert passes_tr == passes and ket.last_kernel() == expected_kernel(n, False), what
        assert np.array_equal(bra.to_numpy(), lam) and np.array_equal(ket.to_numpy(), psi), what
        report(f"{what}: layer_transition against the reference", np.max(np.abs(T_tr - A.layer_transition(lam, psi, qubits))), entry_bound)
        assert np.array_equal(bra.layer_transition(ket, qubits), T_tr), what
        if kind == "unitaries":      # unitaries on the other qubits cancel: the walk's values are the entry values, up to rounding
            report(f"{what}: layer_transition against layer_adjoint", np.max(np.abs(T_tr - T)), bound)
        bra.close()
        ket.close()


@pytest.mark.parametrize("n", SIZES)
def test_one_qubit_densities(kets, n):
    psi = 1.3 * kets[n]["psi"]
    norm2 = float(np.vdot(psi, psi).real)
    bound = A.value_bound(n, np.sqrt(norm2), np.sqrt(norm2))
    st = DeviceState.from_numpy(psi)
    rho = st.one_qubit_densities()
    assert rho.shape == (n, 2, 2) and np.array_equal(rho, np.conjugate(np.swapaxes(rho, 1, 2)))      # exactly hermitian
    assert np.array_equal(npq.one_qubit_densities(st), rho)
    report(f"n={n}: one_qubit_densities against the reference", np.max(np.abs(rho - A.one_qubit_densities(psi))), bound)
    report(f"n={n}: traces against norm2", np.max(np.abs(np.trace(rho, axis1=1, axis2=2) - st.norm2())), bound)
    worst = max(np.max(np.abs(rho[q] - st.reduced_density([q]))) for q in range(n))
    report(f"n={n}: one_qubit_densities against reduced_density", worst, bound)
    some = [n - 1, 0]
    report(f"n={n}: a subset", np.max(np.abs(st.one_qubit_densities(some) - rho[some])), bound)
    assert np.array_equal(st.to_numpy(), psi)
    st.close()


# ---- gradients --------------------------------------------------------------------------------------------------------------------
def gradient_tolerance(n, gates, scale):
    return 2.0 * (4.0 * (1 << n) + 16.0 * gates) * EPS * scale


@pytest.mark.parametrize("n", (12, 13))
def test_ansatz_gradient_against_the_rotation_route(n):
    circuit = ansatz.Ansatz(n)
    for _ in range(2):
        circuit.rotation_layer("ry").rotation_layer("rz").fixed(ansatz.cz_line(n))
    terms = A.heisenberg_chain(n)
    scale = sum(abs(c) for c, _, _ in terms)
    gates = circuit.num_gates()
    params = np.random.default_rng(n).uniform(-np.pi, np.pi, circuit.num_parameters)
    start = L.random_ket(n, 3 * n)
    state = DeviceState.from_numpy(start)
    energy, grad = circuit.energy_and_gradient(params, terms, state)
    report(f"n={n}: the register after the walk", np.linalg.norm(state.to_numpy() - start), 16 * gates * EPS)
    other = DeviceState.from_numpy(start)
    want_energy, values = other.energy_and_gradient(circuit.rotations(params), terms)
    tol = gradient_tolerance(n, gates, scale)
    report(f"n={n}: ansatz energy against the rotation route", abs(energy - want_energy), tol)
    report(f"n={n}: ansatz gradient against the rotation route", np.max(np.abs(grad - values[circuit.parameter_positions()])), tol)
    assert np.max(np.abs(grad)) > 1e-3                     # the comparison is not between zeros
    # |0...0> by default, and the same numbers from a fresh register
    zero = DeviceState.zeros(n)
    assert circuit.energy_and_gradient(params, terms)[0] == circuit.energy_and_gradient(params, terms, zero)[0]
    for st in (state, other, zero):
        st.close()


@pytest.mark.parametrize("n", (12, 13))
def test_qaoa_fused_walk_against_the_calls(n):
    p = 2
    z_terms = R.random_z_terms(n, 12, seed=n)
    diag = DiagonalOperator.from_terms(n, z_terms)
    scale = sum(abs(c) for c, _, _ in z_terms)
    rng = np.random.default_rng(30 + n)
    gammas, betas = rng.uniform(-1, 1, p), rng.uniform(-1, 1, p)
    calls = qaoa.energy_and_gradient(diag, gammas, betas, mixer="layer")
    start = qaoa.plus_state(n)
    before = start.to_numpy()
    fused = qaoa.energy_and_gradient(diag, gammas, betas, start, mixer="layer", walk="fused")
    gates = p * (n + 1)
    tol = gradient_tolerance(n, gates, scale)
    assert fused[0] == calls[0]                              # the forward walk is the same calls
    report(f"n={n}: fused d_gamma against the calls", np.max(np.abs(fused[1] - calls[1])), tol)
    report(f"n={n}: fused d_beta against the calls", np.max(np.abs(fused[2] - calls[2])), tol)
    report(f"n={n}: the register after the fused walk", np.linalg.norm(start.to_numpy() - before), 16 * gates * EPS)
    assert np.max(np.abs(fused[2])) > 1e-3
    with pytest.raises(ValueError):
        qaoa.energy_and_gradient(diag, gammas, betas, mixer="gates", walk="fused")
    with pytest.raises(ValueError):
        qaoa.energy_and_gradient(diag, gammas, betas, mixer="layer", walk="both")
    start.close()
    diag.close()


# ---- passes, kernels, refusals, the deferred queue -----------------------------------------------------------------------------
def test_documented_passes_and_k_zero():
    for n, want in ((11, 1), (12, 1), (13, 2), (18, 2), (19, 3)):
        a, b = DeviceState.zeros(n), DeviceState.zeros(n)
        T, passes = a._layer_adjoint(layers.hadamard(), b, range(n))
        assert passes == want == L.pass_count(n, range(n)) and T.shape == (n, 2, 2)
        assert a.last_kernel() == expected_kernel(n, True)
        assert a._layer_transition(b, range(n))[1] == want and b.last_kernel() == expected_kernel(n, False)
        T, passes = a._layer_adjoint(np.zeros((0, 2, 2)), b, [])
        assert passes == 0 and T.shape == (0, 2, 2)
        a.close()
        b.close()


def test_refusals_raise_and_change_nothing():
    n = 5
    psi, lam = L.random_ket(n, 1), L.random_ket(n, 2)
    a, b, small = DeviceState.from_numpy(psi), DeviceState.from_numpy(lam), DeviceState.zeros(n - 1)
    h = layers.hadamard()
    for bad in ([0, 0], [n], [-1]):
        with pytest.raises(ValueError):
            a.layer_adjoint(h, b, bad)
        with pytest.raises(ValueError):
            a.layer_transition(b, bad)
    with pytest.raises(ValueError):
        a.layer_adjoint(np.full((2, 2), np.nan), b)
    with pytest.raises(ValueError):
        a.layer_adjoint(np.zeros((3, 2, 2)), b, [0, 1])        # the shape of the table
    with pytest.raises(ValueError):
        a.layer_adjoint(h, a)                                   # the same register
    with pytest.raises(ValueError):
        a.layer_adjoint(h, small, [0])
    with pytest.raises(ValueError):
        a.layer_transition(small, [0])
    modes = QuditState.zeros(2, 3)
    lib = _lib.load()
    values = np.zeros(8)
    one = (1, (_lib.C.c_int * 1)(0))
    dbl = lambda x: x.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))
    m = np.ascontiguousarray(h).view(np.float64)
    assert lib.qsv_layer_adjoint(a._h, modes._h, *one, dbl(m), dbl(values), None) == _lib.QSV_ESTATE
    assert lib.qsv_layer_transition(modes._h, a._h, *one, dbl(values), None) == _lib.QSV_ESTATE
    assert lib.qsv_layer_adjoint(a._h, b._h, *one, None, dbl(values), None) == _lib.QSV_EINVAL
    assert lib.qsv_layer_adjoint(a._h, b._h, *one, dbl(m), None, None) == _lib.QSV_EINVAL
    rho = DensityState.from_numpy(np.eye(4) / 4)
    for call in (lambda: rho.layer_adjoint(h, a), lambda: rho.layer_transition(a), lambda: rho.one_qubit_densities(),
                 lambda: a.layer_adjoint(h, rho), lambda: a.layer_transition(rho)):
        with pytest.raises(ValueError):
            call()
    # the ansatz refuses a wrong register before it runs the circuit on it
    circuit = ansatz.Ansatz(n).rotation_layer("ry")
    rho_before = rho.to_numpy()
    for wrong in (rho, small):
        with pytest.raises(ValueError):
            circuit.energy_and_gradient(np.ones(n), [(1.0, "Z", [0])], wrong)
    assert np.array_equal(rho.to_numpy(), rho_before) and np.array_equal(small.to_numpy(), np.eye(1, 1 << (n - 1))[0])
    assert np.array_equal(a.to_numpy(), psi) and np.array_equal(b.to_numpy(), lam)
    for st in (a, b, small, modes, rho):
        st.close()


def test_pending_deferred_queues_are_flushed_first():
    import test_gpu_deferred as D
    n = 22
    W = L.random_unitaries((n,), 4)
    a, b = D.pending_pair(n)                              # a has gates queued, b is its un-deferred twin
    c, d = D.pending_pair(n, seed=6)
    queued = a.defer_stats()[0], c.defer_stats()[0]
    assert np.array_equal(c.layer_transition(a), d.layer_transition(b))
    a, b = D.pending_pair(n)
    c, d = D.pending_pair(n, seed=6)
    assert np.array_equal(a.layer_adjoint(W, c), b.layer_adjoint(W, d))
    assert (a.defer_stats()[0], c.defer_stats()[0]) == queued      # the call was never queued itself
    assert np.array_equal(a.to_numpy(), b.to_numpy()) and np.array_equal(c.to_numpy(), d.to_numpy())
