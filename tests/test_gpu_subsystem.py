"""Subsystem read-out on the device (qsv_reduced_density_state, qsv_marginal_probabilities and
``quantum_computations_amd.entanglement``) against tests/subsystem_reference.py, which tests/test_subsystem_reference_host.py
pins on the CPU.

Tolerances:

* reduced states and marginals: max-abs ``TERM_TOL = 1e-13``, the project's convention.  Entries are bounded by 1 and the
  NumPy statement itself is within 1e-16 of a long-double evaluation (checked on the CPU);
* the trace: ``|tr - 1| <= 1e-13``; agreement with ``reduced_density`` (k <= 6) and of the marginals with the diagonal of
  the reduced state: 1e-14;
* entropies, Schmidt values and mutual information against the SVD route of the reference: 1e-10 absolute, in nats (the
  eigenvalue and SVD routes agree to 1e-13 on random kets, checked on the CPU; a product state gives 2e-13).

Shapes are the smallest at which each path can go wrong: n = 14 is the smallest register on the
matrix cores, k = 7 there gives two row blocks and two tiles of groups, k = 8 exactly one tile, k = 9 fewer groups than a
tile (the per-entry form); n = 18 with k = 12 is the widest matrix on exactly one tile; n = 19 with k = 7 the longest traced
index; QSV_OPT_GRID_CAP = 2 makes workgroups loop over work items; n = 7 / 12 with k = n and n = 13 take the per-entry form.
Kets are unit-norm random (``workloads.random_ket``) unless named.  Worst errors are printed with their bounds (run with -s).
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import subsystem_reference as R
from quantum_computations_amd import _lib, noise
from quantum_computations_amd import workloads as W
from quantum_computations_amd.device import DensityState, DeviceState
from quantum_computations_amd.dv_simulator import numpy_quantum as npq

pytestmark = pytest.mark.gpu

TERM_TOL = 1e-13
TIGHT_TOL = 1e-14
ENTROPY_TOL = 1e-10
LN2 = float(np.log(2.0))


def maxabs(a):
    return float(np.max(np.abs(a))) if np.size(a) else 0.0


def report(what, err, bound):
    print(f"{what}: {err:.3e} (bound {bound:.3e})")
    assert err <= bound, what


@functools.lru_cache(maxsize=None)
def host_ket(n):
    ket = W.random_ket(n, 300 + n)
    ket.setflags(write=False)
    return ket


_DEVICE = {}


def device_ket(n):
    """One upload per register size, shared by the tests (none of them changes it)."""
    if n not in _DEVICE:
        _DEVICE[n] = DeviceState.from_numpy(host_ket(n))
    return _DEVICE[n]


def expected_form(n, k):
    return "k_subsys_tile" if n >= 14 and n - max(k, 6) >= 6 else "k_subsys_entry"


def check_reduced_state(dev, ket, n, k, name, qubits, form):
    rho = dev.reduced_density_state(qubits)
    assert isinstance(rho, DensityState) and rho.num_qubits == k
    assert dev.last_kernel() == form, (n, k, name, dev.last_kernel())
    got = rho.to_numpy()
    want = R.reduced_density(ket, qubits)
    report(f"n={n} k={k} {name} {form}", maxabs(got - want), TERM_TOL)
    assert np.array_equal(got, got.conj().T), "the stored matrix is not exactly Hermitian"
    assert not np.any(np.diagonal(got).imag), "the diagonal is not exactly real"
    report(f"n={n} k={k} {name} trace", abs(float(np.sum(np.diagonal(got).real)) - 1.0), TERM_TOL)
    again = dev.reduced_density_state(qubits)
    assert np.array_equal(again.to_numpy().view(np.uint64), got.view(np.uint64)), "a second call gave other bits"
    again.close()
    return rho, got


SHAPES = [(14, 7), (14, 8), (14, 9), (16, 7), (16, 8), (16, 9), (16, 10), (7, 7), (12, 12), (13, 9)]
CASES = [(n, k, name) for n, k in SHAPES for name in R.placements(n, k, 0)]


@pytest.mark.parametrize("n,k,name", CASES)
def test_reduced_state_against_the_reference(n, k, name):
    qubits = R.placements(n, k, 100 * n + k)[name]
    rho, _ = check_reduced_state(device_ket(n), host_ket(n), n, k, name, qubits, expected_form(n, k))
    rho.close()


def test_expected_forms_cover_both_kernels():
    forms = {(n, k): expected_form(n, k) for n, k in SHAPES}
    assert forms[(14, 7)] == forms[(14, 8)] == forms[(16, 10)] == "k_subsys_tile"
    assert forms[(14, 9)] == forms[(7, 7)] == forms[(12, 12)] == forms[(13, 9)] == "k_subsys_entry"


def test_widest_matrix_on_exactly_one_tile():
    n, k = 18, 12
    qubits = R.placements(n, k, 1812)["random0"]
    rho, _ = check_reduced_state(device_ket(n), host_ket(n), n, k, "random0", qubits, "k_subsys_tile")
    rho.close()


def test_longest_traced_index_takes_many_slices():
    n, k = 19, 7
    qubits = R.placements(n, k, 1907)["random1"]
    rho, _ = check_reduced_state(device_ket(n), host_ket(n), n, k, "random1", qubits, "k_subsys_tile")
    rho.close()


@pytest.mark.parametrize("name", ["low", "top", "random0"])
def test_workgroups_loop_over_work_items_under_a_grid_cap(name):
    n, k = 16, 7
    dev = DeviceState.from_numpy(host_ket(n))
    dev.set_option(_lib.OPT_GRID_CAP, 2)
    qubits = R.placements(n, k, 1607)[name]
    rho, capped = check_reduced_state(dev, host_ket(n), n, k, name + " grid_cap=2", qubits, "k_subsys_tile")
    free = device_ket(n).reduced_density_state(qubits)
    assert np.array_equal(free.to_numpy().view(np.uint64), capped.view(np.uint64))     # the grid does not change the sums
    for r in (rho, free, dev):
        r.close()


@pytest.mark.parametrize("n", (14, 16))
def test_one_to_six_qubits_agree_with_reduced_density(n):
    dev, ket = device_ket(n), host_ket(n)
    worst = 0.0
    for k in range(1, 7):
        for name, qubits in R.placements(n, k, 50 * n + k).items():
            rho = dev.reduced_density_state(qubits)
            assert dev.last_kernel() == "k_subsys_tile"
            got = rho.to_numpy()
            rho.close()
            assert np.array_equal(got, got.conj().T) and not np.any(np.diagonal(got).imag)
            worst = max(worst, maxabs(got - dev.reduced_density(qubits)))
            assert maxabs(got - R.reduced_density(ket, qubits)) <= TERM_TOL, (n, k, name)
    report(f"n={n} k=1..6 against reduced_density", worst, TIGHT_TOL)


def test_the_deferred_queue_is_flushed_first():
    """n = 22 is the smallest register that defers: gates are queued, the call is made without a flush, and the result is
    that of the same gates applied one launch each."""
    n, k = 22, 7
    rng = np.random.default_rng(22)
    gates = []
    for _ in range(12):
        q = rng.normal(size=(2, 2)) + 1j * rng.normal(size=(2, 2))
        gates.append((np.linalg.qr(q)[0], [int(rng.integers(n))]))
    qubits = R.placements(n, k, 2207)["random2"]
    results = []
    for defer in (1, 0):
        dev = DeviceState.random(n, 5)
        dev.set_option(_lib.OPT_DEFER, defer)
        for u, where in gates:
            dev.apply_matrix(u, where)
        queued_before = dev.defer_stats()
        rho = dev.reduced_density_state(qubits)
        if defer:
            assert queued_before[0] >= len(gates), queued_before                 # the gates went into the queue
            assert dev.defer_stats()[1] > queued_before[1]                         # and the call launched what was pending
        else:
            assert queued_before[0] == 0
        assert dev.last_kernel() == "k_subsys_tile"
        results.append(rho.to_numpy())
        report(f"n={n} defer={defer} trace", abs(rho.trace() - 1.0), TERM_TOL)
        rho.close()
        dev.close()
    report(f"n={n} deferred against per-gate", maxabs(results[0] - results[1]), TERM_TOL)


def test_a_reduced_state_is_a_density_register():
    n, k = 14, 7
    qubits = R.placements(n, k, 1407)["random0"]
    want = R.reduced_density(host_ket(n), qubits)
    rho = device_ket(n).reduced_density_state(qubits)
    report("purity", abs(rho.purity() - float(np.sum(np.abs(want) ** 2))), TERM_TOL)
    report("trace", abs(rho.trace() - 1.0), TERM_TOL)
    z0 = np.kron(np.diag([1.0, -1.0]), np.eye(1 << (k - 1)))
    report("expect_terms", abs(rho.expect_terms([(1.0, "Z", [0])]) - np.trace(z0 @ want)), TERM_TOL)
    report("eigenvalues", maxabs(rho.eigenvalues() - np.linalg.eigvalsh(want).clip(min=0.0)), TERM_TOL)
    report("von_neumann_entropy", abs(rho.von_neumann_entropy() - R.entanglement_entropy(host_ket(n), qubits)), ENTROPY_TOL)
    rho.apply_channel(noise.KrausChannel.amplitude_damping(1.0), [0])              # qubit 0 of the subsystem is reset
    after = rho.to_numpy()
    report("apply_channel", maxabs(np.diagonal(after)[1 << (k - 1):]), TERM_TOL)
    rho.close()
    assert isinstance(npq.reduced_density(device_ket(n), qubits), DensityState)


# ---- marginals --------------------------------------------------------------------------------------------------------
def diagonal_of(rho, k):
    """The diagonal of a density register; entry by entry where the matrix is too large to download for it."""
    if k <= 10:
        return np.diagonal(rho.to_numpy()).copy()
    dim = 1 << k
    return np.array([DeviceState.download(rho, i * (dim + 1), 1)[0] for i in range(dim)])


def marginal_form(n, qubits):
    high = sum(1 for q in qubits if n - 1 - q >= 6)
    return "k_marginal_stream" if n >= 14 and len(qubits) <= 12 and n - 6 - high >= 6 else "k_marginal_entry"


@pytest.mark.parametrize("n,k", [(n, k) for n in (14, 16) for k in range(1, n + 1)])
def test_marginals_against_the_reference(n, k):
    dev, ket = device_ket(n), host_ket(n)
    worst = [0.0, 0.0, 0.0]
    forms = set()
    for name, qubits in R.placements(n, k, 10 * n + k).items():
        got = dev.marginal_probabilities(qubits)
        assert dev.last_kernel() == marginal_form(n, qubits), (n, k, name, dev.last_kernel())
        forms.add(dev.last_kernel())
        assert got.shape == (1 << k,) and got.dtype == np.float64
        worst[0] = max(worst[0], maxabs(got - R.marginal_probabilities(ket, qubits)))
        worst[1] = max(worst[1], abs(float(np.sum(got)) - 1.0))
        assert np.array_equal(dev.marginal_probabilities(qubits).view(np.uint64), got.view(np.uint64)), "a second call gave other bits"
        if k <= 12:
            rho = dev.reduced_density_state(qubits)
            diag = diagonal_of(rho, k)
            rho.close()
            assert not np.any(diag.imag)
            worst[2] = max(worst[2], maxabs(got - diag.real))
    report(f"n={n} k={k} marginal {sorted(forms)}", worst[0], TERM_TOL)
    report(f"n={n} k={k} sum", worst[1], TERM_TOL)
    report(f"n={n} k={k} against the diagonal of the reduced state", worst[2], TIGHT_TOL)
    if k == n:                                              # the permuted |amplitude|^2
        qubits = R.placements(n, k, 10 * n + k)["random0"]
        want = (np.abs(ket) ** 2).reshape((2,) * n).transpose(qubits).reshape(-1)
        assert maxabs(dev.marginal_probabilities(qubits) - want) <= TERM_TOL


def test_marginal_on_the_capped_reduction_grid():
    n, k = 19, 3
    dev, ket = device_ket(n), host_ket(n)
    for name in ("low", "random0"):
        qubits = R.placements(n, k, 1903)[name]
        got = dev.marginal_probabilities(qubits)
        assert dev.last_kernel() == "k_marginal_stream"
        report(f"n={n} k={k} {name} marginal", maxabs(got - R.marginal_probabilities(ket, qubits)), TERM_TOL)
        report(f"n={n} k={k} {name} sum", abs(float(np.sum(got)) - 1.0), TERM_TOL)
        assert np.array_equal(dev.marginal_probabilities(qubits).view(np.uint64), got.view(np.uint64))
    assert maxabs(npq.marginal_probabilities(dev, [0, 5]) - R.marginal_probabilities(ket, [0, 5])) <= TERM_TOL


# ---- entropies and friends ----------------------------------------------------------------------------------------------
def test_entropies_of_a_random_ket_against_the_svd_reference():
    n = 16
    dev, ket = device_ket(n), host_ket(n)
    for k, name in ((7, "random0"), (9, "random1"), (3, "low"), (8, "top")):
        qubits = R.placements(n, k, 1600 + k)[name]
        value, info = dev.entanglement_entropy(qubits, return_info=True)
        assert info["complemented"] == (k > n - k) and len(info["side"]) == min(k, n - k)
        report(f"k={k} von Neumann", abs(value - R.entanglement_entropy(ket, qubits)), ENTROPY_TOL)
        report(f"k={k} Renyi 2", abs(dev.renyi2_entropy(qubits) - R.entanglement_entropy(ket, qubits, 2.0)), ENTROPY_TOL)
        report(f"k={k} Renyi 1/2", abs(dev.entanglement_entropy(qubits, alpha=0.5) - R.entanglement_entropy(ket, qubits, 0.5)), ENTROPY_TOL)
        report(f"k={k} base 2", abs(dev.entanglement_entropy(qubits, base=2.0) - R.entanglement_entropy(ket, qubits) / LN2), ENTROPY_TOL)
        report(f"k={k} purity", abs(dev.subsystem_purity(qubits) - R.subsystem_purity(ket, qubits)), TERM_TOL)
        report(f"k={k} Schmidt values", maxabs(dev.schmidt_values(qubits) - R.schmidt_values(ket, qubits)), ENTROPY_TOL)
        report(f"k={k} npq", abs(npq.entanglement_entropy(dev, qubits) - R.entanglement_entropy(ket, qubits)), ENTROPY_TOL)
    a, b = [0, 9], [15, 3]
    report("mutual information", abs(dev.mutual_information(a, b) - R.mutual_information(ket, a, b)), ENTROPY_TOL)


def test_ghz_cuts_and_the_smaller_side():
    n = 16
    dev = DeviceState.from_numpy(R.ghz(n))
    seven = [int(q) for q in np.random.default_rng(7).permutation(n)[:7]]
    nine = [int(q) for q in np.random.default_rng(9).permutation(n)[:9]]
    value, info = dev.entanglement_entropy(seven, return_info=True)
    report("GHZ 7-qubit cut", abs(value - LN2), ENTROPY_TOL)
    assert info == {"side": seven, "complemented": False, "kernel": "k_subsys_tile"}
    value, info = dev.entanglement_entropy(nine, return_info=True)
    report("GHZ 9-qubit cut", abs(value - LN2), ENTROPY_TOL)
    assert info["complemented"] and sorted(info["side"] + nine) == list(range(n)) and len(info["side"]) == 7    # through the 7-qubit side
    assert info["kernel"] == "k_subsys_tile"
    report("GHZ mutual information", abs(dev.mutual_information([0, 1], [9, 15]) - LN2), ENTROPY_TOL)
    report("GHZ purity", abs(dev.subsystem_purity(nine) - 0.5), TERM_TOL)
    report("GHZ whole register", abs(dev.entanglement_entropy(list(range(n)))), 0.0)
    dev.close()


def test_bell_pairs_and_product_states():
    n = 16
    pairs = [(0, 15), (1, 14), (2, 13), (3, 4)]
    dev = DeviceState.from_numpy(R.bell_pairs(n, pairs))
    for left, crossing in ((list(range(8)), 3), ([0, 1], 2), ([3, 4], 0), ([15, 3, 1, 9], 3), (list(range(2, 16)), 2)):
        report(f"{crossing} Bell pairs across the cut", abs(dev.entanglement_entropy(left) - crossing * LN2), ENTROPY_TOL)
    dev.close()
    dev = DeviceState.from_numpy(R.product_state(n, 3))
    for k, name in ((7, "random0"), (8, "low"), (10, "random1")):
        report(f"product state k={k}", abs(dev.entanglement_entropy(R.placements(n, k, k)[name])), ENTROPY_TOL)
    dev.close()


def test_python_refusals():
    n = 16
    dev = device_ket(n)
    for call in (dev.reduced_density_state, dev.marginal_probabilities, dev.entanglement_entropy, dev.subsystem_purity, dev.schmidt_values):
        for bad in ([0, 0], [n], [-1], []):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError):
        dev.reduced_density_state(list(range(13)))                                   # k = 13
    with pytest.raises(ValueError):
        dev.mutual_information([0, 1], [1, 2])
    rho = dev.reduced_density_state([0, 1])
    with pytest.raises(ValueError):
        rho.reduced_density_state([0])                                               # the partial trace of a density register: out of scope
    with pytest.raises(ValueError):
        rho.marginal_probabilities([0])
    # the library refuses by itself what Python checks first (QSV_EINVAL surfaces as ValueError)
    flat = DeviceState.zeros(4)
    for qubits in ([0, 0], [0, n]):
        with pytest.raises(ValueError):
            _lib.call("qsv_reduced_density_state", dev._h, 2, (C.c_int * 2)(*qubits), flat._h)
    with pytest.raises(ValueError, match="twice the kept qubits"):
        _lib.call("qsv_reduced_density_state", dev._h, 3, (C.c_int * 3)(0, 1, 2), flat._h)         # rho of the wrong size
    with pytest.raises(ValueError, match="must not be the ket"):
        _lib.call("qsv_reduced_density_state", flat._h, 2, (C.c_int * 2)(0, 1), flat._h)           # rho == ket
    flat.close()
    rho.close()

