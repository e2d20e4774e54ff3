"""Canonical forms, Schmidt spectra, compression and overlaps of matrix-product states on the GPU
(``qsv_tensor_site_orthogonalise`` through ``SiteRegister.canonicalise`` / ``compress`` / ``overlap`` and the ``MPS``
methods) against the NumPy restatement of tests/canonical_reference.py and the registers the reference produced
(tests/golden/mps_canonical.npz).

Tolerances.  The restatement (Householder QR / LAPACK SVD in f64) run on the same input is the baseline of every
comparison; the GPU route, which orthogonalises through Gram sums, gets ``MARGIN = 10`` times the baseline's own figure.
A baseline can come out as an exact 0 (a bond of width 1, a single site): only then is it replaced by ``FLOOR = 4 eps``,
the rounding of one f64 operation on numbers of size one, which no route can go below; a baseline that is not zero is
used as it is.  Every test prints its figures before it asserts;
tools/bench_canonical.py writes its own accuracy figures and timings to profiles/r07_canonical.json.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import canonical_reference as ref
from quantum_computations_amd import _lib
from quantum_computations_amd.concurrent import map_on_streams
from quantum_computations_amd.cv_simulator.mps import MPS
from quantum_computations_amd.cv_simulator.site_register import SiteRegister, _torch

EPS = np.finfo(np.float64).eps
MARGIN = 10.0
FLOOR = 4 * EPS
RANK_TOL = 1e-8          # rank-deficient cases: in the middle of the gap tests/test_canonical_host.py checks

GOLDEN_NAMES = ("gates", "bell", "tight")
# (d, inner bonds): m = 1 ... 6, a bond of 1, a bond wider than L d (40 > 1 * 16), bonds up to 40
RANDOM_SPECS = [(16, []), (16, [40]), (16, [1, 5]), (16, [7, 12, 9]), (64, [10, 40]), (257, [33]), (16, [3, 8, 8, 3]),
                (16, [4, 9, 17, 9, 4])]


def golden_sites(g, name):
    return [np.array(g[f"{name}_site_{i}"]) for i in range(int(g[f"{name}_modes"]))]


def domain_for(d: int) -> np.ndarray:
    return np.linspace(-8.0, 8.0, d)


def bound(baseline: float) -> float:
    return MARGIN * (baseline if baseline > 0.0 else FLOOR)


def check_gauge_and_state(sites, label: str, rank_tol: float = 1e-13):
    """Checks 1 and 2 of the feature's issue for every centre; returns the worst figures."""
    d = sites[0].shape[1]
    psi = ref.contract(sites)
    top = float(np.max(np.abs(psi)))
    worst = {"gauge": 0.0, "gauge_ref": 0.0, "state": 0.0, "state_ref": 0.0}
    for centre in range(len(sites)):
        want_sites, _ = ref.canonicalise(sites, centre, rank_tol)
        base_gauge = ref.gauge_defect(want_sites, centre)
        base_state = float(np.max(np.abs(ref.contract(want_sites) - psi))) / top
        mps = MPS(domain_for(d), sites)
        before = mps.contract()
        mps.canonicalise(centre, rank_tol=rank_tol)
        got_sites = mps.tensors
        gauge = ref.gauge_defect(got_sites, centre)
        after = mps.contract()
        state = max(float(np.max(np.abs(after - before))), float(np.max(np.abs(after - psi)))) / top
        print(f"{label} centre {centre}: gauge defect {gauge:.2e} (restatement {base_gauge:.2e}), "
              f"state change {state:.2e} (restatement {base_state:.2e}), bonds {[t.shape[2] for t in got_sites[:-1]]}")
        assert [t.shape[2] for t in got_sites[:-1]] == [t.shape[2] for t in want_sites[:-1]]
        assert gauge <= bound(base_gauge), (label, centre, gauge, base_gauge)
        assert state <= bound(base_state), (label, centre, state, base_state)
        worst = {"gauge": max(worst["gauge"], gauge), "gauge_ref": max(worst["gauge_ref"], base_gauge),
                 "state": max(worst["state"], state), "state_ref": max(worst["state_ref"], base_state)}
    return worst


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_gauge_and_state_golden(golden, name):
    """Checks 1 and 2 on the reference's registers; the state is also compared with the reference's own ``contract()``
    (the amplitudes the fixture keeps).

    Measured on one MI355X: state change 2.0e-15 (``bell``) ... 3.0e-15 (``tight``, the ``rel_err = 1e-2`` register)
    against the restatement's 9e-16 ... 2.5e-15; gauge defect 7e-16 against 1.2e-15 ... 2.7e-15."""
    g = golden["mps_canonical"]
    sites = golden_sites(g, name)
    check_gauge_and_state(sites, name)
    stride, m = int(g[f"{name}_stride"]), len(sites)
    want = g[f"{name}_contract_strided"]
    top = float(g[f"{name}_max_amplitude"])
    base_sites, _ = ref.canonicalise(sites, 0)
    baseline = float(np.max(np.abs(ref.contract(base_sites)[(slice(None, None, stride),) * m] - want))) / top
    mps = MPS(np.array(g["domain"]), sites)
    mps.canonicalise(0)
    err = float(np.max(np.abs(mps.contract()[(slice(None, None, stride),) * m] - want))) / top
    print(f"{name}: against the reference's contract() {err:.2e} (restatement {baseline:.2e})")
    assert err <= bound(baseline)
    assert abs(mps.norm() - float(g[f"{name}_norm"])) <= 1e-12 * float(g[f"{name}_norm"])


@pytest.mark.parametrize("spec", RANDOM_SPECS, ids=lambda s: f"d{s[0]}-bonds{'-'.join(map(str, s[1])) or 'none'}")
def test_gauge_and_state_random(spec):
    d, bonds = spec
    sites = ref.random_register(np.random.default_rng(100 + d + len(bonds)), d, bonds)
    check_gauge_and_state(sites, f"random d={d} bonds={bonds}")


def test_gauge_and_state_graded():
    """Columns of every site graded over six decades (down to 1e-6 of the largest, i.e. 1e-12 in the Gram matrices, far
    below what one Gram round resolves): the small Schmidt values must survive the sweep."""
    sites = ref.random_register(np.random.default_rng(3), 16, [6, 10, 6], scale_decades=6.0)
    check_gauge_and_state(sites, "graded")


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_schmidt_values_and_entropy(golden, name):
    """Check 3: against the dense-SVD values of the fixture, absolute difference relative to ``s[0]`` (DESIGN.md
    section 13 claims absolute accuracy for all values, so values below ``sqrt(eps) s[0]`` are compared too, in that
    absolute sense); ``sum s^2 == norm2()``; the register is untouched."""
    g = golden["mps_canonical"]
    sites = golden_sites(g, name)
    mps = MPS(np.array(g["domain"]), sites)
    before = mps.tensors
    got = mps.schmidt_values()
    _, restated = ref.canonicalise(sites, 0)
    assert all(np.array_equal(a, b) for a, b in zip(before, mps.tensors))
    norm2 = mps.reg.norm2()
    for b, s in enumerate(got):
        dense = np.array(g[f"{name}_schmidt_{b}"])
        n = len(s)
        baseline = float(np.max(np.abs(restated[b] - dense[: len(restated[b])]))) / dense[0]
        err = float(np.max(np.abs(s - dense[:n]))) / dense[0]
        rest = float(np.max(dense[n:], initial=0.0)) / dense[0]
        print(f"{name} bond {b}: {n} values, |s - dense| / s0 = {err:.2e} (restatement {baseline:.2e}), "
              f"largest dense value not returned {rest:.2e}, sum s^2 / norm2 - 1 = {np.sum(s ** 2) / norm2 - 1:.2e}")
        assert err <= bound(baseline)
        assert rest <= 1e-12
        assert abs(np.sum(s ** 2) / norm2 - 1) <= 1e-12
        assert np.array_equal(s, mps.schmidt_values(b)[: len(s)])
        want_entropy = ref.entropy(dense)
        assert abs(mps.entanglement_entropy(b) - want_entropy) <= 1e-10 * max(1.0, want_entropy)
    assert len(mps.entanglement_entropy()) == len(sites) - 1
    with pytest.raises(IndexError):
        mps.schmidt_values(len(sites) - 1)


@pytest.mark.parametrize("case", ["duplicated_columns", "zero_column", "product_bond8"])
def test_rank_deficient_sites(case):
    """Check 4: bonds come out at the numerical rank, gauge and state as everywhere else."""
    sites, want_bonds = ref.rank_deficient_registers(np.random.default_rng(17))[case]
    mps = MPS(domain_for(16), sites)
    mps.canonicalise(0, rank_tol=RANK_TOL)
    assert mps.reg.bond_dims() == want_bonds
    check_gauge_and_state(sites, case, rank_tol=RANK_TOL)


def test_compress(golden):
    """Check 5."""
    g = golden["mps_canonical"]
    for name in ("gates", "tight"):
        sites = golden_sites(g, name)
        domain = np.array(g["domain"])
        full = MPS(domain, sites)
        schmidt = full.schmidt_values()
        for k in (3, 5):
            want_sites, want_weights = ref.compress(sites, 0, max_bond_dim=k)
            cut = MPS(domain, sites)
            weights = cut.compress(max_bond_dim=k)
            assert cut.reg.bond_dims() == [min(k, len(s)) for s in schmidt]
            print(f"{name} k={k}: weights {weights}, restatement {want_weights}")
            assert np.allclose(weights, want_weights, rtol=1e-9, atol=1e-15)
            assert ref.gauge_defect(cut.tensors, 0) <= bound(ref.gauge_defect(want_sites, 0))
            # the first cut made (the last bond, nothing truncated before it) keeps the k largest Schmidt values: its
            # weight is the tail of the untruncated spectrum; afterwards every bond agrees with the restatement's
            last = schmidt[-1]
            norm2 = full.reg.norm2()
            assert abs(weights[-1] - np.sum(last[k:] ** 2) / norm2) <= 1e-12 * np.sum(last ** 2) / norm2
            _, want_schmidt = ref.canonicalise(want_sites, 0)
            for x, y in zip(cut.schmidt_values(), want_schmidt):
                assert len(x) == len(y) and np.max(np.abs(x - y)) <= 1e-12 * y[0]
            ov = MPS.overlap(full, cut)
            infidelity = 1 - abs(ov) ** 2 / (MPS.overlap(full, full).real * MPS.overlap(cut, cut).real)
            limit = float(np.sum(np.sqrt(weights))) ** 2
            psi = ref.contract(sites)
            base_sites, _ = ref.canonicalise(sites, 0)
            rounding = bound(float(np.max(np.abs(ref.contract(base_sites) - psi)) / np.max(np.abs(psi))))
            print(f"{name} k={k}: infidelity {infidelity:.3e} <= bound {limit:.3e}")
            assert infidelity <= limit + rounding
        # defaults: nothing but rounding-level values goes
        kept = MPS(domain, sites)
        weights = kept.compress()
        print(f"{name} defaults: weights {weights}, bonds {kept.reg.bond_dims()}")
        assert max(weights) <= 1e-20
        assert abs(MPS.fidelity(full, kept) / full.norm() ** 4 - 1) <= 1e-12


def test_overlap_and_fidelity(golden):
    """Check 6."""
    g = golden["mps_canonical"]
    domain = np.array(g["domain"])
    a_sites = golden_sites(g, "gates")
    b_sites = ref.random_register(np.random.default_rng(8), 64, [3, 17])
    a, b = MPS(domain, a_sites), MPS(domain, b_sites)
    measure = a.diff ** 3
    want = np.vdot(a.contract(), b.contract()) * measure
    got = MPS.overlap(a, b)
    scale = a.norm() * b.norm()
    print(f"overlap {got:.6e}, dense {want:.6e}, difference / (|a||b|) {abs(got - want) / scale:.2e}")
    assert abs(got - want) <= 1e-13 * scale
    assert abs(MPS.overlap(b, a) - np.conj(got)) <= 1e-14 * scale
    assert abs(MPS.overlap(a, a) - a.norm() ** 2) <= 1e-13 * a.norm() ** 2
    dense_fidelity = float(np.abs(want) ** 2)
    assert abs(MPS.fidelity(a, b) - dense_fidelity) <= 1e-12 * scale ** 2
    dense_a = MPS(domain, a_sites, layout="dense")
    assert abs(MPS.fidelity(dense_a, dense_a) - a.norm() ** 4) <= 1e-12
    with pytest.raises(ValueError):
        MPS.overlap(a, MPS(domain, ref.random_register(np.random.default_rng(1), 64, [2])))
    with pytest.raises(ValueError):
        MPS.overlap(a, MPS(np.linspace(-7.0, 7.0, 64), a_sites))
    with pytest.raises(ValueError):
        a.reg.overlap(SiteRegister(ref.random_register(np.random.default_rng(1), 16, [2, 2]), 16))


def test_overlap_large_grid():
    """d = 1000, m = 5: the dense tensors would hold 1e15 amplitudes each."""
    d, rng = 1000, np.random.default_rng(21)
    domain = np.linspace(-10.0, 10.0, d)
    a = MPS(domain, ref.random_register(rng, d, [8, 16, 16, 8]))
    b = MPS(domain, ref.random_register(rng, d, [5, 9, 12, 6]))
    fidelity = MPS.fidelity(a, b) / (a.norm() * b.norm()) ** 2
    print(f"d=1000 m=5: normalised fidelity {fidelity:.3e}, self-fidelity {MPS.fidelity(a, a) / a.norm() ** 4:.15f}")
    assert np.isfinite(fidelity) and 0.0 <= fidelity <= 1.0
    assert abs(MPS.fidelity(a, a) / a.norm() ** 4 - 1) <= 1e-12


def test_streams_bit_identical(golden):
    """Check 7: the same register canonicalised serially and inside four concurrent jobs."""
    g = golden["mps_canonical"]
    sites = golden_sites(g, "tight")
    serial = SiteRegister(sites, 64)
    serial.canonicalise(1)
    want = serial.site_arrays()

    def job(_):
        reg = SiteRegister(sites, 64, stream=_torch().cuda.current_stream())
        values = reg.canonicalise(1)
        return reg.site_arrays(), values

    results = map_on_streams(job, range(4), max_concurrent=4)
    for got, values in results:
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
        assert all(np.array_equal(x, y) for x, y in zip(values, results[0][1]))


def test_entry_point_rejects_bad_arguments():
    """Check 8: every QSV_EINVAL case returns before anything is launched (the pointers are never dereferenced)."""
    lib = _lib.load()
    rank = C.c_uint64(0)
    fake = C.c_void_p(0x1000)

    def call(L=2, d=4, R=3, side=0, tol=0.0, site=fake, iso=fake, carry=fake, rank_ptr=C.byref(rank)):
        return lib.qsv_tensor_site_orthogonalise(0, None, site, L, d, R, side, tol, iso, carry, rank_ptr, None)

    assert call(d=1) == _lib.QSV_EINVAL
    assert call(L=0) == _lib.QSV_EINVAL
    assert call(R=0) == _lib.QSV_EINVAL
    assert call(side=2) == _lib.QSV_EINVAL
    assert call(R=_lib.SITE_MAX_BOND + 1) == _lib.QSV_EINVAL
    assert call(L=_lib.SITE_MAX_BOND + 1, side=1) == _lib.QSV_EINVAL
    assert call(tol=-1e-3) == _lib.QSV_EINVAL
    assert call(tol=float("nan")) == _lib.QSV_EINVAL
    assert call(tol=float("inf")) == _lib.QSV_EINVAL
    assert call(site=None) == _lib.QSV_EINVAL
    assert call(iso=None) == _lib.QSV_EINVAL
    assert call(carry=None) == _lib.QSV_EINVAL
    assert call(rank_ptr=None) == _lib.QSV_EINVAL


def test_widest_supported_bond():
    """The stated limit works: a bond of QSV_SITE_MAX_BOND = 128 on both sides of a site."""
    w = _lib.SITE_MAX_BOND
    sites = ref.random_register(np.random.default_rng(5), 16, [w, w])
    reg = SiteRegister(sites, 16)
    norm2 = reg.norm2()
    values = reg.canonicalise(1)
    got = reg.site_arrays()
    want_sites, want_values = ref.canonicalise(sites, 1)
    gauge, base = ref.gauge_defect(got, 1), ref.gauge_defect(want_sites, 1)
    err = max(float(np.max(np.abs(a - b[: len(a)]))) / b[0] for a, b in zip(values, want_values))
    print(f"bond {w}: gauge defect {gauge:.2e} (restatement {base:.2e}), Schmidt values {err:.2e}, bonds {reg.bond_dims()}")
    assert reg.bond_dims() == [16, 16]          # a bond of 128 next to an end site of 16 rows has rank 16
    assert gauge <= bound(base)
    assert err <= 1e-12
    assert abs(reg.norm2() / norm2 - 1) <= 1e-12


def test_python_layer_argument_checks_on_device(golden, caplog):
    """The two checks of the ``MPS`` layer that need a register: a dense register has no canonical form, and
    ``compress`` logs keywords it does not know instead of raising."""
    g = golden["mps_canonical"]
    sites, domain = golden_sites(g, "bell"), np.array(g["domain"])
    dense = MPS(domain, sites, layout="dense")
    for call in (lambda: dense.canonicalise(0), lambda: dense.compress(), lambda: dense.schmidt_values(),
                 lambda: dense.entanglement_entropy(), lambda: MPS.overlap(dense, dense)):
        with pytest.raises(AttributeError):
            call()
    mps = MPS(domain, sites)
    with caplog.at_level("WARNING"):
        weights = mps.compress(max_bond_dim=4, bond_dimension=2)
    assert any("bond_dimension" in record.getMessage() for record in caplog.records)
    assert len(weights) == 2 and mps.reg.bond_dims() == [2, 4]
    with pytest.raises(IndexError):
        mps.canonicalise(3)
    with pytest.raises(ValueError):
        mps.canonicalise(0, rank_tol=-1.0)
