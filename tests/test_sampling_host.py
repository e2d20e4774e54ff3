"""Multi-shot MPS sampling, the parts that need no GPU: the NumPy restatement (tests/sampling_reference.py) against
the chains the reference itself ran (tests/golden/mps_sampling.npz), the C entry point's argument checks, and the
logical read-out helpers."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from quantum_computations_amd import _lib
from quantum_computations_amd.cv_simulator.utils import fourier_matrix, rotation_matrix
from quantum_computations_amd.gkp_simulator import utils as GU
from sampling_reference import sample as restated_sample


def golden_sites(g):
    return [np.array(g[f"site_{i}"]) for i in range(len(g["shapes"]))]


def rotated_sites(g):
    """The sites as the chain of case "rot" measures them: Mp, Homodyne(pi) (= -q), Homodyne(angle), Mq."""
    qs, sites = g["domain"], golden_sites(g)
    ops = [fourier_matrix(qs, inv=True), None, rotation_matrix(qs, -float(g["angles"][0])), None]
    return [t if op is None else np.einsum("ij,ajb -> aib", op, t) for t, op in zip(sites, ops)]


@pytest.mark.parametrize("case", ["q", "rot"])
def test_restatement_reproduces_the_reference_chains(golden, case):
    g = golden["mps_sampling"]
    qs = g["domain"]
    dq = abs(qs[-1] - qs[0]) / (len(qs) - 1)
    assert float(g[f"{case}_margin"]) >= 1e-6          # what makes exact picks a fair demand
    uniforms = np.random.default_rng(int(g[f"{case}_seed"])).random((64, 4))
    got = restated_sample(golden_sites(g), dq, uniforms, measured_sites=rotated_sites(g) if case == "rot" else None)
    assert np.array_equal(got["picks"], g[f"{case}_picks"])
    err = float(np.max(np.abs(got["densities"] / g[f"{case}_densities"] - 1)))
    print(f"{case}: densities rel err {err:.2e}, margin {got['margin']:.2e}")
    assert err <= 1e-12, err
    signs = np.array([1.0, -1.0, 1.0, 1.0]) if case == "rot" else np.ones(4)
    assert np.array_equal(qs[got["picks"]] * signs, g[f"{case}_values"])


def test_entry_point_is_exported_and_bound():
    lib = _lib.load()
    assert "qsv_tensor_sample_site" in _lib.SIGNATURES
    assert hasattr(lib, "qsv_tensor_sample_site")


def test_entry_point_rejects_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    fn = lib.qsv_tensor_sample_site
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(v=p, site=p, env=None, S=4, L=1, d=4, R=1, scale=1.0, u=p, pick=p, density=p, out=None):
        return fn(0, None, v, site, env, S, L, d, R, scale, u, pick, density, out)

    for bad in (dict(S=0), dict(d=1), dict(L=0), dict(R=0), dict(v=None), dict(site=None), dict(u=None), dict(pick=None),
                dict(density=None), dict(scale=0.0), dict(scale=float("nan")), dict(L=513)):
        assert call(**bad) == _lib.QSV_EINVAL, bad
        with pytest.raises(ValueError):
            _lib.check(_lib.QSV_EINVAL)
    assert buf[0] == 0.0          # nothing was written


def test_logical_distribution():
    bits = np.array([[0, 0], [0, 1], [0, 1], [1, 0]], dtype=np.uint8)
    assert np.array_equal(GU.logical_distribution(bits), [0.25, 0.5, 0.25, 0.0])
    three = np.array([[1, 0, 0]] * 3 + [[0, 0, 1]], dtype=np.uint8)          # qubit 0 is the most significant bit
    want = np.zeros(8)
    want[4], want[1] = 0.75, 0.25
    assert np.array_equal(GU.logical_distribution(three), want)
    assert np.array_equal(GU.logical_distribution(np.zeros((5, 1), dtype=np.uint8)), [1.0, 0.0])
    with pytest.raises(ValueError):
        GU.logical_distribution(np.array([[0, 2]]))
    with pytest.raises(ValueError):
        GU.logical_distribution(np.zeros((0, 2)))
    with pytest.raises(ValueError):
        GU.logical_distribution(np.zeros(3))


def test_bits_of_homodyne_values():
    sqpi = np.sqrt(np.pi)
    values = np.array([[0.1, sqpi - 0.2, 2 * sqpi + 0.3, -sqpi, -3.1 * sqpi]])
    assert np.array_equal(GU.cv2dv_information(values).astype(np.uint8), [[0, 1, 0, 1, 1]])
