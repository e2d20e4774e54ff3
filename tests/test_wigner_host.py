"""Wigner functions without a GPU: the NumPy restatement against closed forms, and the argument checks of
``qsv_tensor_wigner``, which all run before the library's first HIP call."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from quantum_computations_amd import _lib
from quantum_computations_amd.cv_simulator import states as S
from wigner_reference import wigner_ket, wigner_rho

X = np.linspace(-20, 20, 400)
Q = np.linspace(-2.3, 2.1, 9)
P = np.linspace(-2.5, 2.2, 7)
QQ, PP = np.meshgrid(Q, P)


def test_vacuum():
    want = np.exp(-QQ ** 2 - PP ** 2) / np.pi
    assert np.abs(wigner_ket(X, S.vacuum(X), Q, P) - want).max() <= 1e-9
    psi = S.vacuum(X)
    assert np.abs(wigner_rho(X, np.outer(psi, psi.conj()), Q, P) - want).max() <= 1e-9


def test_coherent_is_shifted_in_both_quadratures():
    q0, p0 = 0.7, 1.5
    want = np.exp(-(QQ - q0) ** 2 - (PP - p0) ** 2) / np.pi
    assert np.abs(wigner_ket(X, S.coherent(X, q0 + 1j * p0), Q, P) - want).max() <= 1e-9


def test_squeezed_vacuum():
    r = 0.4
    s = np.exp(r)
    want = np.exp(-QQ ** 2 / s ** 2 - s ** 2 * PP ** 2) / np.pi
    assert np.abs(wigner_ket(X, S.squeezed_vac(X, r), Q, P) - want).max() <= 1e-9


def test_fock_one_is_negative_at_the_origin():
    want = (2 * (QQ ** 2 + PP ** 2) - 1) * np.exp(-QQ ** 2 - PP ** 2) / np.pi
    psi = S.fock_state(X, 1)
    assert np.abs(wigner_ket(X, psi, Q, P) - want).max() <= 1e-9
    assert abs(wigner_ket(X, psi, [0.0], [0.0])[0, 0] + 1 / np.pi) <= 1e-9


def _call(batch=1, d=8, x0=-1.0, dx=0.25, q=(0.0, 0.5), p=(0.0, 1.0), normalised=0, rho=16, w=16):
    q = np.ascontiguousarray(q, dtype=np.float64)
    p = np.ascontiguousarray(p, dtype=np.float64)
    dbl = C.POINTER(C.c_double)
    return _lib.load().qsv_tensor_wigner(0, None, C.c_void_p(rho) if rho else None, batch, d, x0, dx,
                                         q.ctypes.data_as(dbl), len(q), p.ctypes.data_as(dbl), len(p), normalised,
                                         C.c_void_p(w) if w else None)


@pytest.mark.parametrize("bad", [
    dict(d=1), dict(d=0), dict(batch=0), dict(batch=-2), dict(q=()), dict(p=()),
    dict(dx=0.0), dict(dx=-0.25), dict(dx=float("nan")), dict(dx=float("inf")),
    dict(q=(0.0, float("nan"))), dict(q=(float("inf"),)), dict(p=(float("-inf"),)), dict(p=(0.0, float("nan"))),
    dict(p=(0.0, np.pi / (2 * 0.25) * (1 + 1e-12))), dict(p=(-7.0,)),
    dict(rho=0), dict(w=0),
])
def test_wigner_rejects_bad_arguments_before_touching_the_device(bad):
    assert _call(**bad) == _lib.QSV_EINVAL
    with pytest.raises(ValueError):
        _lib.check(_call(**bad))

