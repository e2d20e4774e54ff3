"""TEST INFRASTRUCTURE ONLY -- plain NumPy / SciPy statements of the ten site-tensor operations of include/qsv.h that
tests/test_gpu_site_kernels.py compares the HIP kernels with, one function per ``qsv_tensor_*`` entry point, written
from the formulas in the header.  Nothing here imports the package under test.

Sites are ``(L, d, R)`` complex128 arrays, two-site tensors ``(L, d, d, R)``; every function returns a new array.
"""
from __future__ import annotations

import numpy as np
from scipy.interpolate import RegularGridInterpolator


def scale_axis(t: np.ndarray, diag: np.ndarray) -> np.ndarray:
    """``t[l, j, r] * diag[j]``."""
    return t * diag[None, :, None]


def plane_diag(theta: np.ndarray, plane: np.ndarray) -> np.ndarray:
    """``theta[a, j, l, b] * plane[j, l]``."""
    return theta * plane[None, :, :, None]


def plane_gather(theta: np.ndarray, cols: np.ndarray, vals: np.ndarray) -> np.ndarray:
    """``out[a, p, b] = sum_e vals[p, e] theta[a, cols[p, e], b]`` over the ``d * d`` plane points ``p``; table
    entries with ``cols < 0`` are padding and contribute nothing."""
    L, d, _, R = theta.shape
    cols = np.asarray(cols).reshape(d * d, -1)
    vals = np.asarray(vals).reshape(d * d, -1)
    flat = theta.reshape(L, d * d, R)
    out = np.zeros_like(flat)
    for e in range(cols.shape[1]):
        used = cols[:, e] >= 0
        out[:, used, :] += vals[used, e][None, :, None] * flat[:, cols[used, e], :]
    return out.reshape(theta.shape)


def plane_phase(theta: np.ndarray, grid: np.ndarray, strength: float) -> np.ndarray:
    """``theta[a, j, l, b] * exp(i strength q_j q_l)``, the phase evaluated in extended precision and then rounded."""
    q = np.asarray(grid, dtype=np.longdouble)
    arg = np.longdouble(strength) * np.outer(q, q)
    phase = np.cos(arg).astype(np.float64) + 1j * np.sin(arg).astype(np.float64)
    return theta * phase[None, :, :, None]


def affine_sources(grid: np.ndarray, a) -> tuple[np.ndarray, np.ndarray]:
    """Source coordinates ``(a00 x + a01 y, a10 x + a11 y)`` of every output plane point, as NumPy rounds them."""
    a00, a01, a10, a11 = (float(v) for v in a)
    x, y = np.meshgrid(np.asarray(grid, dtype=np.float64), np.asarray(grid, dtype=np.float64), indexing="ij")
    return a00 * x + a01 * y, a10 * x + a11 * y


def plane_affine(theta: np.ndarray, grid: np.ndarray, a):
    """Every ``(q_left, q_right)`` plane of ``theta`` re-sampled at its affine image, bilinear, zero outside the grid.
    Returns ``(out, x_src, y_src)``."""
    grid = np.asarray(grid, dtype=np.float64)
    xs, ys = affine_sources(grid, a)
    out = np.empty_like(theta)
    for l in range(theta.shape[0]):
        for r in range(theta.shape[3]):
            interp = RegularGridInterpolator((grid, grid), np.array(theta[l, :, :, r]), method="linear",
                                             bounds_error=False, fill_value=0)
            out[l, :, :, r] = interp((xs, ys))
    return out, xs, ys


def take_level(t: np.ndarray, level: int, scale: float) -> np.ndarray:
    """``scale * t[l, level, r]``."""
    return scale * t[:, level, :]


def insert_axis(t: np.ndarray, vec: np.ndarray) -> np.ndarray:
    """``out[l, j, r] = vec[j] * t[l, r]``."""
    return vec[None, :, None] * t[:, None, :]


def outer(p: np.ndarray, q: np.ndarray, swap_last: bool) -> np.ndarray:
    """``out[x, y, z, w] = p[x, z] q[y, w]``, or ``out[x, y, w, z]`` with ``swap_last``."""
    return np.einsum("xz,yw->xywz" if swap_last else "xz,yw->xyzw", p, q)


def _long_parts(a: np.ndarray):
    return a.real.astype(np.longdouble), a.imag.astype(np.longdouble)


def axis_overlap(z: np.ndarray, t: np.ndarray):
    """``out[j] = Re sum_{l, r} z[l, j, r] conj(t[l, j, r])`` accumulated in extended precision; also returns
    ``sum |z| |t|`` per entry, the scale of the rounding error of any summation order."""
    zr, zi = _long_parts(z)
    tr, ti = _long_parts(t)
    out = np.einsum("ljr,ljr->j", zr, tr) + np.einsum("ljr,ljr->j", zi, ti)
    return out.astype(np.float64), np.einsum("ljr,ljr->j", np.abs(z), np.abs(t))


def axis_density(z: np.ndarray, t: np.ndarray):
    """``rho[i, j] = sum_{l, r} z[l, i, r] conj(t[l, j, r])`` accumulated in extended precision (real and imaginary
    parts separately); also returns ``sum |z| |t|`` per entry."""
    zr, zi = _long_parts(z)
    tr, ti = _long_parts(t)
    re = np.einsum("lir,ljr->ij", zr, tr) + np.einsum("lir,ljr->ij", zi, ti)
    im = np.einsum("lir,ljr->ij", zi, tr) - np.einsum("lir,ljr->ij", zr, ti)
    return re.astype(np.float64) + 1j * im.astype(np.float64), np.einsum("lir,ljr->ij", np.abs(z), np.abs(t))
