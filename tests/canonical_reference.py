"""TEST INFRASTRUCTURE: canonical forms, Schmidt values, compression and overlaps of a matrix-product state in NumPy, on
lists of ``(chi_l, d, chi_r)`` site tensors in float64 (``numpy.linalg.qr`` / ``svd``).  CPU only, no package import: the
yardstick for the tolerances of ``tests/test_gpu_canonical.py`` (its own rounding on an input is the baseline the GPU
route is held to) and the restatement ``tests/test_canonical_host.py`` pins to the reference's data."""
from __future__ import annotations

import numpy as np


def contract(sites) -> np.ndarray:
    acc = sites[0]
    for t in sites[1:]:
        acc = np.tensordot(acc, t, axes=1)
    return acc.reshape(acc.shape[1:-1])


def kept_rank(s, max_bond_dim=np.inf, abs_err=0.0, rel_err=1e-12) -> int:
    """The truncation rule of the reference's ``tensor_svd`` (mps.py:86-93): drop the longest tail whose sum stays
    ``<= max(abs_err, rel_err * sum)``, then cap; at least one value stays."""
    s = np.asarray(s, dtype=np.float64)
    tails = np.cumsum(s[::-1])[::-1]
    keep = int(np.count_nonzero(tails > max(abs_err, rel_err * float(np.sum(s)))))
    if np.isfinite(max_bond_dim):
        keep = min(keep, int(max_bond_dim))
    return max(1, keep)


def numerical_rank(s, rank_tol: float) -> int:
    s = np.asarray(s)
    return int(np.count_nonzero((s > rank_tol * s[0]) & (s > 0)))


def split_left(site, rank_tol: float):
    """``site[(l,j), r] = iso[(l,j), k] carry[k, r]`` with ``carry = diag(s) Vh`` (SVD route, rank-revealing)."""
    cl, d, cr = site.shape
    u, s, vh = np.linalg.svd(site.reshape(cl * d, cr), full_matrices=False)
    r = max(1, numerical_rank(s, rank_tol))
    return u[:, :r].reshape(cl, d, r), s[:r, None] * vh[:r], s


def split_right(site, rank_tol: float):
    """``site[l, (j,r)] = carry[l, k] iso[k, (j,r)]`` with ``carry = U diag(s)``."""
    cl, d, cr = site.shape
    u, s, vh = np.linalg.svd(site.reshape(cl, d * cr), full_matrices=False)
    r = max(1, numerical_rank(s, rank_tol))
    return vh[:r].reshape(r, d, cr), u[:, :r] * s[None, :r], s


def _sweep_right(sites, stop, rank_tol):
    for k in range(stop):
        iso, carry, _ = split_left(sites[k], rank_tol)
        sites[k] = iso
        sites[k + 1] = np.tensordot(carry, sites[k + 1], axes=1)


def _sweep_left(sites, stop, rank_tol, keep=None):
    met = []
    for k in range(len(sites) - 1, stop, -1):
        iso, carry, s = split_right(sites[k], rank_tol)
        s = s[: iso.shape[0]]
        met.append(s)
        cut = iso.shape[0] if keep is None else max(1, min(iso.shape[0], keep(s)))
        sites[k] = iso[:cut]
        sites[k - 1] = np.tensordot(sites[k - 1], carry[:, :cut], axes=1)
    return met


def canonicalise(sites, centre: int, rank_tol: float = 1e-13):
    """Returns ``(new sites, Schmidt values per bond)``: all the way right, back to site 0, forward to ``centre``."""
    sites = [np.array(t, dtype=np.complex128) for t in sites]
    _sweep_right(sites, len(sites) - 1, rank_tol)
    schmidt = _sweep_left(sites, 0, rank_tol)[::-1]
    _sweep_right(sites, centre, rank_tol)
    return sites, schmidt


def compress(sites, centre: int = 0, *, max_bond_dim=np.inf, abs_err=0.0, rel_err=1e-12, rank_tol: float = 1e-13):
    """Returns ``(new sites, discarded weight per bond)``; weights are ``sum(dropped s^2) / <psi|psi>``."""
    sites = [np.array(t, dtype=np.complex128) for t in sites]
    norm2 = overlap(sites, sites).real
    _sweep_right(sites, len(sites) - 1, rank_tol)
    kept = []

    def keep(s):
        kept.append(kept_rank(s, max_bond_dim, abs_err, rel_err))
        return kept[-1]

    met = _sweep_left(sites, 0, rank_tol, keep)
    weights = [float(np.sum(s[k:] ** 2) / norm2) for s, k in zip(met, kept)][::-1]
    _sweep_right(sites, centre, rank_tol)
    return sites, weights


def overlap(a, b) -> complex:
    """``sum conj(a) b`` by the transfer-matrix recurrence."""
    e = np.ones((1, 1), dtype=np.complex128)
    for x, y in zip(a, b):
        e = np.einsum("ab,ajc,bjd -> cd", e, np.conj(x), y, optimize=True)
    return complex(e[0, 0])


def left_defect(site) -> float:
    cl, d, cr = site.shape
    m = site.reshape(cl * d, cr)
    return float(np.max(np.abs(m.conj().T @ m - np.eye(cr))))


def right_defect(site) -> float:
    cl, d, cr = site.shape
    m = site.reshape(cl, d * cr)
    return float(np.max(np.abs(m @ m.conj().T - np.eye(cl))))


def gauge_defect(sites, centre: int) -> float:
    """Largest isometry defect ``max|A^H A - 1|`` over the sites left of ``centre`` (left) and right of it (right)."""
    worst = 0.0
    for k, t in enumerate(sites):
        if k < centre:
            worst = max(worst, left_defect(t))
        elif k > centre:
            worst = max(worst, right_defect(t))
    return worst


def dense_schmidt(psi: np.ndarray) -> list[np.ndarray]:
    """Singular values of the dense tensor reshaped at every cut."""
    m, d = psi.ndim, psi.shape[0]
    return [np.linalg.svd(psi.reshape(d ** (b + 1), -1), compute_uv=False) for b in range(m - 1)]


def entropy(s) -> float:
    p = np.asarray(s, dtype=np.float64) ** 2
    p = p[p > 0] / np.sum(p)
    return float(-np.sum(p * np.log(p)))


def random_register(rng, d: int, bonds, scale_decades: float = 0.0):
    """Random sites with the given inner bonds; ``scale_decades`` > 0 grades the columns of every site over that many
    decades so that the Schmidt spectrum is wide."""
    dims = [1] + list(bonds) + [1]
    sites = []
    for cl, cr in zip(dims, dims[1:]):
        t = rng.normal(size=(cl, d, cr)) + 1j * rng.normal(size=(cl, d, cr))
        if scale_decades:
            t = t * 10.0 ** (-scale_decades * np.arange(cr) / max(cr - 1, 1))
        sites.append(t / np.sqrt(cl * d))
    return sites


def rank_deficient_registers(rng, d: int = 16):
    """Registers whose sites are rank deficient by construction, with the numerical rank every bond must come out at.
    The gap around any ``rank_tol`` in [1e-10, 1e-6] is at least 1e6 on both sides: the kept Schmidt values are O(1e-2)
    of the largest or more, the others are rounding (1e-15)."""
    cases = {}
    # duplicated columns: bond 6 whose last three columns repeat the first three
    sites = random_register(rng, d, [6, 5])
    sites[0][:, :, 3:] = sites[0][:, :, :3]
    cases["duplicated_columns"] = (sites, [3, 5])
    # a zero column (and the matching row of the neighbour left in place)
    sites = random_register(rng, d, [5, 4])
    sites[1][:, :, 2] = 0.0
    cases["zero_column"] = (sites, [5, 3])
    # a product state stored with bond 8: every site is an outer product
    vecs = [rng.normal(size=d) + 1j * rng.normal(size=d) for _ in range(4)]
    dims = [1, 8, 8, 8, 1]
    sites = []
    for v, cl, cr in zip(vecs, dims, dims[1:]):
        left, right = rng.normal(size=cl) + 0j, rng.normal(size=cr) + 0j
        sites.append(left[:, None, None] * v[None, :, None] * right[None, None, :] / np.sqrt(d))
    cases["product_bond8"] = (sites, [1, 1, 1])
    return cases
