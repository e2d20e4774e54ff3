"""TEST INFRASTRUCTURE: NumPy restatement of multi-shot homodyne sampling of a matrix-product state.

The definition (``MPS.sample``): shot ``s`` measures the modes from the left; for mode ``k``

1. ``w[j]`` = diagonal of ``partial_density_mps`` (mps.py:176-190) of the register collapsed onto the shot's earlier
   picks and renormalised, times ``dq`` (gates.py:95-96),
2. ``pick = searchsorted(cdf, u, "right")`` with ``cdf = cumsum(w / w.sum())``, ``cdf /= cdf[-1]`` -- what
   ``rng.choice(range(d), p=w / w.sum())`` returns for the uniform ``u`` (gates.py:98),
3. ``density = w[pick] / dq`` (gates.py:102),
4. the collapsed left part, a boundary vector ``v``, becomes ``v . A_k[:, pick, :] / sqrt(density)`` (gates.py:108-113).

Everything works on the site tensors (boundary vectors on the left, environments on the right): no ``d^m`` tensor.
"""
from __future__ import annotations

import numpy as np


def right_environments(sites) -> list[np.ndarray]:
    """``E_k``: the contraction of every site to the right of ``k`` with its conjugate (mps.py:185-186)."""
    envs, r = [None] * len(sites), np.ones((1, 1), dtype=np.complex128)
    for k in range(len(sites) - 1, -1, -1):
        envs[k] = r
        t = sites[k]
        r = np.einsum("ica,jcb,ab -> ij", t, np.conj(t), r, optimize=True)
    return envs


def sample(sites, dq: float, uniforms: np.ndarray, picks: np.ndarray | None = None, chunk: int = 256,
           measured_sites=None) -> dict:
    """Follow the definition for every row of ``uniforms`` (shots x m).  With ``picks`` given, those are taken instead
    of the restatement's own (the conditional CDFs are then the ones *given those picks*).  ``measured_sites[k]``: site
    ``k`` after the pre-rotation of its measurement (Mp, Homodyne; gates.py:120-148).  The chain rotates a mode only
    when its turn comes, so the environments to the right of a mode are those of the sites as they are -- which
    matters because a rotation sampled on a finite grid is not exactly unitary.  Returns ``picks``,
    ``densities`` and, per shot and mode, the CDF values around the pick: ``below = cdf[pick - 1]`` (0 for pick 0) and
    ``above = cdf[pick]``; ``margin`` = the smallest distance of any ``u`` from a CDF edge of its own step."""
    sites = [np.asarray(t, dtype=np.complex128) for t in sites]
    uniforms = np.asarray(uniforms, dtype=np.float64)
    shots, m = uniforms.shape
    assert m == len(sites)
    envs = right_environments(sites)
    if measured_sites is not None:
        sites = [np.asarray(t, dtype=np.complex128) for t in measured_sites]
    out_picks = np.zeros((shots, m), dtype=np.int64)
    densities, below, above = (np.zeros((shots, m)) for _ in range(3))
    margin = np.inf
    for s0 in range(0, shots, chunk):
        rows = slice(s0, min(s0 + chunk, shots))
        n = rows.stop - rows.start
        v = np.ones((n, 1), dtype=np.complex128)
        for k, (t, env) in enumerate(zip(sites, envs)):
            w_amp = np.einsum("sa,ajb -> sjb", v, t, optimize=True)
            w = np.einsum("sjb,bc,sjc -> sj", w_amp, env, np.conj(w_amp), optimize=True).real * dq ** (m - k)
            cdf = np.cumsum(w / w.sum(axis=1, keepdims=True), axis=1)
            cdf /= cdf[:, -1:]
            u = uniforms[rows, k]
            own = np.array([np.searchsorted(cdf[i], u[i], side="right") for i in range(n)])
            margin = min(margin, float(np.min(np.abs(cdf - u[:, None]))))
            chosen = own if picks is None else np.asarray(picks)[rows, k]
            idx = np.arange(n)
            out_picks[rows, k] = chosen
            densities[rows, k] = w[idx, chosen] / dq
            above[rows, k] = cdf[idx, chosen]
            below[rows, k] = np.where(chosen > 0, cdf[idx, np.maximum(chosen - 1, 0)], 0.0)
            v = w_amp[idx, chosen, :] / np.sqrt(densities[rows, k])[:, None]
    return {"picks": out_picks, "densities": densities, "below": below, "above": above, "margin": margin}
