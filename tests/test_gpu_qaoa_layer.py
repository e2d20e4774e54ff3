"""QAOA with the mixer as a product layer: ``mixer="layer"`` of ``qaoa.energies``, ``qaoa.landscape``,
``qaoa.run`` and ``qaoa.energy_and_gradient`` against the default code paths, which this keyword leaves untouched.

Instances: MaxCut on the 3-regular ring-and-chord graph of 6 and 8 qubits with p = 3, and one 13-qubit instance with p = 1 (a
member of two tile passes).  A 3-regular graph has an even number of vertices: the 13-qubit graph is the ring with the chords
(i, i + 6), i < 6, which leaves vertex 12 with degree 2.

Tolerance: energies and gradients within ``ADJOINT_TOL sum|c_t|``, ADJOINT_TOL = 1e-12 (tests/test_gpu_qaoa.py).
"""
from __future__ import annotations

import numpy as np
import pytest

from quantum_computations_amd import DiagonalOperator, qaoa
from quantum_computations_amd import workloads as W
from test_gpu_sweep import ADJOINT_TOL, maxabs, report

pytestmark = pytest.mark.gpu


def instance(n):
    edges = W.ring_chord_edges(n) if n % 2 == 0 else [(i, (i + 1) % n) for i in range(n)] + [(i, i + 6) for i in range(6)]
    terms = W.maxcut_terms(n, edges)
    return terms, sum(abs(c) for c, _, _ in terms)


@pytest.mark.parametrize("n, p, points", [(6, 3, 11), (8, 3, 11), (13, 1, 5)])
def test_energies_and_gradients_with_the_layer_mixer(n, p, points):
    terms, weight = instance(n)
    op = DiagonalOperator.from_terms(n, terms)
    rng = np.random.default_rng(n)
    gammas, betas = rng.uniform(-0.7, 0.7, (points, p)), rng.uniform(-0.7, 0.7, (points, p))
    rotations = qaoa.energies(op, gammas, betas, batch=4, mixer="rotations")
    assert np.array_equal(rotations, qaoa.energies(op, gammas, betas, batch=4))          # the default, untouched
    layer = qaoa.energies(op, gammas, betas, batch=4, mixer="layer")
    report(f"n={n} p={p}: energies, layer against rotations", maxabs(layer - rotations), ADJOINT_TOL * weight)
    assert maxabs(rotations) > 1e-2                                       # not a comparison of zeros
    energy, below = qaoa.energies(op, gammas[:3], betas[:3], batch=2, threshold=-0.5 * n, mixer="layer")
    want_energy, want_below = qaoa.energies(op, gammas[:3], betas[:3], batch=2, threshold=-0.5 * n)
    report(f"n={n}: energies with a threshold", maxabs(energy - want_energy), ADJOINT_TOL * weight)
    report(f"n={n}: P(D <= threshold)", maxabs(below - want_below), 2 * ADJOINT_TOL)
    # one point: the state and the adjoint walk
    e0, dg0, db0 = qaoa.energy_and_gradient(op, gammas[0], betas[0])
    e1, dg1, db1 = qaoa.energy_and_gradient(op, gammas[0], betas[0], mixer="layer")
    report(f"n={n} p={p}: energy of the adjoint walk", abs(e1 - e0), ADJOINT_TOL * weight)
    report(f"n={n} p={p}: dE/dgamma", maxabs(dg1 - dg0), ADJOINT_TOL * weight)
    report(f"n={n} p={p}: dE/dbeta", maxabs(db1 - db0), ADJOINT_TOL * weight)
    report(f"n={n} p={p}: energies against the adjoint walk", abs(layer[0] - e0), ADJOINT_TOL * weight)
    assert maxabs(dg0) > 1e-3 and maxabs(db0) > 1e-3
    state = qaoa.run(op, gammas[0], betas[0], mixer="layer")
    want = qaoa.run(op, gammas[0], betas[0])
    report(f"n={n} p={p}: the state of run", float(np.linalg.norm(state.to_numpy() - want.to_numpy())), ADJOINT_TOL)
    state.close()
    want.close()
    for call in (lambda: qaoa.energies(op, gammas, betas, mixer="gates"), lambda: qaoa.run(op, gammas[0], betas[0], mixer="rotations"),
                 lambda: qaoa.energy_and_gradient(op, gammas[0], betas[0], mixer="x")):
        with pytest.raises(ValueError):
            call()
    op.close()


@pytest.mark.parametrize("n", (6, 8))
def test_landscape_with_both_mixers(n):
    terms, weight = instance(n)
    op = DiagonalOperator.from_terms(n, terms)
    gamma_grid, beta_grid = np.linspace(-0.6, 0.6, 4), np.linspace(0.0, 0.7, 4)
    rotations = qaoa.landscape(op, gamma_grid, beta_grid)
    layer = qaoa.landscape(op, gamma_grid, beta_grid, mixer="layer")
    assert layer.shape == rotations.shape == (4, 4)
    report(f"n={n}: landscape, layer against rotations", maxabs(layer - rotations), ADJOINT_TOL * weight)
    assert np.array_equal(rotations, qaoa.landscape(op, gamma_grid, beta_grid, mixer="rotations"))
    op.close()
