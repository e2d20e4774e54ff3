"""The pass planner of the deferred gate queue (quantum_computations_amd/csrc/qsv_plan.h), on the host only.

tests/defer_plan/plan_driver.cpp is compiled against the header with AddressSanitizer + UBSan and fed thousands of random
gate lists; every plan is checked for the rules the device path relies on (each gate exactly once, queue order except
for exact moves of signed permutations past gates on other qubits, six tile bits above bits 0..5, control masks split
correctly between the tile and the tile's base index).  A NumPy model of the pass executor (k_pass_tile: tiles, tile
skipping by outside controls, controls inside the tile) must then reproduce the gates applied one by one EXACTLY.

The gate records, their classification and the model are in tests/defer_plan_model.py, which the tests of the group cutter
and of the pass records use too.
"""
from __future__ import annotations

import numpy as np
import pytest

import hostcheck
from defer_plan_model import apply_rec, check_plan, classify, execute, random_ops, run_driver
from defer_plan_model import WINDOW, tile_index  # noqa: F401  (these two and compiler: tools/bench_deferred.py takes them
from hostcheck import compiler  # noqa: F401                   from this module, where they used to be defined)
from quantum_computations_amd import workloads as W


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return hostcheck.compile_driver(hostcheck.HERE / "defer_plan" / "plan_driver.cpp", tmp_path_factory.mktemp("plan"))


def test_plans_of_random_circuits_obey_the_rules(driver):
    rng = np.random.default_rng(2024)
    lists = []
    for trial in range(3000):
        n = int(rng.integers(8, 31))
        ops = random_ops(rng, n, int(rng.integers(1, 160)))
        lists.append((n, [r for r in (classify(o, n) for o in ops) if r is not None]))
    plans = run_driver(driver, lists)
    launches = gates = 0
    for (n, recs), plan in zip(lists, plans):
        check_plan(n, recs, plan)
        launches += len(plan)
        gates += len(recs)
    assert launches < gates / 2, (launches, gates)


def test_numpy_model_of_the_passes_is_exactly_the_per_gate_path(driver):
    rng = np.random.default_rng(7)
    lists, states = [], []
    for trial in range(60):
        n = int(rng.integers(12, 15))
        ops = random_ops(rng, n, int(rng.integers(20, 90)))
        lists.append((n, [r for r in (classify(o, n) for o in ops) if r is not None]))
        states.append(W.random_ket(n, trial))
    plans = run_driver(driver, lists)
    fused = 0
    for (n, recs), plan, psi in zip(lists, plans, states):
        want = psi.copy()
        for r in recs:
            apply_rec(want, r, lambda b: b, r.ctrl_mask)
        got = execute(n, recs, plan, psi)
        assert np.array_equal(got, want)
        fused += sum(1 for f, _, _ in plan if f)
    assert fused > 100


def test_benchmark_circuit_needs_at_most_12_launches_per_100_gates(driver):
    n = 28
    recs = [classify(o, n) for o in W.random_circuit(n, 100, 100)]
    assert all(r is not None for r in recs)
    one_step, two_steps = run_driver(driver, [(n, recs), (n, recs + recs)])
    check_plan(n, recs, one_step)
    assert len(one_step) <= 12, [(f, len(g)) for f, _, g in one_step]
    assert len(two_steps) <= 24
