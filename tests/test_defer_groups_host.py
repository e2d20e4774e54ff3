"""The group cutter of the pass kernel (qsv_plan::cut_groups in quantum_computations_amd/csrc/qsv_plan.h), on the host only.

k_pass_tile applies the gates of a pass in groups: consecutive gates whose targets fit four tile bits are applied on 16
amplitudes per thread in registers, with one LDS round trip per group.  tests/defer_plan/groups_driver.cpp is compiled
against the header with AddressSanitizer + UBSan and fed thousands of random passes; every cut is checked for the rules the
kernel relies on.  A NumPy model of the grouped executor (tiles, groups as a re-indexing of the tile into thread and
register bits, controls inside the tile as selects, tile and group activity by outside controls) must then reproduce the
gates applied one by one EXACTLY.
"""
from __future__ import annotations

import numpy as np
import pytest

import defer_plan_model as base
import hostcheck
from quantum_computations_amd import workloads as W

REG_BITS, TILE_BITS = 4, 12


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    return {name: hostcheck.compile_driver(hostcheck.HERE / "defer_plan" / f"{name}.cpp", tmp_path_factory.mktemp(name))
            for name in ("plan_driver", "groups_driver")}


def cut(driver, passes):
    """passes: [[need mask per gate]] -> per pass, [(first, count, (reg0..reg3))]."""
    text = "".join(f"{len(p)} " + " ".join(str(m) for m in p) + "\n" for p in passes)
    proc = hostcheck.run_clean(driver, text, timeout=600)
    cuts, lines = [], iter(proc.stdout.split("\n"))
    for line in lines:
        if not line.startswith("groups "):
            continue
        groups = []
        for _ in range(int(line.split()[1])):
            v = [int(t) for t in next(lines).split()[1:]]
            groups.append((v[0], v[1], tuple(v[2:])))
        cuts.append(groups)
    assert len(cuts) == len(passes)
    return cuts


def popcount(x):
    return bin(x).count("1")


def check_cut(need, groups):
    if not need:
        assert groups == []
        return
    at = 0
    for k, (first, count, reg) in enumerate(groups):
        assert first == at and count >= 1, "the groups partition the gate list in order"
        at += count
        assert len(set(reg)) == REG_BITS and all(0 <= t < TILE_BITS for t in reg), reg
        assert list(reg) == sorted(reg)
        mask = sum(1 << t for t in reg)
        used = 0
        for m in need[first:first + count]:
            assert m & ~mask == 0, "every gate's targets lie inside the group's register bits"
            used |= m
        assert popcount(used) <= REG_BITS
        # the fill: the highest tile indices that no gate of the group targets
        free = [t for t in range(TILE_BITS - 1, -1, -1) if not (used >> t) & 1][:REG_BITS - popcount(used)]
        assert mask == used | sum(1 << t for t in free), (reg, used)
        if k:
            assert need[first] != 0, "a gate without targets never starts a group, unless it is first in the pass"
        if first + count < len(need):
            assert popcount(used | need[first + count]) > REG_BITS, "the group could have taken the next gate"
    assert at == len(need)


def random_pass(rng):
    count = int(rng.integers(1, 65))
    style = int(rng.integers(4))
    pool = np.arange(TILE_BITS) if style < 2 else rng.choice(TILE_BITS, size=int(rng.integers(2, 7)), replace=False)
    need = []
    for _ in range(count):
        kind = rng.random()
        if kind < (0.5 if style == 1 else 0.2):
            need.append(0)
        else:
            k = 1 if kind < 0.6 else 2
            need.append(sum(1 << int(t) for t in rng.choice(pool, size=k, replace=False)))
    return need


def test_random_passes_are_cut_by_the_rules(drivers):
    rng = np.random.default_rng(5)
    passes = [random_pass(rng) for _ in range(4000)] + [[], [0], [0, 0, 0], [3, 12, 0, 48, 0, 0, 192]]
    cuts = cut(drivers["groups_driver"], passes)
    groups = gates = 0
    for need, got in zip(passes, cuts):
        check_cut(need, got)
        groups += len(got)
        gates += len(need)
    assert groups < gates / 2, (groups, gates)


def test_fill_prefers_the_highest_free_tile_indices(drivers):
    (a,), (b,), (c, d, e) = cut(drivers["groups_driver"], [[1], [1 << 11 | 1 << 10, 0], [1 | 2, 4 | 8, 16, 0, 32 | 64, 128 | 256]])
    assert a == (0, 1, (0, 9, 10, 11))
    assert b == (0, 2, (8, 9, 10, 11))
    assert (c, d, e) == ((0, 2, (0, 1, 2, 3)), (2, 3, (4, 5, 6, 11)), (5, 1, (7, 8, 10, 11)))


def need_of(rec, tile):
    if rec.kind in ("diag", "phase"):
        return 0
    return sum(1 << base.tile_index(b, tile) for b in rec.targets)


def execute_grouped(n, recs, plan, cuts, psi):
    """base.execute with the gates of a fused pass applied group by group: the tile is re-indexed so that the group's four
    register bits are index bits 0..3 and the thread bits follow (what a thread holds is one row of 16), the gates are
    applied there, and the tile is put back."""
    psi = psi.copy()
    cuts = iter(cuts)
    for fused, tile, gates in plan:
        if not fused:
            base.apply_rec(psi, recs[gates[0][0]], lambda b: b, recs[gates[0][0]].ctrl_mask)
            continue
        groups = next(cuts)
        tbits = list(range(6)) + [b for b in range(6, n) if (tile >> b) & 1]
        others = [b for b in range(n) if b not in tbits]
        local = np.arange(1 << len(tbits))
        offset = sum(((local >> i) & 1) << b for i, b in enumerate(tbits))
        for w in range(1 << len(others)):
            origin = sum(((w >> i) & 1) << b for i, b in enumerate(others))
            active = [origin & outside == outside for _, _, outside in gates]
            if not any(active):
                continue
            v = psi[origin | offset]
            for first, count, reg in groups:
                if not any(active[first:first + count]):
                    continue
                order = list(reg) + [t for t in range(len(tbits)) if t not in reg]     # new index bit -> tile index
                new_of = {t: i for i, t in enumerate(order)}
                perm = sum(((local >> i) & 1) << t for i, t in enumerate(order))        # new index -> tile index
                x = v[perm]
                for k in range(first, first + count):
                    if not active[k]:
                        continue
                    g, inside, _ = gates[k]
                    cmask = sum(1 << new_of[t] for t in range(len(tbits)) if (inside >> t) & 1)
                    base.apply_rec(x, recs[g], lambda b: new_of[base.tile_index(b, tile)], cmask)
                v[perm] = x
            psi[origin | offset] = v
    return psi


def test_numpy_model_of_the_grouped_passes_is_exactly_the_per_gate_path(drivers):
    rng = np.random.default_rng(11)
    lists, states = [], []
    for trial in range(40):
        n = int(rng.integers(13, 15))
        ops = base.random_ops(rng, n, int(rng.integers(20, 90)))
        lists.append((n, [r for r in (base.classify(o, n) for o in ops) if r is not None]))
        states.append(W.random_ket(n, 100 + trial))
    plans = base.run_driver(drivers["plan_driver"], lists)
    passes, per_list = [], []
    for (n, recs), plan in zip(lists, plans):
        mine = [[need_of(recs[g], tile) for g, _, _ in gates] for fused, tile, gates in plan if fused]
        per_list.append(len(mine))
        passes += mine
    cuts = cut(drivers["groups_driver"], passes)
    at = groups = gates = 0
    for (n, recs), plan, psi, k in zip(lists, plans, states, per_list):
        want = psi.copy()
        for r in recs:
            base.apply_rec(want, r, lambda b: b, r.ctrl_mask)
        for need, got in zip(passes[at:at + k], cuts[at:at + k]):
            check_cut(need, got)
            groups += len(got)
            gates += len(need)
        got = execute_grouped(n, recs, plan, cuts[at:at + k], psi)
        at += k
        assert np.array_equal(got, want)
    assert 0 < groups < gates / 2, (groups, gates)


def test_benchmark_circuit_is_cut_into_about_three_groups_per_pass(drivers):
    n = 28
    recs = [base.classify(o, n) for o in W.random_circuit(n, 400, 100)]
    (plan,) = base.run_driver(drivers["plan_driver"], [(n, recs)])
    passes = [[need_of(recs[g], tile) for g, _, _ in gates] for fused, tile, gates in plan if fused]
    cuts = cut(drivers["groups_driver"], passes)
    for need, got in zip(passes, cuts):
        check_cut(need, got)
    groups, gates = sum(len(c) for c in cuts), sum(len(p) for p in passes)
    assert len(plan) <= 48 and groups <= 0.4 * gates, (len(plan), groups, gates)
